"""The sum-of-regularisers model at its edges, against oracle/sumregs_oracle.c.

PDHG (sr_tile_kernel = variant 1, 32 x 32 region; sr_strip_kernel = variant 2, 48 x 48 region): bit-exact
(np.array_equal with bplo_sumregs_pdhg) at sides of 1, 2, 3 and 5 pixels and around the tile cores, at every fusion depth
(T = 1..7 / 1..11 and the clamp), with Huber (rho > 0), accel = 0, custom tau0 / sigma0 and one regulariser switched off,
for vector, patch and map parameters, through one or two launch chains with either parity of the stagger, without the
graph, and with gap checks every 7 / 13 iterations (early stop = the fixed-count run of the iteration it stopped at).

Gradients on the same u as the oracle (u is bit-exact, so the active sets agree): vector, 2 x 2, non-square and
non-dividing patches and the pixel map, both branches, through every factorisation (nd, nd-lu, band-hbm, band-lu) and the
nested-dissection options on the 13-point system, at pinned refinement counts (REFINE below).  Tolerances: 1e-6 of max|g|
for gradient, 1e-7 for gradient_reg; between factorisations 1e-6 / 1e-9; bitwise where the code promises it (nd_staged,
image groups, deterministic shards of a patch parameter).

Rejected calls (rho > 0 with a zero entry, the TV kernel plan, init / order or an unknown variant on this model, block
cyclic reduction in its evaluate, gradient_reg with an array parameter that has a zero entry in either model's evaluate;
a TV sweep with rho > 0 and a zero entry, an unknown variant, or init on a float handle) leave the handle as it was:
duality gap, iteration count, and the next solve."""
import numpy as np
import pytest
from conftest import synth_batch
from test_oracle_sumregs import EDGE_MAXITER, EDGE_SHAPES, edge_case

pytestmark = pytest.mark.gpu

A3 = np.array([0.03, 0.02, 0.05])
P22 = np.stack([np.array([[0.03, 0.05], [0.02, 0.04]]), np.array([[0.02, 0.03], [0.05, 0.02]]),
                np.array([[0.04, 0.02], [0.03, 0.06]])])
R = {1: 32, 2: 48}                        # region side of each kernel
TMAX = {1: 7, 2: 11}                      # (R - 1) // 4: the deepest fusion that leaves a core


def _map(N, M, seed=1, lo=0.02, hi=0.07):
    return lo + (hi - lo) * np.random.default_rng(seed).random((3, N, M))


def _clamped_T(T, M, N, var):
    mt = lambda L: (1 << 20) if L <= R[var] else (R[var] - 1) // 4
    return min(T, mt(M), mt(N))


def _solver(cls, ub, f, **kw):
    O, N, M = f.shape
    s = cls(M, N, O, **kw)
    s.set_data(ub, f)
    return s


# ---------------------------------------------------------------------------------------------------------------------
# PDHG
# ---------------------------------------------------------------------------------------------------------------------
PDHG_SHAPES = EDGE_SHAPES + [(1, 31, 32), (1, 32, 33), (2, 33, 47), (1, 48, 49), (1, 47, 17), (1, 15, 49),
                             (1, 81, 20), (1, 79, 9)]   # R - 1, R, R + 1 of both regions; R + (R - 4T) +- 1 at T = 4


@pytest.mark.parametrize("shape", PDHG_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_pdhg_edge_shapes_both_kernels(gpu_solver_cls, oracle, shape):
    O, N, M = shape
    ub, f = synth_batch(O, N, M, seed=3 + N + 7 * M)
    s = _solver(gpu_solver_cls, ub, f)
    for alpha in (A3, _map(N, M, seed=N * M)):
        for var in (1, 2):
            for it, T in ((37, 4), (23, 3), (9, 1)):
                u = s.sumregs_denoise(alpha, maxiter=it, tile_iters=T, variant=var)
                st = s.stats()
                assert (st["pdhg_variant"], st["region_i"], st["tile_iters"]) == (var, R[var], _clamped_T(T, M, N, var))
                assert np.array_equal(u, oracle.sumregs_pdhg(f, alpha, maxiter=it, nthreads=4)), (np.shape(alpha), var, it, T)
    s.close()


@pytest.mark.parametrize("var", [1, 2])
def test_every_fusion_depth(gpu_solver_cls, oracle, var):
    """T = 1 .. (R - 1) / 4 on an image larger than the region in both axes (no clamp), then the clamp: a deeper T is cut
    to (R - 1) / 4 where a side exceeds the region, and not at all where the image fits one region."""
    ub, f = synth_batch(2, 2 * R[var] + 5, 2 * R[var] - 3, seed=61 + var)
    O, N, M = f.shape
    s = _solver(gpu_solver_cls, ub, f)
    alpha = _map(N, M, seed=var)
    for T in range(1, TMAX[var] + 1):
        it = 3 * T + 2                       # the last launch of every chain is a partial one
        u = s.sumregs_denoise(alpha, maxiter=it, tile_iters=T, variant=var)
        assert s.stats()["tile_iters"] == T
        assert np.array_equal(u, oracle.sumregs_pdhg(f, alpha, maxiter=it, nthreads=4)), T
    u = s.sumregs_denoise(A3, maxiter=40, tile_iters=TMAX[var] + 5, variant=var)
    assert s.stats()["tile_iters"] == TMAX[var]
    assert np.array_equal(u, oracle.sumregs_pdhg(f, A3, maxiter=40, nthreads=4))
    s.close()
    # thin: one side fits the region (no bound from it), the other does not
    ub, f = synth_batch(1, R[var] + 9, 12, seed=5)
    s = _solver(gpu_solver_cls, ub, f)
    u = s.sumregs_denoise(A3, maxiter=33, tile_iters=TMAX[var] + 3, variant=var)
    assert s.stats()["tile_iters"] == TMAX[var]
    assert np.array_equal(u, oracle.sumregs_pdhg(f, A3, maxiter=33, nthreads=4))
    s.close()
    # small: the image is one region, T is not clamped
    ub, f = synth_batch(2, 20, 17, seed=6)
    s = _solver(gpu_solver_cls, ub, f)
    u = s.sumregs_denoise(A3, maxiter=41, tile_iters=TMAX[var] + 2, variant=var)
    assert s.stats()["tile_iters"] == TMAX[var] + 2
    assert np.array_equal(u, oracle.sumregs_pdhg(f, A3, maxiter=41, nthreads=4))
    s.close()


RUNTIME = [dict(rho=0.01), dict(rho=0.3), dict(accel=0), dict(tau0=3.0, sigma0=0.3), dict(rho=0.3, accel=0),
           dict(rho=0.01, accel=0, tau0=2.0, sigma0=0.45)]


@pytest.mark.parametrize("kind", ["vector", "patch", "map"])
def test_runtime_choices(gpu_solver_cls, oracle, kind):
    """Huber (the den = 1 + sigma rho / a branch), accel = 0 and custom steps, alone and combined, on both kernels; every
    parameter entry > 0.  Then one regulariser switched off (its slice all zero, rho = 0)."""
    ub, f = synth_batch(2, 40, 37, seed=71)
    O, N, M = f.shape
    alpha = {"vector": A3, "patch": P22, "map": _map(N, M, seed=4)}[kind]
    s = _solver(gpu_solver_cls, ub, f)
    for kw in RUNTIME:
        for var in (1, 2):
            u = s.sumregs_denoise(alpha, maxiter=60, variant=var, **kw)
            u0 = oracle.sumregs_pdhg(f, alpha, maxiter=60, nthreads=4, **kw)
            assert np.array_equal(u, u0), (kw, var)
    plain = oracle.sumregs_pdhg(f, alpha, maxiter=60, nthreads=4)
    assert not np.array_equal(plain, oracle.sumregs_pdhg(f, alpha, maxiter=60, nthreads=4, rho=0.01))   # rho matters
    for off in range(3):
        a = np.array(alpha, dtype=np.float64, copy=True)
        a[off] = 0.0
        for var in (1, 2):
            assert np.array_equal(s.sumregs_denoise(a, maxiter=60, variant=var), oracle.sumregs_pdhg(f, a, maxiter=60, nthreads=4))
    s.close()


@pytest.mark.parametrize("var", [1, 2])
def test_launch_chains_stagger_and_gap_checks(gpu_solver_cls, oracle, var):
    """Two launch chains run half a launch out of phase when the parity allows it (tiling.hpp's chain_out_of_phase: T >= 2, >= 8
    launches, and the staggered chain ends in the same state set): stats()["launches"] is 2 nl + 1 with the stagger, 2 nl
    without.  One chain, T = 1, fewer than 8 launches, no graph, and gap checks every 7 / 13 iterations at T = 4."""
    ub, f = synth_batch(3, 50, 44, seed=81)
    O, N, M = f.shape
    alpha = _map(N, M, seed=9)
    s = _solver(gpu_solver_cls, ub, f)
    cases = [(40, 4, 1), (43, 4, 1), (38, 4, 0), (41, 4, 0), (42, 4, 0), (39, 3, 1), (38, 3, 1), (37, 3, 0), (20, 4, 0), (12, 1, 0)]
    for it, T, stag in cases:
        nl = -(-it // T)
        h0 = max(1, T // 2)
        assert stag == int(T >= 2 and nl >= 8 and ((1 + -(-(it - h0) // T)) - nl) % 2 == 1)
        u0 = oracle.sumregs_pdhg(f, alpha, maxiter=it, nthreads=4)
        for ch in (1, 2):
            u = s.sumregs_denoise(alpha, maxiter=it, tile_iters=T, variant=var, chains=ch)
            st = s.stats()
            assert st["launch_chains"] == ch and st["graph_used"] == 1
            assert st["launches"] == ch * nl + (stag if ch == 2 else 0), (it, T, ch, st["launches"])
            assert np.array_equal(u, u0), (it, T, ch)
        assert np.array_equal(s.sumregs_denoise(alpha, maxiter=it, tile_iters=T, variant=var, use_graph=0), u0)
        assert s.stats()["graph_used"] == 0
    # gap checks at a period that is no multiple of T: the fixed-count result, and an early stop at a check
    for ce in (7, 13):
        u = s.sumregs_denoise(alpha, maxiter=61, tile_iters=4, variant=var, check_every=ce)
        assert s.stats()["iterations"] == 61 and np.array_equal(u, oracle.sumregs_pdhg(f, alpha, maxiter=61, nthreads=4))
        s.sumregs_denoise(alpha, maxiter=3 * ce, tile_iters=4, variant=var)
        tol = float(s.duality_gap().max())
        u = s.sumregs_denoise(alpha, maxiter=300, tile_iters=4, variant=var, check_every=ce, gap_tol=tol)
        it = s.stats()["iterations"]
        assert it % ce == 0 and it < 300 and 0 <= s.stats()["last_gap"] <= tol
        assert np.array_equal(u, oracle.sumregs_pdhg(f, alpha, maxiter=it, nthreads=4)), (ce, it)
    s.close()


# ---------------------------------------------------------------------------------------------------------------------
# Gradients
# ---------------------------------------------------------------------------------------------------------------------
def _methods(reg, alpha, npx):
    """(name, adjoint_method, sr_force_lu) of every factorisation that applies: gradient_reg with an array parameter is
    row-scaled and non-symmetric, so only the two LU factorisations take it.  A 1 x 1 image has a band of width 0; the
    band solvers are not run there (its gradient is identically 0, which the nested dissection shows)."""
    array = np.ndim(alpha) == 3 and np.size(alpha) > 3
    m = [("nd-lu", "nd", 0), ("band-lu", "band", 0)] if reg and array else \
        [("nd", "nd", 0), ("nd-lu", "nd", 1), ("band-hbm", "band", 0), ("band-lu", "band", 1)]
    return [x for x in m if npx > 1 or x[1] == "nd"]


# Refinement sweeps of the factorisation comparisons.  The oracle refines three times (nref = 3), the device five times by
# default (twice until tests/test_gpu_sumregs_active_set.py); each sweep gains a digit and more with Cholesky on the
# kappa = 1/eps rows of the gradient, so at the oracle's count every factorisation lands within 3e-7 of max|g| of it, thin shapes included (at two sweeps (2, 1, 9), (1, 2, 2)
# and (2, 5, 3) stay at 1.1e-6 / 3.0e-6 / 1.4e-6).  LU without pivoting forced on that symmetric system (option
# sr_force_lu, a test aid) inverts its pivot blocks by Gauss-Jordan without pivoting and gains about one digit per sweep
# there (1 x 2 patch on 4 x 64 x 80: 2.7e-5 / 7.5e-6 / 2.1e-6 / 1.6e-7 / 9e-10 after 2 / 3 / 4 / 6 / 10 sweeps), so it
# gets ten.  gradient_reg (gamma = 1e8 instead of 1/eps) is at rounding level after one sweep in every factorisation.
REFINE, REFINE_FORCED_LU = 3, 10
# The device's former default of two sweeps, on the thin shapes named above (the product path, nd): 5x the gap measured then.
THIN_TOL = {(2, 1, 9): 5e-6, (1, 2, 2): 1.5e-5, (2, 5, 3): 7e-6}


def _grads(s, alpha, delta, maxiter):
    """{method: (u, cost, grad)} through every factorisation on one handle; asserts the method each one reports."""
    reg = not (delta > 1e-3)
    out = {}
    for name, adj, flu in _methods(reg, alpha, s.M * s.N):
        s.set_option("sr_force_lu", flu)
        out[name] = s.sumregs_evaluate(alpha, delta, maxiter=maxiter, adjoint_method=adj,
                                       refine=REFINE_FORCED_LU if (flu and not reg) else REFINE)
        st = s.stats()
        assert st["adjoint_method"] == name and st["reg_gradient_used"] == int(reg), (name, st["adjoint_method"])
        assert st["adjoint_residual"] <= 1e-6, (name, st["adjoint_residual"])   # the gate; (2, 5, 3) after its kappa retry: 2e-7
    s.set_option("sr_force_lu", 0)
    return out


def _check_against_oracle(oracle, res, f, ub, alpha, reg, maxiter):
    """Every factorisation against the oracle on the same u, within 1e-7 of max|g| for gradient_reg and 1e-6 for
    gradient; with each other within 1e-9 (gradient_reg) and 1e-6 (gradient: two results each within 3e-7 of the oracle,
    which is as close as the kappa = 1/eps system determines them)."""
    u0 = oracle.sumregs_pdhg(f, alpha, maxiter=maxiter, nthreads=4)
    g0 = oracle.sumregs_gradient(alpha, u0, ub, reg=reg)
    scale = max(np.abs(g0).max(), 1e-300)
    tol = 1e-7 if reg else 1e-6
    ref = None
    for name, (u, c, g) in res.items():
        assert np.array_equal(u, u0), name
        assert np.isclose(c, oracle.cost(u0, ub), rtol=1e-13)
        assert np.all(np.isfinite(g)) and np.size(g) == np.size(g0)
        g = np.reshape(g, np.shape(g0))
        assert np.abs(g - g0).max() <= tol * scale + 1e-300, (name, np.abs(g - g0).max() / scale)
        if ref is None:
            ref = g
        assert np.abs(g - ref).max() <= (1e-9 if reg else 1e-6) * scale, (name, np.abs(g - ref).max() / scale)
    return g0


@pytest.mark.parametrize("shape", EDGE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_gradients_at_edge_shapes_every_factorisation(gpu_solver_cls, oracle, shape):
    """Every parameter kind and branch through nd, nd-lu, band-hbm and band-lu at the edge shapes.  The one case whose
    literal system is singular (test_oracle_sumregs.EDGE_LITERAL_SINGULAR) must match the oracle or fail with a clean
    BpltvError -- never return non-finite values."""
    from bpldenoising_amd._lib import BpltvError
    from test_oracle_sumregs import EDGE_LITERAL_SINGULAR
    for kind in ("vector", "patch", "map"):
        ub, f, alpha = edge_case(shape, kind)
        s = _solver(gpu_solver_cls, ub, f)
        for delta in (0.1, 1e-4):
            reg = delta <= 1e-3
            if (shape, kind, reg) in EDGE_LITERAL_SINGULAR:
                try:
                    res = _grads(s, alpha, delta, EDGE_MAXITER)
                except BpltvError as e:
                    assert e.code != 0 and str(e)
                    continue
            else:
                res = _grads(s, alpha, delta, EDGE_MAXITER)
            g0 = _check_against_oracle(oracle, res, f, ub, alpha, reg, EDGE_MAXITER)
            if not reg:   # the product path at its default sweep count
                g = np.reshape(s.sumregs_evaluate(alpha, delta, maxiter=EDGE_MAXITER)[2], np.shape(g0))
                assert np.abs(g - g0).max() <= THIN_TOL.get(shape, 1e-6) * max(np.abs(g0).max(), 1e-300), kind
        s.close()


BATCH_ALPHAS = {"vector": lambda N, M: A3, "patch22": lambda N, M: P22,
                "patch12": lambda N, M: np.array([[[0.03, 0.05]], [[0.02, 0.04]], [[0.05, 0.02]]]),
                "patch35": lambda N, M: _map(5, 3, seed=12), "map": lambda N, M: _map(N, M, seed=13)}


@pytest.mark.parametrize("kind", list(BATCH_ALPHAS))
def test_gradients_on_a_batch_every_factorisation(gpu_solver_cls, oracle, kind):
    """4 x 64 x 80 (and 40 x 33 for the non-dividing 3 x 5 patch): all factorisations, both branches; per-image rows
    add up to the gradient and match the oracle's (scalar and patch parameters; a map has no per-image rows)."""
    from bpldenoising_amd._lib import BpltvError
    O, N, M = (3, 40, 33) if kind == "patch35" else (4, 64, 80)
    ub, f = synth_batch(O, N, M, seed=91)
    alpha = BATCH_ALPHAS[kind](N, M)
    s = _solver(gpu_solver_cls, ub, f)
    for delta in (0.1, 1e-4):
        reg = delta <= 1e-3
        res = _grads(s, alpha, delta, 600)
        g0 = _check_against_oracle(oracle, res, f, ub, alpha, reg, 600)
        u, c, g = s.sumregs_evaluate(alpha, delta, maxiter=600)
        if kind == "map":
            with pytest.raises(BpltvError) as e:
                s.per_image()
            assert e.value.code == 6          # BPLTV_E_UNSUPPORTED
            continue
        rows = s.per_image()
        assert rows.shape == (O, 1 + np.size(g)) and np.allclose(rows.sum(0)[1:], np.ravel(g), rtol=1e-12, atol=0)
        assert np.allclose(rows[:, 0], oracle.cost(u, ub, per_image=True)[1], rtol=1e-13)
        _, pi = oracle.sumregs_gradient(alpha, u, ub, reg=reg, per_image=True)
        assert np.abs(rows[:, 1:] - pi).max() <= (1e-7 if reg else 1e-6) * np.abs(g0).max()
    s.close()


@pytest.mark.parametrize("case", ["vector-chol", "map-chol", "vector-lu", "map-lu"])
def test_nested_dissection_options_on_the_13_point_system(gpu_solver_cls, oracle, case):
    """nd_wave 0, nd_skinny 0, nd_skinny2_min 0 (the skinny2 kernel at any batch size), nd_staged 0 and nd_leaf 1 / 8 /
    100 on the 13-point system, in Cholesky and in LU (vector: sr_force_lu; map: gradient_reg, the row-scaled system):
    each matches the oracle and the default to 1e-9 of max|g|; the substitution kernels (nd_staged) give the same bits."""
    kind, fac = case.split("-")
    ub, f = synth_batch(3, 64, 56, seed=93)
    O, N, M = f.shape
    alpha = A3 if kind == "vector" else _map(N, M, seed=14)
    delta = 1e-4 if case == "map-lu" else 0.1
    reg = delta <= 1e-3
    s = _solver(gpu_solver_cls, ub, f)
    s.set_option("sr_force_lu", int(case == "vector-lu"))
    name = "nd-lu" if fac == "lu" else "nd"
    u0 = oracle.sumregs_pdhg(f, alpha, maxiter=500, nthreads=4)
    g0 = np.asarray(oracle.sumregs_gradient(alpha, u0, ub, reg=reg))
    scale = np.abs(g0).max()
    tol = 1e-7 if reg else 1e-6

    def grad():
        g = np.asarray(s.sumregs_evaluate(alpha, delta, maxiter=500)[2])
        assert s.stats()["adjoint_method"] == name
        assert np.abs(g - g0).max() <= tol * scale
        return g
    gd = grad()
    for opt, val, back in [("nd_wave", 0, 1), ("nd_skinny", 0, 1), ("nd_skinny2_min", 0, 256), ("nd_staged", 0, 1),
                           ("nd_leaf", 1, 0), ("nd_leaf", 8, 0), ("nd_leaf", 100, 0)]:
        s.set_option(opt, val)
        g = grad()
        assert np.abs(g - gd).max() <= 1e-9 * scale, (opt, val, np.abs(g - gd).max() / scale)
        if opt == "nd_staged":
            assert np.array_equal(g, gd)
        s.set_option(opt, back)
    s.close()


@pytest.mark.parametrize("O", [3, 7])
def test_image_groups_of_one_and_two_are_bitwise_the_whole_batch(gpu_solver_cls, O):
    """adjoint_budget_mb forces groups of exactly 1 and 2 images on odd batches, for the map and the vector parameter
    (Cholesky: budget grp + 1/2 workspaces) and the patch parameter in gradient_reg (LU: its workspace holds the factor
    and the front workspace twice, budget 2 grp + 1/2 Cholesky workspaces): cost and gradient are bitwise those of the
    whole batch."""
    import os, re, subprocess
    from conftest import ROOT
    N, M = 40, 36
    ub, f = synth_batch(O, N, M, seed=95)
    out = subprocess.run([os.path.join(ROOT, "tools", "_bin", "nd_host_check"), "bytes", str(M), str(N)], capture_output=True,
                         text=True, timeout=120).stdout
    per_image = float(re.search(r"bytes_per_image sr (\d+)", out).group(1))
    amap = _map(N, M, seed=15)
    for alpha, delta, lu in ((amap, 0.1, False), (A3, 0.1, False), (P22, 1e-4, True)):
        res = {}
        for grp in (None, 1, 2):
            s = _solver(gpu_solver_cls, ub, f)
            if grp is not None:
                s.set_option("adjoint_budget_mb", ((2 * grp if lu else grp) + 0.5) * per_image / 1e6)
            _, c, g = s.sumregs_evaluate(alpha, delta, maxiter=200, fetch_u=False)
            st = s.stats()
            assert st["adjoint_method"] == ("nd-lu" if lu else "nd")
            res[grp] = (c, np.asarray(g), st["adjoint_chunks"])
            s.close()
        assert res[None][2] == 1
        for grp in (1, 2):
            c, g, ch = res[grp]
            assert ch == -(-O // grp), (np.shape(alpha), grp, ch)
            assert c == res[None][0] and np.array_equal(g, res[None][1]), (np.shape(alpha), grp)


@pytest.mark.parametrize("devices", [[0, 0], [0, 0, 0]], ids=["2shards", "3shards"])
def test_shards_patch_and_map_parameters(gpu_solver_cls, devices):
    """deterministic = 1 over 2 and 3 shards of one device: the patch parameter bitwise a single handle's, the map
    parameter (whose totals are plain sums over the shards, multi_evaluate) to rounding."""
    O, N, M = 5, 40, 36
    ub, f = synth_batch(O, N, M, seed=97)
    amap = _map(N, M, seed=16)
    s1 = _solver(gpu_solver_cls, ub, f)
    ref = [s1.sumregs_evaluate(a, d, maxiter=300) for a, d in ((P22, 0.1), (P22, 1e-4), (amap, 0.1), (amap, 1e-4))]
    s1.close()
    s = _solver(gpu_solver_cls, ub, f, devices=devices)
    for (a, d), (u0, c0, g0) in zip(((P22, 0.1), (P22, 1e-4), (amap, 0.1), (amap, 1e-4)), ref):
        u, c, g = s.sumregs_evaluate(a, d, maxiter=300, deterministic=1)
        assert np.array_equal(u, u0), (np.shape(a), d)
        if np.shape(a) == P22.shape:    # per-image rows added in image order: bitwise
            assert c == c0 and np.array_equal(g, g0), d
        else:                           # a map has no per-image rows; its shard totals go through the collective
            assert np.isclose(c, c0, rtol=1e-14) and np.allclose(g, g0, rtol=1e-12, atol=1e-15 * np.abs(g0).max()), d
    s.close()


# ---------------------------------------------------------------------------------------------------------------------
# Rejected calls leave the handle as it was
# ---------------------------------------------------------------------------------------------------------------------
def _bad_calls(M, N, dtype=64):
    """(name, call) of every condition that used to be checked after the parameter upload (or, in a TV sweep, after
    the sweep's blocks replaced the handle's parameter)."""
    a0 = _map(N, M, seed=17)
    a0[1, 3, 4] = 0.0                                  # one zero entry: fine without rho, rejected with rho
    p0 = P22.copy()
    p0[2, 1, 0] = 0.0
    t0 = 0.03 + 0.05 * np.random.default_rng(18).random((N, M))
    t0[5, 6] = 0.0
    tp0 = np.array([[0.05, 0.0, 0.04], [0.03, 0.06, 0.02]])
    big = 0.05 * np.ones((3, N, M))                    # a map: would reallocate the parameter buffer
    sw0 = 0.03 + 0.05 * np.random.default_rng(21).random((4, N, M))   # four map blocks of a TV sweep
    sw0[2, 7, 3] = 0.0
    calls = [
        ("tv_rho_zero", lambda s: s.denoise(t0, maxiter=20, rho=0.1)),
        ("tv_eval_rho_zero", lambda s: s.evaluate(t0, 0.1, maxiter=20, rho=0.1)),
        ("tv_variant", lambda s: s.denoise(t0, maxiter=20, variant=99)),
        ("sr_rho_zero", lambda s: s.sumregs_denoise(a0, maxiter=20, rho=0.1)),
        ("sr_eval_rho_zero", lambda s: s.sumregs_evaluate(a0, 0.1, maxiter=20, rho=0.1)),
        ("sr_init", lambda s: s.sumregs_denoise(big, maxiter=20, init=1)),
        ("sr_order", lambda s: s.sumregs_evaluate(big, 0.1, maxiter=20, order=1)),
        ("sr_variant", lambda s: s.sumregs_denoise(big, maxiter=20, variant=3)),
        ("sr_reg_patch_zero", lambda s: s.sumregs_evaluate(p0, 1e-4, maxiter=20)),
        ("sr_reg_map_zero", lambda s: s.sumregs_evaluate(a0, 1e-4, maxiter=20)),
        ("sr_eval_bcr", lambda s: s.sumregs_evaluate(big, 0.1, maxiter=20, adjoint_method="bcr")),
        ("tv_eval_reg_map_zero", lambda s: s.evaluate(t0, 0.0, maxiter=20)),
        ("tv_eval_reg_patch_zero", lambda s: s.evaluate(tp0, 0.0, maxiter=20)),
        ("tv_sweep_rho_zero", lambda s: s.sweep(sw0, maxiter=20, rho=0.1)),
        ("tv_sweep_variant", lambda s: s.sweep(big, maxiter=20, variant=99)),
    ]
    if dtype == 32:   # init / order: Float64 handles only
        calls.append(("tv_sweep_init", lambda s: s.sweep(sw0 + 0.01, maxiter=20, init=1)))
    return calls


@pytest.mark.parametrize("dtype", [64, 32])
@pytest.mark.parametrize("first", ["tv_scalar", "tv_map", "sr_vector", "sr_patch"])
def test_rejected_calls_leave_the_handle_as_it_was(gpu_solver_cls, dtype, first):
    """Every check that used to run after the parameter upload (rho > 0 with a zero entry; the TV kernel plan; init /
    order, the kernel variant and block cyclic reduction on the sum-of-regularisers model; gradient_reg with an array
    parameter that has a zero entry, in both models' evaluate; a TV sweep's rho, variant and float-handle init checks)
    now runs before it: after the BpltvError, duality_gap() and stats()["iterations"] are those of the last solve, bit for bit, and the
    next accepted solve is bitwise a fresh handle's.  f32 handles solve the TV model only in single precision; the
    sum-of-regularisers model is Float64 on either handle."""
    from bpldenoising_amd._lib import BpltvError
    O, N, M = 2, 40, 36
    ub, f = synth_batch(O, N, M, seed=99)
    tmap = 0.03 + 0.1 * np.random.default_rng(19).random((N, M))
    solve = {"tv_scalar": lambda s: s.denoise(0.1, maxiter=60, fetch=False),
             "tv_map": lambda s: s.denoise(tmap, maxiter=60, fetch=False),
             "sr_vector": lambda s: s.sumregs_denoise(A3, maxiter=60, fetch=False),
             "sr_patch": lambda s: s.sumregs_denoise(P22, maxiter=60, fetch=False)}[first]
    s = _solver(gpu_solver_cls, ub, f, dtype=dtype)
    fresh = _solver(gpu_solver_cls, ub, f, dtype=dtype)
    solve(s)
    g0 = s.duality_gap()
    assert np.all(np.isfinite(g0)) and np.all(g0 > 0)
    for name, call in _bad_calls(M, N, dtype):
        with pytest.raises(BpltvError):
            call(s)
        assert np.array_equal(s.duality_gap(), g0), name
        assert s.stats()["iterations"] == 60, name
    # the next accepted solves: bitwise a fresh handle's, in both models
    nxt = [lambda h: h.sumregs_denoise(_map(N, M, seed=20), maxiter=45),
           lambda h: h.denoise(tmap, maxiter=45),
           lambda h: h.sumregs_evaluate(P22, 0.1, maxiter=45)[2]]
    for k, call in enumerate(nxt):
        assert np.array_equal(np.asarray(call(s)), np.asarray(call(fresh))), k
    s.close()
    fresh.close()


def test_rejected_calls_leave_a_sharded_handle_as_it_was(gpu_solver_cls):
    from bpldenoising_amd._lib import BpltvError
    O, N, M = 3, 40, 36
    ub, f = synth_batch(O, N, M, seed=98)
    s = _solver(gpu_solver_cls, ub, f, devices=[0, 0])
    s.sumregs_denoise(P22, maxiter=60, fetch=False)
    g0 = s.duality_gap()
    for name, call in _bad_calls(M, N):
        with pytest.raises(BpltvError):
            call(s)
        assert np.array_equal(s.duality_gap(), g0), name
        assert s.stats()["iterations"] == 60, name
    one = _solver(gpu_solver_cls, ub, f)
    assert np.array_equal(s.sumregs_evaluate(P22, 0.1, maxiter=45, deterministic=1)[2], one.sumregs_evaluate(P22, 0.1, maxiter=45)[2])
    s.close()
    one.close()
