"""GPU checks of the TV model's batched parameter sweep (bpltv_sweep): the reference's generate_cost / generate_2d_cost
as one batch of K*O problems, problem k*O + i solving image i with parameter block k.  Every problem is bit-exact to the
C oracle (oracle.pdhg / pdhg_opts / pdhg_f32), whatever the kernel variant, the launch chains or the grid decode, for
scalar, non-square patch and pixel-map blocks; the sweep never touches the dataset context (the last solve's result,
its parameter and its duality gap)."""
import math

import numpy as np
import pytest
from conftest import synth_batch

pytestmark = pytest.mark.gpu

IT = 53                                   # no multiple of any fusion depth the plans pick (6, 8, ...)
FORMS = ["scalar", "patch23", "patch31", "map"]


def _blocks(form, K, N, M, seed=0):
    """K parameter blocks, every entry in [0.02, 0.17]: (K,) scalars, (K, 2, 3) / (K, 3, 1) patches (am != an, so a
    swapped am / an reads the wrong entries) or (K, N, M) pixel maps."""
    rng = np.random.default_rng(seed)
    shape = {"scalar": (K,), "patch23": (K, 2, 3), "patch31": (K, 3, 1), "map": (K, N, M)}[form]
    return 0.02 + 0.15 * rng.random(shape)


def _ref(oracle, f, a, maxiter, dtype=64, **kw):
    """The oracle's solve of every image of f with parameter a."""
    if dtype == 32:
        return oracle.pdhg_f32(f, a, maxiter=maxiter, **kw)
    if any(k in kw for k in ("init", "order", "L")):
        return oracle.pdhg_opts(f, a, maxiter=maxiter, **kw)
    return oracle.pdhg(f, a, maxiter=maxiter, nthreads=4, **kw)


def _check(oracle, f, ub, blocks, costs, us, maxiter, dtype=64, ks=None, **kw):
    """us[k] bitwise the oracle's solve with blocks[k]; costs[k] its loss to 1e-13."""
    for k in (range(len(blocks)) if ks is None else ks):
        u0 = _ref(oracle, f, blocks[k], maxiter, dtype, **kw)
        assert np.array_equal(us[k], u0.reshape(us[k].shape)), (k, kw)
        c0 = oracle.cost(u0, ub)
        assert abs(costs[k] - c0) <= 1e-13 * abs(c0), (k, costs[k], c0, kw)


def _solver(cls, ub, f, **kw):
    O, N, M = f.shape
    s = cls(M, N, O, **kw)
    s.set_data(ub, f)
    return s


def _tile_count(L, R, T):
    """tiling.hpp tile_count: regions of R pixels with a halo of T along a side of L pixels."""
    if L <= R:
        return 1
    a, c1 = 0, 0
    while True:
        cs = 0 if a == 0 else (R - T) + (a - 1) * (R - 2 * T)
        o = 0 if a == 0 else cs - T
        c1 = L if o + R >= L else o + R - T
        if c1 >= L:
            return a + 1
        a += 1


def _auto_variant(O, N, M, K, ncu):
    """The kernel the automatic plan picks for these cases (tiling.hpp plan_pdhg): the 32 x 32 or 48 x 48 tile kernel
    (launch-cost model) up to 256 px; above that the 48 x 48 tile kernel on images narrower than 64 px, else the 64 x 48
    rows kernel (20) while the 64 x 64 (19) and 64 x 48 regions of all K*O problems fit two workgroups per CU."""
    if M <= 256 and N <= 256:
        return (1, 13)
    if M < 64 or N < 64:
        return (13,)
    rows64 = _tile_count(M, 64, 8) * _tile_count(N, 64, 8) * K * O
    rows48 = _tile_count(M, 64, 8) * _tile_count(N, 48, 8) * K * O
    return (20,) if rows64 <= 2 * ncu and rows48 <= 2 * ncu else (19,)


# (shape O x N x M, forced variant (0 = automatic), K values): K != O everywhere, so a block index taken from the wrong
# axis fails.  2 x 40 x 33 / 3 x 40 x 33: a tile kernel; 1 x 300 x 40: the 48 x 48 tile kernel (wider than 256 px,
# narrower than a 64 px rows region); 1 x 290 x 270: the rows kernel, 64 x 48 at K = 3, 64 x 64 at K = 12 on 256 CUs.
PLANS = [((2, 40, 33), 0, (1, 3, 5)), ((3, 40, 33), 0, (1, 5)), ((2, 40, 33), 1, (3,)), ((2, 40, 33), 13, (5,)),
         ((1, 300, 40), 0, (3, 5)), ((1, 300, 40), 1, (3,)),
         ((1, 290, 270), 0, (3, 12)), ((1, 290, 270), 19, (3,)), ((1, 290, 270), 20, (5,)), ((1, 290, 270), 13, (3,)),
         ((1, 290, 270), 1, (3,))]


@pytest.mark.parametrize("dtype", [64, 32])
@pytest.mark.parametrize("shape,var,Ks", PLANS, ids=["x".join(map(str, c[0])) + "-v%d" % c[1] for c in PLANS])
def test_every_plan_and_parameter_form(gpu_solver_cls, oracle, shape, var, Ks, dtype):
    O, N, M = shape
    ub, f = synth_batch(O, N, M, seed=N + 3 * M + O)
    s = _solver(gpu_solver_cls, ub, f, dtype=dtype)
    for K in Ks:
        for form in FORMS:
            blocks = _blocks(form, K, N, M, seed=K + 7 * len(form))
            costs, us = s.sweep(blocks, fetch_u=True, maxiter=IT, variant=var)
            st = s.stats()
            assert us.shape == (K, O, N, M) and st["iterations"] == IT
            assert st["pdhg_variant"] in ((var,) if var else _auto_variant(O, N, M, K, st["ncu"])), (K, form, st["pdhg_variant"])
            _check(oracle, f, ub, blocks, costs, us, IT, dtype)
            assert np.array_equal(s.sweep(blocks, maxiter=IT, variant=var), costs), (K, form)   # fetch_u changes nothing
    s.close()


RUNTIME = [dict(init=1), dict(order=1), dict(init=1, order=1), dict(opnorm=2 * np.sqrt(2) * (1 - 1 / 64)),
           dict(init=1, order=1, opnorm=2.5)]


@pytest.mark.parametrize("shape", [(2, 40, 33), (2, 290, 270)], ids=["tile", "rows"])
def test_run_time_choices_in_a_sweep(gpu_solver_cls, oracle, shape):
    """init / order / opnorm (pdhg_init_kernel reads block img / O of the sweep's parameters), Huber (rho > 0) and
    maxiter = 0, with patch and map blocks, on a tile kernel and on the rows kernel."""
    O, N, M = shape
    ub, f = synth_batch(O, N, M, seed=M + 5)
    s = _solver(gpu_solver_cls, ub, f)
    K, it = 3, 37
    rows = M > 256
    for form in ("patch23", "map"):
        blocks = _blocks(form, K, N, M, seed=len(form))
        for kw in RUNTIME:
            costs, us = s.sweep(blocks, fetch_u=True, maxiter=it, **kw)
            st = s.stats()
            assert st["iterations"] == it and (st["pdhg_variant"] in (19, 20)) == rows, (kw, st["pdhg_variant"])
            okw = {"L" if k == "opnorm" else k: v for k, v in kw.items()}
            _check(oracle, f, ub, blocks, costs, us, it, **okw)
        for rho in (0.3, 0.01):
            costs, us = s.sweep(blocks, fetch_u=True, maxiter=it, rho=rho)
            _check(oracle, f, ub, blocks, costs, us, it, rho=rho)
        for init in (0, 1):
            costs, us = s.sweep(blocks, fetch_u=True, maxiter=0, init=init)
            x0 = np.zeros_like(f) if init else f                       # u = x0
            # the loss alone, against a correctly rounded sum (the oracle's running sum of 0.5 ||ub||^2 over 2 x 290 x
            # 270 pixels is itself 1.3e-13 off)
            c0 = 0.5 * math.fsum(((x0 - ub) ** 2).ravel().tolist())
            assert s.stats()["iterations"] == 0
            assert all(np.array_equal(us[k], x0) for k in range(K)), init
            assert np.allclose(costs, c0, rtol=1e-13, atol=0), init
    assert not np.array_equal(_ref(oracle, f, blocks[0], it), _ref(oracle, f, blocks[0], it, rho=0.3))   # rho matters
    s.close()


def test_launch_chains_split_a_parameter_block(gpu_solver_cls, oracle):
    """3 x 128^2 with K = 5: 15 problems; two launch chains split them at problem 7, inside parameter block 2 (problems
    6..8), and chain 1 starts half a launch out of phase at 96 iterations.  Bitwise one chain, the 1-D grid decode
    (xcd) and the oracle, on both tile kernels."""
    O, N, M, K, it = 3, 128, 128, 5, 96
    ub, f = synth_batch(O, N, M, seed=128)
    s = _solver(gpu_solver_cls, ub, f)
    for form in ("patch31", "map"):
        blocks = _blocks(form, K, N, M, seed=9)
        for var in (1, 13):
            costs, us = s.sweep(blocks, fetch_u=True, maxiter=it, variant=var, chains=2)
            st = s.stats()
            assert st["launch_chains"] == 2 and st["graph_used"] == 1 and st["pdhg_variant"] == var
            T = st["tile_iters"]
            nl = -(-it // T)
            assert ((1 + -(-(it - T // 2) // T)) - nl) % 2 == 1 and nl >= 8, T    # tiling.hpp chain_out_of_phase
            assert st["launches"] == 2 * nl + 1, st          # the staggered chain has one launch more
            for kw in (dict(chains=1), dict(xcd=True, chains=1), dict(xcd=True, chains=2)):
                c, u = s.sweep(blocks, fetch_u=True, maxiter=it, variant=var, **kw)
                st = s.stats()
                assert st["pdhg_variant"] == var and st["launch_chains"] == kw["chains"], (kw, st)
                assert np.array_equal(u, us) and np.array_equal(c, costs), (form, var, kw)
            _check(oracle, f, ub, blocks, costs, us, it)
    s.close()


def test_more_than_65535_problems(gpu_solver_cls, oracle):
    """K = 70000 scalars on one 16 x 16 image: past a grid dimension, so one launch chain of all problems takes the
    PDHG kernels' 1-D grid decode (two chains of 35000 do not), and the loss runs over 70000 problems.  Bitwise the same
    parameters as two sweeps of 35000; every 997th block the oracle's."""
    N, M, K, it = 16, 16, 70000, 30
    ub, f = synth_batch(1, N, M, seed=70)
    alphas = np.linspace(0.005, 0.35, K)
    s = _solver(gpu_solver_cls, ub, f)
    costs, us = s.sweep(alphas, fetch_u=True, maxiter=it, chains=1)
    st = s.stats()
    assert st["iterations"] == it and st["launch_chains"] == 1 and us.shape == (K, 1, N, M)
    assert np.array_equal(s.sweep(alphas, maxiter=it), costs)      # the automatic plan: two chains
    assert s.stats()["launch_chains"] == 2
    h = K // 2
    c1, u1 = s.sweep(alphas[:h], fetch_u=True, maxiter=it)
    assert np.array_equal(c1, costs[:h]) and np.array_equal(u1, us[:h])
    del u1
    c2, u2 = s.sweep(alphas[h:], fetch_u=True, maxiter=it)
    assert np.array_equal(c2, costs[h:]) and np.array_equal(u2, us[h:])
    del u2
    _check(oracle, f, ub, alphas, costs, us, it, ks=list(range(0, K, 997)) + [K - 1])
    s.close()


@pytest.mark.parametrize("dtype", [64, 32])
def test_sweep_and_dataset_contexts_do_not_mix(gpu_solver_cls, oracle, dtype):
    """denoise(map) -> sweep: the last solve is still the denoise (duality gap, u in HBM, iteration count); a K = 1 map
    sweep (as many problems as the dataset, the same parameter shape and plan) replays no graph of the dataset's and the
    dataset's none of its.  sumregs_denoise -> TV sweep: the duality gap is still the sum-of-regularisers one.  The
    next denoise / evaluate are bitwise a fresh handle's."""
    import torch
    O, N, M = 2, 48, 40
    ub, f = synth_batch(O, N, M, seed=23)
    it = 60
    tmap = 0.03 + 0.1 * np.random.default_rng(24).random((N, M))
    s = _solver(gpu_solver_cls, ub, f, dtype=dtype)
    fresh = _solver(gpu_solver_cls, ub, f, dtype=dtype)
    u0 = s.denoise(tmap, maxiter=it)
    assert np.array_equal(u0, _ref(oracle, f, tmap, it, dtype))
    gap0 = s.duality_gap()
    dev = torch.empty(O * N * M, dtype=torch.float64, device="cuda")
    for form, K in (("patch23", 3), ("map", 1), ("map", 3)):
        blocks = _blocks(form, K, N, M, seed=K)
        costs, us = s.sweep(blocks, fetch_u=True, maxiter=it)
        _check(oracle, f, ub, blocks, costs, us, it, dtype)
        assert np.array_equal(s.duality_gap(), gap0), form
        torch.cuda.synchronize()
        s.copy_u_device(dev.data_ptr())
        assert np.array_equal(dev.cpu().numpy().reshape(O, N, M), u0), form
        assert s.stats()["iterations"] == it
        assert np.array_equal(s.denoise(tmap, maxiter=it), u0), form
    s.sumregs_denoise(np.array([0.03, 0.02, 0.05]), maxiter=it, fetch=False)
    gsr = s.duality_gap()
    s.sweep(_blocks("map", 2, N, M, seed=2), maxiter=it)
    assert np.array_equal(s.duality_gap(), gsr)
    nxt = [lambda h: h.denoise(0.7 * tmap, maxiter=45),
           lambda h: h.evaluate(np.array([[0.05, 0.08]]), 0.1, maxiter=45)[2],
           lambda h: h.denoise(0.09, maxiter=45)]
    for k, call in enumerate(nxt):
        assert np.array_equal(np.asarray(call(s)), np.asarray(call(fresh))), k
    s.close()
    fresh.close()
