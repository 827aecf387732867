"""GPU checks of the sum-of-regularisers adjoint solvers on images with a real active set.

Every other adjoint test of this model takes u from a long solve of synth_batch, on which no element of any of the three
operators has |G_k u| < 1e-12 apart from the forced border rows: the kap branch of sr_adj_setup_*_kernel, h_k = 0 in
sr_adj_gradpix_kernel and sr_tangent_rhs_kernel, the seven-diagonal assembly with 1e14 beside entries of order one and the
four factorisations of that matrix (nested dissection Cholesky and LU, the band in HBM, the banded LU) were never compared
with an independent solve on an image large enough to have a tree, a band and image groups.  Here u is the numpy twin's
iterate with a layout planted (tests/sumregs_active_ref.py: blocks, a period-2 window on which the centred operator alone
is active, crossing strips, a constant image) and the reference is the literal unreduced 7n^2 system with kappa =
stats["kappa_used"], solved once per (case, kappa) with ten extended-precision sweeps and pinned on the CPU by
tests/test_sumregs_active_ref.py.  The bound everywhere without regularisation is |a - b| <= 1e-8 max|p| + 1e-6 |b|,
elementwise, for grad_f, grad_x and du (p = du there)."""
import functools

import numpy as np
import pytest

import sumregs_active_ref as sa
from test_gpu_sumregs_each import _sr_bytes_per_image

pytestmark = pytest.mark.gpu

KINDS = ["vector", "patch22", "map"]
# name (what stats["adjoint_method"] reports), adjoint_method, option sr_force_lu, the sweep count at which further sweeps
# change nothing (forced LU on the symmetric system gains about a digit per sweep: tests/test_gpu_sumregs_vjp._methods)
METHODS = [("nd", "nd", 0, 6), ("nd-lu", "nd", 1, 10), ("band-hbm", "band", 0, 6), ("band-lu", "band", 1, 10)]
METHOD_IDS = [m[0] for m in METHODS]
# the default factorisation and one LU path, for the entry points that share run_sr_gradient with sumregs_vjp
TWO = [METHODS[0], METHODS[1]]
TWO_IDS = [m[0] for m in TWO]


def _same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b))


def _dist(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max())


def _close(a, b, scale):
    """|a - b| <= 1e-8 scale + 1e-6 |b| elementwise."""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and bool(np.all(np.abs(a - b) <= 1e-8 * scale + 1e-6 * np.abs(b)))


def _du_close(a, b):
    return _close(a, b, float(np.abs(b).max()))


def _handle(cls, shape, method):
    O, N, M = shape
    s = cls(M, N, O)
    s.set_option("sr_force_lu", method[2])
    return s


def _check_stats(st, method, reg=0, chunks=1):
    assert st["adjoint_method"] == method[0] and st["reg_gradient_used"] == reg, st
    assert st["adjoint_attempts"] == 1 and st["adjoint_residual"] <= 1e-6 and st["adjoint_chunks"] == chunks, st


def _each_xs(x, O):
    """One block per image: the case's own, scaled by 1, 0.7, 1.3."""
    sc = np.array([1.0, 0.7, 1.3])[:O]
    return sc.reshape((O,) + (1,) * np.ndim(x)) * np.asarray(x)[None]


@functools.lru_cache(maxsize=None)
def _bytes_per_image(M, N):
    return _sr_bytes_per_image(M, N)


# ---- sumregs_vjp, reg = 0 ---------------------------------------------------------------------------------------------------
VJP_CASES = [(shape, kind, layout) for shape, layout in sa.CASES for kind in KINDS]
VJP_IDS = [sa.case_id(sh, lay, k) for sh, k, lay in VJP_CASES]
OFF_CASES = [(shape, "vector-off", layout) for shape, layout in sa.CASES if layout in ("blocks", "stripes")]
OFF_IDS = [sa.case_id(sh, lay, k) for sh, k, lay in OFF_CASES]


def vjp_distances(cls, shape, kind, layout, method, refine):
    """One sumregs_vjp call on a planted case against the literal system at kappa_used: (stats, grad_f within the bound,
    grad_x within the bound).  Prints the distances before anything is asserted."""
    x, f, u, gu, df, dx = sa.case(shape, kind, layout)
    s = _handle(cls, shape, method)
    kw = {} if refine is None else {"refine": refine}
    gf, gx = s.sumregs_vjp(u, x, gu, adjoint_method=method[1], **kw)
    st = s.stats()
    s.close()
    rf, rx, pmax = sa.vjp_ref(shape, kind, layout, st["kappa_used"])
    print("%s %s refine %s: method %s attempts %d kappa_used %.3e residual %.3e max|d| grad_f %.3e grad_x %.3e (max|p| %.3e, "
          "max|g| %.3e, bound %.1e)" % (sa.case_id(shape, layout, kind), method[0], refine, st["adjoint_method"],
                                        st["adjoint_attempts"], st["kappa_used"], st["adjoint_residual"], _dist(gf, rf),
                                        _dist(gx, rx), pmax, np.abs(rx).max(), 1e-8 * pmax))
    assert np.shape(gx) == np.shape(x) and gf.shape == u.shape
    return st, _close(gf, rf, pmax), _close(gx, rx, pmax)


@pytest.mark.parametrize("method", METHODS, ids=METHOD_IDS)
@pytest.mark.parametrize("shape,kind,layout", VJP_CASES, ids=VJP_IDS)
def test_vjp_at_converged_refinement_matches_the_literal_system(gpu_solver_cls, shape, kind, layout, method):
    """refine = 6 on the Cholesky paths, 10 where the LU is forced on the symmetric system: what the kernels and the
    factorisations compute on active elements, apart from the sweep count.

    Measured on the MI355X, largest |difference| of grad_f / grad_x over the cases (max|p| 1.2 ... 2.5, max|g| up to 76,
    kappa_used 1e14, adjoint_attempts 1 and adjoint_residual <= 6e-15 everywhere):
        nested dissection        vector 3.8e-11 / 2.6e-10    patch, map 5.6e-11 / 2.4e-10    at most 0.0029 of the bound
        band in HBM              vector 8.5e-11 / 5.7e-10    patch, map 8.4e-11 / 4.2e-10    at most 0.0025
        nd-lu, band-lu (forced)  vector 1.8e-12 / 9.6e-12    patch, map 7.4e-13 / 3.7e-12    at most 0.0001
    Until the gate of run_sr_gradient left out the rows that carry the weight, both "flat" batches were refused at
    kappa = 1e14 and again at 1e12 on every factorisation, whatever the sweep count, and solved with 1e10 (adjoint_attempts 3,
    residual 9.6e-8): DESIGN.md section 4.4, "Held to the literal system on active sets"."""
    st, okf, okx = vjp_distances(gpu_solver_cls, shape, kind, layout, method, method[3])
    _check_stats(st, method)
    assert okf, "grad_f"
    assert okx, "grad_x"


@pytest.mark.parametrize("method", METHODS, ids=METHOD_IDS)
@pytest.mark.parametrize("shape,kind,layout", VJP_CASES, ids=VJP_IDS)
def test_vjp_at_the_default_refinement_matches_the_literal_system(gpu_solver_cls, shape, kind, layout, method):
    """The same calls with the sweep count left to the library (AdjPlan::nref of run_sr_gradient: five).

    Measured on the MI355X, grad_f / grad_x and the worst fraction of the elementwise bound: nested dissection 1.4e-9 / 7.0e-9,
    0.059 (3 x 33 x 17 "flat", vector); band in HBM 1.9e-9 / 1.6e-8, 0.038; nd-lu 1.7e-10 / 5.2e-10, 0.0015; band-lu 2.3e-10 /
    9.4e-10, 0.0023.  With the two sweeps the library ran until this test existed: 2.0e-5 / 1.8e-4, 5.0e2 times the bound
    (nested dissection), 2.3e-5 / 3.4e-4, 4.0e2 (band in HBM), 79 (nd-lu), 1.1e2 (band-lu); 87 of these 120 cases failed.  Three
    sweeps leave 24 / 15 / 2.1 / 2.7 times the bound, four 1.2 / 0.60 / 0.055 / 0.078, six 0.0029 / 0.0025 / 6e-5 / 7e-5."""
    st, okf, okx = vjp_distances(gpu_solver_cls, shape, kind, layout, method, None)
    _check_stats(st, method)
    assert okf, "grad_f"
    assert okx, "grad_x"


@pytest.mark.parametrize("refine", ["converged", "default"])
@pytest.mark.parametrize("method", METHODS, ids=METHOD_IDS)
@pytest.mark.parametrize("shape,kind,layout", OFF_CASES, ids=OFF_IDS)
def test_vjp_with_one_regulariser_switched_off(gpu_solver_cls, shape, kind, layout, method, refine):
    """x_2 = 0: the backward operator enters the matrix through its active elements alone (c = 0 elsewhere), and all three
    gradient components, the backward one included, stay within the bound.  Measured: at most 8.5e-11 / 2.3e-10 at converged
    refinement, 1.9e-9 / 5.4e-9 at the default (0.011 of the bound)."""
    st, okf, okx = vjp_distances(gpu_solver_cls, shape, kind, layout, method, method[3] if refine == "converged" else None)
    _check_stats(st, method)
    assert okf, "grad_f"
    assert okx, "grad_x"


@pytest.mark.parametrize("method", METHODS, ids=METHOD_IDS)
def test_a_constant_image_has_no_map_gradient(gpu_solver_cls, method):
    """h_k = 0 on every element of all three operators: a one-image handle on image 0 of "flat" returns exactly zero in the
    three slices of a map's gradient, and the literal system's grad_f at the first weight it tries (measured: 6.2e-12 with
    nested dissection, 1.1e-11 with the band in HBM, below 1e-17 on the LU paths, at max|p| 2.4e-3: p is all but constant)."""
    shape, kind, layout = (3, 40, 48), "map", "flat"
    O, N, M = shape
    x, f, u, gu, df, dx = sa.case(shape, kind, layout)
    assert (sa.active_counts(u[:1]) == N * M).all()
    s = _handle(gpu_solver_cls, (1, N, M), method)
    gf, gx = s.sumregs_vjp(u[:1], x, gu[:1], adjoint_method=method[1])
    st = s.stats()
    s.close()
    rf, _, _ = sa.vjp_ref(shape, kind, layout, st["kappa_used"])
    pmax = float(np.abs(rf[0]).max())
    print("constant image, %s: attempts %d kappa_used %.3e residual %.3e max|d grad_f| %.3e (max|p| %.3e)"
          % (method[0], st["adjoint_attempts"], st["kappa_used"], st["adjoint_residual"], _dist(gf[0], rf[0]), pmax))
    _check_stats(st, method)
    assert st["adjoint_residual"] == 0.0          # every row carries the weight: none is left for the scaled pair
    assert gx.shape == (3, N, M) and not np.any(gx)
    assert _close(gf[0], rf[0], pmax)


@pytest.mark.parametrize("method", METHODS, ids=METHOD_IDS)
def test_rows_without_the_weight_still_count_in_the_residual_gate(gpu_solver_cls, method):
    """Image 0 of "stripes" alone: 532 centred elements are active and put kappa / 4 or more on the diagonals of the rows they
    touch, which the gate leaves out; the other rows of the image have diagonals of order one and still make up the
    statistic, which is not zero (measured: 1.4e-15 ... 1.7e-15; the unscaled one 1.5e-4 ... 1.7e-4) and well under the gate."""
    shape, kind, layout = (2, 40, 48), "vector", "stripes"
    O, N, M = shape
    x, f, u, gu, df, dx = sa.case(shape, kind, layout)
    assert sa.active_counts(u[:1]).tolist() == [[1, 1, 532]]
    s = _handle(gpu_solver_cls, (1, N, M), method)
    gf, gx = s.sumregs_vjp(u[:1], x, gu[:1], adjoint_method=method[1])
    st = s.stats()
    s.close()
    print("stripes image 0, %s: residual %.3e raw %.3e" % (method[0], st["adjoint_residual"], st["adjoint_residual_raw"]))
    _check_stats(st, method)
    assert 0.0 < st["adjoint_residual"] <= 1e-12
    rf, _, _ = sa.vjp_ref(shape, kind, layout, st["kappa_used"])
    assert _close(gf[0], rf[0], float(np.abs(rf[0]).max()))


# ---- sumregs_vjp, reg = 1 ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _reg_ref(shape, kind, layout):
    """(grad_x of the C oracle's sumregs_gradient_reg, p of the twin's literal gradient_reg_image per image), cotangent gu."""
    from oracle import c_oracle as co
    from oracle import np_twin_sumregs as ts
    co.build()
    O, N, M = shape
    x, f, u, gu, df, dx = sa.case(shape, kind, layout)
    p = np.stack([ts.gradient_reg_image(x, u[k], u[k] - gu[k])[1].reshape(N, M) for k in range(O)])
    return np.asarray(co.sumregs_gradient(x, u, u - gu, reg=True)), p


def _reg_methods(kind):
    """sumregs_gradient_reg with an array parameter is row-scaled: only the two LU factorisations take it."""
    if kind == "vector":
        return METHODS
    return [("nd-lu", "nd", 0, 3), ("band-lu", "band", 0, 3)]


REG_CASES = [(shape, kind, layout, m) for shape, kind, layout in VJP_CASES for m in _reg_methods(kind)]
REG_IDS = [sa.case_id(sh, lay, k) + "-" + m[0] for sh, k, lay, m in REG_CASES]


@pytest.mark.parametrize("shape,kind,layout,method", REG_CASES, ids=REG_IDS)
def test_regularised_vjp_on_planted_u_matches_the_oracle(gpu_solver_cls, shape, kind, layout, method):
    """reg = 1 with exactly zero gradients in the smoothed branch (h = gamma G_k u = 0): grad_f = -p of the twin's literal
    gradient_reg_image within 5e-6 max|p|, grad_x of the oracle within 1e-7 max|g|, the tolerances of
    tests/test_gpu_sumregs_vjp.py, at the library's own sweep count.  Measured: at most 1.9e-10 max|p| and 3.0e-13 max|g|."""
    x, f, u, gu, df, dx = sa.case(shape, kind, layout)
    s = _handle(gpu_solver_cls, shape, method)
    gf, gx = s.sumregs_vjp(u, x, gu, reg=1, adjoint_method=method[1])
    st = s.stats()
    s.close()
    g0, p = _reg_ref(shape, kind, layout)
    pmax, gmax = float(np.abs(p).max()), float(np.abs(g0).max())
    print("%s %s reg 1: attempts %d residual %.3e max|d| grad_f %.3e = %.3e max|p|, grad_x %.3e = %.3e max|g|"
          % (sa.case_id(shape, layout, kind), method[0], st["adjoint_attempts"], st["adjoint_residual"], _dist(gf, -p),
             _dist(gf, -p) / pmax, _dist(gx, g0), _dist(gx, g0) / gmax))
    _check_stats(st, method, reg=1)
    assert np.shape(gx) == np.shape(g0) and _dist(gx, g0) <= 1e-7 * gmax
    assert _dist(gf, -p) <= 5e-6 * pmax


# ---- u - ubar as the cotangent, equal blocks, image groups ----------------------------------------------------------------
@pytest.mark.parametrize("reg", [0, 1])
@pytest.mark.parametrize("shape,kind,layout", VJP_CASES, ids=VJP_IDS)
def test_vjp_of_u_minus_ubar_is_vjp_each_with_equal_blocks_bitwise(gpu_solver_cls, shape, kind, layout, reg):
    """sumregs_vjp(u, x, u - ubar) and sumregs_vjp_each with O copies of x: the same grad_f bits, and grad_x the per-image
    terms added in image order from 0.0 (sum_final_kernel / map_sum_kernel); with a budget of 1.5 images' workspace
    (one image per group) the same bits again."""
    O, N, M = shape
    x, f, u, gu, df, dx = sa.case(shape, kind, layout)
    ubar = u - gu
    s = gpu_solver_cls(M, N, O)
    gf, gx = s.sumregs_vjp(u, x, u - ubar, reg=reg)
    st = s.stats()
    ef, ex = s.sumregs_vjp_each(u, np.stack([x] * O), u - ubar, reg=reg)
    st_each = s.stats()
    s.close()
    assert st["adjoint_attempts"] == 1 and st_each["adjoint_attempts"] == 1 and st_each["kappa_used"] == st["kappa_used"], (st, st_each)
    acc = np.zeros(np.shape(x))
    for k in range(O):
        acc = acc + ex[k]
    assert _same(ef, gf) and _same(acc, gx)
    if O > 1:
        # the row-scaled system runs the LU variant, whose workspace is just under twice the Cholesky's
        lu = reg == 1 and kind != "vector"
        sg = gpu_solver_cls(M, N, O)
        sg.set_option("adjoint_budget_mb", (2.5 if lu else 1.5) * _bytes_per_image(M, N) / 1e6)
        gfg, gxg = sg.sumregs_vjp(u, x, u - ubar, reg=reg)
        stg = sg.stats()
        efg, exg = sg.sumregs_vjp_each(u, np.stack([x] * O), u - ubar, reg=reg)
        chunks_each = sg.stats()["adjoint_chunks"]
        sg.close()
        assert stg["adjoint_chunks"] > 1 and chunks_each > 1 and stg["adjoint_attempts"] == 1, stg
        assert stg["kappa_used"] == st["kappa_used"]
        assert _same(gfg, gf) and _same(gxg, gx) and _same(efg, ef) and _same(exg, ex)


# ---- sumregs_vjp_each -----------------------------------------------------------------------------------------------------
EACH_SHAPES = [((2, 40, 48), "blocks"), ((2, 40, 48), "stripes"), ((3, 33, 17), "flat"), ((3, 40, 48), "flat")]
EACH_CASES = [(shape, kind, layout) for shape, layout in EACH_SHAPES for kind in KINDS]
EACH_IDS = [sa.case_id(sh, lay, k) for sh, k, lay in EACH_CASES]


@functools.lru_cache(maxsize=None)
def _each_ref(shape, kind, layout, kappa):
    x, f, u, gu, df, dx = sa.case(shape, kind, layout)
    return sa.vjp_each(u, _each_xs(x, shape[0]), gu, kappa)


@pytest.mark.parametrize("method", TWO, ids=TWO_IDS)
@pytest.mark.parametrize("shape,kind,layout", EACH_CASES, ids=EACH_IDS)
def test_vjp_each_matches_the_literal_system_image_by_image(gpu_solver_cls, shape, kind, layout, method):
    """Image k with its own block (the case's, scaled by 1, 0.7, 1.3) within the bound of the literal system with xs[k], and
    bitwise a one-image handle's sumregs_vjp: nothing an image gets depends on what the other images look like.  Measured: at
    most 4.7e-10 / 9.5e-9 (grad_f / grad_x)."""
    O, N, M = shape
    x, f, u, gu, df, dx = sa.case(shape, kind, layout)
    xs = _each_xs(x, O)
    s = _handle(gpu_solver_cls, shape, method)
    gf, gx = s.sumregs_vjp_each(u, xs, gu, adjoint_method=method[1])
    st = s.stats()
    s.close()
    rf, rx, pmax = _each_ref(shape, kind, layout, st["kappa_used"])
    for k in range(O):
        print("each %s %s image %d: attempts %d max|d| grad_f %.3e grad_x %.3e (max|p| %.3e)"
              % (sa.case_id(shape, layout, kind), method[0], k, st["adjoint_attempts"], _dist(gf[k], rf[k]), _dist(gx[k], rx[k]), pmax[k]))
    _check_stats(st, method)
    assert gx.shape == xs.shape
    s1 = _handle(gpu_solver_cls, (1, N, M), method)
    for k in range(O):
        assert _close(gf[k], rf[k], pmax[k]) and _close(gx[k], rx[k], pmax[k]), k
        gf1, gx1 = s1.sumregs_vjp(u[k:k + 1], xs[k], gu[k:k + 1], adjoint_method=method[1])
        assert s1.stats()["kappa_used"] == st["kappa_used"] and s1.stats()["adjoint_attempts"] == 1
        assert _same(gf1[0], gf[k]) and _same(gx1, gx[k]), k
    s1.close()
    if kind == "map" and layout == "flat":
        assert not np.any(gx[0])                      # the constant image: h_k = 0 everywhere


# ---- sumregs_jvp, sumregs_jvp_each ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", TWO, ids=TWO_IDS)
@pytest.mark.parametrize("shape,kind,layout", EACH_CASES, ids=EACH_IDS)
def test_jvp_matches_the_literal_system(gpu_solver_cls, shape, kind, layout, method):
    """du for both tangents and each alone: the tangent right-hand side df - sum_k (G_k^T h_k) o up(dx_k) with h_k = 0 on
    active elements, on the matrix the VJP tests hold (the LU path factors its transpose); three directions in one call are
    bitwise three calls.  Measured: at most 1.5e-9 max|du| with nested dissection, 3.8e-11 with the LU."""
    x, f, u, gu, df, dx = sa.case(shape, kind, layout)
    s = _handle(gpu_solver_cls, shape, method)
    got = {"both": s.sumregs_jvp(u, x, df=df, dalpha=dx, adjoint_method=method[1])}
    st = s.stats()
    got["df"] = s.sumregs_jvp(u, x, df=df, adjoint_method=method[1])
    got["dx"] = s.sumregs_jvp(u, x, dalpha=dx, adjoint_method=method[1])
    z, zx = np.zeros_like(df), np.zeros_like(dx)
    stack = s.sumregs_jvp(u, x, df=np.stack([df, df, z]), dalpha=np.stack([dx, zx, dx]), adjoint_method=method[1])
    st3 = s.stats()
    s.close()
    ok = {}
    for which, du in got.items():
        ref = sa.jvp_ref(shape, kind, layout, st["kappa_used"], which)
        print("%s %s jvp %s: attempts %d max|d du| %.3e (max|du| %.3e)"
              % (sa.case_id(shape, layout, kind), method[0], which, st["adjoint_attempts"], _dist(du, ref), np.abs(ref).max()))
        ok[which] = _du_close(du, ref)
    _check_stats(st, method)
    assert st3["kappa_used"] == st["kappa_used"] and st3["adjoint_attempts"] == 1
    assert stack.shape == (3,) + shape
    assert _same(stack[0], got["both"]) and _same(stack[1], got["df"]) and _same(stack[2], got["dx"])
    assert all(ok.values()), ok


def _each_dxs(x, O):
    return np.random.default_rng(77).standard_normal((O,) + np.shape(x))


@functools.lru_cache(maxsize=None)
def _jvp_each_ref(shape, kind, layout, kappa, which):
    x, f, u, gu, df, dx = sa.case(shape, kind, layout)
    xs, dxs = _each_xs(x, shape[0]), _each_dxs(x, shape[0])
    return sa.jvp_each(u, xs, None if which == "dx" else df, None if which == "df" else dxs, kappa)


@pytest.mark.parametrize("method", TWO, ids=TWO_IDS)
@pytest.mark.parametrize("shape,kind,layout", EACH_CASES, ids=EACH_IDS)
def test_jvp_each_matches_the_literal_system(gpu_solver_cls, shape, kind, layout, method):
    """Image k with xs[k] and dxs[k]: both tangents and each alone; three directions bitwise three calls.  Measured: at most
    3.1e-10 max|du| with nested dissection, 8.8e-12 with the LU."""
    O = shape[0]
    x, f, u, gu, df, dx = sa.case(shape, kind, layout)
    xs, dxs = _each_xs(x, O), _each_dxs(x, O)
    s = _handle(gpu_solver_cls, shape, method)
    got = {"both": s.sumregs_jvp_each(u, xs, df=df, dalphas=dxs, adjoint_method=method[1])}
    st = s.stats()
    got["df"] = s.sumregs_jvp_each(u, xs, df=df, adjoint_method=method[1])
    got["dx"] = s.sumregs_jvp_each(u, xs, dalphas=dxs, adjoint_method=method[1])
    z, zx = np.zeros_like(df), np.zeros_like(dxs)
    stack = s.sumregs_jvp_each(u, xs, df=np.stack([df, df, z]), dalphas=np.stack([dxs, zx, dxs]), adjoint_method=method[1])
    s.close()
    ok = {}
    for which, du in got.items():
        ref = _jvp_each_ref(shape, kind, layout, st["kappa_used"], which)
        print("%s %s jvp_each %s: attempts %d max|d du| %.3e (max|du| %.3e)"
              % (sa.case_id(shape, layout, kind), method[0], which, st["adjoint_attempts"], _dist(du, ref), np.abs(ref).max()))
        ok[which] = all(_du_close(du[k], ref[k]) for k in range(O))
    _check_stats(st, method)
    assert _same(stack[0], got["both"]) and _same(stack[1], got["df"]) and _same(stack[2], got["dx"])
    assert all(ok.values()), ok


# ---- sumregs_gauss_newton -------------------------------------------------------------------------------------------------
GN_SHAPES = [((2, 40, 48), "blocks"), ((2, 40, 48), "stripes"), ((3, 33, 17), "flat")]


@functools.lru_cache(maxsize=None)
def _gn_ref(shape, kind, layout, kappa):
    x, f, u, gu, df, dx = sa.case(shape, kind, layout)
    return sa.gauss_newton(u, u - gu, x, kappa)


@pytest.mark.parametrize("method", TWO, ids=TWO_IDS)
@pytest.mark.parametrize("kind", ["vector", "patch22"])
@pytest.mark.parametrize("shape,layout", GN_SHAPES, ids=[sa.case_id(sh, lay) for sh, lay in GN_SHAPES])
def test_gauss_newton_matches_columns_of_the_literal_system(gpu_solver_cls, shape, layout, kind, method):
    """J^T (u - ubar) and J^T J, J's columns from the reference jvp of each parameter entry: rtol 1e-6, atol 1e-8 max|entry|.
    Measured: J^T (u - ubar) within 5.3e-9 of entries up to 31, J^T J within 9.3e-8 of entries up to 3.1e3 (2.4e-10 of them)."""
    x, f, u, gu, df, dx = sa.case(shape, kind, layout)
    s = _handle(gpu_solver_cls, shape, method)
    g, H = s.sumregs_gauss_newton(u, u - gu, x, adjoint_method=method[1])
    st = s.stats()
    s.close()
    g0, H0 = _gn_ref(shape, kind, layout, st["kappa_used"])
    print("gauss_newton %s %s: attempts %d max|d grad| %.3e (max %.3e) max|d H| %.3e (max %.3e)"
          % (sa.case_id(shape, layout, kind), method[0], st["adjoint_attempts"], _dist(g, g0), np.abs(g0).max(), _dist(H, H0), np.abs(H0).max()))
    _check_stats(st, method)
    assert np.shape(g) == np.shape(x) and H.shape == H0.shape
    assert _close(g, g0, float(np.abs(g0).max()))
    assert _close(H, H0, float(np.abs(H0).max()))
