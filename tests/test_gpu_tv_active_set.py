"""GPU checks of the unweighted TV adjoint solvers on images with a real active set.

Every other unweighted adjoint test takes u from a long solve of synth_batch, whose only element with |G u| < 1e-12 is the last
pixel: the active branch of adj_setup_body, h = 0 in adj_gradpix_kernel, the tangent right-hand side on active elements and the
factorisations of a matrix with 1e14 (scalar) or 6.7e7 (patch, map) entries beside O(1) ones were never compared with an
independent solve.  Here u is the numpy twin's iterate with flat regions planted (tests/tv_active_ref.py: two blocks, strips that
cross tile seams and separators, a fully flat image) and the reference is the literal unreduced system of tests/weighted_ref.py
with w = 1, kappa = stats["kappa_used"], solved once per (case, kappa) with ten extended-precision sweeps and pinned on the CPU by
tests/test_tv_active_ref.py.  The bound everywhere is |a - b| <= 1e-8 max|p| + 1e-6 |b|, elementwise."""
import functools

import numpy as np
import pytest

import tv_active_ref as ta
from test_gpu_vjp import _nd_bytes_per_image

pytestmark = pytest.mark.gpu

E_UNSUPPORTED = 6
KINDS = list(ta.KINDS)
# params.reserved[4]: band (LDS; HBM from M = 139 on), block cyclic reduction (M <= 128), nested dissection (also the default)
METHODS = {1: "band", 2: "bcr", 3: "nd"}
METHOD_IDS = [METHODS[m] for m in sorted(METHODS)]


def _expected_method(m, M):
    return {0: "nd", 1: "band" if M <= 138 else "band-hbm", 2: "bcr", 3: "nd"}[m]


def _same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b))


def _dist(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max())


def _close(a, b, scale):
    """|a - b| <= 1e-8 scale + 1e-6 |b| elementwise."""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and bool(np.all(np.abs(a - b) <= 1e-8 * scale + 1e-6 * np.abs(b)))


def _handle(cls, shape, method):
    """A handle and the factorisation it will run: block cyclic reduction is refused with E_UNSUPPORTED above M = 128, after
    which the handle goes on working (with the default factorisation)."""
    from bpldenoising_amd._lib import BpltvError
    O, N, M = shape
    s = cls(M, N, O)
    if method == 2 and M > 128:
        z = np.zeros(shape)
        with pytest.raises(BpltvError) as e:
            s.vjp(z, 0.1, z, adjoint_method=2)
        assert e.value.code == E_UNSUPPORTED
        method = 0
    return s, method


def _check_stats(st, method, M, chunks=1):
    assert st["adjoint_method"] == _expected_method(method, M), st
    assert st["adjoint_attempts"] == 1 and st["adjoint_residual"] <= 1e-6 and st["adjoint_chunks"] == chunks, st


def _each_alphas(alpha, O):
    """One parameter per image: the case's own, scaled by 1, 0.7, 1.3, ..."""
    sc = np.array([1.0, 0.7, 1.3, 0.85])[:O]
    a = np.asarray(alpha, dtype=np.float64)
    return sc if a.ndim == 0 else sc[:, None, None] * a[None]


# ---- (a), (b) bpltv_vjp -------------------------------------------------------------------------------------------------
VJP_CASES = [(shape, kind, layout) for shape, layout in ta.CASES[:-1] for kind in KINDS]
VJP_IDS = [ta.case_id(sh, lay, k) for sh, k, lay in VJP_CASES]


def vjp_distances(cls, shape, kind, layout, method, refine):
    """One bpltv_vjp call on a planted case against the literal system: (grad_f within the bound, grad_alpha within the bound,
    max|d grad_f|, max|d grad_alpha|, max|p|)."""
    O, N, M = shape
    alpha, f, u, gu, df, da = ta.case(shape, kind, layout)
    s, method = _handle(cls, shape, method)
    kw = {} if refine is None else {"refine": refine}
    gf, ga = s.vjp(u, alpha, gu, adjoint_method=method, **kw)
    st = s.stats()
    s.close()
    _check_stats(st, method, M)
    rf, ra, pmax = ta.vjp_ref(shape, kind, layout, st["kappa_used"])
    print("%s %s refine %s: method %s kappa_used %.3e residual %.3e max|d| grad_f %.3e grad_alpha %.3e (max|p| %.3e, bound %.1e)"
          % (ta.case_id(shape, layout, kind), METHODS.get(method, "auto"), refine, st["adjoint_method"], st["kappa_used"],
             st["adjoint_residual"], _dist(gf, rf), _dist(ga, ra), pmax, 1e-8 * pmax))
    assert np.shape(ga) == np.shape(alpha)
    return _close(gf, rf, pmax), _close(ga, ra, pmax), _dist(gf, rf), _dist(ga, ra), pmax


@pytest.mark.parametrize("method", sorted(METHODS), ids=METHOD_IDS)
@pytest.mark.parametrize("shape,kind,layout", VJP_CASES, ids=VJP_IDS)
def test_vjp_at_converged_refinement_matches_the_literal_system(gpu_solver_cls, shape, kind, layout, method):
    """refine = 6, where further sweeps change nothing: what the kernels and factorisations compute on
    active elements, apart from the sweep count.

    Measured on the MI355X, largest |difference| of grad_f / grad_alpha over the cases (max|p| 1.6 ... 4.3, kappa_used 1e14 for a
    scalar, 6.7e7 for a patch or a map, adjoint_attempts 1 and adjoint_residual <= 1.5e-14 everywhere):
        scalar       LDS band, block cyclic reduction, nested dissection   4.3e-11 / 1.1e-10
        scalar       band in HBM, M = 140                                  5.1e-12 / 6.9e-12
        patch, map   every method                                          2.4e-10 / 3.6e-10
    The constant image of 3 x 40 x 48 "flat" with a scalar was refused by the residual gate at kappa = 1e14 on every
    factorisation, whatever the sweep count, and solved with 1e12 (3 x 33 x 17: 1e10) until adj_resnorm_kernel left the rows that
    carry the weight out of the gate ("Held to the literal system on active sets")."""
    okf, oka, _, _, _ = vjp_distances(gpu_solver_cls, shape, kind, layout, method, 6)
    assert okf, "grad_f"
    assert oka, "grad_alpha"


@pytest.mark.parametrize("method", sorted(METHODS), ids=METHOD_IDS)
@pytest.mark.parametrize("shape,kind,layout", VJP_CASES, ids=VJP_IDS)
def test_vjp_at_the_default_refinement_matches_the_literal_system(gpu_solver_cls, shape, kind, layout, method):
    """The same calls with the sweep count left to the library (AdjPlan::nref of run_gradient).

    Measured on the MI355X with a scalar (patch and map as above): LDS band (3 sweeps) 2.6e-8 / 2.0e-7, 0.67 of the bound on
    3 x 33 x 17; block cyclic reduction (3) 3.5e-10 / 1.6e-8; nested dissection (4) 4.3e-11 / 3.5e-9; band in HBM (4) 5.1e-12 /
    1.2e-11.  With the two sweeps nested dissection ran until this test existed it left 1.8e-7 / 2.1e-5, 2.2 times the bound, and
    failed here on 3 x 33 x 17, 2 x 70 x 72 and 1 x 12 x 140; three leave 2.4e-9 / 2.7e-7."""
    okf, oka, _, _, _ = vjp_distances(gpu_solver_cls, shape, kind, layout, method, None)
    assert okf, "grad_f"
    assert oka, "grad_alpha"


@pytest.mark.parametrize("method", sorted(METHODS), ids=METHOD_IDS)
def test_a_flat_image_has_no_map_gradient(gpu_solver_cls, method):
    """h = 0 on every element of a constant image: its own grad_alpha is exactly zero for a map (a one-image handle; in the batch
    sum the other images' terms cover it), while its grad_f is the literal system's."""
    shape, kind, layout = (3, 40, 48), "map", "flat"
    O, N, M = shape
    alpha, f, u, gu, df, da = ta.case(shape, kind, layout)
    assert ta.active_counts(u)[0] == N * M - 1
    s = gpu_solver_cls(M, N, 1)
    gf, ga = s.vjp(u[0], alpha, gu[0], adjoint_method=method)
    st = s.stats()
    s.close()
    _check_stats(st, method, M)
    assert ga.shape == (N, M) and not np.any(ga)
    rf, _, pmax = ta.vjp_ref(shape, kind, layout, st["kappa_used"])
    print("flat image, %s: max|d grad_f| %.3e" % (METHODS[method], _dist(gf[0], rf[0])))
    assert _close(gf[0], rf[0], pmax)


# ---- (c) bpltv_gradient -------------------------------------------------------------------------------------------------
GRAD_CASES = [(shape, kind, layout) for shape, layout in ta.CASES for kind in KINDS]
GRAD_IDS = [ta.case_id(sh, lay, k) for sh, k, lay in GRAD_CASES]


@pytest.mark.parametrize("reg", [0, 1])
@pytest.mark.parametrize("shape,kind,layout", GRAD_CASES, ids=GRAD_IDS)
def test_gradient_on_planted_u_is_the_vjp_bitwise(gpu_solver_cls, shape, kind, layout, reg):
    """adj_setup_body<false> (right-hand side u - ubar) against adj_setup_body<true> with the cotangent u - ubar, ubar = u - gu:
    the same bits; without regularisation also within the bound of the literal system (u - (u - gu) is gu to an ulp of u)."""
    O, N, M = shape
    alpha, f, u, gu, df, da = ta.case(shape, kind, layout)
    ubar = u - gu
    s = gpu_solver_cls(M, N, O)
    g0 = s.gradient(u, ubar, alpha, reg=reg)
    st = s.stats()
    _, ga = s.vjp(u, alpha, u - ubar, reg=reg, want_f=False)
    s.close()
    assert st["reg_gradient_used"] == reg and st["adjoint_attempts"] == 1, st
    assert np.shape(g0) == np.shape(alpha) and _same(g0, ga)
    if not reg:
        _, ra, pmax = ta.vjp_ref(shape, kind, layout, st["kappa_used"])
        print("%s gradient: max|d| %.3e (bound %.1e)" % (ta.case_id(shape, layout, kind), _dist(g0, ra), 1e-8 * pmax))
        assert _close(g0, ra, pmax)


@functools.lru_cache(maxsize=None)
def _oracle_reg(shape, kind, layout):
    """(gradient, p per image) of the C oracle's gradient_reg on the planted case, cotangent gu."""
    from oracle import c_oracle as co
    co.build()
    O, N, M = shape
    alpha, f, u, gu, df, da = ta.case(shape, kind, layout)
    amap = co.patch_upsample(alpha, M, N) if kind != "scalar" else np.full((N, M), alpha)
    p = np.stack([co.gradient_image(u[k], u[k] - gu[k], amap, patch=kind != "scalar", reg=True)[1] for k in range(O)])
    return co.gradient(alpha, u, u - gu, reg=True), p


@pytest.mark.parametrize("method", sorted(METHODS), ids=METHOD_IDS)
@pytest.mark.parametrize("shape,kind,layout", GRAD_CASES, ids=GRAD_IDS)
def test_regularised_vjp_on_planted_u_matches_the_oracle(gpu_solver_cls, shape, kind, layout, method):
    """reg = 1 with exactly zero gradients in the smoothed branch (|G u| <= 1e-8: weight 1e8, h = 1e8 G u = 0): grad_f = -p and
    grad_alpha of the oracle's gradient_reg at tests/test_gpu_vjp.py's tolerances (rtol 1e-6, atol 1e-8 max|p| / max|g|); the
    oracle is pinned to the literal numpy restatement on these u by tests/test_tv_active_ref.py."""
    O, N, M = shape
    alpha, f, u, gu, df, da = ta.case(shape, kind, layout)
    s, method = _handle(gpu_solver_cls, shape, method)
    gf, ga = s.vjp(u, alpha, gu, reg=1, adjoint_method=method)
    st = s.stats()
    s.close()
    _check_stats(st, method, M)
    g0, p = _oracle_reg(shape, kind, layout)
    print("%s %s reg 1: max|d| grad_f %.3e grad_alpha %.3e (max|p| %.3e max|g| %.3e)"
          % (ta.case_id(shape, layout, kind), METHODS.get(method, "auto"), _dist(gf, -p), _dist(ga, g0), np.abs(p).max(), np.abs(g0).max()))
    for k in range(O):
        assert np.allclose(gf[k], -p[k], rtol=1e-6, atol=1e-8 * np.abs(p[k]).max()), k
    assert np.allclose(ga, g0, rtol=1e-6, atol=1e-8 * np.abs(g0).max())


# ---- (d) bpltv_vjp_each -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", sorted(METHODS), ids=METHOD_IDS)
@pytest.mark.parametrize("kind", KINDS)
def test_vjp_each_on_a_batch_that_mixes_active_sets(gpu_solver_cls, kind, method):
    """3 x 33 x 17: a constant image, one with two blocks, an untouched one, each with its own parameter.  Image k within the
    bound of the literal system with alphas[k], and bitwise a one-image handle's bpltv_vjp: nothing an image gets (sweeps,
    weight, pivots) depends on what the other images of the batch look like."""
    shape, layout = (3, 33, 17), "flat"
    O, N, M = shape
    alpha, f, u, gu, df, da = ta.case(shape, kind, layout)
    alphas = _each_alphas(alpha, O)
    s = gpu_solver_cls(M, N, O)
    gf, ga = s.vjp_each(u, alphas, gu, adjoint_method=method)
    st = s.stats()
    s.close()
    _check_stats(st, method, M)
    assert ga.shape == alphas.shape
    rf, ra, p = _each_ref(kind, st["kappa_used"])
    s1 = gpu_solver_cls(M, N, 1)
    for k in range(O):
        pmax = float(np.abs(p[k]).max())
        print("each %s %s image %d: max|d| grad_f %.3e grad_alpha %.3e (max|p| %.3e)"
              % (kind, METHODS[method], k, _dist(gf[k], rf[k]), _dist(ga[k], ra[k]), pmax))
        assert _close(gf[k], rf[k], pmax) and _close(ga[k], ra[k], pmax), k
        ak = float(alphas[k]) if kind == "scalar" else alphas[k]
        gf1, ga1 = s1.vjp(u[k], ak, gu[k], adjoint_method=method)
        assert s1.stats()["kappa_used"] == st["kappa_used"] and s1.stats()["adjoint_attempts"] == 1
        assert _same(gf1[0], gf[k]) and _same(ga1, ga[k]), k
    s1.close()
    if kind == "map":
        assert not np.any(ga[0])                      # the constant image: h = 0 everywhere


@functools.lru_cache(maxsize=None)
def _each_ref(kind, kappa):
    shape, layout = (3, 33, 17), "flat"
    alpha, f, u, gu, df, da = ta.case(shape, kind, layout)
    return ta.vjp_each(u, _each_alphas(alpha, shape[0]), gu, kappa, refine=10)


# ---- (e) bpltv_jvp, bpltv_jvp_each ----------------------------------------------------------------------------------------
JVP_CASES = [(shape, kind, layout) for shape, layout in (((2, 40, 48), "blocks"), ((2, 40, 48), "strips"), ((1, 12, 140), "blocks"))
             for kind in KINDS]
JVP_IDS = [ta.case_id(sh, lay, k) for sh, k, lay in JVP_CASES]


def _du_close(a, b):
    return a.shape == b.shape and bool(np.all(np.abs(a - b) <= 1e-8 * np.abs(b).max() + 1e-6 * np.abs(b)))


@pytest.mark.parametrize("method", sorted(METHODS), ids=METHOD_IDS)
@pytest.mark.parametrize("shape,kind,layout", JVP_CASES, ids=JVP_IDS)
def test_jvp_matches_the_literal_system(gpu_solver_cls, shape, kind, layout, method):
    """du for both tangents and each alone: the tangent right-hand side df - G^T (dalpha o h) with h = 0 on active elements, on the
    matrix the VJP tests hold; three directions in one call are bitwise three calls."""
    O, N, M = shape
    alpha, f, u, gu, df, da = ta.case(shape, kind, layout)
    s, method = _handle(gpu_solver_cls, shape, method)
    got = {"both": s.jvp(u, alpha, df=df, dalpha=da, adjoint_method=method)}
    st = s.stats()
    _check_stats(st, method, M)
    got["df"] = s.jvp(u, alpha, df=df, adjoint_method=method)
    got["dalpha"] = s.jvp(u, alpha, dalpha=da, adjoint_method=method)
    z, za = np.zeros_like(df), np.zeros(np.shape(da))
    stack = s.jvp(u, alpha, df=np.stack([df, df, z]), dalpha=np.stack([da, za, da]), adjoint_method=method)
    assert s.stats()["kappa_used"] == st["kappa_used"] and s.stats()["adjoint_attempts"] == 1
    s.close()
    assert stack.shape == (3,) + shape
    assert _same(stack[0], got["both"]) and _same(stack[1], got["df"]) and _same(stack[2], got["dalpha"])
    for which, du in got.items():
        ref = ta.jvp_ref(shape, kind, layout, st["kappa_used"], which)
        print("%s %s jvp %s: max|d du| %.3e (max|du| %.3e)" % (ta.case_id(shape, layout, kind), METHODS.get(method, "auto"), which,
                                                           _dist(du, ref), np.abs(ref).max()))
        assert _du_close(du, ref), which


@functools.lru_cache(maxsize=None)
def _jvp_each_ref(shape, kind, layout, kappa, which):
    alpha, f, u, gu, df, da = ta.case(shape, kind, layout)
    alphas, das = _each_alphas(alpha, shape[0]), _each_dalphas(alpha, shape[0])
    return ta.jvp_each(u, alphas, None if which == "dalpha" else df, None if which == "df" else das, kappa, refine=10)


def _each_dalphas(alpha, O):
    return np.random.default_rng(77).standard_normal((O,) + np.shape(alpha))


@pytest.mark.parametrize("method", sorted(METHODS), ids=METHOD_IDS)
@pytest.mark.parametrize("shape,kind,layout", JVP_CASES, ids=JVP_IDS)
def test_jvp_each_matches_the_literal_system(gpu_solver_cls, shape, kind, layout, method):
    """Image k with alphas[k] and dalphas[k]: both tangents and each alone; three directions bitwise three calls."""
    O, N, M = shape
    alpha, f, u, gu, df, da = ta.case(shape, kind, layout)
    alphas, das = _each_alphas(alpha, O), _each_dalphas(alpha, O)
    s, method = _handle(gpu_solver_cls, shape, method)
    got = {"both": s.jvp_each(u, alphas, df=df, dalphas=das, adjoint_method=method)}
    st = s.stats()
    _check_stats(st, method, M)
    got["df"] = s.jvp_each(u, alphas, df=df, adjoint_method=method)
    got["dalpha"] = s.jvp_each(u, alphas, dalphas=das, adjoint_method=method)
    z, za = np.zeros_like(df), np.zeros_like(das)
    stack = s.jvp_each(u, alphas, df=np.stack([df, df, z]), dalphas=np.stack([das, za, das]), adjoint_method=method)
    s.close()
    assert _same(stack[0], got["both"]) and _same(stack[1], got["df"]) and _same(stack[2], got["dalpha"])
    for which, du in got.items():
        ref = _jvp_each_ref(shape, kind, layout, st["kappa_used"], which)
        print("%s %s jvp_each %s: max|d du| %.3e (max|du| %.3e)" % (ta.case_id(shape, layout, kind), METHODS.get(method, "auto"),
                                                                which, _dist(du, ref), np.abs(ref).max()))
        assert _du_close(du, ref), which


# ---- (f) bpltv_gauss_newton -----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _gn_ref(kind, kappa):
    shape, layout = (2, 40, 48), "blocks"
    alpha, f, u, gu, df, da = ta.case(shape, kind, layout)
    return ta.gauss_newton(u, u - gu, alpha, kappa, refine=10)


@pytest.mark.parametrize("method", sorted(METHODS), ids=METHOD_IDS)
@pytest.mark.parametrize("kind", ["scalar", "patch"])
def test_gauss_newton_matches_columns_of_the_literal_system(gpu_solver_cls, kind, method):
    """J^T (u - ubar) and J^T J, J's columns from the reference jvp of each parameter entry: rtol 1e-6, atol 1e-8 max|entry|."""
    shape, layout = (2, 40, 48), "blocks"
    O, N, M = shape
    alpha, f, u, gu, df, da = ta.case(shape, kind, layout)
    s = gpu_solver_cls(M, N, O)
    g, H = s.gauss_newton(u, u - gu, alpha, adjoint_method=method)
    st = s.stats()
    s.close()
    _check_stats(st, method, M)
    g0, H0 = _gn_ref(kind, st["kappa_used"])
    print("gauss_newton %s %s: max|d grad| %.3e (max %.3e) max|d H| %.3e (max %.3e)"
          % (kind, METHODS[method], _dist(g, g0), np.abs(g0).max(), _dist(H, H0), np.abs(H0).max()))
    assert np.shape(g) == np.shape(alpha) and H.shape == H0.shape
    assert np.allclose(g, g0, rtol=1e-6, atol=1e-8 * np.abs(g0).max())
    assert np.allclose(H, H0, rtol=1e-6, atol=1e-8 * np.abs(H0).max())


# ---- (g) image groups -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_image_groups_on_a_mixed_batch_are_the_ungrouped_result_bitwise(gpu_solver_cls, kind):
    """A budget of 2.5 images' nested-dissection workspace on 3 x 33 x 17 "flat": the constant image and the one with blocks in one
    group, the untouched one in the next."""
    shape, layout = (3, 33, 17), "flat"
    O, N, M = shape
    alpha, f, u, gu, df, da = ta.case(shape, kind, layout)
    s = gpu_solver_cls(M, N, O)
    gf, ga = s.vjp(u, alpha, gu)
    st = s.stats()
    _check_stats(st, 0, M)
    du = s.jvp(u, alpha, df=df, dalpha=da)
    s.close()
    rf, ra, pmax = ta.vjp_ref(shape, kind, layout, st["kappa_used"])
    assert _close(gf, rf, pmax) and _close(ga, ra, pmax)
    sg = gpu_solver_cls(M, N, O)
    sg.set_option("adjoint_budget_mb", 2.5 * _nd_bytes_per_image(M, N) / 1e6)
    gfg, gag = sg.vjp(u, alpha, gu)
    stg = sg.stats()
    dug = sg.jvp(u, alpha, df=df, dalpha=da)
    chunks_jvp = sg.stats()["adjoint_chunks"]
    sg.close()
    assert stg["adjoint_chunks"] > 1 and chunks_jvp > 1 and stg["kappa_used"] == st["kappa_used"] and stg["adjoint_attempts"] == 1, stg
    assert _same(gfg, gf) and _same(gag, ga) and _same(dug, du)


# ---- (h) unit weight --------------------------------------------------------------------------------------------------------
UNIT_CASES = [((2, 40, 48), "blocks"), ((1, 12, 140), "blocks"), ((3, 33, 17), "flat")]


@pytest.mark.parametrize("method", sorted(METHODS), ids=METHOD_IDS)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape,layout", UNIT_CASES, ids=[ta.case_id(sh, lay) for sh, lay in UNIT_CASES])
def test_unit_weight_vjp_on_planted_u_is_the_unweighted_vjp_bitwise(gpu_solver_cls, shape, layout, kind, method):
    """bpltv_weighted_vjp with w = 1 everywhere (one plane, one per image) against bpltv_vjp where the active set is real: the
    same sweeps on the same system."""
    O, N, M = shape
    alpha, f, u, gu, df, da = ta.case(shape, kind, layout)
    s, method = _handle(gpu_solver_cls, shape, method)
    gf0, ga0 = s.vjp(u, alpha, gu, adjoint_method=method)
    st0 = s.stats()
    _check_stats(st0, method, M)
    for w in (np.ones((N, M)), np.ones((O, N, M))):
        gf, ga, gw = s.weighted_vjp(u, f, alpha, w, gu, adjoint_method=method)
        st = s.stats()
        assert _same(gf, gf0) and _same(ga, ga0), w.shape
        assert st["adjoint_method"] == st0["adjoint_method"] and st["kappa_used"] == st0["kappa_used"] and st["adjoint_attempts"] == 1
    s.close()
