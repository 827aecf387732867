"""GPU checks of forward mode through the PDHG iterations of the weighted model (bpltv_weighted_unrolled_jvp, its device form
and bpltv_weighted_unrolled_gauss_newton).

The sweep's primal is tied to bpltv_weighted_denoise bit for bit, for real weights, masks and w == 1; its tangent is held
against the numpy twin tests/weighted_unrolled_jvp_ref.py (pinned on the CPU by tests/test_weighted_unrolled_jvp_abi.py),
against the reverse sweep bpltv_weighted_unrolled_vjp by the transpose identity (dw against grad_w included), against central
differences of bpltv_weighted_denoise itself and, at w == 1, against bpltv_unrolled_jvp; every plan (fusion depth, launch
chains, graphs, host or device form, one direction or several) gives the same bits; and a sweep, accepted or rejected, leaves
the handle's last solve, tapes and statistics as they were."""
import ctypes as C
import functools

import numpy as np
import pytest

import unrolled_ref as ur
import weighted_unrolled_jvp_ref as wuj
import weighted_unrolled_ref as wur
from oracle import np_twin as tw

pytestmark = pytest.mark.gpu

E_ARG, E_NODATA, E_UNSUPPORTED = 1, 3, 6
_dp = C.POINTER(C.c_double)
SHAPES = wur.GPU_SHAPES
_alpha = wur.alpha_of
METHOD = "weighted-unrolled-jvp"


def _same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b))


def _ptr(a):
    return a.ctypes.data_as(_dp) if a is not None else None


@functools.lru_cache(maxsize=None)
def _data(name):
    """(f, cotangent gu, tangent df) of a shape; read-only."""
    f, gu = wur.gpu_data(name)
    df = np.random.default_rng(305).standard_normal(f.shape)
    for a in (f, gu, df):
        a.setflags(write=False)
    return f, gu, df


@functools.lru_cache(maxsize=None)
def _weight(name, wkind):
    """(w, tangent dw in the shape of w); read-only."""
    w = wur.weight_of(wkind, *SHAPES[name])
    dw = np.random.default_rng(306).standard_normal(w.shape)
    w.setflags(write=False)
    dw.setflags(write=False)
    return w, dw


def _dalpha(alpha, seed=11):
    """A standard-normal tangent in the type / shape of alpha."""
    g = np.random.default_rng(seed).standard_normal(np.shape(alpha))
    return float(g) if np.ndim(alpha) == 0 else g


def _damap(dalpha, M, N):
    return np.full((N, M), dalpha) if np.ndim(dalpha) == 0 else tw.alpha_to_map(dalpha, M, N)


# ---- 1. the primal is bpltv_weighted_denoise's, bit for bit ------------------------------------------------------------
@pytest.mark.parametrize("kind", ["scalar", "patch", "map"])
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_primal_is_the_weighted_denoise_bitwise(gpu_solver_cls, name, kind):
    O, N, M = SHAPES[name]
    f, _, df = _data(name)
    alpha = _alpha(kind, N, M)
    s = gpu_solver_cls(M, N, O)
    s.set_data(f, f)
    for wkind in ("real", "mask", "ones"):
        w, dw = _weight(name, wkind)
        for accel in (1, 0):
            for maxiter in (1, 7, 203):
                u0 = s.weighted_denoise(alpha, w, maxiter=maxiter, accel=accel)
                du, u1 = s.weighted_unrolled_jvp(alpha, w, df=df, dalpha=_dalpha(alpha), dw=dw, want_u=True, maxiter=maxiter,
                                                 accel=accel)
                assert _same(u1, u0), (wkind, accel, maxiter, float(np.abs(u1 - u0).max()))
                assert np.isfinite(du).all() and du.any()
                assert s.stats()["adjoint_method"] == METHOD and s.stats()["adjoint_ms"] > 0.0
    s.close()


# ---- 2. the tangent against the twin -----------------------------------------------------------------------------------
@pytest.mark.parametrize("wkind", ["real", "mask"])
@pytest.mark.parametrize("kind", ["scalar", "patch", "map"])
@pytest.mark.parametrize("name", wur.GRADIENT_SHAPES)
def test_tangent_matches_the_twin(gpu_solver_cls, name, kind, wkind):
    """1e-11 * max|ref|, the bound the TV sweep meets (DESIGN.md section 4.11 holds the measured maximum): each tangent alone
    and all three together."""
    O, N, M = SHAPES[name]
    f, _, df = _data(name)
    w, dw = _weight(name, wkind)
    alpha = _alpha(kind, N, M)
    amap = tw.alpha_to_map(alpha, M, N)
    da = _dalpha(alpha)
    dam = _damap(da, M, N)
    s = gpu_solver_cls(M, N, O)
    s.set_data(f, f)
    for K in wur.GRADIENT_K:
        for tf, ta, tam, tw_ in ((df, None, None, None), (None, da, dam, None), (None, None, None, dw), (df, da, dam, dw)):
            _, du0 = wuj.forward_tangent(f, amap, w, K, tf, tam, tw_)
            du = s.weighted_unrolled_jvp(alpha, w, df=tf, dalpha=ta, dw=tw_, maxiter=K)
            d, m = float(np.abs(du - du0).max()), float(np.abs(du0).max())
            print("%s %s %s K %d df %d dalpha %d dw %d: du %.2e (bound %.2e, max|ref| %.2e, rel %.1e)"
                  % (name, kind, wkind, K, tf is not None, ta is not None, tw_ is not None, d, 1e-11 * m, m, d / m))
            assert d <= 1e-11 * m
    s.close()


# ---- 3. the transpose identity against the reverse sweep ---------------------------------------------------------------
@pytest.mark.parametrize("wkind", ["real", "mask"])       # real: wo = O, mask: wo = 1
@pytest.mark.parametrize("kind", ["scalar", "patch", "map"])
@pytest.mark.parametrize("name", wur.GRADIENT_SHAPES)
def test_tangent_is_the_transpose_of_the_reverse_sweep(gpu_solver_cls, name, kind, wkind):
    """<du, gu> = <df, grad_f(gu)> + <dalpha, grad_alpha(gu)> + <dw, grad_w(gu)> to 1e-11 * sum|du * gu|, all three calls on
    one handle."""
    O, N, M = SHAPES[name]
    f, gu, df = _data(name)
    w, dw = _weight(name, wkind)
    assert w.ndim == (3 if wkind == "real" else 2)
    alpha = _alpha(kind, N, M)
    da = _dalpha(alpha)
    s = gpu_solver_cls(M, N, O)
    s.set_data(f, f)
    for K in wur.GRADIENT_K:
        s.weighted_unrolled_denoise(alpha, w, maxiter=K)
        du = s.weighted_unrolled_jvp(alpha, w, df=df, dalpha=da, dw=dw, maxiter=K)
        gf, ga, gw = s.weighted_unrolled_vjp(alpha, w, gu, maxiter=K)
        lhs = float((du * gu).sum())
        rhs = float((df * gf).sum()) + float((np.asarray(da) * np.asarray(ga)).sum()) + float((dw * gw).sum())
        scale = float(np.abs(du * gu).sum())
        print("%s %s %s K %d: |lhs - rhs| %.2e  bound %.2e" % (name, kind, wkind, K, abs(lhs - rhs), 1e-11 * scale))
        assert abs(lhs - rhs) <= 1e-11 * scale
    s.close()


# ---- 4. central differences of bpltv_weighted_denoise itself -----------------------------------------------------------
@pytest.mark.parametrize("wkind", ["mask", "real"])
@pytest.mark.parametrize("K", [30, 300])
def test_tangents_against_central_differences_on_the_device(gpu_solver_cls, K, wkind):
    """The case, step (h = 1e-7) and bound (1e-5 relative in the maximum norm) of tests/test_weighted_unrolled_jvp_abi.py,
    where the twin alone meets it: one direction each in alpha, f and w."""
    f, alpha, w, directions = wuj.central_difference_case(wkind)
    h = wuj.CD_H
    s = gpu_solver_cls(28, 24, 1)
    for what, df, da, dw in directions:
        s.set_data(f, f)
        du = s.weighted_unrolled_jvp(alpha, w, df=df, dalpha=da, dw=dw, maxiter=K)
        ap, am = (alpha + h * da, alpha - h * da) if da is not None else (alpha, alpha)
        wp, wm = (w + h * dw, w - h * dw) if dw is not None else (w, w)
        if df is not None:
            s.set_data(f + h * df, f + h * df)
        up = s.weighted_denoise(ap, wp, maxiter=K)
        if df is not None:
            s.set_data(f - h * df, f - h * df)
        fd = (up - s.weighted_denoise(am, wm, maxiter=K)) / (2 * h)
        d, m = float(np.abs(du - fd).max()), float(np.abs(fd).max())
        print("%s K %d d/d%s: max|du - fd| %.3e  max|fd| %.3e  rel %.2e" % (wkind, K, what, d, m, d / m))
        assert d <= wuj.CD_RTOL * m, what
    s.close()


# ---- 5. w == 1: the TV sweep's tangent ---------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["scalar", "patch", "map"])
@pytest.mark.parametrize("name", wur.GRADIENT_SHAPES)
def test_unit_weight_gives_the_unrolled_jvp_s_tangent(gpu_solver_cls, name, kind):
    """u bit for bit, du to rounding within the bound settled on the CPU (weighted_unrolled_jvp_ref.UNIT_WEIGHT_RTOL)."""
    O, N, M = SHAPES[name]
    f, _, df = _data(name)
    w, _ = _weight(name, "ones")
    alpha = _alpha(kind, N, M)
    da = _dalpha(alpha)
    s = gpu_solver_cls(M, N, O)
    s.set_data(f, f)
    for K in wur.GRADIENT_K:
        du0, u0 = s.unrolled_jvp(alpha, df=df, dalpha=da, want_u=True, maxiter=K)
        du, u = s.weighted_unrolled_jvp(alpha, w, df=df, dalpha=da, want_u=True, maxiter=K)
        d, m = float(np.abs(du - du0).max()), float(np.abs(du0).max())
        print("%s %s K %d: du %.2e (bound %.2e, rel %.1e)" % (name, kind, K, d, wuj.UNIT_WEIGHT_RTOL * m, d / m))
        assert _same(u, u0)
        assert d <= wuj.UNIT_WEIGHT_RTOL * m
        assert _same(s.weighted_unrolled_jvp(alpha, w, df=df, dalpha=da, dw=np.zeros_like(w), maxiter=K), du)
    s.close()


# ---- 6. every plan gives the same bits --------------------------------------------------------------------------------
@pytest.mark.parametrize("wkind", ["real", "mask"])       # real: wo = O, mask: wo = 1
@pytest.mark.parametrize("kind", ["scalar", "map"])
def test_results_do_not_depend_on_the_plan(gpu_solver_cls, kind, wkind):
    import torch
    name = "2x70x72"
    O, N, M = SHAPES[name]
    f, _, _ = _data(name)
    w, _ = _weight(name, wkind)
    wo = O if w.ndim == 3 else 1
    alpha = _alpha(kind, N, M)
    a = np.atleast_1d(np.asarray(alpha, dtype=np.float64))
    an, am = (1, 1) if kind == "scalar" else a.shape
    rng = np.random.default_rng(21)
    df3 = rng.standard_normal((3,) + f.shape)
    da3 = rng.standard_normal((3,) + np.shape(alpha))
    dw3 = rng.standard_normal((3,) + w.shape)
    s = gpu_solver_cls(M, N, O)
    s.set_data(f, f)
    for K in (203, 200):   # 200 iterations at depth 8: the second chain runs half a launch out of phase
        du0, u0 = s.weighted_unrolled_jvp(alpha, w, df=df3, dalpha=da3, dw=dw3, want_u=True, maxiter=K)
        assert _same(u0, s.weighted_denoise(alpha, w, maxiter=K))
        for d in range(3):   # direction d of a call is the single call
            assert _same(s.weighted_unrolled_jvp(alpha, w, df=df3[d], dalpha=da3[d], dw=dw3[d], maxiter=K), du0[d])
        plans = [dict(), dict(tile_iters=1), dict(tile_iters=3), dict(tile_iters=8), dict(chains=1), dict(chains=2),
                 dict(use_graph=0), dict(chains=2, use_graph=0), dict(tile_iters=3, chains=2)]
        for kw in plans:
            for rep in range(2):   # (the second call replays the cached graphs)
                du, u = s.weighted_unrolled_jvp(alpha, w, df=df3, dalpha=da3, dw=dw3, want_u=True, maxiter=K, **kw)
                assert _same(du, du0) and _same(u, u0), (kw, rep)
        # one tangent at a time: a NULL tangent is an explicit zero
        zf, za, zw = np.zeros_like(f), np.zeros_like(da3[0]), np.zeros_like(w)
        only_f = s.weighted_unrolled_jvp(alpha, w, df=df3[0], maxiter=K)
        only_a = s.weighted_unrolled_jvp(alpha, w, dalpha=da3[0], maxiter=K)
        only_w = s.weighted_unrolled_jvp(alpha, w, dw=dw3[0], maxiter=K)
        assert _same(only_f, s.weighted_unrolled_jvp(alpha, w, df=df3[0], dalpha=za, dw=zw, maxiter=K))
        assert _same(only_a, s.weighted_unrolled_jvp(alpha, w, df=zf, dalpha=da3[0], dw=zw, maxiter=K))
        assert _same(only_w, s.weighted_unrolled_jvp(alpha, w, df=zf, dalpha=za, dw=dw3[0], maxiter=K))
        assert only_f.any() and only_a.any() and only_w.any()
        # the device form
        at, wt = torch.tensor(a, device="cuda"), torch.tensor(w, device="cuda")
        dft, dat, dwt = torch.tensor(df3, device="cuda"), torch.tensor(da3, device="cuda"), torch.tensor(dw3, device="cuda")
        dud = torch.empty(3, O, N, M, dtype=torch.float64, device="cuda")
        ud = torch.empty(O, N, M, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        for kw in (dict(), dict(), dict(chains=1, use_graph=0), dict(tile_iters=3, chains=2)):
            dud.zero_(); ud.zero_(); torch.cuda.synchronize()
            s.weighted_unrolled_jvp_device(wt.data_ptr(), wo, at.data_ptr(), am, an, dft.data_ptr(), dat.data_ptr(), dwt.data_ptr(),
                                           dud.data_ptr(), ud.data_ptr(), ndir=3, maxiter=K, **kw)
            assert _same(dud.cpu().numpy(), du0) and _same(ud.cpu().numpy(), u0), kw
        for ptrs, ref in (((dft.data_ptr(), None, None), only_f), ((None, dat.data_ptr(), None), only_a),
                          ((None, None, dwt.data_ptr()), only_w)):
            dud.zero_(); torch.cuda.synchronize()
            s.weighted_unrolled_jvp_device(wt.data_ptr(), wo, at.data_ptr(), am, an, *ptrs, dud.data_ptr(), None, ndir=1, maxiter=K)
            assert _same(dud[0].cpu().numpy(), ref)
    s.close()


# ---- 7. the handle stays as it was --------------------------------------------------------------------------------------
def test_a_sweep_leaves_the_last_solve_the_tapes_and_the_statistics(gpu_solver_cls):
    import torch
    name = "2x17x33"
    O, N, M = SHAPES[name]
    f, gu, df = _data(name)
    w, dw = _weight(name, "mask")
    s = gpu_solver_cls(M, N, O)
    s.set_data(f, f)
    amap = _alpha("map", N, M)
    s.unrolled_denoise(0.08, maxiter=20)                     # a TV tape ...
    tv0 = s.unrolled_vjp(0.08, gu, maxiter=20)
    s.weighted_unrolled_denoise(0.08, w, maxiter=20)         # ... and a weighted one
    wt0 = s.weighted_unrolled_vjp(0.08, w, gu, maxiter=20)
    u0 = s.denoise(amap, maxiter=57)                         # the last solve: another model, parameter and shape
    gap0 = s.duality_gap()
    st0 = s.stats()
    out = torch.empty(O, N, M, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    s.copy_u_device(out.data_ptr())
    ptr0 = s.u_device_ptr()
    du = s.weighted_unrolled_jvp(0.05, w, df=df, dalpha=1.0, dw=dw, maxiter=33)
    assert du.any()
    st1 = s.stats()
    assert st1["adjoint_method"] == METHOD and st1["adjoint_ms"] > 0.0
    for k in st0:
        if k not in ("adjoint_ms", "adjoint_method"):
            assert st1[k] == st0[k], (k, st0[k], st1[k])
    assert s.u_device_ptr() == ptr0
    out2 = torch.empty_like(out)
    torch.cuda.synchronize()
    s.copy_u_device(out2.data_ptr())
    assert _same(out2.cpu().numpy(), u0) and _same(out.cpu().numpy(), u0)
    assert _same(s.duality_gap(), gap0)
    for a, b in zip(s.weighted_unrolled_vjp(0.08, w, gu, maxiter=20), wt0):   # the earlier tapes
        assert _same(a, b)
    for a, b in zip(s.unrolled_vjp(0.08, gu, maxiter=20), tv0):
        assert _same(a, b)
    s.close()


def test_rejections_leave_the_handle_as_it_was(gpu_solver_cls):
    import torch
    from bpldenoising_amd._lib import BpltvError
    name = "2x17x33"
    O, N, M = SHAPES[name]
    f, gu, df = _data(name)
    w, dw = _weight(name, "mask")
    s = gpu_solver_cls(M, N, O)
    s.set_data(f, f)
    amap = _alpha("map", N, M)
    s.unrolled_denoise(0.08, maxiter=20)
    tv0 = s.unrolled_vjp(0.08, gu, maxiter=20)
    s.weighted_unrolled_denoise(0.08, w, maxiter=20)
    wt0 = s.weighted_unrolled_vjp(0.08, w, gu, maxiter=20)
    u0 = s.denoise(amap, maxiter=57)
    gap0 = s.duality_gap()
    ptr0 = s.u_device_ptr()
    out = torch.empty(O, N, M, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()

    def unchanged(st0):
        st1 = s.stats()
        assert st1 == st0, {k: (st0[k], st1[k]) for k in st0 if st0[k] != st1[k]}
        assert s.u_device_ptr() == ptr0
        s.copy_u_device(out.data_ptr())
        assert _same(out.cpu().numpy(), u0)
        assert _same(s.duality_gap(), gap0)
        assert _same(s.denoise(amap, maxiter=57), u0) and _same(s.duality_gap(), gap0)

    def rejected(code, call, *a, **k):
        st0 = s.stats()
        with pytest.raises(BpltvError) as e:
            call(*a, **k)
        assert e.value.code == code, (e.value.code, str(e.value))
        unchanged(st0)

    jvp, gn = s.weighted_unrolled_jvp, s.weighted_unrolled_gauss_newton
    bad_df = df.copy(); bad_df[1, 3, 4] = np.inf
    bad_dw = dw.copy(); bad_dw[3, 4] = np.nan
    nan_map = amap.copy(); nan_map[2, 5] = np.nan
    neg_w = w.copy(); neg_w[3, 4] = -0.5
    nan_w = w.copy(); nan_w[3, 4] = np.nan
    for bad in (float("nan"), -0.1, nan_map):
        rejected(E_ARG, jvp, bad, w, df=df, maxiter=20)
        if np.ndim(bad) == 0:
            rejected(E_ARG, gn, bad, w, maxiter=20)
    for bad in (neg_w, nan_w):
        rejected(E_ARG, jvp, 0.08, bad, df=df, maxiter=20)
        rejected(E_ARG, gn, 0.08, bad, maxiter=20)
    rejected(E_ARG, jvp, 0.08, w, df=bad_df, maxiter=20)
    rejected(E_ARG, jvp, 0.08, w, dalpha=float("nan"), maxiter=20)
    rejected(E_ARG, jvp, 0.08, w, dw=bad_dw, maxiter=20)
    rejected(E_ARG, jvp, 0.08, w, df=df, maxiter=0)
    rejected(E_ARG, gn, 0.08, w, maxiter=0)
    for kw in (dict(rho=0.01), dict(init=1), dict(order=1)):
        rejected(E_UNSUPPORTED, jvp, 0.08, w, df=df, maxiter=20, **kw)
        rejected(E_UNSUPPORTED, gn, 0.08, w, maxiter=20, **kw)
    p = s.params(maxiter=20)
    a1 = np.array([0.08])
    du = np.empty_like(df)
    lib, h = s._lib, s._h
    st0 = s.stats()
    fn = lib.bpltv_weighted_unrolled_jvp
    assert fn(h, _ptr(w), 1, _ptr(a1), 1, 1, C.byref(p), 1, None, None, None, _ptr(du), None) == E_ARG         # all tangents NULL
    assert fn(h, _ptr(w), 1, _ptr(a1), 1, 1, C.byref(p), 0, _ptr(df), None, None, _ptr(du), None) == E_ARG     # ndir < 1
    assert fn(h, _ptr(w), 1, _ptr(a1), 1, 1, C.byref(p), 1, _ptr(df), None, None, None, None) == E_ARG         # no du_out
    assert fn(h, None, 1, _ptr(a1), 1, 1, C.byref(p), 1, _ptr(df), None, None, _ptr(du), None) == E_ARG        # no w
    assert fn(h, _ptr(w), 3, _ptr(a1), 1, 1, C.byref(p), 1, _ptr(df), None, None, _ptr(du), None) == E_ARG     # wo not in {1, O}
    assert fn(h, _ptr(w), 1, _ptr(a1), M + 1, 1, C.byref(p), 1, _ptr(df), None, None, _ptr(du), None) == E_ARG   # shape
    assert fn(h, _ptr(w), 1, _ptr(a1), 0, 1, C.byref(p), 1, _ptr(df), None, None, _ptr(du), None) == E_ARG
    cost, g1, h1 = C.c_double(0.0), np.empty(1), np.empty(1)
    assert lib.bpltv_weighted_unrolled_gauss_newton(h, None, 1, _ptr(a1), 1, 1, C.byref(p), C.byref(cost), _ptr(g1), _ptr(h1)) == E_ARG
    assert lib.bpltv_weighted_unrolled_gauss_newton(h, _ptr(w), 3, _ptr(a1), 1, 1, C.byref(p), C.byref(cost), _ptr(g1), _ptr(h1)) == E_ARG
    unchanged(st0)
    # the device form
    good = torch.tensor([0.08], dtype=torch.float64, device="cuda")
    wt = torch.tensor(w, device="cuda")
    dft, dud = torch.tensor(df, device="cuda"), torch.empty(O, N, M, dtype=torch.float64, device="cuda")
    dwt = torch.tensor(dw, device="cuda")
    bdt, bdw = torch.tensor(bad_df, device="cuda"), torch.tensor(bad_dw, device="cuda")
    bda = torch.tensor([float("inf")], dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    dev = s.weighted_unrolled_jvp_device
    for bad in (float("nan"), -0.1):
        bt = torch.tensor([bad], dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        rejected(E_ARG, dev, wt.data_ptr(), 1, bt.data_ptr(), 1, 1, dft.data_ptr(), None, None, dud.data_ptr(), maxiter=20)
    for bad in (neg_w, nan_w):
        bw = torch.tensor(bad, device="cuda")
        torch.cuda.synchronize()
        rejected(E_ARG, dev, bw.data_ptr(), 1, good.data_ptr(), 1, 1, dft.data_ptr(), None, None, dud.data_ptr(), maxiter=20)
    rejected(E_ARG, dev, wt.data_ptr(), 1, good.data_ptr(), 1, 1, bdt.data_ptr(), None, None, dud.data_ptr(), maxiter=20)
    rejected(E_ARG, dev, wt.data_ptr(), 1, good.data_ptr(), 1, 1, dft.data_ptr(), bda.data_ptr(), None, dud.data_ptr(), maxiter=20)
    rejected(E_ARG, dev, wt.data_ptr(), 1, good.data_ptr(), 1, 1, dft.data_ptr(), None, bdw.data_ptr(), dud.data_ptr(), maxiter=20)
    rejected(E_ARG, dev, wt.data_ptr(), 1, good.data_ptr(), 1, 1, None, None, None, dud.data_ptr(), maxiter=20)
    rejected(E_ARG, dev, wt.data_ptr(), 1, good.data_ptr(), 1, 1, dft.data_ptr(), None, dwt.data_ptr(), dud.data_ptr(), ndir=0, maxiter=20)
    rejected(E_ARG, dev, wt.data_ptr(), 3, good.data_ptr(), 1, 1, dft.data_ptr(), None, None, dud.data_ptr(), maxiter=20)
    # the tapes recorded before all this
    for a, b in zip(s.weighted_unrolled_vjp(0.08, w, gu, maxiter=20), wt0):
        assert _same(a, b)
    for a, b in zip(s.unrolled_vjp(0.08, gu, maxiter=20), tv0):
        assert _same(a, b)
    n = gpu_solver_cls(M, N, O)                # no dataset
    with pytest.raises(BpltvError) as e:
        n.weighted_unrolled_jvp(0.08, w, df=df, maxiter=5)
    assert e.value.code == E_NODATA
    with pytest.raises(BpltvError) as e:
        n.weighted_unrolled_gauss_newton(0.08, w, maxiter=5)
    assert e.value.code == E_NODATA
    n.close()
    s.close()


def test_two_shards_are_unsupported(gpu_solver_cls):
    from bpldenoising_amd._lib import BpltvError
    name = "2x17x33"
    O, N, M = SHAPES[name]
    f, _, df = _data(name)
    w, dw = _weight(name, "mask")
    m = gpu_solver_cls(M, N, O, devices=[0, 0])
    m.set_data(f, f)
    u0 = m.denoise(0.07, maxiter=30)
    gap0 = m.duality_gap()
    for call, args, kw in ((m.weighted_unrolled_jvp, (0.07, w), dict(df=df)), (m.weighted_unrolled_gauss_newton, (0.07, w), dict()),
                           (m.weighted_unrolled_jvp_device, (1, 1, 1, 1, 1, 1, 1, 1, 1), dict())):
        with pytest.raises(BpltvError) as e:     # (the device form is refused before any pointer is read)
            call(*args, maxiter=30, **kw)
        assert e.value.code == E_UNSUPPORTED
        assert _same(m.duality_gap(), gap0) and _same(m.denoise(0.07, maxiter=30), u0)
    m.close()
    one = gpu_solver_cls(M, N, O, ngpus=1)       # one shard holds everything: forwarded
    one.set_data(f, f)
    s = gpu_solver_cls(M, N, O)
    s.set_data(f, f)
    kw = dict(df=df, dalpha=1.0, dw=dw, maxiter=30)
    assert _same(one.weighted_unrolled_jvp(0.07, w, **kw), s.weighted_unrolled_jvp(0.07, w, **kw))
    for a, b in zip(one.weighted_unrolled_gauss_newton(0.07, w, maxiter=30), s.weighted_unrolled_gauss_newton(0.07, w, maxiter=30)):
        assert _same(a, b)
    one.close()
    s.close()


def test_interleaved_calls_change_none_of_the_results(gpu_solver_cls):
    name = "3x40x48"
    O, N, M = SHAPES[name]
    f, gu, df = _data(name)
    w, dw = _weight(name, "mask")
    alpha, K = 0.08, 57

    def fresh(call):
        h = gpu_solver_cls(M, N, O)
        h.set_data(f, f)
        r = call(h)
        h.close()
        return r

    def sweep(h):
        return h.weighted_unrolled_jvp(alpha, w, df=df, dalpha=1.0, dw=dw, maxiter=K)
    u_plain = fresh(lambda h: h.weighted_denoise(alpha, w, maxiter=K))
    u_un, g_un = fresh(lambda h: (h.weighted_unrolled_denoise(alpha, w, maxiter=K), h.weighted_unrolled_vjp(alpha, w, gu, maxiter=K)))
    du_tv = fresh(lambda h: h.unrolled_jvp(alpha, df=df, dalpha=1.0, maxiter=K))
    du0 = fresh(sweep)
    assert _same(u_un, u_plain)
    for order in ("sweep first", "sweep last"):
        h = gpu_solver_cls(M, N, O)
        h.set_data(f, f)
        for rnd in range(2):   # the second round replays what the first one cached
            if order == "sweep first":
                assert _same(sweep(h), du0)
            assert _same(h.weighted_denoise(alpha, w, maxiter=K), u_plain)
            assert _same(h.weighted_unrolled_denoise(alpha, w, maxiter=K), u_un)
            assert _same(sweep(h), du0)   # between the taped solve and its reverse sweep
            assert _same(h.unrolled_jvp(alpha, df=df, dalpha=1.0, maxiter=K), du_tv)   # the TV sweep: planes and graphs of its own
            for a, b in zip(h.weighted_unrolled_vjp(alpha, w, gu, maxiter=K), g_un):
                assert _same(a, b)
            if order == "sweep last":
                assert _same(sweep(h), du0)
            assert _same(h.weighted_denoise(alpha, w, maxiter=K), u_plain)
        h.close()


# ---- 8. the Gauss-Newton model of the K-step loss -----------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["scalar", "patch"])
def test_gauss_newton_of_the_k_step_loss(gpu_solver_cls, kind):
    from conftest import synth_batch
    from bpldenoising_amd._lib import BpltvError
    name, K = "3x40x48", 50
    O, N, M = SHAPES[name]
    f, _, _ = _data(name)
    ub, f2 = synth_batch(O, N, M, seed=5 + M)
    assert _same(f2, f)
    w, _ = _weight(name, "mask")
    alpha = _alpha(kind, N, M)
    P = int(np.size(alpha))
    s = gpu_solver_cls(M, N, O)
    s.set_data(ub, f)
    cost, grad, H = s.weighted_unrolled_gauss_newton(alpha, w, maxiter=K)
    assert H.shape == (P, P) and _same(H, H.T)
    eye = np.eye(P).reshape((P,) + np.shape(alpha))
    J, u = s.weighted_unrolled_jvp(alpha, w, dalpha=eye if P > 1 else 1.0, want_u=True, maxiter=K)
    J = J.reshape(P, -1)
    H0 = J @ J.T
    dH = float(np.abs(H - H0).max())
    print("%s: max|H - J J^T| %.2e (bound %.2e)" % (kind, dH, 1e-11 * float(np.abs(H0).max())))
    assert dH <= 1e-11 * float(np.abs(H0).max())
    # the gradient against the reverse sweep, within the dL/dalpha bound of tests/test_gpu_weighted_unrolled.py
    assert _same(s.weighted_unrolled_denoise(alpha, w, maxiter=K), u)
    _, ga, _ = s.weighted_unrolled_vjp(alpha, w, u - ub, want_f=False, want_w=False, maxiter=K)
    amap = tw.alpha_to_map(alpha, M, N)
    u_t, tape, tab = wur.fwd_tape(f, amap, w, K)
    _, ga0, _ = wur.reverse(u_t - ub, tape, tab, amap, w, f)
    ba = 1e-11 * float(np.abs(ga0).max()) * O * ur.pixels_per_entry(alpha, M, N)
    dg = float(np.abs(np.asarray(grad) - np.asarray(ga)).max())
    print("%s: max|grad - reverse sweep| %.2e (bound %.2e)" % (kind, dg, ba))
    assert dg <= ba
    c0 = 0.5 * float(((u - ub) ** 2).sum())
    print("%s: cost %.15g numpy %.15g rel %.1e" % (kind, cost, c0, abs(cost - c0) / c0))
    assert cost == pytest.approx(c0, rel=1e-12, abs=0.0)
    for bad in (_alpha("map", N, M), np.full((1, 17), 0.08)):
        with pytest.raises(BpltvError) as e:
            s.weighted_unrolled_gauss_newton(bad, w, maxiter=K)
        assert e.value.code == E_UNSUPPORTED
    s.close()
