"""GPU checks of forward mode through the channel-coupled iterations (bpltv_color_unrolled_jvp, its device form and
bpltv_color_unrolled_gauss_newton).

The sweep's primal is tied to bpltv_color_denoise bit for bit, and channels = 1 to bpltv_unrolled_jvp; its tangent is held
against the numpy twin tests/color_jvp_ref.py (pinned on the CPU by tests/test_color_jvp_abi.py), against the reverse sweep
bpltv_color_unrolled_vjp by the transpose identity, against central differences of bpltv_color_denoise itself and, on identical
channels, against bpltv_unrolled_jvp; every plan (fusion depth, launch chains, graphs, host or device form, one direction or
several) gives the same bits; and a sweep, accepted or rejected, leaves the handle's last solve, colour tape and statistics as
they were."""
import ctypes as C

import numpy as np
import pytest
from conftest import synth_batch

import color_jvp_ref as cj
import color_ref as cr
from oracle import np_twin as tw

pytestmark = pytest.mark.gpu

E_ARG, E_NODATA, E_UNSUPPORTED = 1, 3, 6
_dp = C.POINTER(C.c_double)


def _same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b))


def _ptr(a):
    return a.ctypes.data_as(_dp) if a is not None else None


def _solver(cls, name):
    B, Cc, N, M = cr.SHAPES[name]
    f, gu = cr.gpu_data(name)
    s = cls(M, N, B * Cc)
    s.set_data(f, f)
    return s, f, gu


# ---- 1. the primal is bpltv_color_denoise's, bit for bit; one channel is bpltv_unrolled_jvp ------------------------------------
@pytest.mark.parametrize("kind", cr.KINDS)
@pytest.mark.parametrize("name", sorted(cr.SHAPES))
def test_primal_is_the_color_denoise_bitwise(gpu_solver_cls, name, kind):
    B, Cc, N, M = cr.SHAPES[name]
    s, f, _ = _solver(gpu_solver_cls, name)
    alpha = cr.alpha_of(kind, N, M)
    df, da, _ = cj.tangents(name, kind)
    for accel in (1, 0):
        for maxiter in (1, 7, 203):
            u0 = s.color_denoise(alpha, Cc, maxiter=maxiter, accel=accel)
            du, u1 = s.color_unrolled_jvp(alpha, Cc, df=df, dalpha=da, want_u=True, maxiter=maxiter, accel=accel)
            assert _same(u1, u0), (accel, maxiter, float(np.abs(u1 - u0).max()))
            assert np.isfinite(du).all() and du.any()
            assert s.stats()["adjoint_method"] == "color-unrolled-jvp" and s.stats()["adjoint_ms"] > 0.0
    s.close()


@pytest.mark.parametrize("kind", cr.KINDS)
@pytest.mark.parametrize("name", ["2x3x17x33", "1x3x40x48", "1x2x9x1", "1x4x1x9"])
def test_one_channel_is_the_unrolled_tv_jvp_bitwise(gpu_solver_cls, name, kind):
    B, Cc, N, M = cr.SHAPES[name]
    s, f, _ = _solver(gpu_solver_cls, name)
    alpha = cr.alpha_of(kind, N, M)
    df, da, _ = cj.tangents(name, kind)
    for K in cr.KS:
        du0, u0 = s.unrolled_jvp(alpha, df=df, dalpha=da, want_u=True, maxiter=K)
        du, u = s.color_unrolled_jvp(alpha, 1, df=df, dalpha=da, want_u=True, maxiter=K)
        assert s.stats()["adjoint_method"] == "color-unrolled-jvp"
        assert _same(du, du0) and _same(u, u0), (K, float(np.abs(du - du0).max()))
    s.close()


# ---- 2. the tangent against the twin -----------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", cr.KINDS)
@pytest.mark.parametrize("name", sorted(cr.SHAPES))
def test_tangent_matches_the_twin(gpu_solver_cls, name, kind):
    """1e-11 * max|du0| (DESIGN.md section 4.13 holds the measured maxima)."""
    B, Cc, N, M = cr.SHAPES[name]
    s, f, _ = _solver(gpu_solver_cls, name)
    alpha = cr.alpha_of(kind, N, M)
    df, da, _ = cj.tangents(name, kind)
    for K in (50, 203):
        for which in cj.WHICH:
            _, du0 = cj.twin_tangent(name, kind, K, which)
            du = s.color_unrolled_jvp(alpha, Cc, df=df if which != "dalpha" else None, dalpha=da if which != "df" else None, maxiter=K)
            d, m = float(np.abs(du - du0).max()), float(np.abs(du0).max())
            print("%s %s K %d %s: du %.2e (bound %.2e, max|ref| %.2e)" % (name, kind, K, which, d, 1e-11 * m, m))
            assert d <= 1e-11 * m
    s.close()


# ---- 3. the transpose identity against the reverse sweep ---------------------------------------------------------------
@pytest.mark.parametrize("kind", cr.KINDS)
@pytest.mark.parametrize("name", sorted(cr.SHAPES))
def test_tangent_is_the_transpose_of_the_reverse_sweep(gpu_solver_cls, name, kind):
    """<du, w> = <df, grad_f(w)> + <dalpha, grad_alpha(w)> to 1e-11 * sum|du * w|, all three calls on one handle."""
    B, Cc, N, M = cr.SHAPES[name]
    s, f, w = _solver(gpu_solver_cls, name)
    alpha = cr.alpha_of(kind, N, M)
    df, da, _ = cj.tangents(name, kind)
    for K in (50, 203):
        s.color_unrolled_denoise(alpha, Cc, maxiter=K)
        du = s.color_unrolled_jvp(alpha, Cc, df=df, dalpha=da, maxiter=K)
        gf, ga = s.color_unrolled_vjp(alpha, Cc, w, maxiter=K)
        lhs = float((du * w).sum())
        rhs = float((df * gf).sum()) + float((np.asarray(da) * np.asarray(ga)).sum())
        scale = float(np.abs(du * w).sum())
        print("%s %s K %d: |lhs - rhs| %.2e  bound %.2e" % (name, kind, K, abs(lhs - rhs), 1e-11 * scale))
        assert abs(lhs - rhs) <= 1e-11 * scale
    s.close()


# ---- 4. central differences of bpltv_color_denoise itself ---------------------------------------------------------------
@pytest.mark.parametrize("K", [30, 300])
def test_scalar_tangent_against_central_differences_on_the_device(gpu_solver_cls, K):
    """du/dalpha (dalpha = 1, df = 0), synth_batch(3, 24, 28, seed=9) as one colour image, alpha = 0.08, h = 1e-6, 1e-5 relative
    in the maximum norm: the direction and step at which the twin alone meets it (tests/test_color_jvp_abi.py)."""
    _, f = synth_batch(3, 24, 28, seed=9)
    alpha, h = 0.08, 1e-6
    s = gpu_solver_cls(28, 24, 3)
    s.set_data(f, f)
    du = s.color_unrolled_jvp(alpha, 3, dalpha=1.0, maxiter=K)
    fd = (s.color_denoise(alpha + h, 3, maxiter=K) - s.color_denoise(alpha - h, 3, maxiter=K)) / (2 * h)
    d, m = float(np.abs(du - fd).max()), float(np.abs(fd).max())
    print("K %d: max|du - fd| %.3e  max|fd| %.3e  rel %.2e" % (K, d, m, d / m))
    assert d <= 1e-5 * m
    s.close()


# ---- 5. identical channels are the TV tangent with alpha / sqrt(C) ---------------------------------------------------------
@pytest.mark.parametrize("Cc", [2, 3, 4])
def test_identical_channels_are_the_tv_tangent_with_alpha_over_sqrt_c(gpu_solver_cls, Cc):
    """C copies of each image and of its tangent: every channel of the colour tangent is bpltv_unrolled_jvp with alpha / sqrt(C)
    and dalpha / sqrt(C), to 1e-11 * max|ref|."""
    _, f1 = synth_batch(2, 17, 33, seed=38)
    rng = np.random.default_rng(39)
    df1 = rng.standard_normal(f1.shape)
    f, df = np.ascontiguousarray(np.repeat(f1, Cc, axis=0)), np.ascontiguousarray(np.repeat(df1, Cc, axis=0))
    s, t = gpu_solver_cls(33, 17, 2 * Cc), gpu_solver_cls(33, 17, 2)
    s.set_data(f, f)
    t.set_data(f1, f1)
    for alpha, da in ((0.08, 0.7), (cr.alpha_of("map", 17, 33), rng.standard_normal((17, 33)))):
        for K in cr.KS:
            du = s.color_unrolled_jvp(alpha, Cc, df=df, dalpha=da, maxiter=K)
            du1 = t.unrolled_jvp(alpha / np.sqrt(Cc), df=df1, dalpha=da / np.sqrt(Cc), maxiter=K)
            d, m = float(np.abs(du - np.repeat(du1, Cc, axis=0)).max()), float(np.abs(du1).max())
            print("C %d K %d: %.2e (bound %.2e)" % (Cc, K, d, 1e-11 * m))
            assert d <= 1e-11 * m
    s.close()
    t.close()


# ---- 6. every plan gives the same bits --------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["scalar", "map"])
@pytest.mark.parametrize("name", ["2x4x33x70", "2x3x17x33"])
def test_results_do_not_depend_on_the_plan(gpu_solver_cls, name, kind):
    import torch
    B, Cc, N, M = cr.SHAPES[name]
    O = B * Cc
    s, f, _ = _solver(gpu_solver_cls, name)
    alpha = cr.alpha_of(kind, N, M)
    a = np.atleast_1d(np.asarray(alpha, dtype=np.float64))
    an, am = (1, 1) if kind == "scalar" else a.shape
    rng = np.random.default_rng(21)
    df3 = rng.standard_normal((3,) + f.shape)
    da3 = rng.standard_normal((3,) + np.shape(alpha))
    for K in (203, 200):   # 200 iterations at depth 8: the second chain runs half a launch out of phase
        du0, u0 = s.color_unrolled_jvp(alpha, Cc, df=df3, dalpha=da3, want_u=True, maxiter=K)
        assert _same(u0, s.color_denoise(alpha, Cc, maxiter=K))
        for d in range(3):   # direction d of a call is the single call
            assert _same(s.color_unrolled_jvp(alpha, Cc, df=df3[d], dalpha=da3[d], maxiter=K), du0[d])
        plans = [dict(), dict(tile_iters=1), dict(tile_iters=3), dict(tile_iters=8), dict(chains=1), dict(chains=2),
                 dict(use_graph=0), dict(chains=2, use_graph=0), dict(tile_iters=3, chains=2)]
        for kw in plans:
            for rep in range(2):   # (the second call replays the cached graphs)
                du, u = s.color_unrolled_jvp(alpha, Cc, df=df3, dalpha=da3, want_u=True, maxiter=K, **kw)
                assert _same(du, du0) and _same(u, u0), (kw, rep)
        # one tangent at a time
        only_f = s.color_unrolled_jvp(alpha, Cc, df=df3[0], maxiter=K)
        only_a = s.color_unrolled_jvp(alpha, Cc, dalpha=da3[0], maxiter=K)
        assert _same(only_f, s.color_unrolled_jvp(alpha, Cc, df=df3[0], dalpha=np.zeros_like(da3[0]), maxiter=K))
        assert _same(only_a, s.color_unrolled_jvp(alpha, Cc, df=np.zeros_like(f), dalpha=da3[0], maxiter=K))
        # the device form
        at = torch.tensor(a, device="cuda")
        dft, dat = torch.tensor(df3, device="cuda"), torch.tensor(da3, device="cuda")
        dud = torch.empty(3, O, N, M, dtype=torch.float64, device="cuda")
        ud = torch.empty(O, N, M, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        for kw in (dict(), dict(), dict(chains=1, use_graph=0), dict(tile_iters=3, chains=2)):
            dud.zero_(); ud.zero_(); torch.cuda.synchronize()
            s.color_unrolled_jvp_device(Cc, at.data_ptr(), am, an, dft.data_ptr(), dat.data_ptr(), dud.data_ptr(), ud.data_ptr(),
                                        ndir=3, maxiter=K, **kw)
            assert _same(dud.cpu().numpy(), du0) and _same(ud.cpu().numpy(), u0), kw
        dud.zero_(); torch.cuda.synchronize()
        s.color_unrolled_jvp_device(Cc, at.data_ptr(), am, an, dft.data_ptr(), None, dud.data_ptr(), None, ndir=1, maxiter=K)
        assert _same(dud[0].cpu().numpy(), only_f)
        s.color_unrolled_jvp_device(Cc, at.data_ptr(), am, an, None, dat.data_ptr(), dud.data_ptr(), None, ndir=1, maxiter=K)
        assert _same(dud[0].cpu().numpy(), only_a)
    s.close()


# ---- 7. the Gauss-Newton model of the K-step loss -----------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["scalar", "patch"])
def test_gauss_newton_of_the_k_step_loss(gpu_solver_cls, kind):
    """cost against np_twin.l2_cost to 1e-13 relative; grad against color_unrolled_vjp(u - ubar) and H against the Gram matrix of
    the P columns of color_unrolled_jvp, each to 1e-11 * max|ref|."""
    from bpldenoising_amd._lib import BpltvError
    name, K = "2x3x17x33", 50
    B, Cc, N, M = cr.SHAPES[name]
    O = B * Cc
    ub, f = synth_batch(O, N, M, seed=5 + M)
    assert _same(f, cr.gpu_data(name)[0])
    alpha = cr.alpha_of(kind, N, M)
    P = int(np.size(alpha))
    s = gpu_solver_cls(M, N, O)
    s.set_data(ub, f)
    cost, grad, H = s.color_unrolled_gauss_newton(alpha, Cc, maxiter=K)
    assert s.stats()["adjoint_method"] == "color-unrolled-jvp"
    assert H.shape == (P, P) and _same(H, H.T)
    eye = np.eye(P).reshape((P,) + np.shape(alpha))
    J, u = s.color_unrolled_jvp(alpha, Cc, dalpha=eye if P > 1 else 1.0, want_u=True, maxiter=K)
    J = J.reshape(P, -1)
    H0 = J @ J.T
    dH, bH = float(np.abs(H - H0).max()), 1e-11 * float(np.abs(H0).max())
    print("%s: max|H - J^T J| %.2e (bound %.2e)" % (kind, dH, bH))
    assert dH <= bH
    assert _same(s.color_unrolled_denoise(alpha, Cc, maxiter=K), u)
    _, ga = s.color_unrolled_vjp(alpha, Cc, u - ub, want_f=False, maxiter=K)
    dg, bg = float(np.abs(np.asarray(grad) - np.asarray(ga)).max()), 1e-11 * float(np.abs(np.asarray(ga)).max())
    print("%s: max|grad - reverse sweep| %.2e (bound %.2e)" % (kind, dg, bg))
    assert dg <= bg
    c0 = tw.l2_cost(u, ub)
    print("%s: cost %.17g  l2_cost %.17g  rel %.2e" % (kind, cost, c0, abs(cost - c0) / c0))
    assert abs(cost - c0) <= 1e-13 * c0
    for bad in (cr.alpha_of("map", N, M), np.full((1, 17), 0.08)):
        with pytest.raises(BpltvError) as e:
            s.color_unrolled_gauss_newton(bad, Cc, maxiter=K)
        assert e.value.code == E_UNSUPPORTED
    s.close()


# ---- 8. the handle stays as it was --------------------------------------------------------------------------------------
def test_a_sweep_leaves_the_last_solve_the_tape_and_the_statistics(gpu_solver_cls):
    import torch
    name = "2x3x17x33"
    B, Cc, N, M = cr.SHAPES[name]
    O = B * Cc
    s, f, w = _solver(gpu_solver_cls, name)
    df, _, _ = cj.tangents(name, "scalar")
    amap = cr.alpha_of("map", N, M)
    s.color_unrolled_denoise(0.08, Cc, maxiter=20)
    gf0, ga0 = s.color_unrolled_vjp(0.08, Cc, w, maxiter=20)
    u0 = s.color_denoise(amap, Cc, maxiter=57)           # the last solve: another parameter, another shape
    st0 = s.stats()
    out = torch.empty(O, N, M, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    s.copy_u_device(out.data_ptr())
    ptr0 = s.u_device_ptr()
    du = s.color_unrolled_jvp(0.05, Cc, df=df, dalpha=1.0, maxiter=33)
    assert du.any()
    st1 = s.stats()
    assert st1["adjoint_method"] == "color-unrolled-jvp" and st1["adjoint_ms"] > 0.0
    for k in st0:
        if k not in ("adjoint_ms", "adjoint_method"):
            assert st1[k] == st0[k], (k, st0[k], st1[k])
    assert s.u_device_ptr() == ptr0
    out2 = torch.empty_like(out)
    torch.cuda.synchronize()
    s.copy_u_device(out2.data_ptr())
    assert _same(out2.cpu().numpy(), u0) and _same(out.cpu().numpy(), u0)
    gf, ga = s.color_unrolled_vjp(0.08, Cc, w, maxiter=20)   # the earlier colour tape
    assert _same(gf, gf0) and _same(ga, ga0)
    s.close()


# ---- 9. the contract ----------------------------------------------------------------------------------------------------
def test_rejections_leave_the_handle_as_it_was(gpu_solver_cls):
    import torch
    from bpldenoising_amd._lib import BpltvError
    name = "2x3x17x33"
    B, Cc, N, M = cr.SHAPES[name]
    O = B * Cc
    s, f, w = _solver(gpu_solver_cls, name)
    df, _, _ = cj.tangents(name, "scalar")
    amap = cr.alpha_of("map", N, M)
    s.color_unrolled_denoise(0.08, Cc, maxiter=20)
    gf0, ga0 = s.color_unrolled_vjp(0.08, Cc, w, maxiter=20)
    u0 = s.color_denoise(amap, Cc, maxiter=57)
    st0 = {k: v for k, v in s.stats().items() if k not in ("adjoint_ms", "adjoint_method")}
    ud = torch.empty(O, N, M, dtype=torch.float64, device="cuda")

    def unchanged():
        assert {k: v for k, v in s.stats().items() if k in st0} == st0
        s.copy_u_device(ud.data_ptr())
        assert _same(ud.cpu().numpy(), u0)

    def rejected(code, call, *a, **k):
        with pytest.raises(BpltvError) as e:
            call(*a, **k)
        assert e.value.code == code, (e.value.code, str(e.value))
        unchanged()

    for ch in (0, 5, 4):                       # outside 1 ... 4, or not dividing the handle's 6 planes
        rejected(E_ARG, s.color_unrolled_jvp, 0.08, ch, df=df, maxiter=20)
        rejected(E_ARG, s.color_unrolled_gauss_newton, 0.08, ch, maxiter=20)
    bad_df = df.copy(); bad_df[1, 3, 4] = np.inf
    nan_map = amap.copy(); nan_map[2, 5] = np.nan
    for bad in (float("nan"), -0.1, nan_map):
        rejected(E_ARG, s.color_unrolled_jvp, bad, Cc, df=df, maxiter=20)
        if np.ndim(bad) == 0:
            rejected(E_ARG, s.color_unrolled_gauss_newton, bad, Cc, maxiter=20)
    rejected(E_ARG, s.color_unrolled_jvp, 0.08, Cc, df=bad_df, maxiter=20)
    rejected(E_ARG, s.color_unrolled_jvp, 0.08, Cc, dalpha=float("nan"), maxiter=20)
    rejected(E_ARG, s.color_unrolled_jvp, 0.08, Cc, df=df, maxiter=0)
    rejected(E_ARG, s.color_unrolled_gauss_newton, 0.08, Cc, maxiter=0)
    for kw in (dict(rho=0.01), dict(init=1), dict(order=1)):
        rejected(E_UNSUPPORTED, s.color_unrolled_jvp, 0.08, Cc, df=df, maxiter=20, **kw)
        rejected(E_UNSUPPORTED, s.color_unrolled_gauss_newton, 0.08, Cc, maxiter=20, **kw)
    p = s.params(maxiter=20)
    a1 = np.array([0.08])
    du = np.empty_like(df)
    lib, h = s._lib, s._h
    assert lib.bpltv_color_unrolled_jvp(h, Cc, _ptr(a1), 1, 1, C.byref(p), 1, None, None, _ptr(du), None) == E_ARG      # both tangents NULL
    assert lib.bpltv_color_unrolled_jvp(h, Cc, _ptr(a1), 1, 1, C.byref(p), 0, _ptr(df), None, _ptr(du), None) == E_ARG  # ndir < 1
    assert lib.bpltv_color_unrolled_jvp(h, Cc, _ptr(a1), 1, 1, C.byref(p), 1, _ptr(df), None, None, None) == E_ARG      # no du_out
    assert lib.bpltv_color_unrolled_jvp(h, Cc, _ptr(a1), M + 1, 1, C.byref(p), 1, _ptr(df), None, _ptr(du), None) == E_ARG   # shape
    assert lib.bpltv_color_unrolled_jvp(h, Cc, _ptr(a1), 0, 1, C.byref(p), 1, _ptr(df), None, _ptr(du), None) == E_ARG
    unchanged()
    # the device form
    good = torch.tensor([0.08], dtype=torch.float64, device="cuda")
    dft, dud = torch.tensor(df, device="cuda"), torch.empty(O, N, M, dtype=torch.float64, device="cuda")
    bdt = torch.tensor(bad_df, device="cuda")
    bda = torch.tensor([float("inf")], dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    for bad in (float("nan"), -0.1):
        bt = torch.tensor([bad], dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        rejected(E_ARG, s.color_unrolled_jvp_device, Cc, bt.data_ptr(), 1, 1, dft.data_ptr(), None, dud.data_ptr(), maxiter=20)
    rejected(E_ARG, s.color_unrolled_jvp_device, Cc, good.data_ptr(), 1, 1, bdt.data_ptr(), None, dud.data_ptr(), maxiter=20)
    rejected(E_ARG, s.color_unrolled_jvp_device, Cc, good.data_ptr(), 1, 1, dft.data_ptr(), bda.data_ptr(), dud.data_ptr(), maxiter=20)
    rejected(E_ARG, s.color_unrolled_jvp_device, Cc, good.data_ptr(), 1, 1, None, None, dud.data_ptr(), maxiter=20)
    rejected(E_ARG, s.color_unrolled_jvp_device, Cc, good.data_ptr(), 1, 1, dft.data_ptr(), None, dud.data_ptr(), ndir=0, maxiter=20)
    rejected(E_ARG, s.color_unrolled_jvp_device, 5, good.data_ptr(), 1, 1, dft.data_ptr(), None, dud.data_ptr(), maxiter=20)
    gf, ga = s.color_unrolled_vjp(0.08, Cc, w, maxiter=20)      # the colour tape is still the first solve's
    assert _same(gf, gf0) and _same(ga, ga0)
    n = gpu_solver_cls(M, N, O)                # no dataset
    with pytest.raises(BpltvError) as e:
        n.color_unrolled_jvp(0.08, Cc, df=df, maxiter=5)
    assert e.value.code == E_NODATA
    with pytest.raises(BpltvError) as e:
        n.color_unrolled_gauss_newton(0.08, Cc, maxiter=5)
    assert e.value.code == E_NODATA
    n.close()
    s.close()


def test_two_shards_are_unsupported(gpu_solver_cls):
    import torch
    from bpldenoising_amd._lib import BpltvError
    name = "2x3x17x33"
    B, Cc, N, M = cr.SHAPES[name]
    f, _ = cr.gpu_data(name)
    df, _, _ = cj.tangents(name, "scalar")
    m = gpu_solver_cls(M, N, B * Cc, devices=[0, 0])
    m.set_data(f, f)
    u0 = m.denoise(0.07, maxiter=30)
    for call, args, kw in ((m.color_unrolled_jvp, (0.07, Cc), dict(df=df)), (m.color_unrolled_gauss_newton, (0.07, Cc), dict()),
                           (m.color_unrolled_jvp_device, (Cc, 1, 1, 1, 1, 1, 1), dict())):
        with pytest.raises(BpltvError) as e:     # (the device form is refused before any pointer is read)
            call(*args, maxiter=30, **kw)
        assert e.value.code == E_UNSUPPORTED
        assert _same(m.denoise(0.07, maxiter=30), u0)
    m.close()
    one = gpu_solver_cls(M, N, B * Cc, ngpus=1)       # one shard holds everything: forwarded
    one.set_data(f, f)
    s = gpu_solver_cls(M, N, B * Cc)
    s.set_data(f, f)
    assert _same(one.color_unrolled_jvp(0.07, Cc, df=df, dalpha=1.0, maxiter=30), s.color_unrolled_jvp(0.07, Cc, df=df, dalpha=1.0, maxiter=30))
    # the forwarding handle leaves "channels divides O" to its shard: 4 on 6 planes is refused there, nothing changed
    u1 = one.color_denoise(0.07, Cc, maxiter=30)
    st1 = {k: v for k, v in one.stats().items() if k not in ("adjoint_ms", "adjoint_method")}
    ud = torch.empty(B * Cc, N, M, dtype=torch.float64, device="cuda")
    dft = torch.tensor(df, device="cuda")
    a = torch.tensor([0.07], dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    for call, args, kw in ((one.color_unrolled_jvp, (0.07, 4), dict(df=df)), (one.color_unrolled_gauss_newton, (0.07, 4), dict()),
                           (one.color_unrolled_jvp_device, (4, a.data_ptr(), 1, 1, dft.data_ptr(), None, ud.data_ptr()), dict())):
        with pytest.raises(BpltvError) as e:
            call(*args, maxiter=30, **kw)
        assert e.value.code == E_ARG, (e.value.code, str(e.value))
        assert {k: v for k, v in one.stats().items() if k in st1} == st1
        one.copy_u_device(ud.data_ptr())
        assert _same(ud.cpu().numpy(), u1)
    one.close()
    s.close()
