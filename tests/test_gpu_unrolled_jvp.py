"""GPU checks of forward mode through the PDHG iterations (bpltv_unrolled_jvp, its device form and
bpltv_unrolled_gauss_newton).

The sweep's primal is tied to bpltv_denoise bit for bit, which pins the kernel's primal half to the oracle; its tangent is held
against the numpy twin tests/unrolled_jvp_ref.py (pinned on the CPU by tests/test_unrolled_jvp_abi.py), against the reverse
sweep bpltv_unrolled_vjp by the transpose identity, and against central differences of bpltv_denoise itself; every plan
(fusion depth, launch chains, graphs, host or device form, one direction or several) gives the same bits; and a sweep,
accepted or rejected, leaves the handle's last solve, tape and statistics as they were."""
import ctypes as C
import functools

import numpy as np
import pytest
from conftest import synth_batch

import unrolled_jvp_ref as uj
import unrolled_ref as ur
from oracle import np_twin as tw

pytestmark = pytest.mark.gpu

E_ARG, E_NODATA, E_UNSUPPORTED = 1, 3, 6
_dp = C.POINTER(C.c_double)
SHAPES = {"3x40x48": (3, 40, 48), "2x17x33": (2, 17, 33), "1x1x9": (1, 1, 9), "1x9x1": (1, 9, 1), "2x70x72": (2, 70, 72)}


def _alpha(kind, N, M):
    """scalar, a 2 x 3 patch (cut down where the image has a single row / column), or a map."""
    if kind == "scalar":
        return 0.08
    if kind == "patch":
        return np.array([[0.05, 0.1, 0.07], [0.12, 0.06, 0.09]])[:min(2, N), :min(3, M)].copy()
    return 0.05 + 0.1 * np.random.default_rng(8).random((N, M))


def _same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b))


def _ptr(a):
    return a.ctypes.data_as(_dp) if a is not None else None


@functools.lru_cache(maxsize=None)
def _data(name, seed=5):
    """(ubar, f, cotangent w, tangent df) of a shape; read-only."""
    O, N, M = SHAPES[name]
    ub, f = synth_batch(O, N, M, seed=seed + M)
    rng = np.random.default_rng(seed + 300)
    w, df = rng.standard_normal(f.shape), rng.standard_normal(f.shape)
    for a in (ub, f, w, df):
        a.setflags(write=False)
    return ub, f, w, df


def _dalpha(alpha, seed=11):
    """A standard-normal tangent in the type / shape of alpha."""
    g = np.random.default_rng(seed).standard_normal(np.shape(alpha))
    return float(g) if np.ndim(alpha) == 0 else g


def _damap(dalpha, M, N):
    return np.full((N, M), dalpha) if np.ndim(dalpha) == 0 else tw.alpha_to_map(dalpha, M, N)


# ---- 1. the primal is bpltv_denoise's, bit for bit --------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["scalar", "patch", "map"])
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_primal_is_the_plain_denoise_bitwise(gpu_solver_cls, name, kind):
    O, N, M = SHAPES[name]
    _, f, _, df = _data(name)
    alpha = _alpha(kind, N, M)
    s = gpu_solver_cls(M, N, O)
    s.set_data(f, f)
    for accel in (1, 0):
        for maxiter in (1, 7, 203):
            u0 = s.denoise(alpha, maxiter=maxiter, accel=accel)
            du, u1 = s.unrolled_jvp(alpha, df=df, dalpha=_dalpha(alpha), want_u=True, maxiter=maxiter, accel=accel)
            assert _same(u1, u0), (accel, maxiter, float(np.abs(u1 - u0).max()))
            assert np.isfinite(du).all() and du.any()
            assert s.stats()["adjoint_method"] == "unrolled-jvp" and s.stats()["adjoint_ms"] > 0.0
    s.close()


# ---- 2. the tangent against the twin -----------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["scalar", "patch", "map"])
@pytest.mark.parametrize("name", ["3x40x48", "2x17x33", "1x1x9", "1x9x1"])
def test_tangent_matches_the_twin(gpu_solver_cls, name, kind):
    """1e-11 * max|ref| (DESIGN.md section 4.7 holds the measured maxima)."""
    O, N, M = SHAPES[name]
    _, f, _, df = _data(name)
    alpha = _alpha(kind, N, M)
    amap = tw.alpha_to_map(alpha, M, N)
    da = _dalpha(alpha)
    dam = _damap(da, M, N)
    s = gpu_solver_cls(M, N, O)
    s.set_data(f, f)
    for K in (50, 203):
        for tf, ta, tam in ((df, None, None), (None, da, dam), (df, da, dam)):
            _, du0 = uj.forward_tangent(f, amap, K, tf, tam)
            du = s.unrolled_jvp(alpha, df=tf, dalpha=ta, maxiter=K)
            d, b = float(np.abs(du - du0).max()), 1e-11 * float(np.abs(du0).max())
            print("%s %s K %d df %d dalpha %d: du %.2e (bound %.2e, max|ref| %.2e)"
                  % (name, kind, K, tf is not None, ta is not None, d, b, float(np.abs(du0).max())))
            assert d <= b
    s.close()


# ---- 3. the transpose identity against the reverse sweep ---------------------------------------------------------------
@pytest.mark.parametrize("kind", ["scalar", "patch", "map"])
@pytest.mark.parametrize("name", ["3x40x48", "2x17x33", "1x1x9", "1x9x1"])
def test_tangent_is_the_transpose_of_the_reverse_sweep(gpu_solver_cls, name, kind):
    """<du, w> = <df, grad_f(w)> + <dalpha, grad_alpha(w)> to 1e-11 * sum|du * w|, all three calls on one handle."""
    O, N, M = SHAPES[name]
    _, f, w, df = _data(name)
    alpha = _alpha(kind, N, M)
    da = _dalpha(alpha)
    s = gpu_solver_cls(M, N, O)
    s.set_data(f, f)
    for K in (50, 203):
        s.unrolled_denoise(alpha, maxiter=K)
        du = s.unrolled_jvp(alpha, df=df, dalpha=da, maxiter=K)
        gf, ga = s.unrolled_vjp(alpha, w, maxiter=K)
        lhs = float((du * w).sum())
        rhs = float((df * gf).sum()) + float((np.asarray(da) * np.asarray(ga)).sum())
        scale = float(np.abs(du * w).sum())
        print("%s %s K %d: |lhs - rhs| %.2e  bound %.2e" % (name, kind, K, abs(lhs - rhs), 1e-11 * scale))
        assert abs(lhs - rhs) <= 1e-11 * scale
    s.close()


# ---- 4. central differences of bpltv_denoise itself ---------------------------------------------------------------------
@pytest.mark.parametrize("K", [30, 300])
def test_scalar_tangent_against_central_differences_on_the_device(gpu_solver_cls, K):
    """du/dalpha (dalpha = 1, df = 0), 1 x 24 x 28, alpha = 0.08, h = 1e-6, 1e-5 relative in the maximum norm: the direction and
    step at which the twin alone meets it (tests/test_unrolled_jvp_abi.py)."""
    _, f = synth_batch(1, 24, 28, seed=9)
    alpha, h = 0.08, 1e-6
    s = gpu_solver_cls(28, 24, 1)
    s.set_data(f, f)
    du = s.unrolled_jvp(alpha, dalpha=1.0, maxiter=K)
    fd = (s.denoise(alpha + h, maxiter=K) - s.denoise(alpha - h, maxiter=K)) / (2 * h)
    d, m = float(np.abs(du - fd).max()), float(np.abs(fd).max())
    print("K %d: max|du - fd| %.3e  max|fd| %.3e  rel %.2e" % (K, d, m, d / m))
    assert d <= 1e-5 * m
    s.close()


# ---- 5. every plan gives the same bits --------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["scalar", "map"])
def test_results_do_not_depend_on_the_plan(gpu_solver_cls, kind):
    import torch
    name = "2x70x72"
    O, N, M = SHAPES[name]
    _, f, _, df = _data(name)
    alpha = _alpha(kind, N, M)
    a = np.atleast_1d(np.asarray(alpha, dtype=np.float64))
    an, am = (1, 1) if kind == "scalar" else a.shape
    rng = np.random.default_rng(21)
    df3 = rng.standard_normal((3,) + f.shape)
    da3 = rng.standard_normal((3,) + np.shape(alpha))
    s = gpu_solver_cls(M, N, O)
    s.set_data(f, f)
    for K in (203, 200):   # 200 iterations at depth 8: the second chain runs half a launch out of phase
        du0, u0 = s.unrolled_jvp(alpha, df=df3, dalpha=da3, want_u=True, maxiter=K)
        assert _same(u0, s.denoise(alpha, maxiter=K))
        for d in range(3):   # direction d of a call is the single call
            assert _same(s.unrolled_jvp(alpha, df=df3[d], dalpha=da3[d], maxiter=K), du0[d])
        plans = [dict(), dict(tile_iters=1), dict(tile_iters=3), dict(tile_iters=8), dict(chains=1), dict(chains=2),
                 dict(use_graph=0), dict(chains=2, use_graph=0), dict(tile_iters=3, chains=2)]
        for kw in plans:
            for rep in range(2):   # (the second call replays the cached graphs)
                du, u = s.unrolled_jvp(alpha, df=df3, dalpha=da3, want_u=True, maxiter=K, **kw)
                assert _same(du, du0) and _same(u, u0), (kw, rep)
        # one tangent at a time
        only_f = s.unrolled_jvp(alpha, df=df3[0], maxiter=K)
        only_a = s.unrolled_jvp(alpha, dalpha=da3[0], maxiter=K)
        assert _same(only_f, s.unrolled_jvp(alpha, df=df3[0], dalpha=np.zeros_like(da3[0]), maxiter=K))
        assert _same(only_a, s.unrolled_jvp(alpha, df=np.zeros_like(f), dalpha=da3[0], maxiter=K))
        # the device form
        at = torch.tensor(a, device="cuda")
        dft, dat = torch.tensor(df3, device="cuda"), torch.tensor(da3, device="cuda")
        dud = torch.empty(3, O, N, M, dtype=torch.float64, device="cuda")
        ud = torch.empty(O, N, M, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        for kw in (dict(), dict(), dict(chains=1, use_graph=0), dict(tile_iters=3, chains=2)):
            dud.zero_(); ud.zero_(); torch.cuda.synchronize()
            s.unrolled_jvp_device(at.data_ptr(), am, an, dft.data_ptr(), dat.data_ptr(), dud.data_ptr(), ud.data_ptr(), ndir=3,
                                  maxiter=K, **kw)
            assert _same(dud.cpu().numpy(), du0) and _same(ud.cpu().numpy(), u0), kw
        dud.zero_(); torch.cuda.synchronize()
        s.unrolled_jvp_device(at.data_ptr(), am, an, dft.data_ptr(), None, dud.data_ptr(), None, ndir=1, maxiter=K)
        assert _same(dud[0].cpu().numpy(), only_f)
        s.unrolled_jvp_device(at.data_ptr(), am, an, None, dat.data_ptr(), dud.data_ptr(), None, ndir=1, maxiter=K)
        assert _same(dud[0].cpu().numpy(), only_a)
    s.close()


# ---- 6. the handle stays as it was --------------------------------------------------------------------------------------
def test_a_sweep_leaves_the_last_solve_the_tape_and_the_statistics(gpu_solver_cls):
    import torch
    name = "2x17x33"
    O, N, M = SHAPES[name]
    _, f, w, df = _data(name)
    s = gpu_solver_cls(M, N, O)
    s.set_data(f, f)
    amap = _alpha("map", N, M)
    s.unrolled_denoise(0.08, maxiter=20)
    gf0, ga0 = s.unrolled_vjp(0.08, w, maxiter=20)
    u0 = s.denoise(amap, maxiter=57)           # the last solve: another parameter, another shape
    gap0 = s.duality_gap()
    st0 = s.stats()
    out = torch.empty(O, N, M, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    s.copy_u_device(out.data_ptr())
    ptr0 = s.u_device_ptr()
    du = s.unrolled_jvp(0.05, df=df, dalpha=1.0, maxiter=33)
    assert du.any()
    st1 = s.stats()
    assert st1["adjoint_method"] == "unrolled-jvp" and st1["adjoint_ms"] > 0.0
    for k in st0:
        if k not in ("adjoint_ms", "adjoint_method"):
            assert st1[k] == st0[k], (k, st0[k], st1[k])
    assert s.u_device_ptr() == ptr0
    out2 = torch.empty_like(out)
    torch.cuda.synchronize()
    s.copy_u_device(out2.data_ptr())
    assert _same(out2.cpu().numpy(), u0) and _same(out.cpu().numpy(), u0)
    assert _same(s.duality_gap(), gap0)
    gf, ga = s.unrolled_vjp(0.08, w, maxiter=20)   # the earlier tape
    assert _same(gf, gf0) and _same(ga, ga0)
    s.close()


def test_rejections_leave_the_handle_as_it_was(gpu_solver_cls):
    import torch
    from bpldenoising_amd._lib import BpltvError
    name = "2x17x33"
    O, N, M = SHAPES[name]
    _, f, w, df = _data(name)
    s = gpu_solver_cls(M, N, O)
    s.set_data(f, f)
    amap = _alpha("map", N, M)
    u0 = s.denoise(amap, maxiter=57)
    gap0 = s.duality_gap()

    def unchanged():
        assert _same(s.duality_gap(), gap0)
        assert _same(s.denoise(amap, maxiter=57), u0) and _same(s.duality_gap(), gap0)

    def rejected(code, call, *a, **k):
        with pytest.raises(BpltvError) as e:
            call(*a, **k)
        assert e.value.code == code, (e.value.code, str(e.value))
        unchanged()

    bad_df = df.copy(); bad_df[1, 3, 4] = np.inf
    nan_map = amap.copy(); nan_map[2, 5] = np.nan
    for bad in (float("nan"), -0.1, nan_map):
        rejected(E_ARG, s.unrolled_jvp, bad, df=df, maxiter=20)
        if np.ndim(bad) == 0:
            rejected(E_ARG, s.unrolled_gauss_newton, bad, maxiter=20)
    rejected(E_ARG, s.unrolled_jvp, 0.08, df=bad_df, maxiter=20)
    rejected(E_ARG, s.unrolled_jvp, 0.08, dalpha=float("nan"), maxiter=20)
    rejected(E_ARG, s.unrolled_jvp, 0.08, df=df, maxiter=0)
    rejected(E_ARG, s.unrolled_gauss_newton, 0.08, maxiter=0)
    for kw in (dict(rho=0.01), dict(init=1), dict(order=1)):
        rejected(E_UNSUPPORTED, s.unrolled_jvp, 0.08, df=df, maxiter=20, **kw)
        rejected(E_UNSUPPORTED, s.unrolled_gauss_newton, 0.08, maxiter=20, **kw)
    p = s.params(maxiter=20)
    a1 = np.array([0.08])
    du = np.empty_like(df)
    lib, h = s._lib, s._h
    assert lib.bpltv_unrolled_jvp(h, _ptr(a1), 1, 1, C.byref(p), 1, None, None, _ptr(du), None) == E_ARG      # both tangents NULL
    assert lib.bpltv_unrolled_jvp(h, _ptr(a1), 1, 1, C.byref(p), 0, _ptr(df), None, _ptr(du), None) == E_ARG  # ndir < 1
    assert lib.bpltv_unrolled_jvp(h, _ptr(a1), 1, 1, C.byref(p), 1, _ptr(df), None, None, None) == E_ARG      # no du_out
    assert lib.bpltv_unrolled_jvp(h, _ptr(a1), M + 1, 1, C.byref(p), 1, _ptr(df), None, _ptr(du), None) == E_ARG   # shape
    assert lib.bpltv_unrolled_jvp(h, _ptr(a1), 0, 1, C.byref(p), 1, _ptr(df), None, _ptr(du), None) == E_ARG
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
        rejected(E_ARG, s.unrolled_jvp_device, bt.data_ptr(), 1, 1, dft.data_ptr(), None, dud.data_ptr(), maxiter=20)
    rejected(E_ARG, s.unrolled_jvp_device, good.data_ptr(), 1, 1, bdt.data_ptr(), None, dud.data_ptr(), maxiter=20)
    rejected(E_ARG, s.unrolled_jvp_device, good.data_ptr(), 1, 1, dft.data_ptr(), bda.data_ptr(), dud.data_ptr(), maxiter=20)
    rejected(E_ARG, s.unrolled_jvp_device, good.data_ptr(), 1, 1, None, None, dud.data_ptr(), maxiter=20)
    rejected(E_ARG, s.unrolled_jvp_device, good.data_ptr(), 1, 1, dft.data_ptr(), None, dud.data_ptr(), ndir=0, maxiter=20)
    n = gpu_solver_cls(M, N, O)                # no dataset
    with pytest.raises(BpltvError) as e:
        n.unrolled_jvp(0.08, df=df, maxiter=5)
    assert e.value.code == E_NODATA
    with pytest.raises(BpltvError) as e:
        n.unrolled_gauss_newton(0.08, maxiter=5)
    assert e.value.code == E_NODATA
    n.close()
    s.close()


def test_two_shards_are_unsupported(gpu_solver_cls):
    from bpldenoising_amd._lib import BpltvError
    name = "2x17x33"
    O, N, M = SHAPES[name]
    _, f, _, df = _data(name)
    m = gpu_solver_cls(M, N, O, devices=[0, 0])
    m.set_data(f, f)
    u0 = m.denoise(0.07, maxiter=30)
    gap0 = m.duality_gap()
    for call, args, kw in ((m.unrolled_jvp, (0.07,), dict(df=df)), (m.unrolled_gauss_newton, (0.07,), dict()),
                           (m.unrolled_jvp_device, (1, 1, 1, 1, 1, 1), dict())):
        with pytest.raises(BpltvError) as e:     # (the device form is refused before any pointer is read)
            call(*args, maxiter=30, **kw)
        assert e.value.code == E_UNSUPPORTED
        assert _same(m.duality_gap(), gap0) and _same(m.denoise(0.07, maxiter=30), u0)
    m.close()
    one = gpu_solver_cls(M, N, O, ngpus=1)       # one shard holds everything: forwarded
    one.set_data(f, f)
    s = gpu_solver_cls(M, N, O)
    s.set_data(f, f)
    assert _same(one.unrolled_jvp(0.07, df=df, dalpha=1.0, maxiter=30), s.unrolled_jvp(0.07, df=df, dalpha=1.0, maxiter=30))
    one.close()
    s.close()


def test_interleaved_calls_change_none_of_the_results(gpu_solver_cls):
    name = "3x40x48"
    O, N, M = SHAPES[name]
    _, f, w, df = _data(name)
    alpha, K = 0.08, 57

    def fresh(call):
        h = gpu_solver_cls(M, N, O)
        h.set_data(f, f)
        r = call(h)
        h.close()
        return r
    u_plain = fresh(lambda h: h.denoise(alpha, maxiter=K))
    u_un, g_un = fresh(lambda h: (h.unrolled_denoise(alpha, maxiter=K), h.unrolled_vjp(alpha, w, maxiter=K)))
    du0 = fresh(lambda h: h.unrolled_jvp(alpha, df=df, dalpha=1.0, maxiter=K))
    assert _same(u_un, u_plain)
    for order in ("sweep first", "sweep last"):
        h = gpu_solver_cls(M, N, O)
        h.set_data(f, f)
        for rnd in range(2):   # the second round replays what the first one cached
            if order == "sweep first":
                assert _same(h.unrolled_jvp(alpha, df=df, dalpha=1.0, maxiter=K), du0)
            assert _same(h.denoise(alpha, maxiter=K), u_plain)
            assert _same(h.unrolled_denoise(alpha, maxiter=K), u_un)
            assert _same(h.unrolled_jvp(alpha, df=df, dalpha=1.0, maxiter=K), du0)   # between the taped solve and its reverse sweep
            gf, ga = h.unrolled_vjp(alpha, w, maxiter=K)
            assert _same(gf, g_un[0]) and _same(ga, g_un[1])
            if order == "sweep last":
                assert _same(h.unrolled_jvp(alpha, df=df, dalpha=1.0, maxiter=K), du0)
            assert _same(h.denoise(alpha, maxiter=K), u_plain)
        h.close()


# ---- 7. the Gauss-Newton model of the K-step loss -----------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["scalar", "patch"])
def test_gauss_newton_of_the_k_step_loss(gpu_solver_cls, kind):
    from bpldenoising_amd._lib import BpltvError
    name, K = "3x40x48", 50
    O, N, M = SHAPES[name]
    ub, f, _, _ = _data(name)
    alpha = _alpha(kind, N, M)
    P = int(np.size(alpha))
    s = gpu_solver_cls(M, N, O)
    s.set_data(ub, f)
    cost, grad, H = s.unrolled_gauss_newton(alpha, maxiter=K)
    assert H.shape == (P, P) and _same(H, H.T)
    eye = np.eye(P).reshape((P,) + np.shape(alpha))
    J, u = s.unrolled_jvp(alpha, dalpha=eye if P > 1 else 1.0, want_u=True, maxiter=K)
    J = J.reshape(P, -1)
    H0 = J @ J.T
    dH = float(np.abs(H - H0).max())
    print("%s: max|H - J^T J| %.2e (bound %.2e)" % (kind, dH, 1e-11 * float(np.abs(H0).max())))
    assert dH <= 1e-11 * float(np.abs(H0).max())
    # the gradient against the reverse sweep, within the dL/dalpha bound of tests/test_gpu_unrolled.py
    assert _same(s.unrolled_denoise(alpha, maxiter=K), u)
    _, ga = s.unrolled_vjp(alpha, u - ub, want_f=False, maxiter=K)
    amap = tw.alpha_to_map(alpha, M, N)
    u_t, tape, tab = ur.fwd_tape(f, amap, K)
    _, ga0 = ur.reverse(u_t - ub, tape, tab, amap)
    ba = 1e-11 * float(np.abs(ga0).max()) * O * ur.pixels_per_entry(alpha, M, N)
    dg = float(np.abs(np.asarray(grad) - np.asarray(ga)).max())
    print("%s: max|grad - reverse sweep| %.2e (bound %.2e)" % (kind, dg, ba))
    assert dg <= ba
    _, c0, _ = s.evaluate(alpha, 0.1, maxiter=K)   # bpltv_evaluate's cost reduction on the same u
    assert cost == pytest.approx(c0, rel=1e-13, abs=0.0)
    for bad in (_alpha("map", N, M), np.full((1, 17), 0.08)):
        with pytest.raises(BpltvError) as e:
            s.unrolled_gauss_newton(bad, maxiter=K)
        assert e.value.code == E_UNSUPPORTED
    s.close()
