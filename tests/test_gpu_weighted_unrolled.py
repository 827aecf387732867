"""GPU checks of reverse mode through the iterations of the weighted model (bpltv_weighted_unrolled_denoise /
bpltv_weighted_unrolled_vjp and their device forms).

u is tied to bpltv_weighted_denoise bit for bit, for real weights, masks and w == 1; the three gradients are held against the
numpy twin tests/weighted_unrolled_ref.py (pinned on the CPU by tests/test_weighted_unrolled_abi.py), against
bpltv_unrolled_vjp for w == 1 and against central differences of bpltv_weighted_denoise itself; every plan (fusion depth,
launch chains, graphs, host or device form, whose tape) gives the same bits; and a rejected call leaves the handle as it was."""
import ctypes as C
import functools

import numpy as np
import pytest
from conftest import synth_batch

import unrolled_ref as ur
import weighted_unrolled_ref as wur
from oracle import np_twin as tw

pytestmark = pytest.mark.gpu

E_ARG, E_NODATA, E_UNSUPPORTED = 1, 3, 6
_dp = C.POINTER(C.c_double)
SHAPES = wur.GPU_SHAPES
_alpha = wur.alpha_of


def _same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b))


def _ptr(a):
    return a.ctypes.data_as(_dp) if a is not None else None


@functools.lru_cache(maxsize=None)
def _data(name):
    f, gu = wur.gpu_data(name)
    for a in (f, gu):
        a.setflags(write=False)
    return f, gu


@functools.lru_cache(maxsize=None)
def _weight(name, wkind):
    w = wur.weight_of(wkind, *SHAPES[name])
    w.setflags(write=False)
    return w


# ---- 1. u is bpltv_weighted_denoise's, bit for bit ----------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["scalar", "patch", "map"])
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_u_is_the_weighted_denoise_bitwise(gpu_solver_cls, name, kind):
    from bpldenoising_amd._lib import BpltvError
    O, N, M = SHAPES[name]
    f, _ = _data(name)
    alpha = _alpha(kind, N, M)
    s = gpu_solver_cls(M, N, O)
    s.set_data(f, f)
    for wkind in ("real", "mask", "ones"):
        w = _weight(name, wkind)
        for maxiter in (1, 7, 203):
            by_accel = {}
            for accel in (1, 0):
                u0 = s.weighted_denoise(alpha, w, maxiter=maxiter, accel=accel)
                g0 = s.duality_gap() if w.min() > 0 else None
                u1 = s.weighted_unrolled_denoise(alpha, w, maxiter=maxiter, accel=accel)
                assert _same(u1, u0), (wkind, accel, maxiter, float(np.abs(u1 - u0).max()))
                st = s.stats()
                assert st["iterations"] == maxiter and st["pdhg_variant"] == 0 and st["launches"] >= 1 and st["tiles"] >= O, st
                assert st["bytes_per_px_iter"] == (96.0 if kind == "map" and N * M > 1 else 88.0)
                assert s.weighted_unrolled_tape_doubles(maxiter=maxiter) == 3 * maxiter * M * N * O
                # the solve is the handle's last weighted solve: its gap is the weighted solve's, bit for bit
                if g0 is not None:
                    assert _same(s.duality_gap(), g0)
                else:
                    with pytest.raises(BpltvError) as e:
                        s.duality_gap()
                    assert e.value.code == E_UNSUPPORTED
                if wkind == "ones":
                    assert _same(u1, s.denoise(alpha, maxiter=maxiter, accel=accel))
                by_accel[accel] = u1
            if wkind == "mask":   # gamma = 0: omega == 1 with or without the acceleration
                assert _same(by_accel[1], by_accel[0])
    s.close()


# ---- 2. the gradients against the twin --------------------------------------------------------------------------------
def _bounds(gf0, ga0, gw0, alpha, w, O, N, M):
    """1e-11 * max|ref| for grad_f; for grad_alpha relative to the largest per-pixel term of the reference times the number
    of terms summed into one entry (tests/test_gpu_unrolled.py's _bounds); for grad_w 1e-11 * max|ref|, times O where the
    images are summed into one plane."""
    return (1e-11 * float(np.abs(gf0).max()), 1e-11 * float(np.abs(ga0).max()) * O * ur.pixels_per_entry(alpha, M, N),
            1e-11 * float(np.abs(gw0).max()) * (O if np.ndim(w) == 2 else 1))


@pytest.mark.parametrize("wkind", ["real", "mask"])
@pytest.mark.parametrize("kind", ["scalar", "patch", "map"])
@pytest.mark.parametrize("name", wur.GRADIENT_SHAPES)
def test_gradients_match_the_twin(gpu_solver_cls, name, kind, wkind):
    """Measured on MI355X: see the table there."""
    O, N, M = SHAPES[name]
    f, gu = _data(name)
    alpha = _alpha(kind, N, M)
    w = _weight(name, wkind)
    amap = tw.alpha_to_map(alpha, M, N)
    s = gpu_solver_cls(M, N, O)
    s.set_data(f, f)
    for K in wur.GRADIENT_K:
        u0, tape, tab = wur.fwd_tape(f, amap, w, K)
        gf0, ga0, gw0 = wur.reverse(gu, tape, tab, amap, w, f)
        u = s.weighted_unrolled_denoise(alpha, w, maxiter=K)
        st0 = s.stats()
        gf, ga, gw = s.weighted_unrolled_vjp(alpha, w, gu, maxiter=K)
        st = s.stats()
        assert st["adjoint_method"] == "weighted-unrolled" and st["adjoint_ms"] > 0.0 and st["iterations"] == K, st
        changed = {k for k in st if st[k] != st0[k]}
        assert changed <= {"adjoint_ms", "adjoint_method"}, changed
        bf, ba, bw = _bounds(gf0, ga0, gw0, alpha, w, O, N, M)
        df = float(np.abs(gf - gf0).max())
        da = float(np.abs(np.asarray(ga) - np.asarray(ur.reduce_alpha(ga0, alpha))).max())
        dw = float(np.abs(gw - wur.reduce_w(gw0, w)).max())
        print("%s %s %s K %d: max|du| %.2e  grad_f %.2e (bound %.2e)  grad_alpha %.2e (bound %.2e)  grad_w %.2e (bound %.2e)"
              % (name, kind, wkind, K, float(np.abs(u - u0).max()), df, bf, da, ba, dw, bw))
        assert gw.shape == w.shape and np.isfinite(gw).all()
        assert df <= bf
        assert da <= ba
        assert dw <= bw
    s.close()


# ---- 3. w == 1: the unweighted reverse sweep's gradients ---------------------------------------------------------------
@pytest.mark.parametrize("kind", ["scalar", "patch", "map"])
@pytest.mark.parametrize("name", wur.GRADIENT_SHAPES)
def test_unit_weight_gives_the_unrolled_vjp_s_gradients(gpu_solver_cls, name, kind):
    """u bit for bit; grad_f and grad_alpha to rounding (bpltv_unrolled_vjp factors tau * c out of the stencil), within the
    bounds the twin is held to."""
    O, N, M = SHAPES[name]
    f, gu = _data(name)
    alpha = _alpha(kind, N, M)
    w = _weight(name, "ones")
    amap = tw.alpha_to_map(alpha, M, N)
    s = gpu_solver_cls(M, N, O)
    s.set_data(f, f)
    for K in wur.GRADIENT_K:
        _, tape, tab = ur.fwd_tape(f, amap, K)
        gfr, gar = ur.reverse(gu, tape, tab, amap)           # (the per-pixel magnitudes the bounds are relative to)
        bf, ba, _ = _bounds(gfr, gar, np.ones(1), alpha, w, O, N, M)
        u0 = s.unrolled_denoise(alpha, maxiter=K)
        gf0, ga0 = s.unrolled_vjp(alpha, gu, maxiter=K)
        u = s.weighted_unrolled_denoise(alpha, w, maxiter=K)
        gf, ga, _ = s.weighted_unrolled_vjp(alpha, w, gu, maxiter=K)
        df, da = float(np.abs(gf - gf0).max()), float(np.abs(np.asarray(ga) - np.asarray(ga0)).max())
        print("%s %s K %d: grad_f %.2e (bound %.2e)  grad_alpha %.2e (bound %.2e)" % (name, kind, K, df, bf, da, ba))
        assert _same(u, u0)
        assert df <= bf
        assert da <= ba
    s.close()


# ---- 4. every plan gives the same bits --------------------------------------------------------------------------------
@pytest.mark.parametrize("wkind", ["real", "mask"])       # real: wo = O, mask: wo = 1
@pytest.mark.parametrize("kind", ["scalar", "map"])
def test_results_do_not_depend_on_the_plan(gpu_solver_cls, kind, wkind):
    import torch
    name = "2x70x72"
    O, N, M = SHAPES[name]
    f, gu = _data(name)
    alpha = _alpha(kind, N, M)
    w = _weight(name, wkind)
    wo = O if w.ndim == 3 else 1
    a = np.atleast_1d(np.asarray(alpha, dtype=np.float64))
    an, am = (1, 1) if kind == "scalar" else a.shape
    s = gpu_solver_cls(M, N, O)
    s.set_data(f, f)
    for K in (203, 200):   # 200 iterations at depth 8: the second chain runs half a launch out of phase
        u0 = s.weighted_unrolled_denoise(alpha, w, maxiter=K)
        gf0, ga0, gw0 = s.weighted_unrolled_vjp(alpha, w, gu, maxiter=K)
        assert _same(u0, s.weighted_denoise(alpha, w, maxiter=K))
        plans = [dict(), dict(tile_iters=4), dict(tile_iters=8), dict(chains=1), dict(chains=2), dict(use_graph=0),
                 dict(chains=2, use_graph=0), dict(tile_iters=4, chains=2)]
        for kw in plans:
            u = s.weighted_unrolled_denoise(alpha, w, maxiter=K, **kw)
            if "chains" in kw:
                assert s.stats()["launch_chains"] == (kw["chains"] if kw.get("use_graph", 1) else 1)
            gf, ga, gw = s.weighted_unrolled_vjp(alpha, w, gu, maxiter=K, **kw)
            assert _same(u, u0) and _same(gf, gf0) and _same(ga, ga0) and _same(gw, gw0), kw
        # the device forms, on the handle's tape and on a caller's
        at, gt, wt = torch.tensor(a, device="cuda"), torch.tensor(gu, device="cuda"), torch.tensor(w, device="cuda")
        out, gfd = torch.empty(O, N, M, dtype=torch.float64, device="cuda"), torch.empty(O, N, M, dtype=torch.float64, device="cuda")
        gad = torch.empty(am * an, dtype=torch.float64, device="cuda")
        gwd = torch.empty(w.shape, dtype=torch.float64, device="cuda")
        tape = torch.empty(s.weighted_unrolled_tape_doubles(maxiter=K), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        for tp in (None, tape.data_ptr(), tape.data_ptr()):   # (a repeated call replays the cached graphs)
            gfd.zero_(); gad.zero_(); gwd.zero_(); torch.cuda.synchronize()
            s.weighted_unrolled_denoise_device(wt.data_ptr(), wo, at.data_ptr(), am, an, tape_ptr=tp, maxiter=K)
            s.copy_u_device(out.data_ptr())
            s.weighted_unrolled_vjp_device(tp, wt.data_ptr(), wo, at.data_ptr(), am, an, gt.data_ptr(), gfd.data_ptr(),
                                           gad.data_ptr(), gwd.data_ptr(), maxiter=K)
            assert _same(out.cpu().numpy(), u0) and _same(gfd.cpu().numpy(), gf0) and _same(gwd.cpu().numpy(), gw0)
            assert _same(gad.cpu().numpy().reshape(np.shape(ga0)), ga0)
        # one output at a time
        assert _same(s.weighted_unrolled_vjp(alpha, w, gu, want_alpha=False, want_w=False, maxiter=K)[0], gf0)
        assert _same(s.weighted_unrolled_vjp(alpha, w, gu, want_f=False, want_w=False, maxiter=K)[1], ga0)
        assert _same(s.weighted_unrolled_vjp(alpha, w, gu, want_f=False, want_alpha=False, maxiter=K)[2], gw0)
    s.close()


# ---- 5. finite differences of bpltv_weighted_denoise itself -------------------------------------------------------------
@pytest.mark.parametrize("K", [30, 300])
def test_gradients_against_central_differences_on_the_device(gpu_solver_cls, K):
    """0.5 |u_K - ubar|^2 on a masked 1 x 24 x 28, alpha = 0.08, h = 1e-6, in alpha and in w (direction on the kept pixels),
    relative 1e-5: the margin of the CPU test."""
    ub, f = synth_batch(1, 24, 28, seed=9)
    alpha, h = 0.08, 1e-6
    w = wur.weight_of("mask", 1, 24, 28)
    dw = np.random.default_rng(21).standard_normal(w.shape) * w
    s = gpu_solver_cls(28, 24, 1)
    s.set_data(ub, f)
    u = s.weighted_unrolled_denoise(alpha, w, maxiter=K)
    _, ga, gw = s.weighted_unrolled_vjp(alpha, w, u - ub, want_f=False, maxiter=K)
    loss = lambda aa, ww: tw.l2_cost(s.weighted_denoise(aa, ww, maxiter=K), ub)
    for what, g, fd in (("alpha", ga, (loss(alpha + h, w) - loss(alpha - h, w)) / (2 * h)),
                        ("w", float((gw * dw).sum()), (loss(alpha, w + h * dw) - loss(alpha, w - h * dw)) / (2 * h))):
        print("K %d, d/d%s: reverse sweep %.10g central difference %.10g rel %.2e" % (K, what, g, fd, abs(g - fd) / abs(fd)))
        assert abs(g - fd) <= 1e-5 * abs(fd), what
    s.close()


# ---- 6. the tape's contract -------------------------------------------------------------------------------------------
def test_the_handle_s_weighted_tape(gpu_solver_cls):
    from bpldenoising_amd._lib import BpltvError
    name = "2x17x33"
    O, N, M = SHAPES[name]
    f, gu = _data(name)
    w, mask = _weight(name, "real"), _weight(name, "mask")
    s = gpu_solver_cls(M, N, O)
    s.set_data(f, f)

    def code(call, *a, **k):
        with pytest.raises(BpltvError) as e:
            call(*a, **k)
        return e.value.code

    assert code(s.weighted_unrolled_vjp, 0.08, w, gu, maxiter=20) == E_NODATA          # no tape yet
    s.unrolled_denoise(0.08, maxiter=20)                                               # a TV tape is not a weighted tape ...
    assert code(s.weighted_unrolled_vjp, 0.08, w, gu, maxiter=20) == E_NODATA
    n = gpu_solver_cls(M, N, O)
    n.set_data(f, f)
    n.weighted_unrolled_denoise(0.08, w, maxiter=20)                                   # ... nor the reverse
    assert code(n.unrolled_vjp, 0.08, gu, maxiter=20) == E_NODATA
    n.close()
    s.weighted_unrolled_denoise(0.08, w, maxiter=20)
    st0 = s.stats()
    assert st0["iterations"] == 20 and st0["tiles"] >= O and st0["tile_iters"] >= 1 and st0["launch_chains"] >= 1, st0

    def sweep_stats(method="weighted-unrolled"):
        """what a reverse sweep leaves: its adjoint_method, and the solve fields the taped solve left"""
        st = s.stats()
        assert st["adjoint_method"] == method, st
        assert all(st[k] == st0[k] for k in ("iterations", "tile_iters", "tiles", "launch_chains")), (st, st0)
        return st

    gf, ga, gw = s.weighted_unrolled_vjp(0.08, w, np.zeros_like(gu), maxiter=20)
    assert sweep_stats()["total_ms"] == st0["total_ms"]    # (the weighted sweep leaves the solve's wall time too)
    assert not gf.any() and ga == 0.0 and not gw.any()
    gf, ga, gw = s.weighted_unrolled_vjp(0.08, w, gu, maxiter=20)
    sweep_stats()
    assert gf.any() and ga != 0.0 and gw.any()
    g_tv = s.unrolled_vjp(0.08, gu, maxiter=20)                                        # both tapes live side by side
    st = sweep_stats("unrolled")
    assert st["adjoint_attempts"] == 1 and st["adjoint_residual"] == 0.0, st
    assert g_tv[0].any()
    s.weighted_unrolled_denoise(0.08, w, maxiter=12)       # a second, shorter solve: the tape is now its
    st0 = s.stats()
    assert st0["iterations"] == 12, st0
    assert code(s.weighted_unrolled_vjp, 0.08, w, gu, maxiter=20) == E_ARG
    for kw in (dict(accel=0), dict(tau0=4.0), dict(sigma0=0.1), dict(opnorm=2.5)):     # other steps than the tape's
        assert code(s.weighted_unrolled_vjp, 0.08, w, gu, maxiter=12, **kw) == E_ARG
    assert code(s.weighted_unrolled_vjp, np.full((2, 2), 0.08), w, gu, maxiter=12) == E_ARG   # another parameter shape
    assert code(s.weighted_unrolled_vjp, 0.08, w[0], gu, maxiter=12) == E_ARG          # another wo
    w2 = w.copy()
    w2[w2 == w2.min()] *= 0.5
    assert code(s.weighted_unrolled_vjp, 0.08, w2, gu, maxiter=12) == E_ARG            # another gamma
    assert code(s.weighted_unrolled_vjp, 0.08, np.broadcast_to(mask, w.shape), gu, maxiter=12) == E_ARG   # (gamma = 0)
    a, b = s.weighted_unrolled_vjp(0.08, w, gu, maxiter=12), s.weighted_unrolled_vjp(0.08, w, gu, maxiter=12)
    assert all(_same(x, y) for x, y in zip(a, b))
    sweep_stats()                                          # (the rejected sweeps in between changed nothing either)
    assert all(_same(x, y) for x, y in zip(s.unrolled_vjp(0.08, gu, maxiter=20), g_tv))    # the TV tape survived all of it
    sweep_stats("unrolled")
    n = gpu_solver_cls(M, N, O)                # no dataset
    assert code(n.weighted_unrolled_denoise, 0.08, w, maxiter=5) == E_NODATA
    n.close()
    s.close()


# ---- 7. rejections leave the handle as it was ---------------------------------------------------------------------------
def test_rejections_leave_the_handle_as_it_was(gpu_solver_cls):
    import torch
    from bpldenoising_amd._lib import BpltvError
    name = "2x17x33"
    O, N, M = SHAPES[name]
    f, gu = _data(name)
    w = _weight(name, "real")
    s = gpu_solver_cls(M, N, O)
    s.set_data(f, f)
    amap = _alpha("map", N, M)
    s.weighted_unrolled_denoise(0.08, w, maxiter=20)
    g0 = s.weighted_unrolled_vjp(0.08, w, gu, maxiter=20)
    w1 = _weight(name, "real")[0] + 0.5
    u0 = s.weighted_denoise(amap, w1, maxiter=57)          # the last solve: another parameter, another weight, another wo
    gap0 = s.duality_gap()

    def unchanged():
        assert _same(s.duality_gap(), gap0)
        assert _same(s.weighted_denoise(amap, w1, maxiter=57), u0) and _same(s.duality_gap(), gap0)
        g = s.weighted_unrolled_vjp(0.08, w, gu, maxiter=20)      # ... and the tape is still the first solve's
        assert all(_same(x, y) for x, y in zip(g, g0))
        assert _same(s.duality_gap(), gap0)                       # the VJP staged its w apart

    def rejected(code, call, *a, **k):
        with pytest.raises(BpltvError) as e:
            call(*a, **k)
        assert e.value.code == code, (e.value.code, str(e.value))
        unchanged()

    bad_gu = gu.copy(); bad_gu[1, 3, 4] = np.inf
    nan_map = amap.copy(); nan_map[2, 5] = np.nan
    for bad in (np.nan, -0.25, np.inf):
        bw = w.copy(); bw[1, 4, 7] = bad
        rejected(E_ARG, s.weighted_unrolled_denoise, 0.08, bw, maxiter=20)
        rejected(E_ARG, s.weighted_unrolled_vjp, 0.08, bw, gu, maxiter=20)
    for bad in (float("nan"), -0.1, nan_map):
        rejected(E_ARG, s.weighted_unrolled_denoise, bad, w, maxiter=20)
        rejected(E_ARG, s.weighted_unrolled_vjp, bad, w, gu, maxiter=20)
    rejected(E_ARG, s.weighted_unrolled_vjp, 0.08, w, bad_gu, maxiter=20)
    rejected(E_ARG, s.weighted_unrolled_denoise, 0.08, w, maxiter=0)
    for kw in (dict(rho=0.01), dict(init=1), dict(order=1)):
        rejected(E_UNSUPPORTED, s.weighted_unrolled_denoise, 0.08, w, maxiter=20, **kw)
        rejected(E_UNSUPPORTED, s.weighted_unrolled_vjp, 0.08, w, gu, maxiter=20, **kw)
    p = s.params(maxiter=20)
    a1 = np.array([0.08])
    lib = s._lib
    assert lib.bpltv_weighted_unrolled_vjp(s._h, _ptr(w), O, _ptr(a1), 1, 1, C.byref(p), _ptr(gu), None, None, None) == E_ARG
    unchanged()
    gfh = np.empty_like(gu)
    for wo in (0, O + 1):                                          # a bad wo
        assert lib.bpltv_weighted_unrolled_denoise(s._h, _ptr(w), wo, _ptr(a1), 1, 1, C.byref(p), None) == E_ARG
        assert lib.bpltv_weighted_unrolled_vjp(s._h, _ptr(w), wo, _ptr(a1), 1, 1, C.byref(p), _ptr(gu), _ptr(gfh), None, None) == E_ARG
        unchanged()
    # the device forms
    gt, gfd = torch.tensor(gu, device="cuda"), torch.empty(O, N, M, dtype=torch.float64, device="cuda")
    good = torch.tensor([0.08], dtype=torch.float64, device="cuda")
    wt = torch.tensor(w, device="cuda")
    torch.cuda.synchronize()
    for bad in (np.nan, -0.25, np.inf):
        bwt = wt.clone(); bwt[1, 4, 7] = bad
        torch.cuda.synchronize()
        rejected(E_ARG, s.weighted_unrolled_denoise_device, bwt.data_ptr(), O, good.data_ptr(), 1, 1, maxiter=20)
        rejected(E_ARG, s.weighted_unrolled_vjp_device, None, bwt.data_ptr(), O, good.data_ptr(), 1, 1, gt.data_ptr(),
                 gfd.data_ptr(), None, None, maxiter=20)
    for bad in (float("nan"), -0.1):
        bt = torch.tensor([bad], dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        rejected(E_ARG, s.weighted_unrolled_denoise_device, wt.data_ptr(), O, bt.data_ptr(), 1, 1, maxiter=20)
        rejected(E_ARG, s.weighted_unrolled_vjp_device, None, wt.data_ptr(), O, bt.data_ptr(), 1, 1, gt.data_ptr(),
                 gfd.data_ptr(), None, None, maxiter=20)
    bgt = torch.tensor(bad_gu, device="cuda")
    torch.cuda.synchronize()
    rejected(E_ARG, s.weighted_unrolled_vjp_device, None, wt.data_ptr(), O, good.data_ptr(), 1, 1, bgt.data_ptr(),
             gfd.data_ptr(), None, None, maxiter=20)
    rejected(E_ARG, s.weighted_unrolled_vjp_device, None, wt.data_ptr(), O, good.data_ptr(), 1, 1, gt.data_ptr(),
             None, None, None, maxiter=20)
    for wo in (0, O + 1):
        rejected(E_ARG, s.weighted_unrolled_denoise_device, wt.data_ptr(), wo, good.data_ptr(), 1, 1, maxiter=20)
        rejected(E_ARG, s.weighted_unrolled_vjp_device, None, wt.data_ptr(), wo, good.data_ptr(), 1, 1, gt.data_ptr(),
                 gfd.data_ptr(), None, None, maxiter=20)
    for kw in (dict(rho=0.01), dict(init=1), dict(order=1)):
        rejected(E_UNSUPPORTED, s.weighted_unrolled_denoise_device, wt.data_ptr(), O, good.data_ptr(), 1, 1, maxiter=20, **kw)
        rejected(E_UNSUPPORTED, s.weighted_unrolled_vjp_device, None, wt.data_ptr(), O, good.data_ptr(), 1, 1, gt.data_ptr(),
                 gfd.data_ptr(), None, None, maxiter=20, **kw)
    # grad_w without a dataset: host and device forms, on a caller's tape (the handle has none)
    n = gpu_solver_cls(M, N, O)
    tape = torch.zeros(s.weighted_unrolled_tape_doubles(maxiter=20), dtype=torch.float64, device="cuda")
    gwd = torch.empty(O, N, M, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    with pytest.raises(BpltvError) as e:
        n.weighted_unrolled_vjp_device(tape.data_ptr(), wt.data_ptr(), O, good.data_ptr(), 1, 1, gt.data_ptr(), None, None,
                                       gwd.data_ptr(), maxiter=20)
    assert e.value.code == E_NODATA
    with pytest.raises(BpltvError) as e:
        n.weighted_unrolled_vjp(0.08, w, gu, maxiter=20)
    assert e.value.code == E_NODATA
    n.close()
    s.close()


# ---- 8. shards, float handles, graphs ------------------------------------------------------------------------------------
def test_two_shards_are_unsupported(gpu_solver_cls):
    from bpldenoising_amd._lib import BpltvError
    name = "2x17x33"
    O, N, M = SHAPES[name]
    f, gu = _data(name)
    w = _weight(name, "mask")
    m = gpu_solver_cls(M, N, O, devices=[0, 0])
    m.set_data(f, f)
    u0 = m.denoise(0.07, maxiter=30)
    gap0 = m.duality_gap()
    for call, args in ((m.weighted_unrolled_denoise, (0.07, w)), (m.weighted_unrolled_vjp, (0.07, w, gu)),
                       (m.weighted_unrolled_denoise_device, (1, 1, 1, 1, 1)),
                       (m.weighted_unrolled_vjp_device, (None, 1, 1, 1, 1, 1, 1, 1, 1, 1))):
        with pytest.raises(BpltvError) as e:     # (the device forms are refused before any pointer is read)
            call(*args, maxiter=30)
        assert e.value.code == E_UNSUPPORTED
        assert _same(m.duality_gap(), gap0) and _same(m.denoise(0.07, maxiter=30), u0)
    m.close()
    one = gpu_solver_cls(M, N, O, ngpus=1)       # one shard holds everything: forwarded
    one.set_data(f, f)
    s = gpu_solver_cls(M, N, O)
    s.set_data(f, f)
    assert _same(one.weighted_unrolled_denoise(0.07, w, maxiter=30), s.weighted_unrolled_denoise(0.07, w, maxiter=30))
    a, b = one.weighted_unrolled_vjp(0.07, w, gu, maxiter=30), s.weighted_unrolled_vjp(0.07, w, gu, maxiter=30)
    assert all(_same(x, y) for x, y in zip(a, b))
    one.close()
    s.close()


def test_float_handles_run_the_weighted_unrolled_solve_in_float64(gpu_solver_cls):
    name = "2x17x33"
    O, N, M = SHAPES[name]
    f, gu = _data(name)
    w = _weight(name, "real")
    s, s32 = gpu_solver_cls(M, N, O), gpu_solver_cls(M, N, O, dtype=32)
    for h in (s, s32):
        h.set_data(f, f)
    assert _same(s32.weighted_unrolled_denoise(0.08, w, maxiter=40), s.weighted_unrolled_denoise(0.08, w, maxiter=40))
    a, b = s32.weighted_unrolled_vjp(0.08, w, gu, maxiter=40), s.weighted_unrolled_vjp(0.08, w, gu, maxiter=40)
    assert all(_same(x, y) for x, y in zip(a, b))
    s.close()
    s32.close()


def test_no_graph_is_shared_with_the_other_solves(gpu_solver_cls):
    name = "3x40x48"
    O, N, M = SHAPES[name]
    f, gu = _data(name)
    w = np.ones((N, M))      # the hardest case: every model computes the same u, on the same table, with the same shapes
    alpha, K = 0.08, 57

    def fresh(call):
        h = gpu_solver_cls(M, N, O)
        h.set_data(f, f)
        r = call(h)
        h.close()
        return r
    u_plain = fresh(lambda h: h.denoise(alpha, maxiter=K))
    u_un, g_un = fresh(lambda h: (h.unrolled_denoise(alpha, maxiter=K), h.unrolled_vjp(alpha, gu, maxiter=K)))
    u_wu, g_wu = fresh(lambda h: (h.weighted_unrolled_denoise(alpha, w, maxiter=K), h.weighted_unrolled_vjp(alpha, w, gu, maxiter=K)))
    assert _same(u_un, u_plain) and _same(u_wu, u_plain)
    for order in ("weighted unrolled first", "weighted unrolled last"):
        h = gpu_solver_cls(M, N, O)
        h.set_data(f, f)
        for rnd in range(2):   # the second round replays what the first one cached
            if order == "weighted unrolled first":
                assert _same(h.weighted_unrolled_denoise(alpha, w, maxiter=K), u_wu)
            assert _same(h.denoise(alpha, maxiter=K), u_plain)
            assert _same(h.weighted_denoise(alpha, w, maxiter=K), u_plain)
            assert _same(h.unrolled_denoise(alpha, maxiter=K), u_un)
            if order == "weighted unrolled last":
                assert _same(h.weighted_unrolled_denoise(alpha, w, maxiter=K), u_wu)
            g = h.unrolled_vjp(alpha, gu, maxiter=K)                       # each tape holds what its own solve recorded
            assert _same(g[0], g_un[0]) and _same(g[1], g_un[1])
            g = h.weighted_unrolled_vjp(alpha, w, gu, maxiter=K)
            assert all(_same(x, y) for x, y in zip(g, g_wu))
        h.close()
