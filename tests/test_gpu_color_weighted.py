"""GPU checks of channel-coupled TV with a per-pixel fidelity weight (bpltv_color_weighted_denoise,
bpltv_color_weighted_unrolled_denoise / bpltv_color_weighted_unrolled_vjp and their device forms).

w = 1 is tied to bpltv_color_denoise and channels = 1 to the bpltv_weighted_unrolled_* calls bit for bit; u and the gradients
in f, alpha and w of 2 ... 4 channels are held against the numpy twin tests/color_weighted_ref.py (pinned on the CPU by
tests/test_color_weighted_abi.py); every plan (fusion depth, launch chains, graphs, host or device form, whose tape,
checkpoints) gives the same bits; the coupling and the weight both act; and a rejected call leaves the handle as it was."""
import ctypes as C

import numpy as np
import pytest

import color_weighted_ref as cw
import unrolled_ref as ur

pytestmark = pytest.mark.gpu

E_ARG, E_NODATA, E_UNSUPPORTED = 1, 3, 6
U_CAP = 1e-13   # HIP against its plain-numpy restatement: the margin of tests/test_gpu_color.py


def _same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b))


def _all_same(xs, ys):
    return len(xs) == len(ys) and all(_same(x, y) for x, y in zip(xs, ys))


def _solver(cls, name):
    B, Cc, N, M = cw.SHAPES[name]
    f, gu = cw.gpu_data(name)
    s = cls(M, N, B * Cc)
    s.set_data(f, f)
    return s, f, gu


# ---- 1. bitwise ties ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(cw.SHAPES))
def test_unit_weight_is_the_color_solve_bitwise(gpu_solver_cls, name):
    """With w == 1.0 every weighted operation returns the bits of the one it replaces: fma(-1, f, div) = div - f, and 1 / fma(tau,
    1, 1) is the table's 1 / (1 + tau)."""
    B, Cc, N, M = cw.SHAPES[name]
    s, f, gu = _solver(gpu_solver_cls, name)
    w = cw.weight_of("ones", B, Cc, N, M)
    for kind in cw.KINDS:
        alpha = cw.alpha_of(kind, N, M)
        for K in (1, 7, 203):
            for accel in (0, 1):
                u0 = s.color_denoise(alpha, Cc, maxiter=K, accel=accel)
                assert _same(s.color_weighted_denoise(alpha, Cc, w, maxiter=K, accel=accel), u0), (kind, K, accel)
                assert _same(s.color_weighted_unrolled_denoise(alpha, Cc, w, maxiter=K, accel=accel), u0), (kind, K, accel)
    s.close()


@pytest.mark.parametrize("wkind", ["real", "mask"])
@pytest.mark.parametrize("name", ["2x3x17x33", "1x3x40x48", "1x2x9x1", "1x4x1x9"])
def test_one_channel_is_the_weighted_unrolled_solve_bitwise(gpu_solver_cls, name, wkind):
    B, Cc, N, M = cw.SHAPES[name]
    s, f, gu = _solver(gpu_solver_cls, name)
    w = cw.weight_of(wkind, B * Cc, 1, N, M)
    for kind in cw.KINDS:
        alpha = cw.alpha_of(kind, N, M)
        for K in (7, 50, 203):
            u0 = s.weighted_unrolled_denoise(alpha, w, maxiter=K)
            g0 = s.weighted_unrolled_vjp(alpha, w, gu, maxiter=K)
            u = s.color_weighted_unrolled_denoise(alpha, 1, w, maxiter=K)
            g = s.color_weighted_unrolled_vjp(alpha, 1, w, gu, maxiter=K)
            assert s.stats()["adjoint_method"] == "color-weighted-unrolled"
            assert _same(u, u0) and _all_same(g, g0), (kind, K)
            assert _same(s.color_weighted_denoise(alpha, 1, w, maxiter=K), u0)
    s.close()


@pytest.mark.parametrize("name", ["2x3x17x33", "2x4x33x70"])
def test_a_mask_makes_acceleration_a_no_op(gpu_solver_cls, name):
    """gamma = min w = 0: omega = 1 and constant steps with accel = 1, the table of accel = 0."""
    B, Cc, N, M = cw.SHAPES[name]
    s, f, gu = _solver(gpu_solver_cls, name)
    for wkind in ("mask", "mosaic"):
        w = cw.weight_of(wkind, B, Cc, N, M)
        for K in (7, 203):
            u0 = s.color_weighted_unrolled_denoise(0.08, Cc, w, maxiter=K, accel=0)
            g0 = s.color_weighted_unrolled_vjp(0.08, Cc, w, gu, maxiter=K, accel=0)
            u1 = s.color_weighted_unrolled_denoise(0.08, Cc, w, maxiter=K, accel=1)
            g1 = s.color_weighted_unrolled_vjp(0.08, Cc, w, gu, maxiter=K, accel=1)
            assert _same(u0, u1) and _all_same(g0, g1), (wkind, K)
    s.close()


# ---- 2. u and the gradients against the twin ------------------------------------------------------------------------------
def _bounds(gf0, ga0, gw0, alpha, w, B, Cc, N, M):
    """(grad_f, grad_alpha, grad_w): 1e-11 * max|gf0|; 1e-11 * max|ga0| * B * pixels_per_entry, ga0 the per-pixel terms; 1e-11 *
    max|gw0|, times O = B * Cc for a one-plane weight (tests/test_gpu_tile_depths.py imports them)."""
    return (1e-11 * float(np.abs(gf0).max()), 1e-11 * float(np.abs(ga0).max()) * B * ur.pixels_per_entry(alpha, M, N),
            1e-11 * float(np.abs(gw0).max()) * (B * Cc if np.ndim(w) == 2 else 1))


@pytest.mark.parametrize("wkind", ["real", "mask", "mosaic"])
@pytest.mark.parametrize("kind", cw.KINDS)
@pytest.mark.parametrize("name", sorted(cw.SHAPES))
def test_u_and_gradients_match_the_twin(gpu_solver_cls, name, kind, wkind):
    """u at most 1e-13 from the twin (the kernel's explicit fma against plain numpy: rounding only); grad_f within 1e-11 *
    max|gf0|; grad_alpha within 1e-11 * max|ga0| * B * pixels_per_entry, ga0 the per-pixel terms (the reduced sum cancels: on
    1x3x2x2 with the mask it is seven orders below its terms); grad_w within 1e-11 * max|gw0|, times O for a one-plane weight:
    test_gpu_color.py's and test_gpu_weighted_unrolled.py's bounds.  Measured on MI355X: max|u - u0|
    8.9e-16 over all cases; grad_f at most 1.3e-14, 0.063 % of its bound; grad_alpha at most 2.9e-13, 0.12 % of its bound;
    grad_w at most 2.2e-13, 0.22 % of its bound."""
    B, Cc, N, M = cw.SHAPES[name]
    s, f, gu = _solver(gpu_solver_cls, name)
    alpha = cw.alpha_of(kind, N, M)
    w = cw.weight_of(wkind, B, Cc, N, M)
    amap = np.shape(alpha) == (N, M) and N * M > 1      # (a 2 x 2 patch on a 2 x 2 image is a map)
    for K in cw.KS:
        u0, _, _, gf0, ga0, gw0 = cw.twin_case(name, kind, wkind, K)
        u = s.color_weighted_unrolled_denoise(alpha, Cc, w, maxiter=K)
        st = s.stats()
        assert st["iterations"] == K and st["pdhg_variant"] == 0 and st["launches"] >= 1 and st["tiles"] >= B, st
        assert st["bytes_per_px_iter"] == (88.0 + 8.0 / Cc if amap else 88.0), st
        assert _same(s.color_weighted_denoise(alpha, Cc, w, maxiter=K), u)      # the plain solve: the same bits, no tape touched
        assert s.stats()["bytes_per_px_iter"] == (64.0 + 8.0 / Cc if amap else 64.0)
        gf, ga, gw = s.color_weighted_unrolled_vjp(alpha, Cc, w, gu, maxiter=K)
        st = s.stats()
        assert st["adjoint_method"] == "color-weighted-unrolled" and st["adjoint_ms"] > 0.0 and st["iterations"] == K, st
        bf, ba, bw = _bounds(gf0, ga0, gw0, alpha, w, B, Cc, N, M)
        du = float(np.abs(u - u0).max())
        df = float(np.abs(gf - gf0).max())
        da = float(np.abs(np.asarray(ga) - np.asarray(ur.reduce_alpha(ga0, alpha))).max())
        dw = float(np.abs(gw - cw.reduce_w(gw0, w)).max())
        print("%s %s %s K %d: max|du| %.2e (cap %.0e)  grad_f %.2e (bound %.2e)  grad_alpha %.2e (bound %.2e)  grad_w %.2e (bound %.2e)"
              % (name, kind, wkind, K, du, U_CAP, df, bf, da, ba, dw, bw))
        assert gw.shape == w.shape
        assert du <= U_CAP
        assert df <= bf
        assert da <= ba
        assert dw <= bw
    s.close()


# ---- 3. every plan gives the same bits --------------------------------------------------------------------------------
@pytest.mark.parametrize("wkind", ["real", "mask"])
@pytest.mark.parametrize("kind", ["scalar", "map"])
@pytest.mark.parametrize("name", ["2x4x33x70", "2x3x17x33"])
def test_results_do_not_depend_on_the_plan(gpu_solver_cls, name, kind, wkind):
    import torch
    B, Cc, N, M = cw.SHAPES[name]
    O, K = B * Cc, 203
    s, f, gu = _solver(gpu_solver_cls, name)
    alpha = cw.alpha_of(kind, N, M)
    w = cw.weight_of(wkind, B, Cc, N, M)
    wo = O if w.ndim == 3 else 1
    a = np.atleast_1d(np.asarray(alpha, dtype=np.float64))
    an, am = (1, 1) if kind == "scalar" else a.shape
    u0 = s.color_weighted_unrolled_denoise(alpha, Cc, w, maxiter=K)
    g0 = s.color_weighted_unrolled_vjp(alpha, Cc, w, gu, maxiter=K)
    assert _same(s.color_weighted_denoise(alpha, Cc, w, maxiter=K), u0)      # no tape: the same u, and the tape survives it
    assert _all_same(s.color_weighted_unrolled_vjp(alpha, Cc, w, gu, maxiter=K), g0)
    plans = [dict(), dict(tile_iters=1), dict(tile_iters=3), dict(chains=1), dict(chains=2), dict(use_graph=0),
             dict(chains=2, use_graph=0), dict(tile_iters=3, chains=2)]
    for kw in plans:
        for rep in range(2):   # (the second call replays the cached graphs)
            u = s.color_weighted_unrolled_denoise(alpha, Cc, w, maxiter=K, **kw)
            if "chains" in kw:
                assert s.stats()["launch_chains"] == (min(kw["chains"], B) if kw.get("use_graph", 1) else 1)
            g = s.color_weighted_unrolled_vjp(alpha, Cc, w, gu, maxiter=K, **kw)
            assert _same(u, u0) and _all_same(g, g0), (kw, rep)
        assert _same(s.color_weighted_denoise(alpha, Cc, w, maxiter=K, **kw), u0), kw
    # checkpoints instead of the tape
    for ck in (-1, 5):
        assert s.weighted_unrolled_tape_doubles(maxiter=K, checkpoint_every=ck) < 3 * K * M * N * O
        u = s.color_weighted_unrolled_denoise(alpha, Cc, w, maxiter=K, checkpoint_every=ck)
        g = s.color_weighted_unrolled_vjp(alpha, Cc, w, gu, maxiter=K, checkpoint_every=ck)
        assert _same(u, u0) and _all_same(g, g0), ck
    assert _same(s.color_weighted_unrolled_denoise(alpha, Cc, w, maxiter=K), u0)      # the full tape again
    # one output at a time: without grad_w the sweep loads neither f nor x+, and grad_f, grad_alpha keep their bits
    gf, ga, gw = s.color_weighted_unrolled_vjp(alpha, Cc, w, gu, want_w=False, maxiter=K)
    assert gw is None and _same(gf, g0[0]) and _same(ga, g0[1])
    assert _same(s.color_weighted_unrolled_vjp(alpha, Cc, w, gu, want_alpha=False, want_w=False, maxiter=K)[0], g0[0])
    assert _same(s.color_weighted_unrolled_vjp(alpha, Cc, w, gu, want_f=False, want_w=False, maxiter=K)[1], g0[1])
    assert _same(s.color_weighted_unrolled_vjp(alpha, Cc, w, gu, want_f=False, want_alpha=False, maxiter=K)[2], g0[2])
    # the device forms, on the handle's tape and on a caller's
    at, gt, wt = torch.tensor(a, device="cuda"), torch.tensor(gu, device="cuda"), torch.tensor(w, device="cuda")
    out, gfd = torch.empty(O, N, M, dtype=torch.float64, device="cuda"), torch.empty(O, N, M, dtype=torch.float64, device="cuda")
    gad, gwd = torch.empty(am * an, dtype=torch.float64, device="cuda"), torch.empty_like(wt)
    assert s.weighted_unrolled_tape_doubles(maxiter=K) == 3 * K * M * N * O
    tape = torch.empty(s.weighted_unrolled_tape_doubles(maxiter=K), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    for tp in (None, tape.data_ptr(), tape.data_ptr()):   # (a repeated call replays the cached graphs)
        gfd.zero_(); gad.zero_(); gwd.zero_(); torch.cuda.synchronize()
        s.color_weighted_unrolled_denoise_device(Cc, wt.data_ptr(), wo, at.data_ptr(), am, an, tape_ptr=tp, maxiter=K)
        s.copy_u_device(out.data_ptr())
        s.color_weighted_unrolled_vjp_device(Cc, tp, wt.data_ptr(), wo, at.data_ptr(), am, an, gt.data_ptr(), gfd.data_ptr(),
                                             gad.data_ptr(), gwd.data_ptr(), maxiter=K)
        assert _same(out.cpu().numpy(), u0) and _same(gfd.cpu().numpy(), g0[0]) and _same(gwd.cpu().numpy(), g0[2])
        assert _same(gad.cpu().numpy().reshape(np.shape(g0[1])), g0[1])
        gfd.zero_(); gad.zero_(); torch.cuda.synchronize()   # grad_w_out = NULL
        s.color_weighted_unrolled_vjp_device(Cc, tp, wt.data_ptr(), wo, at.data_ptr(), am, an, gt.data_ptr(), gfd.data_ptr(),
                                             gad.data_ptr(), None, maxiter=K)
        assert _same(gfd.cpu().numpy(), g0[0]) and _same(gad.cpu().numpy().reshape(np.shape(g0[1])), g0[1])
    s.color_weighted_denoise_device(Cc, wt.data_ptr(), wo, at.data_ptr(), am, an, maxiter=K)
    s.copy_u_device(out.data_ptr())
    assert _same(out.cpu().numpy(), u0)
    s.close()


# ---- 4. the coupling and the weight are both real ---------------------------------------------------------------------
def test_the_coupling_and_the_weight_both_act(gpu_solver_cls):
    name = "2x3x17x33"
    B, Cc, N, M = cw.SHAPES[name]
    s, f, gu = _solver(gpu_solver_cls, name)
    w = cw.weight_of("mosaic", B, Cc, N, M)
    u = s.color_weighted_denoise(0.08, Cc, w, maxiter=203)
    assert float(np.abs(u - s.weighted_denoise(0.08, w, maxiter=203)).max()) > 1e-4      # channel by channel, the same w
    assert float(np.abs(u - s.color_denoise(0.08, Cc, maxiter=203)).max()) > 1e-4        # coupled, no weight
    s.close()


# ---- 5. the contract ----------------------------------------------------------------------------------------------------
def test_rejections_leave_the_handle_as_it_was(gpu_solver_cls):
    import torch
    from bpldenoising_amd._lib import BpltvError
    from bpldenoising_amd.learning_function import _ptr
    name = "2x3x17x33"
    B, Cc, N, M = cw.SHAPES[name]
    O, K = B * Cc, 20
    s, f, gu = _solver(gpu_solver_cls, name)
    amap = cw.alpha_of("map", N, M)
    w = cw.weight_of("real", B, Cc, N, M)
    mask = cw.weight_of("mask", B, Cc, N, M)
    ones = cw.weight_of("ones", B, Cc, N, M)
    # a TV, a weighted and a colour tape, and no colour-weighted one yet: none of them is taken
    s.unrolled_denoise(0.08, maxiter=K)
    g_tv = s.unrolled_vjp(0.08, gu, maxiter=K)
    s.weighted_unrolled_denoise(0.08, ones, maxiter=K)
    g_w = s.weighted_unrolled_vjp(0.08, ones, gu, maxiter=K)
    s.color_unrolled_denoise(0.08, Cc, maxiter=K)
    g_c = s.color_unrolled_vjp(0.08, Cc, gu, maxiter=K)
    for ch in (1, Cc):
        with pytest.raises(BpltvError) as e:
            s.color_weighted_unrolled_vjp(0.08, ch, ones, gu, maxiter=K)
        assert e.value.code == E_NODATA, str(e.value)
    s.color_weighted_unrolled_denoise(0.08, Cc, w, maxiter=K)
    g0 = s.color_weighted_unrolled_vjp(0.08, Cc, w, gu, maxiter=K)
    for call, args in ((s.unrolled_vjp, (0.08, gu)), (s.weighted_unrolled_vjp, (0.08, ones, gu)), (s.color_unrolled_vjp, (0.08, Cc, gu))):
        g = call(*args, maxiter=K)      # ... nor this tape by theirs: each sweep reads what its own solve recorded
        assert _all_same(g, g_tv if call == s.unrolled_vjp else (g_w if call == s.weighted_unrolled_vjp else g_c))
    u0 = s.color_weighted_denoise(amap, Cc, mask, maxiter=57)   # the last solve: another parameter, another weight
    s.color_weighted_unrolled_vjp(0.08, Cc, w, gu, maxiter=K)
    st0 = s.stats()
    ud = torch.empty(O, N, M, dtype=torch.float64, device="cuda")

    def unchanged():
        st = s.stats()
        assert {k for k in st if st[k] != st0[k]} <= {"adjoint_ms"}, [(k, st[k], st0[k]) for k in st if st[k] != st0[k]]
        s.copy_u_device(ud.data_ptr())
        assert _same(ud.cpu().numpy(), u0)
        assert _all_same(s.weighted_unrolled_vjp(0.08, ones, gu, maxiter=K), g_w)
        assert _all_same(s.color_unrolled_vjp(0.08, Cc, gu, maxiter=K), g_c)
        assert _all_same(s.color_weighted_unrolled_vjp(0.08, Cc, w, gu, maxiter=K), g0)   # (last: adjoint_method is its own again)

    def rejected(code, call, *a, **k):
        with pytest.raises(BpltvError) as e:
            call(*a, **k)
        assert e.value.code == code, (e.value.code, str(e.value))
        unchanged()

    solves = (s.color_weighted_unrolled_denoise, s.color_weighted_denoise)
    for ch in (5, 0, -1, 4):                   # outside 1 ... 4, or not dividing the handle's 6 planes
        for solve in solves:
            rejected(E_ARG, solve, 0.08, ch, w, maxiter=K)
        rejected(E_ARG, s.color_weighted_unrolled_vjp, 0.08, ch, w, gu, maxiter=K)
    for ch in (1, 2, 6):                       # a sweep with other channels than its tape
        rejected(E_ARG, s.color_weighted_unrolled_vjp, 0.08, ch, w, gu, maxiter=K)
    rejected(E_ARG, s.color_weighted_unrolled_vjp, 0.08, Cc, w[0], gu, maxiter=K)               # ... other weight planes
    rejected(E_ARG, s.color_weighted_unrolled_vjp, 0.08, Cc, 0.5 * w, gu, maxiter=K)            # ... another gamma
    rejected(E_ARG, s.color_weighted_unrolled_vjp, 0.08, Cc, w, gu, maxiter=K + 1)              # ... other step parameters
    rejected(E_ARG, s.color_weighted_unrolled_vjp, 0.08, Cc, w, gu, maxiter=K, accel=0)
    rejected(E_ARG, s.color_weighted_unrolled_vjp, amap, Cc, w, gu, maxiter=K)
    neg, nan = w.copy(), mask.copy()
    neg[4, 3, 2] = -1e-300
    nan[5, 7] = np.nan
    for bad in (neg, nan, np.full((N, M), np.inf)):
        for solve in solves:
            rejected(E_ARG, solve, 0.08, Cc, bad, maxiter=K)
        rejected(E_ARG, s.color_weighted_unrolled_vjp, 0.08, Cc, bad, gu, maxiter=K)
    # wo = B: one plane per colour image is not a form of its own (the caller expands it to O planes)
    p, a1, wb, uo = s.params(maxiter=K), np.array([0.08]), np.ones((B, N, M)), np.empty((O, N, M))
    for wo in (B, 0, O + 1):
        assert s._lib.bpltv_color_weighted_unrolled_denoise(s._h, Cc, _ptr(wb), wo, _ptr(a1), 1, 1, C.byref(p), _ptr(uo)) == E_ARG
        assert s._lib.bpltv_color_weighted_denoise(s._h, Cc, _ptr(wb), wo, _ptr(a1), 1, 1, C.byref(p), _ptr(uo)) == E_ARG
        assert s._lib.bpltv_color_weighted_unrolled_vjp(s._h, Cc, _ptr(wb), wo, _ptr(a1), 1, 1, C.byref(p), _ptr(gu), _ptr(uo), None, None) == E_ARG
        unchanged()
    bad_gu = gu.copy(); bad_gu[1, 3, 4] = np.inf
    nan_map = amap.copy(); nan_map[2, 5] = np.nan
    for bad in (float("nan"), -0.1, nan_map):
        for solve in solves:
            rejected(E_ARG, solve, bad, Cc, w, maxiter=K)
        rejected(E_ARG, s.color_weighted_unrolled_vjp, bad, Cc, w, gu, maxiter=K)
    rejected(E_ARG, s.color_weighted_unrolled_vjp, 0.08, Cc, w, bad_gu, maxiter=K)
    for solve in solves:
        rejected(E_ARG, solve, 0.08, Cc, w, maxiter=0)
        for kw in (dict(rho=0.01), dict(init=1), dict(order=1)):
            rejected(E_UNSUPPORTED, solve, 0.08, Cc, w, maxiter=K, **kw)
    rejected(E_UNSUPPORTED, s.color_weighted_unrolled_vjp, 0.08, Cc, w, gu, maxiter=K, rho=0.01)
    # the device forms
    gt, gfd = torch.tensor(gu, device="cuda"), torch.empty(O, N, M, dtype=torch.float64, device="cuda")
    good, wt = torch.tensor([0.08], dtype=torch.float64, device="cuda"), torch.tensor(w, device="cuda")
    bw = torch.tensor(neg, device="cuda")
    torch.cuda.synchronize()
    rejected(E_ARG, s.color_weighted_unrolled_denoise_device, Cc, bw.data_ptr(), O, good.data_ptr(), 1, 1, maxiter=K)
    rejected(E_ARG, s.color_weighted_denoise_device, Cc, bw.data_ptr(), O, good.data_ptr(), 1, 1, maxiter=K)
    rejected(E_ARG, s.color_weighted_unrolled_vjp_device, Cc, None, bw.data_ptr(), O, good.data_ptr(), 1, 1, gt.data_ptr(), gfd.data_ptr(),
             None, None, maxiter=K)
    rejected(E_ARG, s.color_weighted_unrolled_denoise_device, Cc, wt.data_ptr(), B, good.data_ptr(), 1, 1, maxiter=K)
    rejected(E_ARG, s.color_weighted_unrolled_denoise_device, 5, wt.data_ptr(), O, good.data_ptr(), 1, 1, maxiter=K)
    rejected(E_ARG, s.color_weighted_unrolled_vjp_device, Cc, None, wt.data_ptr(), O, good.data_ptr(), 1, 1, gt.data_ptr(), None, None, None,
             maxiter=K)
    assert _all_same(s.unrolled_vjp(0.08, gu, maxiter=K), g_tv)      # the TV tape too (its sweep resets the adjoint statistics)
    # the gap of the coupled model is not implemented, weighted or not
    s.color_weighted_denoise(0.08, Cc, w, maxiter=K)
    with pytest.raises(BpltvError) as e:
        s.duality_gap()
    assert e.value.code == E_UNSUPPORTED and "channel" in str(e.value)
    s.close()
    n = gpu_solver_cls(M, N, O)                # no dataset: no solve, and no grad_w on a caller's tape
    with pytest.raises(BpltvError) as e:
        n.color_weighted_unrolled_denoise(0.08, Cc, w, maxiter=5)
    assert e.value.code == E_NODATA
    tape = torch.zeros(3 * 5 * M * N * O, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    with pytest.raises(BpltvError) as e:
        n.color_weighted_unrolled_vjp_device(Cc, tape.data_ptr(), wt.data_ptr(), O, good.data_ptr(), 1, 1, gt.data_ptr(), gfd.data_ptr(),
                                             None, gfd.data_ptr(), maxiter=5)
    assert e.value.code == E_NODATA
    n.close()
    o3 = gpu_solver_cls(M, N, 3)               # channels = 2 on O = 3
    o3.set_data(f[:3], f[:3])
    with pytest.raises(BpltvError) as e:
        o3.color_weighted_unrolled_denoise(0.08, 2, w[:3], maxiter=5)
    assert e.value.code == E_ARG
    o3.close()
    m = gpu_solver_cls(M, N, O, devices=[0, 0])   # two shards
    m.set_data(f, f)
    for call, args in ((m.color_weighted_denoise, (0.07, Cc, w)), (m.color_weighted_unrolled_denoise, (0.07, Cc, w)),
                       (m.color_weighted_unrolled_vjp, (0.07, Cc, w, gu))):
        with pytest.raises(BpltvError) as e:
            call(*args, maxiter=30)
        assert e.value.code == E_UNSUPPORTED
    m.close()


def test_no_graph_is_shared_with_the_other_solves(gpu_solver_cls):
    """w == 1 is the hardest case: the colour, the weighted, the TV and this model run the same shapes, the same table and (the
    coupled ones) compute the same u.  In both call orders, over two rounds -- the second replays what the first cached."""
    name = "2x3x17x33"
    B, Cc, N, M = cw.SHAPES[name]
    f, gu = cw.gpu_data(name)
    w = cw.weight_of("ones", B, Cc, N, M)
    alpha, K = 0.08, 57

    def fresh(call):
        h = gpu_solver_cls(M, N, B * Cc)
        h.set_data(f, f)
        r = call(h)
        h.close()
        return r
    u_tv, g_tv = fresh(lambda h: (h.unrolled_denoise(alpha, maxiter=K), h.unrolled_vjp(alpha, gu, maxiter=K)))
    u_w, g_w = fresh(lambda h: (h.weighted_unrolled_denoise(alpha, w, maxiter=K), h.weighted_unrolled_vjp(alpha, w, gu, maxiter=K)))
    u_c, g_c = fresh(lambda h: (h.color_unrolled_denoise(alpha, Cc, maxiter=K), h.color_unrolled_vjp(alpha, Cc, gu, maxiter=K)))
    u_cw, g_cw = fresh(lambda h: (h.color_weighted_unrolled_denoise(alpha, Cc, w, maxiter=K),
                                  h.color_weighted_unrolled_vjp(alpha, Cc, w, gu, maxiter=K)))
    g_cw2 = fresh(lambda h: (h.color_weighted_unrolled_denoise(alpha, Cc, w, maxiter=K),
                             h.color_weighted_unrolled_vjp(alpha, Cc, w, gu, want_w=False, maxiter=K)))[1]
    assert _same(u_cw, u_c) and _same(u_w, u_tv) and not _same(u_c, u_tv)
    assert _same(g_cw2[0], g_cw[0]) and _same(g_cw2[1], g_cw[1])
    for first in (True, False):
        h = gpu_solver_cls(M, N, B * Cc)
        h.set_data(f, f)
        for rnd in range(2):
            if first:
                assert _same(h.color_weighted_unrolled_denoise(alpha, Cc, w, maxiter=K), u_cw)
                assert _same(h.color_weighted_denoise(alpha, Cc, w, maxiter=K), u_cw)
            assert _same(h.denoise(alpha, maxiter=K), u_tv)
            assert _same(h.weighted_denoise(alpha, w, maxiter=K), u_tv)
            assert _same(h.unrolled_denoise(alpha, maxiter=K), u_tv)
            assert _same(h.weighted_unrolled_denoise(alpha, w, maxiter=K), u_w)
            assert _same(h.color_unrolled_denoise(alpha, Cc, maxiter=K), u_c)
            assert _same(h.color_denoise(alpha, Cc, maxiter=K), u_c)
            if not first:
                assert _same(h.color_weighted_denoise(alpha, Cc, w, maxiter=K), u_cw)
                assert _same(h.color_weighted_unrolled_denoise(alpha, Cc, w, maxiter=K), u_cw)
            assert _all_same(h.unrolled_vjp(alpha, gu, maxiter=K), g_tv)                 # each tape holds what its own solve recorded
            assert _all_same(h.weighted_unrolled_vjp(alpha, w, gu, maxiter=K), g_w)
            assert _all_same(h.color_unrolled_vjp(alpha, Cc, gu, maxiter=K), g_c)
            assert _all_same(h.color_weighted_unrolled_vjp(alpha, Cc, w, gu, maxiter=K), g_cw)
            g = h.color_weighted_unrolled_vjp(alpha, Cc, w, gu, want_w=False, maxiter=K)
            assert _same(g[0], g_cw[0]) and _same(g[1], g_cw[1])
        h.close()
