"""GPU checks of channel-coupled TV for colour images (bpltv_color_denoise, bpltv_color_unrolled_denoise /
bpltv_color_unrolled_vjp and their device forms).

channels = 1 is tied to the bpltv_unrolled_* calls bit for bit; u and the gradients of 2 ... 4 channels are held against the
numpy twin tests/color_ref.py (pinned on the CPU by tests/test_color_abi.py); every plan (fusion depth, launch chains, graphs,
host or device form, whose tape, checkpoints) gives the same bits; and a rejected call leaves the handle as it was."""
import numpy as np
import pytest

import color_ref as cr
import unrolled_ref as ur

pytestmark = pytest.mark.gpu

E_ARG, E_NODATA, E_UNSUPPORTED = 1, 3, 6
U_CAP = 1e-13   # HIP against its plain-numpy restatement: the margin of tests/test_unpinned.py (5000 iterations)


def _same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b))


def _solver(cls, name):
    B, Cc, N, M = cr.SHAPES[name]
    f, gu = cr.gpu_data(name)
    s = cls(M, N, B * Cc)
    s.set_data(f, f)
    return s, f, gu


# ---- 1. one channel is the TV model, bit for bit --------------------------------------------------------------------------
@pytest.mark.parametrize("kind", cr.KINDS)
@pytest.mark.parametrize("name", ["2x3x17x33", "1x3x40x48", "1x2x9x1", "1x4x1x9"])
def test_one_channel_is_the_unrolled_tv_solve_bitwise(gpu_solver_cls, name, kind):
    B, Cc, N, M = cr.SHAPES[name]
    s, f, gu = _solver(gpu_solver_cls, name)
    alpha = cr.alpha_of(kind, N, M)
    for K in cr.KS:
        u0 = s.unrolled_denoise(alpha, maxiter=K)
        gf0, ga0 = s.unrolled_vjp(alpha, gu, maxiter=K)
        u = s.color_unrolled_denoise(alpha, 1, maxiter=K)
        gf, ga = s.color_unrolled_vjp(alpha, 1, gu, maxiter=K)
        assert s.stats()["adjoint_method"] == "color-unrolled"
        assert _same(u, u0) and _same(gf, gf0) and _same(ga, ga0), (K, float(np.abs(u - u0).max()))
        assert _same(s.color_denoise(alpha, 1, maxiter=K), u0)
    s.close()


# ---- 2. u and the gradients against the twin ------------------------------------------------------------------------------
def _bounds(gf0, ga0, alpha, B, N, M):
    """test_gpu_unrolled.py's: 1e-11 * max|ref| for grad_f; for grad_alpha relative to the largest per-pixel term of the
    reference times the number of terms summed into one entry (colour images x pixels of the entry)."""
    return 1e-11 * float(np.abs(gf0).max()), 1e-11 * float(np.abs(ga0).max()) * B * ur.pixels_per_entry(alpha, M, N)


@pytest.mark.parametrize("kind", cr.KINDS)
@pytest.mark.parametrize("name", sorted(cr.SHAPES))
def test_u_and_gradients_match_the_twin(gpu_solver_cls, name, kind):
    """u at most 1e-13 from the twin (the kernel's explicit fma against plain numpy: rounding only); grad_f and grad_alpha
    within test_gpu_unrolled.py's bounds.  Measured on MI355X: max|u - u0| 1.1e-15 over all cases; grad_f at
    most 5.6e-14 against bounds of 1.5e-11 and more, at most 0.25 % of its bound; grad_alpha at most 7.0e-13, at most 0.11 % of
    its bound (3.6e-12 for a map ... 2.1e-7 for the scalar on 2x4x33x70)."""
    B, Cc, N, M = cr.SHAPES[name]
    s, f, gu = _solver(gpu_solver_cls, name)
    alpha = cr.alpha_of(kind, N, M)
    for K in cr.KS:
        u0, _, _, gf0, ga0 = cr.twin_case(name, kind, K)
        u = s.color_unrolled_denoise(alpha, Cc, maxiter=K)
        st = s.stats()
        assert st["iterations"] == K and st["pdhg_variant"] == 0 and st["launches"] >= 1 and st["tiles"] >= B, st
        amap = np.shape(alpha) == (N, M) and N * M > 1      # (a 2 x 2 patch on a 2 x 2 image is a map)
        assert st["bytes_per_px_iter"] == (72.0 + 8.0 / Cc if amap else 72.0), st
        gf, ga = s.color_unrolled_vjp(alpha, Cc, gu, maxiter=K)
        st = s.stats()
        assert st["adjoint_method"] == "color-unrolled" and st["adjoint_ms"] > 0.0 and st["iterations"] == K, st
        bf, ba = _bounds(gf0, ga0, alpha, B, N, M)
        du = float(np.abs(u - u0).max())
        df = float(np.abs(gf - gf0).max())
        da = float(np.abs(np.asarray(ga) - np.asarray(ur.reduce_alpha(ga0, alpha))).max())
        print("%s %s K %d: max|du| %.2e (cap %.0e)  grad_f %.2e (bound %.2e)  grad_alpha %.2e (bound %.2e)"
              % (name, kind, K, du, U_CAP, df, bf, da, ba))
        assert du <= U_CAP
        assert df <= bf
        assert da <= ba
    s.close()


@pytest.mark.parametrize("Cc", [2, 3, 4])
def test_identical_channels_are_tv_with_alpha_over_sqrt_c(gpu_solver_cls, Cc):
    """C copies of each image: every channel of the colour solve is bpltv_denoise with alpha / sqrt(C), to the cap of u
    against the twin."""
    from conftest import synth_batch
    _, f1 = synth_batch(2, 17, 33, seed=38)
    f = np.ascontiguousarray(np.repeat(f1, Cc, axis=0))
    s, t = gpu_solver_cls(33, 17, 2 * Cc), gpu_solver_cls(33, 17, 2)
    s.set_data(f, f)
    t.set_data(f1, f1)
    for alpha in (0.08, cr.alpha_of("map", 17, 33)):
        for K in cr.KS:
            u = s.color_denoise(alpha, Cc, maxiter=K)
            u1 = t.denoise(np.asarray(alpha) / np.sqrt(Cc) if np.ndim(alpha) else alpha / np.sqrt(Cc), maxiter=K)
            d = float(np.abs(u - np.repeat(u1, Cc, axis=0)).max())
            print("C %d K %d: %.2e" % (Cc, K, d))
            assert d <= U_CAP
    s.close()
    t.close()


def test_the_coupling_is_real(gpu_solver_cls):
    s, f, gu = _solver(gpu_solver_cls, "2x3x17x33")
    u = s.color_unrolled_denoise(0.08, 3, maxiter=203)
    v = s.unrolled_denoise(0.08, maxiter=203)
    assert float(np.abs(u - v).max()) > 1e-4
    s.close()


# ---- 3. every plan gives the same bits --------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["scalar", "map"])
@pytest.mark.parametrize("name", ["2x4x33x70", "2x3x17x33", "1x3x40x48"])
def test_results_do_not_depend_on_the_plan(gpu_solver_cls, name, kind):
    import torch
    B, Cc, N, M = cr.SHAPES[name]
    O = B * Cc
    s, f, gu = _solver(gpu_solver_cls, name)
    alpha = cr.alpha_of(kind, N, M)
    a = np.atleast_1d(np.asarray(alpha, dtype=np.float64))
    an, am = (1, 1) if kind == "scalar" else a.shape
    for K in (50, 203):
        u0 = s.color_unrolled_denoise(alpha, Cc, maxiter=K)
        gf0, ga0 = s.color_unrolled_vjp(alpha, Cc, gu, maxiter=K)
        assert _same(s.color_denoise(alpha, Cc, maxiter=K), u0)      # no tape: the same u, and the tape survives it
        gf, ga = s.color_unrolled_vjp(alpha, Cc, gu, maxiter=K)
        assert _same(gf, gf0) and _same(ga, ga0)
        plans = [dict(), dict(tile_iters=1), dict(tile_iters=3), dict(chains=1), dict(chains=2), dict(use_graph=0),
                 dict(chains=2, use_graph=0), dict(tile_iters=3, chains=2)]
        for kw in plans:
            u = s.color_unrolled_denoise(alpha, Cc, maxiter=K, **kw)
            if "chains" in kw:
                assert s.stats()["launch_chains"] == (min(kw["chains"], B) if kw.get("use_graph", 1) else 1)
            gf, ga = s.color_unrolled_vjp(alpha, Cc, gu, maxiter=K, **kw)
            assert _same(u, u0) and _same(gf, gf0) and _same(ga, ga0), kw
            assert _same(s.color_denoise(alpha, Cc, maxiter=K, **kw), u0), kw
        # checkpoints instead of the tape
        for ck in (-1, 5):
            assert s.unrolled_tape_doubles(maxiter=K, checkpoint_every=ck) < 2 * K * M * N * O
            u = s.color_unrolled_denoise(alpha, Cc, maxiter=K, checkpoint_every=ck)
            gf, ga = s.color_unrolled_vjp(alpha, Cc, gu, maxiter=K, checkpoint_every=ck)
            assert _same(u, u0) and _same(gf, gf0) and _same(ga, ga0), ck
        # the device forms, on the handle's tape and on a caller's
        at, gt = torch.tensor(a, device="cuda"), torch.tensor(gu, device="cuda")
        out, gfd = torch.empty(O, N, M, dtype=torch.float64, device="cuda"), torch.empty(O, N, M, dtype=torch.float64, device="cuda")
        gad = torch.empty(am * an, dtype=torch.float64, device="cuda")
        assert s.unrolled_tape_doubles(maxiter=K) == 2 * K * M * N * O
        tape = torch.empty(s.unrolled_tape_doubles(maxiter=K), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        tapes = []
        for tp in (None, tape.data_ptr(), tape.data_ptr()):   # (a repeated call replays the cached graphs)
            gfd.zero_(); gad.zero_(); torch.cuda.synchronize()
            s.color_unrolled_denoise_device(Cc, at.data_ptr(), am, an, tape_ptr=tp, maxiter=K)
            s.copy_u_device(out.data_ptr())
            s.color_unrolled_vjp_device(Cc, tp, at.data_ptr(), am, an, gt.data_ptr(), gfd.data_ptr(), gad.data_ptr(), maxiter=K)
            assert _same(out.cpu().numpy(), u0) and _same(gfd.cpu().numpy(), gf0)
            assert _same(gad.cpu().numpy().reshape(np.shape(ga0)), ga0)
        # one output at a time
        assert _same(s.color_unrolled_vjp(alpha, Cc, gu, want_alpha=False, maxiter=K)[0], gf0)
        assert _same(s.color_unrolled_vjp(alpha, Cc, gu, want_f=False, maxiter=K)[1], ga0)
    s.close()


# ---- 4. the contract ----------------------------------------------------------------------------------------------------
def test_rejections_leave_the_handle_as_it_was(gpu_solver_cls):
    import torch
    from bpldenoising_amd._lib import BpltvError
    name = "2x3x17x33"
    B, Cc, N, M = cr.SHAPES[name]
    s, f, gu = _solver(gpu_solver_cls, name)
    amap = cr.alpha_of("map", N, M)
    with pytest.raises(BpltvError) as e:       # no colour tape yet
        s.color_unrolled_vjp(0.08, 3, gu, maxiter=20)
    assert e.value.code == E_NODATA
    s.color_unrolled_denoise(0.08, 3, maxiter=20)
    gf0, ga0 = s.color_unrolled_vjp(0.08, 3, gu, maxiter=20)
    u0 = s.color_denoise(amap, 3, maxiter=57)   # the last solve: another parameter, another shape
    ud = torch.empty(B * Cc, N, M, dtype=torch.float64, device="cuda")

    def unchanged():
        s.copy_u_device(ud.data_ptr())
        assert _same(ud.cpu().numpy(), u0)
        gf, ga = s.color_unrolled_vjp(0.08, 3, gu, maxiter=20)      # ... and the tape is still the first solve's
        assert _same(gf, gf0) and _same(ga, ga0)

    def rejected(code, call, *a, **k):
        with pytest.raises(BpltvError) as e:
            call(*a, **k)
        assert e.value.code == code, (e.value.code, str(e.value))
        unchanged()

    for ch in (5, 0, -1, 4):                   # outside 1 ... 4, or not dividing the handle's 6 planes
        rejected(E_ARG, s.color_unrolled_denoise, 0.08, ch, maxiter=20)
        rejected(E_ARG, s.color_denoise, 0.08, ch, maxiter=20)
        rejected(E_ARG, s.color_unrolled_vjp, 0.08, ch, gu, maxiter=20)
    for ch in (1, 2, 6):                       # a sweep with other channels than the solve's
        rejected(E_ARG, s.color_unrolled_vjp, 0.08, ch, gu, maxiter=20)
    bad_gu = gu.copy(); bad_gu[1, 3, 4] = np.inf
    nan_map = amap.copy(); nan_map[2, 5] = np.nan
    for bad in (float("nan"), -0.1, nan_map):
        rejected(E_ARG, s.color_unrolled_denoise, bad, 3, maxiter=20)
        rejected(E_ARG, s.color_denoise, bad, 3, maxiter=20)
        rejected(E_ARG, s.color_unrolled_vjp, bad, 3, gu, maxiter=20)
    rejected(E_ARG, s.color_unrolled_vjp, 0.08, 3, bad_gu, maxiter=20)
    rejected(E_ARG, s.color_unrolled_denoise, 0.08, 3, maxiter=0)
    rejected(E_ARG, s.color_denoise, 0.08, 3, maxiter=0)
    rejected(E_ARG, s.color_unrolled_vjp, 0.08, 3, gu, maxiter=21)
    for kw in (dict(rho=0.01), dict(init=1), dict(order=1)):
        rejected(E_UNSUPPORTED, s.color_unrolled_denoise, 0.08, 3, maxiter=20, **kw)
        rejected(E_UNSUPPORTED, s.color_denoise, 0.08, 3, maxiter=20, **kw)
        rejected(E_UNSUPPORTED, s.color_unrolled_vjp, 0.08, 3, gu, maxiter=20, **kw)
    # the device forms
    gt, gfd = torch.tensor(gu, device="cuda"), torch.empty(B * Cc, N, M, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    for bad in (float("nan"), -0.1):
        bt = torch.tensor([bad], dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        rejected(E_ARG, s.color_unrolled_denoise_device, 3, bt.data_ptr(), 1, 1, maxiter=20)
        rejected(E_ARG, s.color_unrolled_vjp_device, 3, None, bt.data_ptr(), 1, 1, gt.data_ptr(), gfd.data_ptr(), None, maxiter=20)
    good = torch.tensor([0.08], dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    rejected(E_ARG, s.color_unrolled_denoise_device, 5, good.data_ptr(), 1, 1, maxiter=20)
    rejected(E_ARG, s.color_unrolled_vjp_device, 3, None, good.data_ptr(), 1, 1, gt.data_ptr(), None, None, maxiter=20)
    n = gpu_solver_cls(M, N, B * Cc)           # no dataset
    with pytest.raises(BpltvError) as e:
        n.color_unrolled_denoise(0.08, 3, maxiter=5)
    assert e.value.code == E_NODATA
    n.close()
    o3 = gpu_solver_cls(M, N, 3)               # channels = 2 on O = 3
    o3.set_data(f[:3], f[:3])
    with pytest.raises(BpltvError) as e:
        o3.color_unrolled_denoise(0.08, 2, maxiter=5)
    assert e.value.code == E_ARG
    o3.close()
    s.close()


def test_the_tapes_survive_each_other_and_the_gap_is_refused(gpu_solver_cls):
    from bpldenoising_amd._lib import BpltvError
    name = "2x3x17x33"
    s, f, gu = _solver(gpu_solver_cls, name)
    K = 30
    uc = s.color_unrolled_denoise(0.08, 3, maxiter=K)
    gc = s.color_unrolled_vjp(0.08, 3, gu, maxiter=K)
    with pytest.raises(BpltvError) as e:       # only a colour tape so far: the TV sweep does not take it
        s.unrolled_vjp(0.08, gu, maxiter=K)
    assert e.value.code == E_NODATA
    with pytest.raises(BpltvError) as e:
        s.duality_gap()
    assert e.value.code == E_UNSUPPORTED and "channel" in str(e.value)
    ut = s.unrolled_denoise(0.08, maxiter=K)   # the TV model: its own tape; the gap works again
    gap = s.duality_gap()
    gt = s.unrolled_vjp(0.08, gu, maxiter=K)
    assert not _same(ut, uc) and not _same(gt[0], gc[0])
    g = s.color_unrolled_vjp(0.08, 3, gu, maxiter=K)            # the colour tape survived the TV solve
    assert _same(g[0], gc[0]) and _same(g[1], gc[1])
    assert _same(s.color_unrolled_denoise(0.08, 3, maxiter=K), uc)
    with pytest.raises(BpltvError) as e:
        s.duality_gap()
    assert e.value.code == E_UNSUPPORTED
    g = s.unrolled_vjp(0.08, gu, maxiter=K)                     # ... and the TV tape the colour solve
    assert _same(g[0], gt[0]) and _same(g[1], gt[1])
    assert _same(s.denoise(0.08, maxiter=K), ut)
    assert _same(s.duality_gap(), gap)
    s.close()


def test_the_sweep_changes_two_statistics_only(gpu_solver_cls):
    s, f, gu = _solver(gpu_solver_cls, "2x3x17x33")
    s.color_unrolled_denoise(0.08, 3, maxiter=20)
    st0 = s.stats()
    assert st0["iterations"] == 20 and st0["tiles"] == 4 and st0["region_i"] == 32 and st0["bytes_per_px_iter"] == 72.0, st0
    assert st0["algorithmic_bytes"] == 72.0 * 17 * 33 * 6 * 20, st0
    s.color_unrolled_vjp(0.08, 3, gu, maxiter=20)
    st = s.stats()
    assert st["adjoint_method"] == "color-unrolled" and st["adjoint_ms"] > 0.0
    changed = {k for k in st if st[k] != st0[k]}
    assert changed <= {"adjoint_ms", "adjoint_method"}, changed
    s.color_denoise(0.08, 3, maxiter=20)
    assert s.stats()["bytes_per_px_iter"] == 56.0
    s.close()


def test_two_shards_are_unsupported(gpu_solver_cls):
    from bpldenoising_amd._lib import BpltvError
    name = "2x3x17x33"
    B, Cc, N, M = cr.SHAPES[name]
    f, gu = cr.gpu_data(name)
    m = gpu_solver_cls(M, N, B * Cc, devices=[0, 0])
    m.set_data(f, f)
    u0 = m.denoise(0.07, maxiter=30)
    for call, args in ((m.color_denoise, (0.07, 3)), (m.color_unrolled_denoise, (0.07, 3)), (m.color_unrolled_vjp, (0.07, 3, gu)),
                       (m.color_unrolled_denoise_device, (3, 1, 1, 1)), (m.color_unrolled_vjp_device, (3, None, 1, 1, 1, 1, 1, 1))):
        with pytest.raises(BpltvError) as e:     # (the device forms are refused before any pointer is read)
            call(*args, maxiter=30)
        assert e.value.code == E_UNSUPPORTED
        assert _same(m.denoise(0.07, maxiter=30), u0)
    m.close()
    one = gpu_solver_cls(M, N, B * Cc, ngpus=1)   # one shard holds everything: forwarded
    one.set_data(f, f)
    s = gpu_solver_cls(M, N, B * Cc)
    s.set_data(f, f)
    assert _same(one.color_unrolled_denoise(0.07, 3, maxiter=30), s.color_unrolled_denoise(0.07, 3, maxiter=30))
    assert _same(one.color_unrolled_vjp(0.07, 3, gu, maxiter=30)[0], s.color_unrolled_vjp(0.07, 3, gu, maxiter=30)[0])
    one.close()
    s.close()


def test_float_handles_compute_in_float64(gpu_solver_cls):
    name = "2x3x17x33"
    B, Cc, N, M = cr.SHAPES[name]
    f, gu = cr.gpu_data(name)
    s, s32 = gpu_solver_cls(M, N, B * Cc), gpu_solver_cls(M, N, B * Cc, dtype=32)
    for h in (s, s32):
        h.set_data(f, f)
    assert _same(s32.color_unrolled_denoise(0.08, 3, maxiter=40), s.color_unrolled_denoise(0.08, 3, maxiter=40))
    a, b = s32.color_unrolled_vjp(0.08, 3, gu, maxiter=40), s.color_unrolled_vjp(0.08, 3, gu, maxiter=40)
    assert _same(a[0], b[0]) and _same(a[1], b[1])
    s.close()
    s32.close()
