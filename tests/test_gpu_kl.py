"""GPU checks of TV-KL denoising (bpltv_kl_denoise, bpltv_kl_unrolled_denoise, bpltv_kl_unrolled_vjp and their device forms,
DESIGN.md section 4.19).

u and the three gradients are held against the numpy twin tests/kl_ref.py (pinned on the CPU by tests/test_kl_abi.py) and against
central differences of bpltv_kl_denoise itself; the limits of the model hold on the device; every plan (fusion depth, launch
chains, graphs, host or device form, whose tape, checkpoints) gives the same bits; no tape and no graph is shared with another
model; and a rejected call -- a dataset with a negative entry among them -- leaves the handle as it was."""
import ctypes as C
import functools

import numpy as np
import pytest

import kl_ref as kr
import unrolled_ref as ur
from oracle import np_twin as tw

pytestmark = pytest.mark.gpu

E_ARG, E_NODATA, E_UNSUPPORTED = 1, 3, 6
_dp = C.POINTER(C.c_double)
SHAPES = kr.GPU_SHAPES
_alpha = kr.alpha_of


def _same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b))


def _ptr(a):
    return a.ctypes.data_as(_dp) if a is not None else None


@functools.lru_cache(maxsize=None)
def _data(name):
    f, gu = kr.gpu_data(name)
    for a in (f, gu):
        a.setflags(write=False)
    return f, gu


@functools.lru_cache(maxsize=None)
def _weight(name, wkind):
    w = kr.weight_of(wkind, *SHAPES[name])
    w.setflags(write=False)
    return w


def _code(call, *a, **k):
    from bpldenoising_amd._lib import BpltvError
    with pytest.raises(BpltvError) as e:
        call(*a, **k)
    return e.value.code


# ---- 1. u and the gradients against the twin ----------------------------------------------------------------------------
def _bounds(gf0, ga0, gw0, alpha, w, O, N, M):
    """tests/test_gpu_l1.py's: 1e-11 * max|ref| for grad_f; for grad_alpha relative to the largest per-pixel term of the
    reference times the number of terms summed into one entry; for grad_w 1e-11 * max|ref|, times O where the images are summed
    into one plane."""
    return (1e-11 * float(np.abs(gf0).max()), 1e-11 * float(np.abs(ga0).max()) * O * ur.pixels_per_entry(alpha, M, N),
            1e-11 * float(np.abs(gw0).max()) * (O if np.ndim(w) == 2 else 1))


@pytest.mark.parametrize("wkind", kr.WEIGHTS)
@pytest.mark.parametrize("kind", kr.KINDS)
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_u_and_gradients_match_the_twin(gpu_solver_cls, name, kind, wkind):
    """u to 1e-13, the gradients to _bounds; the plain solve, the taped solve and accel = 0 give the same bits.  Measured on
    MI355X: see the table of DESIGN.md section 4.19."""
    O, N, M = SHAPES[name]
    f, gu = _data(name)
    alpha = _alpha(kind, N, M)
    w = _weight(name, wkind)
    s = gpu_solver_cls(M, N, O)
    s.set_data(f, f)
    for K in kr.GRADIENT_K:
        u0, gf0, ga0, gw0, _ = kr.twin_case(name, kind, wkind, K)
        up = s.kl_denoise(alpha, w, maxiter=K)
        stp = s.stats()
        u = s.kl_unrolled_denoise(alpha, w, maxiter=K)
        st0 = s.stats()
        assert _same(u, up)
        assert _same(u, s.kl_unrolled_denoise(alpha, w, maxiter=K, accel=0)) and _same(u, s.kl_denoise(alpha, w, maxiter=K, accel=0))
        amap = kind == "map" and N * M > 1
        assert stp["bytes_per_px_iter"] == (72.0 if amap else 64.0) and st0["bytes_per_px_iter"] == (96.0 if amap else 88.0)
        assert st0["iterations"] == K and st0["pdhg_variant"] == 0 and st0["launches"] >= 1 and st0["tiles"] >= O, st0
        u = s.kl_unrolled_denoise(alpha, w, maxiter=K)
        st0 = s.stats()
        gf, ga, gw = s.kl_unrolled_vjp(alpha, w, gu, maxiter=K)
        st = s.stats()
        assert st["adjoint_method"] == "kl-unrolled" and st["adjoint_ms"] > 0.0 and st["iterations"] == K, st
        changed = {k for k in st if st[k] != st0[k]}
        assert changed <= {"adjoint_ms", "adjoint_method"}, changed
        bf, ba, bw = _bounds(gf0, ga0, gw0, alpha, w, O, N, M)
        du = float(np.abs(u - u0).max())
        df = float(np.abs(gf - gf0).max())
        da = float(np.abs(np.asarray(ga) - np.asarray(ur.reduce_alpha(ga0, alpha))).max())
        dw = float(np.abs(gw - kr.reduce_w(gw0, w)).max())
        print("%s %s %s K %d: max|du| %.2e (bound 1e-13)  grad_f %.2e (bound %.2e)  grad_alpha %.2e (bound %.2e)  grad_w %.2e (bound %.2e)"
              % (name, kind, wkind, K, du, df, bf, da, ba, dw, bw))
        assert gw.shape == w.shape and np.isfinite(gw).all()
        assert du <= 1e-13
        assert df <= bf
        assert da <= ba
        assert dw <= bw
    s.close()


# ---- 2. every plan gives the same bits --------------------------------------------------------------------------------
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
        u0 = s.kl_unrolled_denoise(alpha, w, maxiter=K)
        gf0, ga0, gw0 = s.kl_unrolled_vjp(alpha, w, gu, maxiter=K)
        assert _same(u0, s.kl_denoise(alpha, w, maxiter=K))
        plans = [dict(), dict(tile_iters=1), dict(tile_iters=3), dict(tile_iters=8), dict(chains=1), dict(chains=2), dict(use_graph=0),
                 dict(chains=2, use_graph=0), dict(tile_iters=3, chains=2), dict(checkpoint_every=-1), dict(checkpoint_every=5),
                 dict(checkpoint_every=5, chains=2, tile_iters=3)]
        for kw in plans:
            for rnd in range(2):   # the second round replays the graphs of the first
                u = s.kl_unrolled_denoise(alpha, w, maxiter=K, **kw)
                if "chains" in kw:
                    assert s.stats()["launch_chains"] == (kw["chains"] if kw.get("use_graph", 1) else 1)
                gf, ga, gw = s.kl_unrolled_vjp(alpha, w, gu, maxiter=K, **kw)
                assert _same(u, u0) and _same(gf, gf0) and _same(ga, ga0) and _same(gw, gw0), (kw, rnd)
            if "checkpoint_every" not in kw:
                assert _same(s.kl_denoise(alpha, w, maxiter=K, **kw), u0), kw
        # the device forms, on the handle's tape and on a caller's
        at, gt, wt = torch.tensor(a, device="cuda"), torch.tensor(gu, device="cuda"), torch.tensor(w, device="cuda")
        out, gfd = torch.empty(O, N, M, dtype=torch.float64, device="cuda"), torch.empty(O, N, M, dtype=torch.float64, device="cuda")
        gad = torch.empty(am * an, dtype=torch.float64, device="cuda")
        gwd = torch.empty(w.shape, dtype=torch.float64, device="cuda")
        tape = torch.empty(s.weighted_unrolled_tape_doubles(maxiter=K), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        for tp in (None, tape.data_ptr(), tape.data_ptr()):   # (a repeated call replays the cached graphs)
            gfd.zero_(); gad.zero_(); gwd.zero_(); out.zero_(); torch.cuda.synchronize()
            s.kl_unrolled_denoise_device(wt.data_ptr(), wo, at.data_ptr(), am, an, tape_ptr=tp, maxiter=K)
            s.copy_u_device(out.data_ptr())
            s.kl_unrolled_vjp_device(tp, wt.data_ptr(), wo, at.data_ptr(), am, an, gt.data_ptr(), gfd.data_ptr(), gad.data_ptr(),
                                     gwd.data_ptr(), maxiter=K)
            assert _same(out.cpu().numpy(), u0) and _same(gfd.cpu().numpy(), gf0) and _same(gwd.cpu().numpy(), gw0)
            assert _same(gad.cpu().numpy().reshape(np.shape(ga0)), ga0)
        out.zero_(); torch.cuda.synchronize()
        s.kl_denoise_device(wt.data_ptr(), wo, at.data_ptr(), am, an, maxiter=K)
        s.copy_u_device(out.data_ptr())
        assert _same(out.cpu().numpy(), u0)
        # one output at a time; grad_w_out = NULL against all three
        assert _same(s.kl_unrolled_vjp(alpha, w, gu, want_alpha=False, want_w=False, maxiter=K)[0], gf0)
        assert _same(s.kl_unrolled_vjp(alpha, w, gu, want_f=False, want_w=False, maxiter=K)[1], ga0)
        assert _same(s.kl_unrolled_vjp(alpha, w, gu, want_f=False, want_alpha=False, maxiter=K)[2], gw0)
        g = s.kl_unrolled_vjp(alpha, w, gu, want_w=False, maxiter=K)
        assert _same(g[0], gf0) and _same(g[1], ga0) and g[2] is None
    s.close()


def test_image_k_of_a_batch_is_the_one_image_handle_s(gpu_solver_cls):
    name = "3x40x48"
    O, N, M = SHAPES[name]
    f, gu = _data(name)
    w = _weight(name, "real")
    alpha, K = _alpha("map", N, M), 57
    s = gpu_solver_cls(M, N, O)
    s.set_data(f, f)
    u = s.kl_unrolled_denoise(alpha, w, maxiter=K)
    gf, _, gw = s.kl_unrolled_vjp(alpha, w, gu, maxiter=K)
    s.close()
    for k in range(O):
        one = gpu_solver_cls(M, N, 1)
        one.set_data(f[k:k + 1], f[k:k + 1])
        assert _same(one.kl_unrolled_denoise(alpha, w[k:k + 1], maxiter=K), u[k:k + 1])
        gf1, _, gw1 = one.kl_unrolled_vjp(alpha, w[k:k + 1], gu[k:k + 1], maxiter=K)
        assert _same(gf1, gf[k:k + 1]) and _same(gw1, gw[k:k + 1])
        one.close()


# ---- 3. the limits on the device ----------------------------------------------------------------------------------------
def test_limits_on_the_device(gpu_solver_cls):
    """tests/test_kl_abi.py's: w = 1e30 and alpha = 0 return f to 1e-13, a constant plane comes back bit for bit, and the raw
    counts, zeros included, give a finite u >= 0 that is the twin's to 1e-13, with finite gradients."""
    for name in sorted(SHAPES):
        O, N, M = SHAPES[name]
        f, _ = _data(name)
        s = gpu_solver_cls(M, N, O)
        s.set_data(f, f)
        for kind in kr.KINDS:
            d1 = float(np.abs(s.kl_denoise(_alpha(kind, N, M), np.full((N, M), 1e30), maxiter=57) - f).max())
            d2 = float(np.abs(s.kl_unrolled_denoise(_alpha(kind, N, M), np.full((O, N, M), 1e30), maxiter=57) - f).max())
            print("%s %s: w = 1e30 max|u - f| %.2e %.2e" % (name, kind, d1, d2))
            assert d1 <= 1e-13 and d2 <= 1e-13
        d = float(np.abs(s.kl_denoise(0.0, _weight(name, "real"), maxiter=57) - f).max())
        print("%s: alpha = 0 max|u - f| %.2e" % (name, d))
        assert d <= 1e-13
        flat = np.full((O, N, M), 0.4)
        s.set_data(flat, flat)
        assert _same(s.kl_denoise(_alpha("scalar", N, M), np.ones((N, M)), maxiter=203), flat)
        s.close()
    name = "2x17x33"
    O, N, M = SHAPES[name]
    raw = kr.poisson_data(name)[1]
    _, gu = _data(name)
    assert raw.min() == 0.0
    s = gpu_solver_cls(M, N, O)
    s.set_data(raw, raw)
    for wkind in kr.WEIGHTS:
        w = _weight(name, wkind)
        u = s.kl_unrolled_denoise(0.15, w, maxiter=50)
        u0 = kr.fwd_tape(raw, tw.alpha_to_map(0.15, M, N), w, 50)[0]
        g = s.kl_unrolled_vjp(0.15, w, gu, maxiter=50)
        print("raw counts %s: min u %.3g max|u - twin| %.2e" % (wkind, float(u.min()), float(np.abs(u - u0).max())))
        assert np.isfinite(u).all() and u.min() >= 0.0 and float(np.abs(u - u0).max()) <= 1e-13
        assert np.isfinite(g[0]).all() and np.isfinite(g[1]) and np.isfinite(g[2]).all()
    s.close()


def test_it_is_another_model_than_the_weighted_and_the_l1_one(gpu_solver_cls):
    name = "2x17x33"
    O, N, M = SHAPES[name]
    f, _ = _data(name)
    s = gpu_solver_cls(M, N, O)
    s.set_data(f, f)
    for wkind in ("real", "ones"):
        w = _weight(name, wkind)
        for kind in kr.KINDS:
            alpha = _alpha(kind, N, M)
            u = s.kl_denoise(alpha, w, maxiter=203)
            dq = float(np.abs(u - s.weighted_denoise(alpha, w, maxiter=203)).max())
            dl = float(np.abs(u - s.l1_denoise(alpha, w, maxiter=203)).max())
            print("%s %s: max|u_kl - u_weighted| %.2e max|u_kl - u_l1| %.2e" % (wkind, kind, dq, dl))
            assert dq > 1e-4 and dl > 1e-4
    s.close()


# ---- 4. central differences of bpltv_kl_denoise itself --------------------------------------------------------------------
def test_gradients_against_central_differences_on_the_device(gpu_solver_cls):
    """tests/test_kl_abi.py's case and step (a masked 1 x 24 x 28, K = 30, alpha = 0.15, h = 1e-6), relative 1e-5, along alpha,
    along a random direction of f and along a random direction of w on the kept pixels."""
    ub, f, w, df, dw = kr.central_difference_case()
    alpha, h, K = kr.CD_ALPHA, kr.CD_H, kr.CD_K
    s = gpu_solver_cls(28, 24, 1)

    def loss(ff, aa, ww):
        s.set_data(ub, ff)
        return tw.l2_cost(s.kl_denoise(aa, ww, maxiter=K), ub)
    s.set_data(ub, f)
    u = s.kl_unrolled_denoise(alpha, w, maxiter=K)
    gf, ga, gw = s.kl_unrolled_vjp(alpha, w, u - ub, maxiter=K)
    for what, g, fd in (("alpha", ga, (loss(f, alpha + h, w) - loss(f, alpha - h, w)) / (2 * h)),
                        ("f", float((gf * df).sum()), (loss(f + h * df, alpha, w) - loss(f - h * df, alpha, w)) / (2 * h)),
                        ("w", float((gw * dw).sum()), (loss(f, alpha, w + h * dw) - loss(f, alpha, w - h * dw)) / (2 * h))):
        print("d/d%s: reverse sweep %.10g central difference %.10g rel %.2e" % (what, g, fd, abs(g - fd) / abs(fd)))
        assert abs(g - fd) <= 1e-5 * abs(fd), what
    s.close()


# ---- 5. the tape's contract: no tape is another model's ---------------------------------------------------------------
def test_the_handle_s_kl_tape(gpu_solver_cls):
    name = "2x17x33"
    O, N, M = SHAPES[name]
    f, gu = _data(name)
    w = _weight(name, "real")
    a = 0.15
    s = gpu_solver_cls(M, N, O)
    s.set_data(f, f)
    assert _code(s.kl_unrolled_vjp, a, w, gu, maxiter=20) == E_NODATA                  # no tape yet
    s.unrolled_denoise(a, maxiter=20)                                                  # no other model's tape is a KL tape ...
    s.weighted_unrolled_denoise(a, w, maxiter=20)
    s.l1_unrolled_denoise(a, w, maxiter=20)
    s.color_weighted_unrolled_denoise(a, 1, w, maxiter=20)
    assert _code(s.kl_unrolled_vjp, a, w, gu, maxiter=20) == E_NODATA
    g_tv, g_w = s.unrolled_vjp(a, gu, maxiter=20), s.weighted_unrolled_vjp(a, w, gu, maxiter=20)
    g_l1 = s.l1_unrolled_vjp(a, w, gu, maxiter=20)
    g_cw = s.color_weighted_unrolled_vjp(a, 1, w, gu, maxiter=20)
    n = gpu_solver_cls(M, N, O)
    n.set_data(f, f)
    n.kl_unrolled_denoise(a, w, maxiter=20)                                            # ... nor the reverse
    assert _code(n.unrolled_vjp, a, gu, maxiter=20) == E_NODATA
    assert _code(n.weighted_unrolled_vjp, a, w, gu, maxiter=20) == E_NODATA
    assert _code(n.l1_unrolled_vjp, a, w, gu, maxiter=20) == E_NODATA
    assert _code(n.color_weighted_unrolled_vjp, a, 1, w, gu, maxiter=20) == E_NODATA
    assert _code(n.sumregs_unrolled_vjp, np.array([0.03, 0.02, 0.05]), gu, maxiter=20) == E_NODATA
    n.close()
    u = s.kl_unrolled_denoise(a, w, maxiter=20)
    st0 = s.stats()
    g = s.kl_unrolled_vjp(a, w, gu, maxiter=20)
    st = s.stats()
    assert st["adjoint_method"] == "kl-unrolled" and st["total_ms"] == st0["total_ms"] and st["iterations"] == 20
    gz = s.kl_unrolled_vjp(a, w, np.zeros_like(gu), maxiter=20)
    assert not gz[0].any() and gz[1] == 0.0 and not gz[2].any()
    assert g[0].any() and g[1] != 0.0 and g[2].any()
    # the other tapes survived the KL solve and its sweeps: their later VJPs give their earlier bits
    assert all(_same(x, y) for x, y in zip(s.unrolled_vjp(a, gu, maxiter=20), g_tv))
    assert all(_same(x, y) for x, y in zip(s.weighted_unrolled_vjp(a, w, gu, maxiter=20), g_w))
    assert all(_same(x, y) for x, y in zip(s.l1_unrolled_vjp(a, w, gu, maxiter=20), g_l1))
    assert all(_same(x, y) for x, y in zip(s.color_weighted_unrolled_vjp(a, 1, w, gu, maxiter=20), g_cw))
    # ... and the KL tape theirs
    s.unrolled_denoise(a, maxiter=12)
    s.weighted_unrolled_denoise(a, w, maxiter=12)
    s.l1_unrolled_denoise(a, w, maxiter=12)
    s.sumregs_unrolled_denoise(np.array([0.03, 0.02, 0.05]), maxiter=12)
    s.color_unrolled_denoise(a, 1, maxiter=12)
    assert all(_same(x, y) for x, y in zip(s.kl_unrolled_vjp(a, w, gu, maxiter=20), g))
    # what the tape remembers
    s.kl_unrolled_denoise(a, w, maxiter=12)
    assert _code(s.kl_unrolled_vjp, a, w, gu, maxiter=20) == E_ARG
    for kw in (dict(tau0=4.0), dict(sigma0=0.1), dict(opnorm=2.5)):                    # other steps than the tape's
        assert _code(s.kl_unrolled_vjp, a, w, gu, maxiter=12, **kw) == E_ARG
    assert _code(s.kl_unrolled_vjp, np.full((2, 2), a), w, gu, maxiter=12) == E_ARG    # another parameter shape
    assert _code(s.kl_unrolled_vjp, a, w[0], gu, maxiter=12) == E_ARG                  # another wo
    assert _code(s.kl_unrolled_vjp, a, w, gu, maxiter=12, checkpoint_every=5) == E_ARG  # another spacing
    n = gpu_solver_cls(M, N, O)                # no dataset
    assert _code(n.kl_unrolled_denoise, a, w, maxiter=5) == E_NODATA
    assert _code(n.kl_denoise, a, w, maxiter=5) == E_NODATA
    n.close()
    assert u.shape == f.shape
    s.close()


# ---- 6. rejections leave the handle as it was ---------------------------------------------------------------------------
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
    s.weighted_unrolled_denoise(0.08, w, maxiter=20)       # a weighted and an L1 tape, rejected and accepted KL calls in between (below)
    gw0 = s.weighted_unrolled_vjp(0.08, w, gu, maxiter=20)
    s.l1_unrolled_denoise(0.7, w, maxiter=20)
    gl0 = s.l1_unrolled_vjp(0.7, w, gu, maxiter=20)
    s.kl_unrolled_denoise(0.15, w, maxiter=20)
    g0 = s.kl_unrolled_vjp(0.15, w, gu, maxiter=20)
    w1 = _weight(name, "real")[0] + 0.5
    u0 = s.kl_denoise(amap, w1, maxiter=57)                # the last solve: another parameter, another weight, another wo
    st0 = s.stats()
    out = torch.empty(O, N, M, dtype=torch.float64, device="cuda")

    def u_device():
        out.zero_(); torch.cuda.synchronize()
        s.copy_u_device(out.data_ptr())
        return out.cpu().numpy()

    def unchanged():
        assert _same(u_device(), u0)
        assert s.stats() == st0

    def rejected(code, call, *a, **k):
        with pytest.raises(BpltvError) as e:
            call(*a, **k)
        assert e.value.code == code, (e.value.code, str(e.value))
        unchanged()
        return str(e.value)

    unchanged()
    bad_gu = gu.copy(); bad_gu[1, 3, 4] = np.inf
    nan_map = amap.copy(); nan_map[2, 5] = np.nan
    for bad in (np.nan, -0.25, np.inf):
        bw = w.copy(); bw[1, 4, 7] = bad
        rejected(E_ARG, s.kl_denoise, 0.15, bw, maxiter=20)
        rejected(E_ARG, s.kl_unrolled_denoise, 0.15, bw, maxiter=20)
        rejected(E_ARG, s.kl_unrolled_vjp, 0.15, bw, gu, maxiter=20)
    for bad in (float("nan"), -0.1, nan_map):
        rejected(E_ARG, s.kl_denoise, bad, w, maxiter=20)
        rejected(E_ARG, s.kl_unrolled_denoise, bad, w, maxiter=20)
        rejected(E_ARG, s.kl_unrolled_vjp, bad, w, gu, maxiter=20)
    rejected(E_ARG, s.kl_unrolled_vjp, 0.15, w, bad_gu, maxiter=20)
    rejected(E_ARG, s.kl_denoise, 0.15, w, maxiter=0)
    rejected(E_ARG, s.kl_unrolled_denoise, 0.15, w, maxiter=0)
    for kw in (dict(rho=0.01), dict(init=1), dict(order=1)):
        rejected(E_UNSUPPORTED, s.kl_denoise, 0.15, w, maxiter=20, **kw)
        rejected(E_UNSUPPORTED, s.kl_unrolled_denoise, 0.15, w, maxiter=20, **kw)
        rejected(E_UNSUPPORTED, s.kl_unrolled_vjp, 0.15, w, gu, maxiter=20, **kw)
    p = s.params(maxiter=20)
    a1 = np.array([0.15])
    lib = s._lib
    gfh = np.empty_like(gu)
    assert lib.bpltv_kl_unrolled_vjp(s._h, _ptr(w), O, _ptr(a1), 1, 1, C.byref(p), _ptr(gu), None, None, None) == E_ARG
    assert lib.bpltv_kl_denoise(s._h, None, O, _ptr(a1), 1, 1, C.byref(p), None) == E_ARG                  # a NULL w
    assert lib.bpltv_kl_unrolled_denoise(s._h, None, O, _ptr(a1), 1, 1, C.byref(p), None) == E_ARG
    assert lib.bpltv_kl_unrolled_vjp(s._h, None, O, _ptr(a1), 1, 1, C.byref(p), _ptr(gu), _ptr(gfh), None, None) == E_ARG
    unchanged()
    for wo in (0, O + 1):                                          # a bad wo
        assert lib.bpltv_kl_denoise(s._h, _ptr(w), wo, _ptr(a1), 1, 1, C.byref(p), None) == E_ARG
        assert lib.bpltv_kl_unrolled_denoise(s._h, _ptr(w), wo, _ptr(a1), 1, 1, C.byref(p), None) == E_ARG
        assert lib.bpltv_kl_unrolled_vjp(s._h, _ptr(w), wo, _ptr(a1), 1, 1, C.byref(p), _ptr(gu), _ptr(gfh), None, None) == E_ARG
        unchanged()
    # the device forms
    gt, gfd = torch.tensor(gu, device="cuda"), torch.empty(O, N, M, dtype=torch.float64, device="cuda")
    good = torch.tensor([0.15], dtype=torch.float64, device="cuda")
    wt = torch.tensor(w, device="cuda")
    torch.cuda.synchronize()
    for bad in (np.nan, -0.25, np.inf):
        bwt = wt.clone(); bwt[1, 4, 7] = bad
        torch.cuda.synchronize()
        rejected(E_ARG, s.kl_denoise_device, bwt.data_ptr(), O, good.data_ptr(), 1, 1, maxiter=20)
        rejected(E_ARG, s.kl_unrolled_denoise_device, bwt.data_ptr(), O, good.data_ptr(), 1, 1, maxiter=20)
        rejected(E_ARG, s.kl_unrolled_vjp_device, None, bwt.data_ptr(), O, good.data_ptr(), 1, 1, gt.data_ptr(), gfd.data_ptr(), None,
                 None, maxiter=20)
    for wo in (0, O + 1):
        rejected(E_ARG, s.kl_denoise_device, wt.data_ptr(), wo, good.data_ptr(), 1, 1, maxiter=20)
        rejected(E_ARG, s.kl_unrolled_denoise_device, wt.data_ptr(), wo, good.data_ptr(), 1, 1, maxiter=20)
        rejected(E_ARG, s.kl_unrolled_vjp_device, None, wt.data_ptr(), wo, good.data_ptr(), 1, 1, gt.data_ptr(), gfd.data_ptr(), None,
                 None, maxiter=20)
    for kw in (dict(rho=0.01), dict(init=1), dict(order=1)):
        rejected(E_UNSUPPORTED, s.kl_denoise_device, wt.data_ptr(), O, good.data_ptr(), 1, 1, maxiter=20, **kw)
        rejected(E_UNSUPPORTED, s.kl_unrolled_denoise_device, wt.data_ptr(), O, good.data_ptr(), 1, 1, maxiter=20, **kw)
        rejected(E_UNSUPPORTED, s.kl_unrolled_vjp_device, None, wt.data_ptr(), O, good.data_ptr(), 1, 1, gt.data_ptr(), gfd.data_ptr(),
                 None, None, maxiter=20, **kw)
    rejected(E_ARG, s.kl_unrolled_vjp_device, None, wt.data_ptr(), O, good.data_ptr(), 1, 1, gt.data_ptr(), None, None, None, maxiter=20)
    # check_every and gap_tol are ignored
    assert _same(s.kl_denoise(amap, w1, maxiter=57, check_every=10, gap_tol=1e-3), u0)
    # the tapes are what they were: the KL tape, and the weighted and L1 tapes across the rejected and the accepted KL calls
    assert all(_same(x, y) for x, y in zip(s.kl_unrolled_vjp(0.15, w, gu, maxiter=20), g0))
    assert all(_same(x, y) for x, y in zip(s.weighted_unrolled_vjp(0.08, w, gu, maxiter=20), gw0))
    assert all(_same(x, y) for x, y in zip(s.l1_unrolled_vjp(0.7, w, gu, maxiter=20), gl0))
    # a sweep without a dataset: the KL tail reads the resident f
    n = gpu_solver_cls(M, N, O)
    tape = torch.zeros(s.weighted_unrolled_tape_doubles(maxiter=20), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    assert _code(n.kl_unrolled_vjp_device, tape.data_ptr(), wt.data_ptr(), O, good.data_ptr(), 1, 1, gt.data_ptr(), gfd.data_ptr(), None,
                 None, maxiter=20) == E_NODATA
    assert _code(n.kl_unrolled_vjp, 0.15, w, gu, maxiter=20) == E_NODATA
    n.close()
    s.close()


@pytest.mark.parametrize("bad", [-1e-300, -0.25, np.nan, np.inf])
def test_a_dataset_with_a_negative_entry_is_rejected_and_only_here(gpu_solver_cls, bad):
    """BPLTV_E_ARG with a message that names f, in host and device form, before anything of the handle changes: the last u, the
    statistics and every tape are what they were; the other models take the same dataset as before; and a good dataset installed
    afterwards is accepted again."""
    import torch
    from bpldenoising_amd._lib import BpltvError
    name = "2x17x33"
    O, N, M = SHAPES[name]
    f, gu = _data(name)
    w = _weight(name, "real")
    fb = f.copy()
    fb[1, 9, 20] = bad
    s = gpu_solver_cls(M, N, O)
    s.set_data(f, f)
    s.kl_unrolled_denoise(0.15, w, maxiter=20)
    g0 = s.kl_unrolled_vjp(0.15, w, gu, maxiter=20)
    s.weighted_unrolled_denoise(0.08, w, maxiter=20)
    gw0 = s.weighted_unrolled_vjp(0.08, w, gu, maxiter=20)
    u0 = s.kl_denoise(0.15, w, maxiter=30)
    s.set_data(f, fb)                                       # (installing a dataset drops the last result, as always)
    ref = gpu_solver_cls(M, N, O)
    ref.set_data(f, fb)
    finite = np.isfinite(bad)
    if finite:                                              # the other models accept it, here and on a fresh handle, with the same bits
        uw = s.weighted_denoise(0.08, w, maxiter=30)
        assert _same(uw, ref.weighted_denoise(0.08, w, maxiter=30))
        assert _same(s.l1_denoise(0.7, w, maxiter=30), ref.l1_denoise(0.7, w, maxiter=30))
        s.weighted_denoise(0.08, w, maxiter=30)
    else:
        uw = None                                           # (no other solve on a NaN or an Inf: set_data left no result)
    st0 = s.stats()
    out = torch.empty(O, N, M, dtype=torch.float64, device="cuda")
    wt = torch.tensor(w, device="cuda")
    good = torch.tensor([0.15], dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()

    def unchanged():
        if uw is None:
            assert _code(s.copy_u_device, out.data_ptr()) == E_NODATA
        else:
            out.zero_(); torch.cuda.synchronize()
            s.copy_u_device(out.data_ptr())
            assert _same(out.cpu().numpy(), uw)
        assert s.stats() == st0

    for call, args in ((s.kl_denoise, (0.15, w)), (s.kl_unrolled_denoise, (0.15, w)),
                       (s.kl_denoise_device, (wt.data_ptr(), O, good.data_ptr(), 1, 1)),
                       (s.kl_unrolled_denoise_device, (wt.data_ptr(), O, good.data_ptr(), 1, 1))):
        for rnd in range(2):                                # (the second call answers from what the first remembered)
            with pytest.raises(BpltvError) as e:
                call(*args, maxiter=20)
            assert e.value.code == E_ARG and " f " in str(e.value) and "dataset" in str(e.value), str(e.value)
            unchanged()
    # the tapes: the weighted one sweeps on (it reads f for grad_w only: ask for the others); the KL tape is still valid
    assert all(_same(x, y) for x, y in zip(s.weighted_unrolled_vjp(0.08, w, gu, want_w=False, maxiter=20), gw0[:2]))
    s.set_data(f, f)
    assert all(_same(x, y) for x, y in zip(s.kl_unrolled_vjp(0.15, w, gu, maxiter=20), g0))
    assert _same(s.kl_denoise(0.15, w, maxiter=30), u0)     # a good dataset again: looked at anew
    ref.close()
    s.close()


def test_the_duality_gap_is_unsupported_until_another_model_solves(gpu_solver_cls):
    name = "2x17x33"
    O, N, M = SHAPES[name]
    f, _ = _data(name)
    w = _weight(name, "real")
    s = gpu_solver_cls(M, N, O)
    s.set_data(f, f)
    s.denoise(0.08, maxiter=30)
    gap0 = s.duality_gap()
    for solve in (lambda: s.kl_denoise(0.15, w, maxiter=30), lambda: s.kl_unrolled_denoise(0.15, w, maxiter=30)):
        solve()
        assert _code(s.duality_gap) == E_UNSUPPORTED
        assert _code(s.duality_gap) == E_UNSUPPORTED
        s.denoise(0.08, maxiter=30)
        assert _same(s.duality_gap(), gap0)
    s.kl_denoise(0.15, w, maxiter=30)
    s.l1_denoise(0.7, w, maxiter=30)                        # (L1's own refusal, not this model's, and the reverse)
    assert _code(s.duality_gap) == E_UNSUPPORTED
    s.kl_denoise(0.15, w, maxiter=30)
    assert _code(s.duality_gap) == E_UNSUPPORTED
    s.weighted_denoise(0.08, w, maxiter=30)
    assert np.isfinite(s.duality_gap()).all()
    s.close()


# ---- 7. shards, float handles, graphs ------------------------------------------------------------------------------------
def test_two_shards_are_unsupported_and_one_is_forwarded(gpu_solver_cls):
    from bpldenoising_amd._lib import BpltvError
    name = "2x17x33"
    O, N, M = SHAPES[name]
    f, gu = _data(name)
    w = _weight(name, "mask")
    m = gpu_solver_cls(M, N, O, devices=[0, 0])
    m.set_data(f, f)
    u0 = m.denoise(0.07, maxiter=30)
    gap0 = m.duality_gap()
    for call, args in ((m.kl_denoise, (0.15, w)), (m.kl_unrolled_denoise, (0.15, w)), (m.kl_unrolled_vjp, (0.15, w, gu)),
                       (m.kl_denoise_device, (1, 1, 1, 1, 1)), (m.kl_unrolled_denoise_device, (1, 1, 1, 1, 1)),
                       (m.kl_unrolled_vjp_device, (None, 1, 1, 1, 1, 1, 1, 1, 1, 1))):
        with pytest.raises(BpltvError) as e:     # (the device forms are refused before any pointer is read)
            call(*args, maxiter=30)
        assert e.value.code == E_UNSUPPORTED
        assert _same(m.duality_gap(), gap0) and _same(m.denoise(0.07, maxiter=30), u0)
    m.close()
    one = gpu_solver_cls(M, N, O, ngpus=1)       # one shard holds everything: forwarded
    one.set_data(f, f)
    s = gpu_solver_cls(M, N, O)
    s.set_data(f, f)
    assert _same(one.kl_denoise(0.15, w, maxiter=30), s.kl_denoise(0.15, w, maxiter=30))
    assert _same(one.kl_unrolled_denoise(0.15, w, maxiter=30), s.kl_unrolled_denoise(0.15, w, maxiter=30))
    a, b = one.kl_unrolled_vjp(0.15, w, gu, maxiter=30), s.kl_unrolled_vjp(0.15, w, gu, maxiter=30)
    assert all(_same(x, y) for x, y in zip(a, b))
    one.close()
    s.close()


def test_float_handles_run_the_kl_model_in_float64(gpu_solver_cls):
    name = "2x17x33"
    O, N, M = SHAPES[name]
    f, gu = _data(name)
    w = _weight(name, "real")
    s, s32 = gpu_solver_cls(M, N, O), gpu_solver_cls(M, N, O, dtype=32)
    for h in (s, s32):
        h.set_data(f, f)
    assert _same(s32.kl_denoise(0.15, w, maxiter=40), s.kl_denoise(0.15, w, maxiter=40))
    assert _same(s32.kl_unrolled_denoise(0.15, w, maxiter=40), s.kl_unrolled_denoise(0.15, w, maxiter=40))
    a, b = s32.kl_unrolled_vjp(0.15, w, gu, maxiter=40), s.kl_unrolled_vjp(0.15, w, gu, maxiter=40)
    assert all(_same(x, y) for x, y in zip(a, b))
    s.close()
    s32.close()


def test_no_graph_is_shared_with_the_weighted_or_the_l1_model(gpu_solver_cls):
    """The same w, alpha, K and shapes, w with min w = 0 so that even the step table is the same buffer for all three models:
    their solves and sweeps, in both orders, twice (the second round replays what the first cached), each give what a fresh
    handle gives."""
    name = "3x40x48"
    O, N, M = SHAPES[name]
    f, gu = _data(name)
    w = _weight(name, "mask")
    alpha, K = 0.15, 57

    def fresh(call):
        h = gpu_solver_cls(M, N, O)
        h.set_data(f, f)
        r = call(h)
        h.close()
        return r
    u_w, g_w = fresh(lambda h: (h.weighted_unrolled_denoise(alpha, w, maxiter=K), h.weighted_unrolled_vjp(alpha, w, gu, maxiter=K)))
    u_l, g_l = fresh(lambda h: (h.l1_unrolled_denoise(alpha, w, maxiter=K), h.l1_unrolled_vjp(alpha, w, gu, maxiter=K)))
    u_k, g_k = fresh(lambda h: (h.kl_unrolled_denoise(alpha, w, maxiter=K), h.kl_unrolled_vjp(alpha, w, gu, maxiter=K)))
    assert float(np.abs(u_w - u_k).max()) > 1e-4 and float(np.abs(u_l - u_k).max()) > 1e-4
    for order in ("kl first", "kl last"):
        h = gpu_solver_cls(M, N, O)
        h.set_data(f, f)
        for rnd in range(2):
            if order == "kl first":
                assert _same(h.kl_unrolled_denoise(alpha, w, maxiter=K), u_k) and _same(h.kl_denoise(alpha, w, maxiter=K), u_k)
            assert _same(h.weighted_unrolled_denoise(alpha, w, maxiter=K), u_w)
            assert _same(h.weighted_denoise(alpha, w, maxiter=K), u_w)
            assert _same(h.l1_unrolled_denoise(alpha, w, maxiter=K), u_l) and _same(h.l1_denoise(alpha, w, maxiter=K), u_l)
            if order == "kl last":
                assert _same(h.kl_denoise(alpha, w, maxiter=K), u_k) and _same(h.kl_unrolled_denoise(alpha, w, maxiter=K), u_k)
            for want_w in (True, False):
                g = h.weighted_unrolled_vjp(alpha, w, gu, want_w=want_w, maxiter=K)   # each tape holds what its own solve recorded
                assert all(_same(x, y) for x, y in zip(g[:2 + want_w], g_w))
                g = h.l1_unrolled_vjp(alpha, w, gu, want_w=want_w, maxiter=K)
                assert all(_same(x, y) for x, y in zip(g[:2 + want_w], g_l))
                g = h.kl_unrolled_vjp(alpha, w, gu, want_w=want_w, maxiter=K)
                assert all(_same(x, y) for x, y in zip(g[:2 + want_w], g_k))
        h.close()
