"""GPU checks of reverse mode through the PDHG iterations (bpltv_unrolled_denoise / bpltv_unrolled_vjp and their device
forms).

u is tied to bpltv_denoise bit for bit, which pins the taped forward kernel to the oracle; the gradients are held against
the numpy twin tests/unrolled_ref.py (pinned on the CPU by tests/test_unrolled_abi.py) and against central differences of
bpltv_denoise itself; every plan (fusion depth, launch chains, graphs, host or device form, whose tape) gives the same
bits; and a rejected call leaves the handle as it was."""
import ctypes as C
import functools

import numpy as np
import pytest
from conftest import synth_batch

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
    O, N, M = SHAPES[name]
    ub, f = synth_batch(O, N, M, seed=seed + M)
    gu = np.random.default_rng(seed + 100).standard_normal(f.shape)
    for a in (ub, f, gu):
        a.setflags(write=False)
    return ub, f, gu


# ---- 1. u is bpltv_denoise's, bit for bit -----------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["scalar", "patch", "map"])
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_u_is_the_plain_denoise_bitwise(gpu_solver_cls, name, kind):
    O, N, M = SHAPES[name]
    _, f, _ = _data(name)
    alpha = _alpha(kind, N, M)
    s = gpu_solver_cls(M, N, O)
    s.set_data(f, f)
    for accel in (1, 0):
        for maxiter in (1, 7, 203):
            u0 = s.denoise(alpha, maxiter=maxiter, accel=accel)
            g0 = s.duality_gap()
            u1 = s.unrolled_denoise(alpha, maxiter=maxiter, accel=accel)
            assert _same(u1, u0), (accel, maxiter, float(np.abs(u1 - u0).max()))
            st = s.stats()
            assert st["iterations"] == maxiter and st["pdhg_variant"] == 0 and st["launches"] >= 1 and st["tiles"] >= O, st
            assert st["bytes_per_px_iter"] == (80.0 if kind == "map" and N * M > 1 else 72.0)
            assert s.unrolled_tape_doubles(maxiter=maxiter) == 2 * maxiter * M * N * O
            # the solve is the handle's last TV solve: its gap is the plain solve's, bit for bit
            assert _same(s.duality_gap(), g0)
    s.close()


# ---- 2. the gradients against the twin --------------------------------------------------------------------------------
def _bounds(gf0, ga0, alpha, O, N, M):
    """1e-11 * max|ref| for grad_f; for grad_alpha relative to the largest per-pixel term of the reference times the number
    of terms summed into one entry."""
    return 1e-11 * float(np.abs(gf0).max()), 1e-11 * float(np.abs(ga0).max()) * O * ur.pixels_per_entry(alpha, M, N)


@pytest.mark.parametrize("kind", ["scalar", "patch", "map"])
@pytest.mark.parametrize("name", ["3x40x48", "2x17x33", "1x1x9", "1x9x1"])
def test_gradients_match_the_twin(gpu_solver_cls, name, kind):
    """Measured on MI355X: grad_f at most 8.4e-14 against bounds of 2e-11, grad_alpha at most
    3.4e-13 against bounds of 6e-11 (map) ... 1.9e-7 (scalar, 3x40x48); the degenerate shapes stay below 1e-15."""
    O, N, M = SHAPES[name]
    _, f, gu = _data(name)
    alpha = _alpha(kind, N, M)
    amap = tw.alpha_to_map(alpha, M, N)
    s = gpu_solver_cls(M, N, O)
    s.set_data(f, f)
    for K in (50, 203):
        u0, tape, tab = ur.fwd_tape(f, amap, K)
        gf0, ga0 = ur.reverse(gu, tape, tab, amap)
        u = s.unrolled_denoise(alpha, maxiter=K)
        gf, ga = s.unrolled_vjp(alpha, gu, maxiter=K)
        st = s.stats()
        assert st["adjoint_method"] == "unrolled" and st["adjoint_ms"] > 0.0 and st["iterations"] == K, st
        bf, ba = _bounds(gf0, ga0, alpha, O, N, M)
        df = float(np.abs(gf - gf0).max())
        da = float(np.abs(np.asarray(ga) - np.asarray(ur.reduce_alpha(ga0, alpha))).max())
        print("%s %s K %d: max|du| %.2e  grad_f %.2e (bound %.2e)  grad_alpha %.2e (bound %.2e)"
              % (name, kind, K, float(np.abs(u - u0).max()), df, bf, da, ba))
        assert df <= bf
        assert da <= ba
    s.close()


# ---- 3. every plan gives the same bits --------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["scalar", "map"])
def test_results_do_not_depend_on_the_plan(gpu_solver_cls, kind):
    import torch
    name = "2x70x72"
    O, N, M = SHAPES[name]
    _, f, gu = _data(name)
    alpha = _alpha(kind, N, M)
    a = np.atleast_1d(np.asarray(alpha, dtype=np.float64))
    an, am = (1, 1) if kind == "scalar" else a.shape
    s = gpu_solver_cls(M, N, O)
    s.set_data(f, f)
    for K in (203, 200):   # 200 iterations at depth 8: the second chain runs half a launch out of phase
        u0 = s.unrolled_denoise(alpha, maxiter=K)
        gf0, ga0 = s.unrolled_vjp(alpha, gu, maxiter=K)
        assert _same(u0, s.denoise(alpha, maxiter=K))
        plans = [dict(), dict(tile_iters=4), dict(tile_iters=8), dict(chains=1), dict(chains=2), dict(use_graph=0),
                 dict(chains=2, use_graph=0), dict(tile_iters=4, chains=2)]
        for kw in plans:
            u = s.unrolled_denoise(alpha, maxiter=K, **kw)
            if "chains" in kw:
                assert s.stats()["launch_chains"] == (kw["chains"] if kw.get("use_graph", 1) else 1)
            gf, ga = s.unrolled_vjp(alpha, gu, maxiter=K, **kw)
            assert _same(u, u0) and _same(gf, gf0) and _same(ga, ga0), kw
        # the device forms, on the handle's tape and on a caller's
        at, gt = torch.tensor(a, device="cuda"), torch.tensor(gu, device="cuda")
        out, gfd = torch.empty(O, N, M, dtype=torch.float64, device="cuda"), torch.empty(O, N, M, dtype=torch.float64, device="cuda")
        gad = torch.empty(am * an, dtype=torch.float64, device="cuda")
        tape = torch.empty(s.unrolled_tape_doubles(maxiter=K), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        for tp in (None, tape.data_ptr(), tape.data_ptr()):   # (a repeated call replays the cached graphs)
            gfd.zero_(); gad.zero_(); torch.cuda.synchronize()
            s.unrolled_denoise_device(at.data_ptr(), am, an, tape_ptr=tp, maxiter=K)
            s.copy_u_device(out.data_ptr())
            s.unrolled_vjp_device(tp, at.data_ptr(), am, an, gt.data_ptr(), gfd.data_ptr(), gad.data_ptr(), maxiter=K)
            assert _same(out.cpu().numpy(), u0) and _same(gfd.cpu().numpy(), gf0)
            assert _same(gad.cpu().numpy().reshape(np.shape(ga0)), ga0)
        # one output at a time
        assert _same(s.unrolled_vjp(alpha, gu, want_alpha=False, maxiter=K)[0], gf0)
        assert _same(s.unrolled_vjp(alpha, gu, want_f=False, maxiter=K)[1], ga0)
    s.close()


# ---- 4. finite differences of bpltv_denoise itself ----------------------------------------------------------------------
@pytest.mark.parametrize("K", [30, 300])
def test_scalar_gradient_against_central_differences_on_the_device(gpu_solver_cls, K):
    """d/dalpha of 0.5 |u_K - ubar|^2, 1 x 24 x 28, alpha = 0.08, h = 1e-6, relative 1e-5: the margin of the CPU test."""
    ub, f = synth_batch(1, 24, 28, seed=9)
    alpha, h = 0.08, 1e-6
    s = gpu_solver_cls(28, 24, 1)
    s.set_data(ub, f)
    u = s.unrolled_denoise(alpha, maxiter=K)
    _, g = s.unrolled_vjp(alpha, u - ub, want_f=False, maxiter=K)
    fd = (tw.l2_cost(s.denoise(alpha + h, maxiter=K), ub) - tw.l2_cost(s.denoise(alpha - h, maxiter=K), ub)) / (2 * h)
    print("K %d: reverse sweep %.10g central difference %.10g rel %.2e" % (K, g, fd, abs(g - fd) / abs(fd)))
    assert abs(g - fd) <= 1e-5 * abs(fd)
    s.close()


# ---- 5. the tape's contract -------------------------------------------------------------------------------------------
def test_zero_cotangent_and_the_handle_s_tape(gpu_solver_cls):
    from bpldenoising_amd._lib import BpltvError
    name = "2x17x33"
    O, N, M = SHAPES[name]
    _, f, gu = _data(name)
    s = gpu_solver_cls(M, N, O)
    s.set_data(f, f)
    with pytest.raises(BpltvError) as e:       # no tape yet
        s.unrolled_vjp(0.08, gu, maxiter=20)
    assert e.value.code == E_NODATA
    s.unrolled_denoise(0.08, maxiter=20)
    st0 = s.stats()
    assert st0["iterations"] == 20 and st0["tiles"] >= O and st0["tile_iters"] >= 1 and st0["launch_chains"] >= 1, st0

    def sweep_stats():
        """what a reverse sweep leaves: its own adjoint fields, and the solve fields the taped solve left"""
        st = s.stats()
        assert st["adjoint_method"] == "unrolled" and st["adjoint_attempts"] == 1 and st["adjoint_residual"] == 0.0, st
        assert all(st[k] == st0[k] for k in ("iterations", "tile_iters", "tiles", "launch_chains")), (st, st0)

    gf, ga = s.unrolled_vjp(0.08, np.zeros_like(gu), maxiter=20)
    sweep_stats()
    assert not gf.any() and ga == 0.0
    gf, ga = s.unrolled_vjp(0.08, gu, maxiter=20)
    sweep_stats()
    assert gf.any() and ga != 0.0
    s.unrolled_denoise(0.08, maxiter=12)       # a second, shorter solve: the tape is now its
    st0 = s.stats()
    assert st0["iterations"] == 12, st0
    with pytest.raises(BpltvError) as e:
        s.unrolled_vjp(0.08, gu, maxiter=20)
    assert e.value.code == E_ARG
    for kw in (dict(accel=0), dict(tau0=4.0), dict(sigma0=0.1), dict(opnorm=2.5)):   # other steps than the tape's
        with pytest.raises(BpltvError) as e:
            s.unrolled_vjp(0.08, gu, maxiter=12, **kw)
        assert e.value.code == E_ARG
    with pytest.raises(BpltvError) as e:       # another parameter shape
        s.unrolled_vjp(np.full((2, 2), 0.08), gu, maxiter=12)
    assert e.value.code == E_ARG
    assert _same(s.unrolled_vjp(0.08, gu, maxiter=12)[0], s.unrolled_vjp(0.08, gu, maxiter=12)[0])
    sweep_stats()                              # (the rejected sweeps in between changed nothing either)
    n = gpu_solver_cls(M, N, O)                # no dataset
    with pytest.raises(BpltvError) as e:
        n.unrolled_denoise(0.08, maxiter=5)
    assert e.value.code == E_NODATA
    n.close()
    s.close()


# ---- 6. rejections leave the handle as it was ---------------------------------------------------------------------------
def test_rejections_leave_the_handle_as_it_was(gpu_solver_cls):
    import torch
    from bpldenoising_amd._lib import BpltvError
    name = "2x17x33"
    O, N, M = SHAPES[name]
    _, f, gu = _data(name)
    s = gpu_solver_cls(M, N, O)
    s.set_data(f, f)
    amap = _alpha("map", N, M)
    s.unrolled_denoise(0.08, maxiter=20)
    gf0, ga0 = s.unrolled_vjp(0.08, gu, maxiter=20)
    u0 = s.denoise(amap, maxiter=57)           # the last solve: another parameter, another shape
    gap0 = s.duality_gap()

    def unchanged():
        assert _same(s.duality_gap(), gap0)
        assert _same(s.denoise(amap, maxiter=57), u0) and _same(s.duality_gap(), gap0)
        gf, ga = s.unrolled_vjp(0.08, gu, maxiter=20)      # ... and the tape is still the first solve's
        assert _same(gf, gf0) and _same(ga, ga0)
        assert _same(s.denoise(amap, maxiter=57), u0)

    def rejected(code, call, *a, **k):
        with pytest.raises(BpltvError) as e:
            call(*a, **k)
        assert e.value.code == code, (e.value.code, str(e.value))
        unchanged()

    bad_gu = gu.copy(); bad_gu[1, 3, 4] = np.inf
    nan_map = amap.copy(); nan_map[2, 5] = np.nan
    for bad in (float("nan"), -0.1, nan_map):
        rejected(E_ARG, s.unrolled_denoise, bad, maxiter=20)
        rejected(E_ARG, s.unrolled_vjp, bad, gu, maxiter=20)
    rejected(E_ARG, s.unrolled_vjp, 0.08, bad_gu, maxiter=20)
    rejected(E_ARG, s.unrolled_denoise, 0.08, maxiter=0)
    for kw in (dict(rho=0.01), dict(init=1), dict(order=1)):
        rejected(E_UNSUPPORTED, s.unrolled_denoise, 0.08, maxiter=20, **kw)
        rejected(E_UNSUPPORTED, s.unrolled_vjp, 0.08, gu, maxiter=20, **kw)
    p = s.params(maxiter=20)
    a1 = np.array([0.08])
    rc = s._lib.bpltv_unrolled_vjp(s._h, _ptr(a1), 1, 1, C.byref(p), _ptr(gu), None, None)   # both outputs NULL
    assert rc == E_ARG
    unchanged()
    # the device forms
    gt, gfd = torch.tensor(gu, device="cuda"), torch.empty(O, N, M, dtype=torch.float64, device="cuda")
    good = torch.tensor([0.08], dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    for bad in (float("nan"), -0.1):
        bt = torch.tensor([bad], dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        rejected(E_ARG, s.unrolled_denoise_device, bt.data_ptr(), 1, 1, maxiter=20)
        rejected(E_ARG, s.unrolled_vjp_device, None, bt.data_ptr(), 1, 1, gt.data_ptr(), gfd.data_ptr(), None, maxiter=20)
    bgt = torch.tensor(bad_gu, device="cuda")
    torch.cuda.synchronize()
    rejected(E_ARG, s.unrolled_vjp_device, None, good.data_ptr(), 1, 1, bgt.data_ptr(), gfd.data_ptr(), None, maxiter=20)
    rejected(E_ARG, s.unrolled_vjp_device, None, good.data_ptr(), 1, 1, gt.data_ptr(), None, None, maxiter=20)
    s.close()


def test_two_shards_are_unsupported(gpu_solver_cls):
    from bpldenoising_amd._lib import BpltvError
    name = "2x17x33"
    O, N, M = SHAPES[name]
    _, f, gu = _data(name)
    m = gpu_solver_cls(M, N, O, devices=[0, 0])
    m.set_data(f, f)
    u0 = m.denoise(0.07, maxiter=30)
    gap0 = m.duality_gap()
    for call, args in ((m.unrolled_denoise, (0.07,)), (m.unrolled_vjp, (0.07, gu)),
                       (m.unrolled_denoise_device, (1, 1, 1)), (m.unrolled_vjp_device, (None, 1, 1, 1, 1, 1, 1))):
        with pytest.raises(BpltvError) as e:     # (the device forms are refused before any pointer is read)
            call(*args, maxiter=30)
        assert e.value.code == E_UNSUPPORTED
        assert _same(m.duality_gap(), gap0) and _same(m.denoise(0.07, maxiter=30), u0)
    m.close()
    one = gpu_solver_cls(M, N, O, ngpus=1)       # one shard holds everything: forwarded
    one.set_data(f, f)
    s = gpu_solver_cls(M, N, O)
    s.set_data(f, f)
    assert _same(one.unrolled_denoise(0.07, maxiter=30), s.unrolled_denoise(0.07, maxiter=30))
    assert _same(one.unrolled_vjp(0.07, gu, maxiter=30)[0], s.unrolled_vjp(0.07, gu, maxiter=30)[0])
    one.close()
    s.close()


def test_float_handles_run_the_unrolled_solve_in_float64(gpu_solver_cls):
    name = "2x17x33"
    O, N, M = SHAPES[name]
    _, f, gu = _data(name)
    s, s32 = gpu_solver_cls(M, N, O), gpu_solver_cls(M, N, O, dtype=32)
    for h in (s, s32):
        h.set_data(f, f)
    assert _same(s32.unrolled_denoise(0.08, maxiter=40), s.unrolled_denoise(0.08, maxiter=40))
    a, b = s32.unrolled_vjp(0.08, gu, maxiter=40), s.unrolled_vjp(0.08, gu, maxiter=40)
    assert _same(a[0], b[0]) and _same(a[1], b[1])
    s.close()
    s32.close()


# ---- 7. no graph is shared with another solve --------------------------------------------------------------------------
def test_unrolled_and_other_solves_never_replay_each_other_s_graphs(gpu_solver_cls):
    name = "3x40x48"
    O, N, M = SHAPES[name]
    _, f, gu = _data(name)
    w = 0.25 + 3.75 * np.random.default_rng(3).random((N, M))
    alpha, K = 0.08, 57

    def fresh(call):
        h = gpu_solver_cls(M, N, O)
        h.set_data(f, f)
        r = call(h)
        h.close()
        return r
    u_plain = fresh(lambda h: h.denoise(alpha, maxiter=K))
    u_w = fresh(lambda h: h.weighted_denoise(alpha, w, maxiter=K))
    u_un, g_un = fresh(lambda h: (h.unrolled_denoise(alpha, maxiter=K), h.unrolled_vjp(alpha, gu, maxiter=K)))
    assert _same(u_un, u_plain) and not _same(u_w, u_plain)
    for order in ("unrolled first", "unrolled last"):
        h = gpu_solver_cls(M, N, O)
        h.set_data(f, f)
        for rnd in range(2):   # the second round replays what the first one cached
            if order == "unrolled first":
                assert _same(h.unrolled_denoise(alpha, maxiter=K), u_un)
            assert _same(h.denoise(alpha, maxiter=K), u_plain)
            assert _same(h.weighted_denoise(alpha, w, maxiter=K), u_w)
            if order == "unrolled last":
                assert _same(h.unrolled_denoise(alpha, maxiter=K), u_un)
            gf, ga = h.unrolled_vjp(alpha, gu, maxiter=K)   # the tape survives the other models' solves
            assert _same(gf, g_un[0]) and _same(ga, g_un[1])
        h.close()
