"""GPU checks of reverse mode through the iterations of the sum-of-regularisers model (bpltv_sumregs_unrolled_denoise /
bpltv_sumregs_unrolled_vjp, their _each and device forms).

u is tied to bpltv_sumregs_denoise bit for bit, for both of its kernel variants; the gradients are held against the numpy
twin tests/sumregs_unrolled_ref.py (pinned on the CPU by tests/test_sumregs_unrolled_abi.py) and against central differences
of bpltv_sumregs_denoise itself; every plan (fusion depth, launch chains, graphs, host or device form, whose tape) gives the
same bits; the per-image forms are the one-image results; and a rejected call leaves the handle as it was."""
import ctypes as C
import functools

import numpy as np
import pytest

import sumregs_unrolled_ref as sur
import unrolled_ref as ur
from oracle import np_twin as tw
from oracle import np_twin_sumregs as sr

pytestmark = pytest.mark.gpu

E_ARG, E_NODATA, E_UNSUPPORTED = 1, 3, 6
_dp = C.POINTER(C.c_double)
SHAPES = sur.GPU_SHAPES
_alpha = sur.alpha_of
VEC = np.array([0.03, 0.02, 0.04])


def _same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b))


def _ptr(a):
    return a.ctypes.data_as(_dp) if a is not None else None


@functools.lru_cache(maxsize=None)
def _data(name, kind="vector"):
    f, gu = sur.gpu_data(name, kind)
    for a in (f, gu):
        a.setflags(write=False)
    return f, gu


@functools.lru_cache(maxsize=None)
def _twin(name, kind, K):
    """(u, grad_f, ga (3, O, N, M)) of the twin for a GPU case: computed once, shared, left unchanged."""
    O, N, M = SHAPES[name]
    f, gu = _data(name, kind)
    alpha = _alpha(kind, N, M)
    u, tape, tab = sur.fwd_tape(f, alpha, K)
    gf, ga = sur.reverse(gu, tape, tab, sr.alpha_maps(alpha, M, N))
    for a in (u, gf, ga):
        a.setflags(write=False)
    return u, gf, ga


def _shape_args(alpha):
    a = np.asarray(alpha, dtype=np.float64)
    return (1, 1) if a.ndim == 1 else (a.shape[2], a.shape[1])   # (am, an)


# ---- 1. u is bpltv_sumregs_denoise's, bit for bit -----------------------------------------------------------------------
@pytest.mark.parametrize("kind", sur.ALPHA_KINDS)
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_u_is_the_sumregs_denoise_bitwise(gpu_solver_cls, name, kind):
    O, N, M = SHAPES[name]
    f, _ = _data(name)
    alpha = _alpha(kind, N, M)
    s = gpu_solver_cls(M, N, O)
    s.set_data(f, f)
    for maxiter in (1, 7, 203):
        for accel in (1, 0):
            u1 = s.sumregs_denoise(alpha, maxiter=maxiter, accel=accel, variant=1)
            g0 = s.duality_gap()
            u2 = s.sumregs_denoise(alpha, maxiter=maxiter, accel=accel, variant=2)
            u = s.sumregs_unrolled_denoise(alpha, maxiter=maxiter, accel=accel)
            assert _same(u, u1) and _same(u, u2), (accel, maxiter, float(np.abs(u - u1).max()))
            st = s.stats()
            assert st["iterations"] == maxiter and st["pdhg_variant"] == 0 and st["launches"] >= 1 and st["tiles"] >= O, st
            assert 1 <= st["tile_iters"] <= 7 and st["pdhg_ms"] > 0.0 and st["total_ms"] >= st["pdhg_ms"], st
            is_map = np.ndim(alpha) == 3 and np.shape(alpha)[1:] == (N, M) and N * M > 1   # (a 2 x 2 patch on 2 x 2 is one)
            assert st["bytes_per_px_iter"] == (192.0 if is_map else 168.0)
            assert s.sumregs_unrolled_tape_doubles(maxiter=maxiter) == 6 * maxiter * M * N * O
            assert _same(s.duality_gap(), g0)      # the handle's last solve is a sum-of-regularisers solve: the plain one's gap
            for v in (1, 2):                       # reserved[0], the forward variant, is ignored
                assert _same(s.sumregs_unrolled_denoise(alpha, maxiter=maxiter, accel=accel, variant=v), u)
    s.close()


# ---- 2. the gradients against the twin --------------------------------------------------------------------------------
def _bounds(gf0, ga0, alpha, O, N, M):
    """tests/test_gpu_unrolled.py's _bounds: 1e-11 * max|ref| for grad_f; for grad_alpha relative to the largest per-pixel
    term of the reference times the number of terms summed into one entry."""
    a = np.asarray(alpha)
    ppe = M * N if a.ndim == 1 else ur.pixels_per_entry(a[0], M, N)
    return 1e-11 * float(np.abs(gf0).max()), 1e-11 * float(np.abs(ga0).max()) * O * ppe


@pytest.mark.parametrize("kind", sur.ALPHA_KINDS)
@pytest.mark.parametrize("name", sur.GRADIENT_SHAPES)
def test_gradients_match_the_twin(gpu_solver_cls, name, kind):
    """Measured on MI355X: see the table in DESIGN.md section 4.9."""
    O, N, M = SHAPES[name]
    f, gu = _data(name, kind)
    alpha = _alpha(kind, N, M)
    s = gpu_solver_cls(M, N, O)
    s.set_data(f, f)
    for K in sur.GRADIENT_K:
        u0, gf0, ga0 = _twin(name, kind, K)
        u = s.sumregs_unrolled_denoise(alpha, maxiter=K)
        st0 = s.stats()
        gf, ga = s.sumregs_unrolled_vjp(alpha, gu, maxiter=K)
        st = s.stats()
        assert st["adjoint_method"] == "sumregs-unrolled" and st["adjoint_ms"] > 0.0 and st["iterations"] == K, st
        changed = {k for k in st if st[k] != st0[k]}
        assert changed <= {"adjoint_ms", "adjoint_method"}, changed
        bf, ba = _bounds(gf0, ga0, alpha, O, N, M)
        df = float(np.abs(gf - gf0).max())
        da = float(np.abs(ga - sur.reduce_alpha(ga0, alpha)).max())
        print("%s %s K %d: max|du| %.2e  grad_f %.2e (bound %.2e)  grad_alpha %.2e (bound %.2e)"
              % (name, kind, K, float(np.abs(u - u0).max()), df, bf, da, ba))
        assert ga.shape == np.shape(alpha) and np.isfinite(ga).all()
        assert df <= bf
        assert da <= ba
    s.close()


# ---- 3. every plan gives the same bits --------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["vector", "patch", "map"])
def test_results_do_not_depend_on_the_plan(gpu_solver_cls, kind):
    import torch
    name = "2x70x72"
    O, N, M = SHAPES[name]
    f, gu = _data(name)
    alpha = _alpha(kind, N, M)
    am, an = _shape_args(alpha)
    s = gpu_solver_cls(M, N, O)
    s.set_data(f, f)
    for K in (203, 200):   # 200 iterations at depth 4: the second chain runs half a launch out of phase
        u0 = s.sumregs_unrolled_denoise(alpha, maxiter=K)
        gf0, ga0 = s.sumregs_unrolled_vjp(alpha, gu, maxiter=K)
        assert _same(u0, s.sumregs_denoise(alpha, maxiter=K))
        plans = [dict(tile_iters=1), dict(tile_iters=2), dict(tile_iters=4), dict(chains=1), dict(chains=2), dict(use_graph=0),
                 dict(chains=2, use_graph=0), dict(tile_iters=2, chains=2)]
        for kw in plans:
            u = s.sumregs_unrolled_denoise(alpha, maxiter=K, **kw)
            if "chains" in kw:
                assert s.stats()["launch_chains"] == (kw["chains"] if kw.get("use_graph", 1) else 1)
            if "tile_iters" in kw:
                assert s.stats()["tile_iters"] == kw["tile_iters"]
            gf, ga = s.sumregs_unrolled_vjp(alpha, gu, maxiter=K, **kw)
            assert _same(u, u0) and _same(gf, gf0) and _same(ga, ga0), kw
        # the device forms, on the handle's tape and on a caller's
        at, gt = torch.tensor(np.ascontiguousarray(alpha), device="cuda"), torch.tensor(gu, device="cuda")
        out, gfd = torch.empty(O, N, M, dtype=torch.float64, device="cuda"), torch.empty(O, N, M, dtype=torch.float64, device="cuda")
        gad = torch.empty(3 * am * an, dtype=torch.float64, device="cuda")
        tape = torch.empty(s.sumregs_unrolled_tape_doubles(maxiter=K), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        for tp in (None, tape.data_ptr(), tape.data_ptr()):   # (a repeated call replays the cached graphs)
            gfd.zero_(); gad.zero_(); torch.cuda.synchronize()
            s.sumregs_unrolled_denoise_device(at.data_ptr(), am, an, tape_ptr=tp, maxiter=K)
            s.copy_u_device(out.data_ptr())
            s.sumregs_unrolled_vjp_device(tp, at.data_ptr(), am, an, gt.data_ptr(), gfd.data_ptr(), gad.data_ptr(), maxiter=K)
            assert _same(out.cpu().numpy(), u0) and _same(gfd.cpu().numpy(), gf0)
            assert _same(gad.cpu().numpy().reshape(np.shape(ga0)), ga0)
        # one output at a time
        assert _same(s.sumregs_unrolled_vjp(alpha, gu, want_alpha=False, maxiter=K)[0], gf0)
        assert _same(s.sumregs_unrolled_vjp(alpha, gu, want_f=False, maxiter=K)[1], ga0)
    s.close()


# ---- 4. one block per image ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["vector", "patch", "map"])
@pytest.mark.parametrize("name", ["2x40x48", "2x17x33"])
def test_each_is_the_one_image_handle_image_by_image(gpu_solver_cls, name, kind):
    from bpldenoising_amd._lib import BpltvError
    O, N, M = SHAPES[name]
    f, gu = _data(name)
    a0 = _alpha(kind, N, M)
    blocks = np.stack([a0, 1.5 * a0])
    K = 57
    s = gpu_solver_cls(M, N, O)
    s.set_data(f, f)
    u = s.sumregs_unrolled_denoise_each(blocks, maxiter=K)
    assert _same(u, s.sumregs_denoise_each(blocks, maxiter=K))
    g_plain = s.duality_gap()
    u = s.sumregs_unrolled_denoise_each(blocks, maxiter=K)
    assert _same(s.duality_gap(), g_plain)
    gf, ga = s.sumregs_unrolled_vjp_each(blocks, gu, maxiter=K)
    assert ga.shape == blocks.shape
    with pytest.raises(BpltvError) as e:        # the shared form on a per-image tape
        s.sumregs_unrolled_vjp(a0, gu, maxiter=K)
    assert e.value.code == E_ARG
    one = gpu_solver_cls(M, N, 1)
    for k in range(O):
        one.set_data(f[k:k + 1], f[k:k + 1])
        uk = one.sumregs_unrolled_denoise(blocks[k], maxiter=K)
        gfk, gak = one.sumregs_unrolled_vjp(blocks[k], gu[k:k + 1], maxiter=K)
        assert _same(u[k], uk[0]) and _same(gf[k], gfk[0]) and _same(ga[k], gak), k
    one.close()
    # equal blocks: the blocks added in image order are the shared gradient, bit for bit
    eq = np.stack([a0, a0])
    us = s.sumregs_unrolled_denoise(a0, maxiter=K)
    gfs, gas = s.sumregs_unrolled_vjp(a0, gu, maxiter=K)
    with pytest.raises(BpltvError) as e:        # the per-image form on a shared tape
        s.sumregs_unrolled_vjp_each(eq, gu, maxiter=K)
    assert e.value.code == E_ARG
    ue = s.sumregs_unrolled_denoise_each(eq, maxiter=K)
    gfe, gae = s.sumregs_unrolled_vjp_each(eq, gu, maxiter=K)
    assert _same(ue, us) and _same(gfe, gfs)
    acc = np.zeros_like(gae[0])
    for k in range(O):
        acc = acc + gae[k]
    assert _same(acc, gas)
    s.close()


# ---- 5. finite differences of bpltv_sumregs_denoise itself ----------------------------------------------------------------
@pytest.mark.parametrize("K", [30, 300])
def test_gradients_against_central_differences_on_the_device(gpu_solver_cls, K):
    """0.5 |u_K - ubar|^2 on synth_batch(1, 24, 28, seed=9), alpha = (0.03, 0.02, 0.04), h = 1e-7, in each of the three
    weights, relative 1e-5 (tests/test_gpu_weighted_unrolled.py's margin for the same check: the device loss carries its
    rounding over 2h)."""
    ub, f, alpha, h = sur.fd_case()
    s = gpu_solver_cls(28, 24, 1)
    s.set_data(ub, f)
    u = s.sumregs_unrolled_denoise(alpha, maxiter=K)
    _, ga = s.sumregs_unrolled_vjp(alpha, u - ub, want_f=False, maxiter=K)
    loss = lambda a: tw.l2_cost(s.sumregs_denoise(a, maxiter=K), ub)
    for r in range(3):
        e = np.zeros(3)
        e[r] = h
        fd = (loss(alpha + e) - loss(alpha - e)) / (2 * h)
        rel = abs(ga[r] - fd) / abs(fd)
        print("K %d, d/da%d: reverse sweep %.10g central difference %.10g rel %.2e" % (K, r + 1, ga[r], fd, rel))
        assert rel <= 1e-5, r
    s.close()


# ---- 6. the tape's contract -------------------------------------------------------------------------------------------
def test_the_handle_s_sumregs_tape(gpu_solver_cls):
    from bpldenoising_amd._lib import BpltvError
    name = "2x17x33"
    O, N, M = SHAPES[name]
    f, gu = _data(name)
    w = np.ones((N, M))
    s = gpu_solver_cls(M, N, O)
    s.set_data(f, f)

    def code(call, *a, **k):
        with pytest.raises(BpltvError) as e:
            call(*a, **k)
        return e.value.code

    assert code(s.sumregs_unrolled_vjp, VEC, gu, maxiter=20) == E_NODATA               # no tape yet
    s.unrolled_denoise(0.08, maxiter=20)                                               # a TV tape is never accepted here ...
    s.weighted_unrolled_denoise(0.08, w, maxiter=20)                                   # ... nor a weighted one
    assert code(s.sumregs_unrolled_vjp, VEC, gu, maxiter=20) == E_NODATA
    g_tv = s.unrolled_vjp(0.08, gu, maxiter=20)
    g_w = s.weighted_unrolled_vjp(0.08, w, gu, maxiter=20)
    n = gpu_solver_cls(M, N, O)
    n.set_data(f, f)
    n.sumregs_unrolled_denoise(VEC, maxiter=20)                                        # ... nor the reverse
    assert code(n.unrolled_vjp, 0.08, gu, maxiter=20) == E_NODATA
    assert code(n.weighted_unrolled_vjp, 0.08, w, gu, maxiter=20) == E_NODATA
    n.close()
    s.sumregs_unrolled_denoise(VEC, maxiter=20)
    st0 = s.stats()
    assert st0["iterations"] == 20 and st0["tiles"] >= O and st0["tile_iters"] >= 1 and st0["launch_chains"] >= 1, st0

    def sweep_stats(method="sumregs-unrolled"):
        """what a reverse sweep leaves: its adjoint_method, and the solve fields the taped solve left"""
        st = s.stats()
        assert st["adjoint_method"] == method, st
        assert all(st[k] == st0[k] for k in ("iterations", "tile_iters", "tiles", "launch_chains")), (st, st0)
        return st

    gf, ga = s.sumregs_unrolled_vjp(VEC, np.zeros_like(gu), maxiter=20)
    assert sweep_stats()["total_ms"] == st0["total_ms"]    # (this sweep leaves the solve's wall time too)
    assert not gf.any() and not ga.any()
    gf, ga = s.sumregs_unrolled_vjp(VEC, gu, maxiter=20)
    sweep_stats()
    assert gf.any() and ga.all()
    s.sumregs_unrolled_denoise(VEC, maxiter=12)            # a second, shorter solve: the tape is now its
    st0 = s.stats()
    assert st0["iterations"] == 12, st0
    assert code(s.sumregs_unrolled_vjp, VEC, gu, maxiter=20) == E_ARG
    for kw in (dict(accel=0), dict(tau0=4.0), dict(sigma0=0.1), dict(opnorm=2.5)):     # other steps than the tape's
        assert code(s.sumregs_unrolled_vjp, VEC, gu, maxiter=12, **kw) == E_ARG
    assert code(s.sumregs_unrolled_vjp, _alpha("patch", N, M), gu, maxiter=12) == E_ARG      # another am, an
    assert code(s.sumregs_unrolled_vjp, _alpha("patch", N, M)[:, :1], gu, maxiter=12) == E_ARG   # another an alone
    a, b = s.sumregs_unrolled_vjp(VEC, gu, maxiter=12), s.sumregs_unrolled_vjp(VEC, gu, maxiter=12)
    assert all(_same(x, y) for x, y in zip(a, b))
    sweep_stats()                                          # (the rejected sweeps in between changed nothing either)
    s.sumregs_denoise(VEC, maxiter=33)                     # a plain solve in the same state sets leaves the tape alone
    st0 = s.stats()
    assert all(_same(x, y) for x, y in zip(s.sumregs_unrolled_vjp(VEC, gu, maxiter=12), a))
    sweep_stats()
    # the TV and weighted tapes survived all of it
    assert all(_same(x, y) for x, y in zip(s.unrolled_vjp(0.08, gu, maxiter=20), g_tv))
    st = sweep_stats("unrolled")
    assert st["adjoint_attempts"] == 1 and st["adjoint_residual"] == 0.0, st
    assert all(_same(x, y) for x, y in zip(s.weighted_unrolled_vjp(0.08, w, gu, maxiter=20), g_w))
    sweep_stats("weighted-unrolled")
    s.unrolled_denoise(0.08, maxiter=9)                    # ... and this one survives theirs
    s.weighted_unrolled_denoise(0.08, w, maxiter=9)
    assert all(_same(x, y) for x, y in zip(s.sumregs_unrolled_vjp(VEC, gu, maxiter=12), a))
    s.close()


# ---- 7. rejections leave the handle as it was ---------------------------------------------------------------------------
def test_rejections_leave_the_handle_as_it_was(gpu_solver_cls):
    import torch
    from bpldenoising_amd._lib import BpltvError
    name = "2x17x33"
    O, N, M = SHAPES[name]
    f, gu = _data(name)
    s = gpu_solver_cls(M, N, O)
    s.set_data(f, f)
    amap = _alpha("map", N, M)
    s.sumregs_unrolled_denoise(VEC, maxiter=20)
    g0 = s.sumregs_unrolled_vjp(VEC, gu, maxiter=20)
    u0 = s.sumregs_denoise(amap, maxiter=57)               # the last solve: another parameter shape
    gap0 = s.duality_gap()
    st0 = s.stats()

    def unchanged():
        assert _same(s.duality_gap(), gap0)
        st = s.stats()
        assert {k for k in st if st[k] != st0[k]} <= {"adjoint_ms", "adjoint_method"}
        out = torch.empty(O, N, M, dtype=torch.float64, device="cuda")
        s.copy_u_device(out.data_ptr())
        assert _same(out.cpu().numpy(), u0)
        g = s.sumregs_unrolled_vjp(VEC, gu, maxiter=20)            # the tape is still the first solve's
        assert all(_same(x, y) for x, y in zip(g, g0))
        assert _same(s.duality_gap(), gap0)                        # the VJP staged its parameter apart

    def rejected(code, call, *a, **k):
        with pytest.raises(BpltvError) as e:
            call(*a, **k)
        assert e.value.code == code, (e.value.code, str(e.value))
        unchanged()

    bad_gu = gu.copy(); bad_gu[1, 3, 4] = np.inf
    nan_map = amap.copy(); nan_map[1, 2, 5] = np.nan
    for bad in (np.array([0.03, np.nan, 0.04]), np.array([0.03, 0.02, -0.1]), np.array([np.inf, 0.02, 0.04]), nan_map):
        rejected(E_ARG, s.sumregs_unrolled_denoise, bad, maxiter=20)
        rejected(E_ARG, s.sumregs_unrolled_vjp, bad, gu, maxiter=20)
    rejected(E_ARG, s.sumregs_unrolled_vjp, VEC, bad_gu, maxiter=20)
    rejected(E_ARG, s.sumregs_unrolled_denoise, VEC, maxiter=0)
    rejected(E_ARG, s.sumregs_unrolled_vjp, VEC, gu, maxiter=0)
    for kw in (dict(rho=0.01), dict(init=1), dict(order=1)):
        rejected(E_UNSUPPORTED, s.sumregs_unrolled_denoise, VEC, maxiter=20, **kw)
        rejected(E_UNSUPPORTED, s.sumregs_unrolled_vjp, VEC, gu, maxiter=20, **kw)
    p = s.params(_sumregs=True, maxiter=20)
    assert s._lib.bpltv_sumregs_unrolled_vjp(s._h, _ptr(VEC), 1, 1, C.byref(p), _ptr(gu), None, None) == E_ARG
    unchanged()
    # the device forms
    gt, gfd = torch.tensor(gu, device="cuda"), torch.empty(O, N, M, dtype=torch.float64, device="cuda")
    good = torch.tensor(VEC, device="cuda")
    torch.cuda.synchronize()
    for bad in ([0.03, float("nan"), 0.04], [0.03, 0.02, -0.1], [float("inf"), 0.02, 0.04]):
        bt = torch.tensor(bad, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        rejected(E_ARG, s.sumregs_unrolled_denoise_device, bt.data_ptr(), 1, 1, maxiter=20)
        rejected(E_ARG, s.sumregs_unrolled_vjp_device, None, bt.data_ptr(), 1, 1, gt.data_ptr(), gfd.data_ptr(), None, maxiter=20)
    bgt = torch.tensor(bad_gu, device="cuda")
    torch.cuda.synchronize()
    rejected(E_ARG, s.sumregs_unrolled_vjp_device, None, good.data_ptr(), 1, 1, bgt.data_ptr(), gfd.data_ptr(), None, maxiter=20)
    rejected(E_ARG, s.sumregs_unrolled_vjp_device, None, good.data_ptr(), 1, 1, gt.data_ptr(), None, None, maxiter=20)
    for kw in (dict(rho=0.01), dict(init=1), dict(order=1)):
        rejected(E_UNSUPPORTED, s.sumregs_unrolled_denoise_device, good.data_ptr(), 1, 1, maxiter=20, **kw)
        rejected(E_UNSUPPORTED, s.sumregs_unrolled_vjp_device, None, good.data_ptr(), 1, 1, gt.data_ptr(), gfd.data_ptr(), None,
                 maxiter=20, **kw)
    # the next accepted call is bit-identical, zeros are legal (a whole slice of them included)
    assert _same(s.sumregs_denoise(amap, maxiter=57), u0) and _same(s.duality_gap(), gap0)
    s.sumregs_unrolled_denoise(np.array([0.0, 0.0, 0.04]), maxiter=20)
    s.sumregs_unrolled_denoise(np.zeros(3), maxiter=20)
    n = gpu_solver_cls(M, N, O)                # no dataset
    with pytest.raises(BpltvError) as e:
        n.sumregs_unrolled_denoise(VEC, maxiter=5)
    assert e.value.code == E_NODATA
    with pytest.raises(BpltvError) as e:
        n.sumregs_unrolled_vjp(VEC, gu, maxiter=5)
    assert e.value.code == E_NODATA
    n.close()
    s.close()


# ---- 8. shards, float handles, graphs ------------------------------------------------------------------------------------
def test_two_shards_are_unsupported(gpu_solver_cls):
    from bpldenoising_amd._lib import BpltvError
    name = "2x17x33"
    O, N, M = SHAPES[name]
    f, gu = _data(name)
    eq = np.stack([VEC, VEC])
    m = gpu_solver_cls(M, N, O, devices=[0, 0])
    m.set_data(f, f)
    u0 = m.sumregs_denoise(VEC, maxiter=30)
    gap0 = m.duality_gap()
    for call, args in ((m.sumregs_unrolled_denoise, (VEC,)), (m.sumregs_unrolled_vjp, (VEC, gu)),
                       (m.sumregs_unrolled_denoise_each, (eq,)), (m.sumregs_unrolled_vjp_each, (eq, gu)),
                       (m.sumregs_unrolled_denoise_device, (1, 1, 1)), (m.sumregs_unrolled_vjp_device, (None, 1, 1, 1, 1, 1, 1)),
                       (m.sumregs_unrolled_denoise_each_device, (1, 1, 1)),
                       (m.sumregs_unrolled_vjp_each_device, (None, 1, 1, 1, 1, 1, 1))):
        with pytest.raises(BpltvError) as e:     # (the device forms are refused before any pointer is read)
            call(*args, maxiter=30)
        assert e.value.code == E_UNSUPPORTED
        assert _same(m.duality_gap(), gap0) and _same(m.sumregs_denoise(VEC, maxiter=30), u0)
    m.close()
    one = gpu_solver_cls(M, N, O, ngpus=1)       # one shard holds everything: forwarded
    one.set_data(f, f)
    s = gpu_solver_cls(M, N, O)
    s.set_data(f, f)
    assert _same(one.sumregs_unrolled_denoise(VEC, maxiter=30), s.sumregs_unrolled_denoise(VEC, maxiter=30))
    a, b = one.sumregs_unrolled_vjp(VEC, gu, maxiter=30), s.sumregs_unrolled_vjp(VEC, gu, maxiter=30)
    assert all(_same(x, y) for x, y in zip(a, b))
    one.close()
    s.close()


def test_float_handles_run_the_sumregs_unrolled_solve_in_float64(gpu_solver_cls):
    name = "2x17x33"
    O, N, M = SHAPES[name]
    f, gu = _data(name)
    s, s32 = gpu_solver_cls(M, N, O), gpu_solver_cls(M, N, O, dtype=32)
    for h in (s, s32):
        h.set_data(f, f)
    assert _same(s32.sumregs_denoise(VEC, maxiter=40), s.sumregs_denoise(VEC, maxiter=40))   # (as the plain solve does today)
    assert _same(s32.sumregs_unrolled_denoise(VEC, maxiter=40), s.sumregs_unrolled_denoise(VEC, maxiter=40))
    a, b = s32.sumregs_unrolled_vjp(VEC, gu, maxiter=40), s.sumregs_unrolled_vjp(VEC, gu, maxiter=40)
    assert all(_same(x, y) for x, y in zip(a, b))
    s.close()
    s32.close()


def test_no_graph_is_shared_with_the_other_solves(gpu_solver_cls):
    name = "2x40x48"
    O, N, M = SHAPES[name]
    f, gu = _data(name)
    K = 57

    def fresh(call):
        h = gpu_solver_cls(M, N, O)
        h.set_data(f, f)
        r = call(h)
        h.close()
        return r
    u_sr = fresh(lambda h: h.sumregs_denoise(VEC, maxiter=K))
    u_tv, g_tv = fresh(lambda h: (h.unrolled_denoise(0.08, maxiter=K), h.unrolled_vjp(0.08, gu, maxiter=K)))
    u_su, g_su = fresh(lambda h: (h.sumregs_unrolled_denoise(VEC, maxiter=K), h.sumregs_unrolled_vjp(VEC, gu, maxiter=K)))
    eq = np.stack([VEC] * O)
    assert _same(u_su, u_sr)
    for order in ("sumregs unrolled first", "sumregs unrolled last"):
        h = gpu_solver_cls(M, N, O)
        h.set_data(f, f)
        for rnd in range(2):   # the second round replays what the first one cached
            if order == "sumregs unrolled first":
                assert _same(h.sumregs_unrolled_denoise(VEC, maxiter=K), u_su)
            assert _same(h.sumregs_denoise(VEC, maxiter=K), u_sr)
            assert _same(h.sumregs_denoise_each(eq, maxiter=K), u_sr)
            assert _same(h.unrolled_denoise(0.08, maxiter=K), u_tv)
            assert _same(h.denoise(0.08, maxiter=K), u_tv)
            if order == "sumregs unrolled last":
                assert _same(h.sumregs_unrolled_denoise(VEC, maxiter=K), u_su)
            g = h.unrolled_vjp(0.08, gu, maxiter=K)                       # each tape holds what its own solve recorded
            assert _same(g[0], g_tv[0]) and _same(g[1], g_tv[1])
            g = h.sumregs_unrolled_vjp(VEC, gu, maxiter=K)
            assert all(_same(x, y) for x, y in zip(g, g_su))
            assert _same(h.sumregs_unrolled_denoise_each(eq, maxiter=K), u_su)     # a per-image solve replays no shared graph
            ge = h.sumregs_unrolled_vjp_each(eq, gu, maxiter=K)
            assert _same(ge[0], g_su[0])
            assert _same(h.sumregs_unrolled_denoise(VEC, maxiter=K), u_su)
        h.close()
