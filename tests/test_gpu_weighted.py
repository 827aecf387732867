"""GPU checks of the TV model with a per-pixel data-fidelity weight (bpltv_weighted_denoise / bpltv_weighted_vjp and
their device forms): min_u 0.5 sum w (u - f)^2 + sum alpha |G u|.

w = 1 ties the new PDHG kernel and the new adjoint mode to the oracle-pinned unweighted chain bit for bit; a random w, a
mask and the duality gap are held against the numpy restatement tests/weighted_ref.py (pinned on the CPU by
tests/test_weighted_abi.py), the VJP against its literal scipy system; the (c w, c alpha) invariance checks the model
itself, and the contracts check that a rejected call leaves the handle as it was."""
import ctypes as C
import functools

import numpy as np
import pytest
from conftest import synth_batch

import weighted_ref as wr

pytestmark = pytest.mark.gpu

E_ARG, E_UNSUPPORTED = 1, 6
_dp = C.POINTER(C.c_double)


def _alpha(kind, N, M):
    """scalar, a 2 x 2 patch (1 x 2 / 2 x 1 where the image has a single row / column), or a map."""
    if kind == "scalar":
        return 0.1
    if kind == "patch":
        return np.array([[0.08, 0.12], [0.1, 0.05]])[:min(2, N), :min(2, M)].copy()
    return 0.05 + 0.1 * np.random.default_rng(8).random((N, M))


def _same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b))


def _ptr(a):
    return a.ctypes.data_as(_dp) if a is not None else None


# ---- 1. w = 1 is bpltv_denoise, bit for bit ------------------------------------------------------------------------
# (3, 40, 48): several tiles in both axes; (2, 17, 33): odd sizes, two tiles along i; one row and one column; (2, 70, 72): four
# tiles per axis, the middle ones with a halo on both sides (rows of halo waves that stop early at either end)
SHAPES = [(3, 40, 48), (2, 17, 33), (1, 1, 9), (1, 9, 1), (2, 70, 72)]


@pytest.mark.parametrize("kind", ["scalar", "patch", "map"])
@pytest.mark.parametrize("shape", SHAPES, ids=["3x40x48", "2x17x33", "1x1x9", "1x9x1", "2x70x72"])
def test_unit_weight_is_the_unweighted_denoise_bitwise(gpu_solver_cls, shape, kind):
    O, N, M = shape
    _, f = synth_batch(O, N, M, seed=5 + M)
    alpha = _alpha(kind, N, M)
    s = gpu_solver_cls(M, N, O)
    s.set_data(f, f)
    for maxiter in (1, 7, 203):
        u0 = s.denoise(alpha, maxiter=maxiter)
        g0 = s.duality_gap()
        for w in (np.ones((N, M)), np.ones((O, N, M))):    # wo = 1 and wo = O
            u1 = s.weighted_denoise(alpha, w, maxiter=maxiter)
            assert _same(u1, u0), (maxiter, w.shape, float(np.abs(u1 - u0).max()))
            st = s.stats()
            assert st["iterations"] == maxiter and st["pdhg_variant"] == 0 and st["launches"] >= 1 and st["tiles"] >= O, st
            assert st["bytes_per_px_iter"] == (72.0 if kind == "map" and N * M > 1 else 64.0)
            # the weighted gap of the same iterate: the unweighted gap up to the rounding of two summation orders
            assert np.allclose(s.duality_gap(), g0, rtol=0, atol=1e-11 * max(1.0, 0.5 * float((f * f).sum(axis=(1, 2)).max())))
    # another fusion depth cuts the iterations into other launches and other tiles: the same bits
    assert _same(s.weighted_denoise(alpha, np.ones((N, M)), maxiter=203, tile_iters=5), u0)
    assert _same(s.weighted_denoise(alpha, np.ones((N, M)), maxiter=203, use_graph=0), u0)
    # two launch chains (what a batch beyond one workgroup per CU gets), the second half a launch out of phase when
    # that leaves both in the same state set (200 iterations at depth 8; not 203)
    for maxiter in (203, 200):
        u0 = s.denoise(alpha, maxiter=maxiter)
        assert _same(s.weighted_denoise(alpha, np.ones((O, N, M)), maxiter=maxiter, chains=2), u0)
        assert s.stats()["launch_chains"] == min(2, O)
    s.close()


def test_device_form_is_the_host_form_bitwise(gpu_solver_cls):
    import torch
    O, N, M = 3, 40, 48
    _, f = synth_batch(O, N, M, seed=6)
    rng = np.random.default_rng(7)
    s = gpu_solver_cls(M, N, O)
    s.set_data(f, f)
    for kind in ("scalar", "map"):
        alpha = _alpha(kind, N, M)
        a = np.atleast_1d(np.asarray(alpha, dtype=np.float64))
        an, am = (1, 1) if kind == "scalar" else a.shape
        for w in (0.25 + 3.75 * rng.random((N, M)), 0.25 + 3.75 * rng.random((O, N, M))):
            u0 = s.weighted_denoise(alpha, w, maxiter=57)
            wt, at = torch.tensor(w, device="cuda"), torch.tensor(a, device="cuda")
            out = torch.empty(O, N, M, dtype=torch.float64, device="cuda")
            torch.cuda.synchronize()
            s.weighted_denoise_device(wt.data_ptr(), 1 if w.ndim == 2 else O, at.data_ptr(), am, an, maxiter=57)
            s.copy_u_device(out.data_ptr())
            assert _same(out.cpu().numpy(), u0)
    s.close()


# ---- 2. a random weight against the twin ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _rand_case():
    O, N, M = 2, 40, 48
    _, f = synth_batch(O, N, M, seed=9)
    rng = np.random.default_rng(10)
    w1 = 0.25 + 3.75 * rng.random((N, M))
    wO = 0.25 + 3.75 * rng.random((O, N, M))
    wO[1, 5, 7] = 0.25          # the global minimum sits in image 1, image 0's own minimum is larger
    wO[0] = np.maximum(wO[0], 0.5)
    return f, w1, wO


@pytest.mark.parametrize("kind", ["scalar", "map"])
def test_random_weight_matches_the_twin(gpu_solver_cls, kind):
    """max|u - twin| <= 1e-13 at the same iteration count (50 and 203), one plane and one plane per image; with planes
    per image gamma is the minimum over ALL of them (the twin's), not each image's own."""
    f, w1, wO = _rand_case()
    O, N, M = f.shape
    alpha = _alpha(kind, N, M)
    s = gpu_solver_cls(M, N, O)
    s.set_data(f, f)
    for maxiter in (50, 203):
        for w in (w1, wO):
            u = s.weighted_denoise(alpha, w, maxiter=maxiter)
            d = float(np.abs(u - wr.pdhg(f, alpha, w, maxiter)).max())
            print("%s maxiter %d w %s: max|du| = %.3e" % (kind, maxiter, w.shape, d))
            assert d <= 1e-13
    # the check has teeth: image 0 solved with its own minimum (0.5) is another iterate
    own = wr.pdhg(f[:1], alpha, wO[:1], 203)
    assert float(np.abs(own[0] - u[0]).max()) > 1e-6
    s.close()


# ---- 3. a mask -------------------------------------------------------------------------------------------------------
def test_mask_inpaints_and_has_no_gap(gpu_solver_cls):
    from bpldenoising_amd._lib import BpltvError
    O, N, M = 1, 24, 28
    _, f = synth_batch(O, N, M, seed=12)
    w = np.ones((N, M))
    w[9:15, 11:17] = 0.0
    s = gpu_solver_cls(M, N, O)
    s.set_data(f, f)
    u = s.weighted_denoise(0.1, w, maxiter=203)
    assert np.all(np.isfinite(u))
    d = float(np.abs(u - wr.pdhg(f, 0.1, w, 203)).max())
    print("mask: max|du| = %.3e" % d)
    assert d <= 1e-13
    with pytest.raises(BpltvError) as e:
        s.duality_gap()
    assert e.value.code == E_UNSUPPORTED
    s.close()


# ---- 4. the duality gap --------------------------------------------------------------------------------------------
def test_gap_is_the_twin_s_and_does_not_increase(gpu_solver_cls):
    f, w1, wO = _rand_case()
    O, N, M = f.shape
    alpha = _alpha("map", N, M)
    s = gpu_solver_cls(M, N, O)
    s.set_data(f, f)
    for w in (w1, wO):
        s.weighted_denoise(alpha, w, maxiter=50, fetch=False)
        g50 = s.duality_gap()
        u, y1, y2 = wr.pdhg(f, alpha, w, 50, return_dual=True)
        ref = wr.gap(u, y1, y2, f, alpha, w)
        energy = wr.primal_energy(u, f, alpha, w)
        print("gap", g50, "twin", ref, "energy", energy)
        assert np.all(np.abs(g50 - ref) <= 1e-11 * energy)    # ~100 x the n eps bound of the four sums
        s.weighted_denoise(alpha, w, maxiter=500, fetch=False)
        g500 = s.duality_gap()
        s.weighted_denoise(alpha, w, maxiter=5000, fetch=False)
        g5000 = s.duality_gap()
        assert s.stats()["last_gap"] == float(g5000.max())
        assert np.all(g5000 <= g500) and np.all(g500 <= g50) and np.all(g5000 >= -1e-11 * energy), (g50, g500, g5000)
    s.close()


# ---- 5. the model, not just the recurrence -------------------------------------------------------------------------
def test_scaling_weight_and_parameter_together_keeps_the_minimiser(gpu_solver_cls):
    """(w = 2, 2 alpha) and (w = 1, alpha) have one minimiser u*: 0.5 |u1 - u*|^2 <= gap1 and |u2 - u*|^2 <= gap2."""
    O, N, M = 1, 16, 20
    _, f = synth_batch(O, N, M, seed=14)
    P = np.array([[0.08, 0.12], [0.1, 0.05]])
    s = gpu_solver_cls(M, N, O)
    s.set_data(f, f)
    u1 = s.weighted_denoise(P, np.ones((N, M)), maxiter=5000)
    g1 = float(s.duality_gap()[0])
    u2 = s.weighted_denoise(2.0 * P, np.full((N, M), 2.0), maxiter=5000)
    g2 = float(s.duality_gap()[0])
    s.close()
    d = float(np.linalg.norm(u1 - u2))
    print("|u1 - u2| = %.3e, bound %.3e (gaps %.3e %.3e)" % (d, np.sqrt(2 * g1) + np.sqrt(g2), g1, g2))
    assert 0.0 <= g1 < 1e-5 and 0.0 <= g2 < 1e-5
    assert d <= np.sqrt(2.0 * g1) + np.sqrt(g2)
    assert d > 0.0     # two different recurrences (gamma = 1 and 2), not one result copied


# ---- 6. / 7. the vector-Jacobian product ---------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["scalar", "patch", "map"])
def test_vjp_with_unit_weight_is_the_unweighted_vjp_bitwise(gpu_solver_cls, kind):
    O, N, M = 3, 20, 16
    _, f = synth_batch(O, N, M, seed=15)
    alpha = _alpha(kind, N, M)
    s = gpu_solver_cls(M, N, O)
    s.set_data(f, f)
    u = s.denoise(alpha, maxiter=300)
    gu = np.random.default_rng(16).standard_normal(u.shape)
    gf0, ga0 = s.vjp(u, alpha, gu)
    k0 = s.stats()["kappa_used"]
    for w in (np.ones((N, M)), np.ones((O, N, M))):
        gf, ga, gw = s.weighted_vjp(u, f, alpha, w, gu)
        st = s.stats()
        assert _same(gf, gf0) and _same(ga, ga0) and np.shape(ga) == np.shape(ga0)
        assert st["kappa_used"] == k0 and st["adjoint_residual"] <= 1e-6 and st["reg_gradient_used"] == 0, st
        want = -(u - f) * gf0
        if w.ndim == 2:
            want = want.sum(axis=0)
        assert gw.shape == w.shape
        assert np.linalg.norm(gw - want) <= 1e-15 * np.linalg.norm(want)
    # each output alone
    assert _same(s.weighted_vjp(u, None, alpha, np.ones((N, M)), gu, want_alpha=False, want_w=False)[0], gf0)
    assert _same(s.weighted_vjp(u, None, alpha, np.ones((N, M)), gu, want_f=False, want_w=False)[1], ga0)
    assert _same(s.weighted_vjp(u, f, alpha, np.ones((O, N, M)), gu, want_f=False, want_alpha=False)[2], gw)
    s.close()


@pytest.mark.parametrize("kind", ["scalar", "patch", "map"])
def test_vjp_with_random_weight_matches_the_literal_system(gpu_solver_cls, kind):
    """All three outputs against tests/weighted_ref.py's scipy solve of (diag(w) + K) p = gu with the kappa the library
    reports, rtol 1e-6 / atol 1e-8 max|p| (tests/test_gpu_vjp.py's); the reference itself moves by 4e-12 under ten
    extended-precision refinement sweeps on this case (tests/test_weighted_abi.py)."""
    import torch
    alpha = _alpha(kind, 16, 20)
    f, w, u, gu = wr.vjp_case(alpha, seed=21)
    O, N, M = u.shape
    s = gpu_solver_cls(M, N, O)
    gf, ga, gw = s.weighted_vjp(u, f, alpha, w, gu)
    st = s.stats()
    assert st["adjoint_residual"] <= 1e-6 and st["adjoint_attempts"] >= 1, st
    rf, ra, rw, p = wr.vjp(u, f, alpha, w, gu, st["kappa_used"], refine=10)
    pmax = float(np.abs(p).max())
    for name, a, b in (("grad_f", gf, rf), ("grad_alpha", ga, ra), ("grad_w", gw, rw)):
        a, b = np.asarray(a), np.asarray(b)
        print("%s %s: max|d| = %.3e (max|ref| %.3e, max|p| %.3e)" % (kind, name, float(np.abs(a - b).max()), float(np.abs(b).max()), pmax))
        assert a.shape == b.shape and np.allclose(a, b, rtol=1e-6, atol=1e-8 * pmax), name
    # one plane for the batch: grad_w is the image sum of the per-image result for equal planes
    w2 = w[0]
    gf1, ga1, gw1 = s.weighted_vjp(u, f, alpha, w2, gu)
    gfO, gaO, gwO = s.weighted_vjp(u, f, alpha, np.broadcast_to(w2, u.shape).copy(), gu)
    assert _same(gf1, gfO) and _same(ga1, gaO)
    assert gw1.shape == (N, M) and np.linalg.norm(gw1 - gwO.sum(axis=0)) <= 1e-13 * np.linalg.norm(gw1)
    # linear in the cotangent
    g2 = np.random.default_rng(23).standard_normal(u.shape)
    b1 = s.weighted_vjp(u, f, alpha, w, g2)
    b3 = s.weighted_vjp(u, f, alpha, w, 2.0 * gu - 0.5 * g2)
    for x3, x1, x2 in zip(b3, (gf, ga, gw), b1):
        want = 2.0 * np.asarray(x1) - 0.5 * np.asarray(x2)
        assert np.linalg.norm(np.ravel(x3) - np.ravel(want)) <= 1e-8 * np.linalg.norm(np.ravel(want))
    # the device form: the same bits
    t = lambda a: torch.tensor(np.ascontiguousarray(a), device="cuda")
    a = np.atleast_1d(np.asarray(alpha, dtype=np.float64))
    an, am = (1, 1) if kind == "scalar" else a.shape
    ut, ft, wt, at, gt = t(u), t(f), t(w), t(a), t(gu)
    of, oa, ow = torch.empty_like(ut), torch.empty(am * an, dtype=torch.float64, device="cuda"), torch.empty_like(wt)
    torch.cuda.synchronize()
    s.weighted_vjp_device(ut.data_ptr(), ft.data_ptr(), wt.data_ptr(), O, at.data_ptr(), am, an, gt.data_ptr(),
                          of.data_ptr(), oa.data_ptr(), ow.data_ptr())
    assert _same(of.cpu().numpy(), gf) and _same(oa.cpu().numpy().reshape(np.shape(ga)), ga) and _same(ow.cpu().numpy(), gw)
    s.close()


# ---- 8. contracts ----------------------------------------------------------------------------------------------------
def _raw_denoise(s, w, wo, alpha, am, an, p):
    return s._lib.bpltv_weighted_denoise(s._h, _ptr(w), wo, _ptr(alpha), am, an, C.byref(p), None)


def _raw_vjp(s, u, f, w, wo, alpha, p, gu, gf, ga, gw):
    return s._lib.bpltv_weighted_vjp(s._h, _ptr(u), _ptr(f), _ptr(w), wo, _ptr(alpha), 1, 1, C.byref(p), _ptr(gu),
                                     _ptr(gf), _ptr(ga), _ptr(gw))


def test_rejected_calls_leave_the_handle_as_it_was(gpu_solver_cls):
    import torch
    O, N, M = 2, 17, 33
    _, f = synth_batch(O, N, M, seed=17)
    s = gpu_solver_cls(M, N, O)
    s.set_data(f, f)
    u0 = s.denoise(0.1, maxiter=60)
    g0 = s.duality_gap()
    p = s.params(maxiter=60)
    a = np.array([0.07])
    gu = np.random.default_rng(18).standard_normal(u0.shape)
    out = np.empty_like(u0)
    good = np.full((N, M), 1.5)

    def untouched():
        assert _same(s.duality_gap(), g0)                      # the last solve's parameter and state
        assert _same(s.denoise(0.1, maxiter=60), u0) and _same(s.duality_gap(), g0)

    for bad in (np.nan, -1.0, np.inf):
        w = good.copy()
        w[3, 4] = bad
        assert _raw_denoise(s, w, 1, a, 1, 1, p) == E_ARG
        untouched()
        wt, at = torch.tensor(w, device="cuda"), torch.tensor(a, device="cuda")
        torch.cuda.synchronize()
        assert s._lib.bpltv_weighted_denoise_device(s._h, C.c_void_p(wt.data_ptr()), 1, C.c_void_p(at.data_ptr()), 1, 1,
                                                    C.byref(p)) == E_ARG
        untouched()
        assert _raw_vjp(s, u0, f, w, 1, a, p, gu, out, None, None) == E_ARG
        untouched()
    for wo in (0, 3, -1):                                      # wo not in {1, O}
        wbig = np.full((3, N, M), 1.5)
        assert _raw_denoise(s, wbig, wo, a, 1, 1, p) == E_ARG
        assert _raw_vjp(s, u0, f, wbig, wo, a, p, gu, out, None, None) == E_ARG
        untouched()
    assert _raw_denoise(s, good, 1, np.array([-0.1]), 1, 1, p) == E_ARG     # a good w with a rejected parameter
    untouched()
    w = good.copy()
    w[0, 0] = 0.0                                              # fine for a solve, not for the adjoint
    assert _raw_vjp(s, u0, f, w, 1, a, p, gu, out, None, None) == E_ARG
    untouched()
    assert _raw_vjp(s, u0, None, good, 1, a, p, gu, out, None, np.empty((N, M))) == E_ARG   # grad_w needs f
    assert _raw_vjp(s, u0, f, good, 1, a, p, gu, None, None, None) == E_ARG                 # no output at all
    bad_gu = gu.copy()
    bad_gu[1, 2, 3] = np.inf
    assert _raw_vjp(s, u0, f, good, 1, a, p, bad_gu, out, None, None) == E_ARG
    untouched()
    # a valid VJP does not touch the last solve either
    s.weighted_vjp(u0, f, 0.07, good, gu)
    assert _same(s.duality_gap(), g0)
    # what the weighted model does not implement
    for kw in (dict(rho=0.01), dict(init=1), dict(order=1)):
        q = s.params(maxiter=60, **kw)
        assert _raw_denoise(s, good, 1, a, 1, 1, q) == E_UNSUPPORTED
        assert _raw_vjp(s, u0, f, good, 1, a, q, gu, out, None, None) == E_UNSUPPORTED
    untouched()
    s.close()


def test_two_shards_are_unsupported(gpu_solver_cls):
    O, N, M = 2, 17, 33
    _, f = synth_batch(O, N, M, seed=17)
    m = gpu_solver_cls(M, N, O, devices=[0, 0])
    m.set_data(f, f)
    p = m.params(maxiter=10)
    a, w, u = np.array([0.07]), np.ones((N, M)), np.empty((O, N, M))
    assert _raw_denoise(m, w, 1, a, 1, 1, p) == E_UNSUPPORTED
    assert _raw_vjp(m, f, f, w, 1, a, p, f, u, None, None) == E_UNSUPPORTED
    dummy = C.c_void_p(u.ctypes.data)     # never read: the handle is refused first
    assert m._lib.bpltv_weighted_denoise_device(m._h, dummy, 1, dummy, 1, 1, C.byref(p)) == E_UNSUPPORTED
    assert m._lib.bpltv_weighted_vjp_device(m._h, dummy, dummy, dummy, 1, dummy, 1, 1, C.byref(p), dummy, dummy, None,
                                            None) == E_UNSUPPORTED
    m.close()
    # one shard holds everything: forwarded
    m = gpu_solver_cls(M, N, O, ngpus=1)
    m.set_data(f, f)
    s = gpu_solver_cls(M, N, O)
    s.set_data(f, f)
    wr_ = 0.25 + 3.75 * np.random.default_rng(19).random((N, M))
    assert _same(m.weighted_denoise(0.1, wr_, maxiter=40), s.weighted_denoise(0.1, wr_, maxiter=40))
    assert _same(m.duality_gap(), s.duality_gap())
    m.close()
    s.close()


def test_weighted_and_unweighted_solves_do_not_cross(gpu_solver_cls):
    """Graph caches: a weighted solve followed by bpltv_denoise gives bpltv_denoise's usual bits, and the reverse; the
    last solve -- bpltv_u_device, bpltv_duality_gap -- is whichever ran last; a dtype = 32 handle runs the weighted model
    in Float64."""
    import torch
    O, N, M = 2, 40, 48
    f, w1, _ = _rand_case()
    fresh = gpu_solver_cls(M, N, O)
    fresh.set_data(f, f)
    u_tv = fresh.denoise(0.1, maxiter=203)
    g_tv = fresh.duality_gap()
    fresh.close()
    fresh = gpu_solver_cls(M, N, O)
    fresh.set_data(f, f)
    u_w = fresh.weighted_denoise(0.1, w1, maxiter=203)
    g_w = fresh.duality_gap()
    fresh.close()
    assert not _same(u_tv, u_w)
    s = gpu_solver_cls(M, N, O)
    s.set_data(f, f)
    out = torch.empty(O, N, M, dtype=torch.float64, device="cuda")
    for _ in range(2):                                         # the second round replays both captured graphs
        assert _same(s.weighted_denoise(0.1, w1, maxiter=203), u_w)
        s.copy_u_device(out.data_ptr())
        assert _same(out.cpu().numpy(), u_w) and _same(s.duality_gap(), g_w)
        assert _same(s.denoise(0.1, maxiter=203), u_tv)
        s.copy_u_device(out.data_ptr())
        assert _same(out.cpu().numpy(), u_tv) and _same(s.duality_gap(), g_tv)
    assert s.stats()["graph_used"] == 1
    # another weight with the same shape replays the same graph on new data
    w2 = w1[::-1].copy()
    u2 = s.weighted_denoise(0.1, w2, maxiter=203)
    assert float(np.abs(u2 - wr.pdhg(f, 0.1, w2, 203)).max()) <= 1e-13
    s.close()
    s32 = gpu_solver_cls(M, N, O, dtype=32)
    s32.set_data(f, f)
    assert _same(s32.weighted_denoise(0.1, w1, maxiter=203), u_w)
    assert _same(s32.duality_gap(), g_w)
    u32 = s32.denoise(0.1, maxiter=203)                        # the float solve still works behind it
    assert 0 < float(np.abs(u32 - u_tv).max()) < 1e-4
    assert _same(s32.weighted_denoise(0.1, w1, maxiter=203), u_w)
    s32.close()
