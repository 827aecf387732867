"""GPU checks of forward mode through the PDHG iterations with one parameter per image (bpltv_unrolled_jvp_each and its
device form).

The primal is tied to bpltv_denoise_each bit for bit; image k's tangent is bitwise a one-image handle's shared sweep, which
catches a parameter or tangent block handed to the wrong image; equal blocks reproduce the shared sweep; the tangent is held
against the numpy twin and, by the transpose identity, against bpltv_unrolled_vjp_each on the same handle; a sweep leaves the
last solve, the tape and the statistics as they were, and so does a rejected call."""
import ctypes as C
import functools

import numpy as np
import pytest
from conftest import synth_batch

import unrolled_each_ref as ue
import unrolled_jvp_ref as uj

pytestmark = pytest.mark.gpu

E_ARG, E_NODATA, E_UNSUPPORTED = 1, 3, 6
_dp = C.POINTER(C.c_double)
SHAPES = {"3x40x48": (3, 40, 48), "2x17x33": (2, 17, 33), "1x1x9": (1, 1, 9), "1x9x1": (1, 9, 1), "2x70x72": (2, 70, 72)}
KINDS = ["scalar", "patch", "map"]


def _same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b))


def _ptr(a):
    return a.ctypes.data_as(_dp) if a is not None else None


def _one(a, k):
    """Block k as the one-image calls take it: a float, or an (n, m) array."""
    return float(a[k]) if a.ndim == 1 else a[k]


def _amn(alphas):
    return (1, 1) if alphas.ndim == 1 else (alphas.shape[2], alphas.shape[1])


@functools.lru_cache(maxsize=None)
def _data(name, seed=5):
    """(f, cotangent w, tangent df) of a shape; read-only."""
    O, N, M = SHAPES[name]
    _, f = synth_batch(O, N, M, seed=seed + M)
    rng = np.random.default_rng(seed + 300)
    w, df = rng.standard_normal(f.shape), rng.standard_normal(f.shape)
    for a in (f, w, df):
        a.setflags(write=False)
    return f, w, df


def _alphas(kind, name):
    O, N, M = SHAPES[name]
    return ue.alphas_of(kind, O, N, M)


def _dalphas(alphas, seed=11, ndir=None):
    """Standard-normal tangents in the shape of alphas (with a leading ndir)."""
    shape = alphas.shape if ndir is None else (ndir,) + alphas.shape
    return np.random.default_rng(seed).standard_normal(shape)


# ---- 1. the primal is bpltv_denoise_each's, bit for bit -------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_primal_is_denoise_each_bitwise(gpu_solver_cls, name, kind):
    O, N, M = SHAPES[name]
    f, _, df = _data(name)
    alphas = _alphas(kind, name)
    s = gpu_solver_cls(M, N, O)
    s.set_data(f, f)
    for accel in (1, 0):
        for maxiter in (1, 7, 203):
            u0 = s.denoise_each(alphas, maxiter=maxiter, accel=accel)
            du, u1 = s.unrolled_jvp_each(alphas, df=df, dalphas=_dalphas(alphas), want_u=True, maxiter=maxiter, accel=accel)
            assert _same(u1, u0), (accel, maxiter, float(np.abs(u1 - u0).max()))
            assert np.isfinite(du).all() and du.any()
            assert s.stats()["adjoint_method"] == "unrolled-jvp" and s.stats()["adjoint_ms"] > 0.0
    s.close()


# ---- 2. directions, images and equal blocks ----------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_directions_and_images_are_independent_bitwise(gpu_solver_cls, name, kind):
    O, N, M = SHAPES[name]
    f, _, _ = _data(name)
    alphas = _alphas(kind, name)
    K = 50
    rng = np.random.default_rng(21)
    df3 = rng.standard_normal((3,) + f.shape)
    da3 = _dalphas(alphas, ndir=3)
    s = gpu_solver_cls(M, N, O)
    s.set_data(f, f)
    du3 = s.unrolled_jvp_each(alphas, df=df3, dalphas=da3, maxiter=K)
    assert du3.shape == (3,) + f.shape
    for d in range(3):   # direction d of a call is the single call
        assert _same(s.unrolled_jvp_each(alphas, df=df3[d], dalphas=da3[d], maxiter=K), du3[d])
    # equal blocks and equal tangent blocks: the shared sweep
    a0, d0 = _one(alphas, 0), _one(da3[0], 0)
    eq = np.stack([np.asarray(a0, dtype=np.float64)] * O)
    deq = np.stack([np.asarray(d0, dtype=np.float64)] * O)
    du_sh, u_sh = s.unrolled_jvp(a0, df=df3[0], dalpha=d0, want_u=True, maxiter=K)
    du_eq, u_eq = s.unrolled_jvp_each(eq, df=df3[0], dalphas=deq, want_u=True, maxiter=K)
    assert _same(du_eq, du_sh) and _same(u_eq, u_sh)
    s.close()
    one = gpu_solver_cls(M, N, 1)
    for k in range(O):   # image k is a one-image handle's sweep with (df_k, dalpha_k)
        one.set_data(f[k:k + 1], f[k:k + 1])
        for d in (0, 2):
            du1 = one.unrolled_jvp(_one(alphas, k), df=df3[d, k:k + 1], dalpha=_one(da3[d], k), maxiter=K)
            assert _same(du3[d, k], du1[0]), (k, d, float(np.abs(du3[d, k] - du1[0]).max()))
    one.close()


# ---- 3. the tangent against the twin -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", ["3x40x48", "2x17x33", "1x1x9", "1x9x1"])
def test_tangent_matches_the_twin(gpu_solver_cls, name, kind):
    """1e-11 * max|ref|.  Measured on MI355X: at most 2.6e-13, at most 8.7e-3 of its bound."""
    O, N, M = SHAPES[name]
    f, _, df = _data(name)
    alphas = _alphas(kind, name)
    amaps = ue.stack_maps(alphas, M, N)
    da = _dalphas(alphas)
    dam = ue.stack_maps(da, M, N)
    s = gpu_solver_cls(M, N, O)
    s.set_data(f, f)
    for K in (50, 203):
        for tf, ta, tam in ((df, None, None), (None, da, dam), (df, da, dam)):
            _, du0 = uj.forward_tangent(f, amaps, K, tf, tam)
            du = s.unrolled_jvp_each(alphas, df=tf, dalphas=ta, maxiter=K)
            d, b = float(np.abs(du - du0).max()), 1e-11 * float(np.abs(du0).max())
            print("%s %s K %d df %d dalpha %d: du %.2e (bound %.2e, max|ref| %.2e)"
                  % (name, kind, K, tf is not None, ta is not None, d, b, float(np.abs(du0).max())))
            assert d <= b
    s.close()


# ---- 4. the transpose identity against the per-image reverse sweep ---------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", ["3x40x48", "2x17x33", "1x1x9", "1x9x1"])
def test_tangent_is_the_transpose_of_the_per_image_reverse_sweep(gpu_solver_cls, name, kind):
    """<du, w> = <df, grad_f(w)> + sum_k <dalpha_k, grad_alpha_k(w)> to 1e-11 * sum|du * w|, all three calls on one handle."""
    O, N, M = SHAPES[name]
    f, w, df = _data(name)
    alphas = _alphas(kind, name)
    da = _dalphas(alphas)
    s = gpu_solver_cls(M, N, O)
    s.set_data(f, f)
    for K in (50, 203):
        s.unrolled_denoise_each(alphas, maxiter=K)
        du = s.unrolled_jvp_each(alphas, df=df, dalphas=da, maxiter=K)
        gf, ga = s.unrolled_vjp_each(alphas, w, maxiter=K)
        lhs = float((du * w).sum())
        rhs = float((df * gf).sum()) + sum(float((da[k] * ga[k]).sum()) for k in range(O))
        scale = float(np.abs(du * w).sum())
        print("%s %s K %d: |lhs - rhs| %.2e  bound %.2e" % (name, kind, K, abs(lhs - rhs), 1e-11 * scale))
        assert abs(lhs - rhs) <= 1e-11 * scale
    s.close()


# ---- 5. every plan gives the same bits ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["scalar", "map"])
def test_results_do_not_depend_on_the_plan(gpu_solver_cls, kind):
    import torch
    name = "2x70x72"
    O, N, M = SHAPES[name]
    f, _, _ = _data(name)
    alphas = _alphas(kind, name)
    am, an = _amn(alphas)
    rng = np.random.default_rng(21)
    df3 = rng.standard_normal((3,) + f.shape)
    da3 = _dalphas(alphas, ndir=3)
    s = gpu_solver_cls(M, N, O)
    s.set_data(f, f)
    for K in (203, 200):
        du0, u0 = s.unrolled_jvp_each(alphas, df=df3, dalphas=da3, want_u=True, maxiter=K)
        assert _same(u0, s.denoise_each(alphas, maxiter=K))
        plans = [dict(), dict(tile_iters=1), dict(tile_iters=3), dict(tile_iters=8), dict(chains=1), dict(chains=2),
                 dict(use_graph=0), dict(chains=2, use_graph=0), dict(tile_iters=3, chains=2)]
        for kw in plans:
            for rep in range(2):   # (the second call replays the cached graphs)
                du, u = s.unrolled_jvp_each(alphas, df=df3, dalphas=da3, want_u=True, maxiter=K, **kw)
                assert _same(du, du0) and _same(u, u0), (kw, rep)
        only_f = s.unrolled_jvp_each(alphas, df=df3[0], maxiter=K)
        only_a = s.unrolled_jvp_each(alphas, dalphas=da3[0], maxiter=K)
        assert _same(only_f, s.unrolled_jvp_each(alphas, df=df3[0], dalphas=np.zeros_like(da3[0]), maxiter=K))
        assert _same(only_a, s.unrolled_jvp_each(alphas, df=np.zeros_like(f), dalphas=da3[0], maxiter=K))
        # the device form
        at = torch.tensor(alphas, device="cuda")
        dft, dat = torch.tensor(df3, device="cuda"), torch.tensor(da3, device="cuda")
        dud = torch.empty(3, O, N, M, dtype=torch.float64, device="cuda")
        ud = torch.empty(O, N, M, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        for kw in (dict(), dict(), dict(chains=1, use_graph=0), dict(tile_iters=3, chains=2)):
            dud.zero_(); ud.zero_(); torch.cuda.synchronize()
            s.unrolled_jvp_each_device(at.data_ptr(), am, an, dft.data_ptr(), dat.data_ptr(), dud.data_ptr(), ud.data_ptr(),
                                       ndir=3, maxiter=K, **kw)
            assert _same(dud.cpu().numpy(), du0) and _same(ud.cpu().numpy(), u0), kw
        dud.zero_(); torch.cuda.synchronize()
        s.unrolled_jvp_each_device(at.data_ptr(), am, an, dft.data_ptr(), None, dud.data_ptr(), None, ndir=1, maxiter=K)
        assert _same(dud[0].cpu().numpy(), only_f)
        s.unrolled_jvp_each_device(at.data_ptr(), am, an, None, dat.data_ptr(), dud.data_ptr(), None, ndir=1, maxiter=K)
        assert _same(dud[0].cpu().numpy(), only_a)
    s.close()


@pytest.mark.parametrize("kind", KINDS)
def test_two_chains_split_three_images(gpu_solver_cls, kind):
    """3 images over two launch chains: 2 + 1, so the second chain starts at image 2 and must read block 2 of both."""
    name = "3x40x48"
    O, N, M = SHAPES[name]
    f, _, df = _data(name)
    alphas = _alphas(kind, name)
    da = _dalphas(alphas)
    s = gpu_solver_cls(M, N, O)
    s.set_data(f, f)
    du0 = s.unrolled_jvp_each(alphas, df=df, dalphas=da, maxiter=57, chains=1)
    for kw in (dict(chains=2), dict(chains=2, tile_iters=3), dict(chains=2, use_graph=0)):
        assert _same(s.unrolled_jvp_each(alphas, df=df, dalphas=da, maxiter=57, **kw), du0), kw
    s.close()


# ---- 6. the handle stays as it was ------------------------------------------------------------------------------------------------
def test_a_sweep_leaves_the_last_solve_the_tape_and_the_statistics(gpu_solver_cls):
    import torch
    name = "2x17x33"
    O, N, M = SHAPES[name]
    f, w, df = _data(name)
    good, maps = _alphas("scalar", name), _alphas("map", name)
    s = gpu_solver_cls(M, N, O)
    s.set_data(f, f)
    s.unrolled_denoise_each(good, maxiter=20)
    gf0, ga0 = s.unrolled_vjp_each(good, w, maxiter=20)
    u0 = s.denoise_each(maps, maxiter=57)           # the last solve: other parameters, another shape
    gap0 = s.duality_gap()
    st0 = s.stats()
    ptr0 = s.u_device_ptr()
    du = s.unrolled_jvp_each(good[::-1].copy(), df=df, dalphas=np.ones(O), maxiter=33)
    assert du.any()
    st1 = s.stats()
    assert st1["adjoint_method"] == "unrolled-jvp" and st1["adjoint_ms"] > 0.0
    for k in st0:
        if k not in ("adjoint_ms", "adjoint_method"):
            assert st1[k] == st0[k], (k, st0[k], st1[k])
    assert s.u_device_ptr() == ptr0
    out = torch.empty(O, N, M, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    s.copy_u_device(out.data_ptr())
    assert _same(out.cpu().numpy(), u0)
    assert _same(s.duality_gap(), gap0)
    gf, ga = s.unrolled_vjp_each(good, w, maxiter=20)   # the earlier per-image tape
    assert _same(gf, gf0) and _same(ga, ga0)
    s.close()


def test_rejections_leave_the_handle_as_it_was(gpu_solver_cls):
    import torch
    from bpldenoising_amd._lib import BpltvError
    name = "2x17x33"
    O, N, M = SHAPES[name]
    f, w, df = _data(name)
    good, maps = _alphas("scalar", name), _alphas("map", name)
    s = gpu_solver_cls(M, N, O)
    s.set_data(f, f)
    u0 = s.denoise_each(maps, maxiter=57)
    gap0 = s.duality_gap()

    def unchanged():
        assert _same(s.duality_gap(), gap0)
        assert _same(s.denoise_each(maps, maxiter=57), u0) and _same(s.duality_gap(), gap0)

    def rejected(code, call, *a, **k):
        with pytest.raises(BpltvError) as e:
            call(*a, **k)
        assert e.value.code == code, (e.value.code, str(e.value))
        unchanged()

    bad_df = df.copy(); bad_df[1, 3, 4] = np.inf
    for blk in (0, O - 1):                            # the first block and the last
        for v in (np.nan, -0.1):
            b = good.copy(); b[blk] = v
            rejected(E_ARG, s.unrolled_jvp_each, b, df=df, maxiter=20)
        b = maps.copy(); b[blk, 2, 5] = np.nan
        rejected(E_ARG, s.unrolled_jvp_each, b, df=df, maxiter=20)
    rejected(E_ARG, s.unrolled_jvp_each, good, df=bad_df, maxiter=20)
    da3 = np.zeros((3, O))
    for d in range(3):                                # a non-finite tangent in any block of any direction
        for blk in range(O):
            b = da3.copy(); b[d, blk] = np.nan if d % 2 else np.inf
            rejected(E_ARG, s.unrolled_jvp_each, good, dalphas=b, maxiter=20)
    dm = np.zeros((2,) + maps.shape); dm[1, O - 1, N - 1, M - 1] = np.inf
    rejected(E_ARG, s.unrolled_jvp_each, maps, dalphas=dm, maxiter=20)
    rejected(E_ARG, s.unrolled_jvp_each, good, df=df, maxiter=0)
    for kw in (dict(rho=0.01), dict(init=1), dict(order=1)):
        rejected(E_UNSUPPORTED, s.unrolled_jvp_each, good, df=df, maxiter=20, **kw)
    p = s.params(maxiter=20)
    du = np.empty_like(df)
    lib, h = s._lib, s._h
    fn = lib.bpltv_unrolled_jvp_each
    assert fn(h, _ptr(good), 1, 1, C.byref(p), 1, None, None, _ptr(du), None) == E_ARG      # both tangents NULL
    assert fn(h, _ptr(good), 1, 1, C.byref(p), 0, _ptr(df), None, _ptr(du), None) == E_ARG  # ndir < 1
    assert fn(h, _ptr(good), 1, 1, C.byref(p), 1, _ptr(df), None, None, None) == E_ARG      # no du_out
    assert fn(h, _ptr(good), M + 1, 1, C.byref(p), 1, _ptr(df), None, _ptr(du), None) == E_ARG   # shape
    assert fn(h, _ptr(good), 0, 1, C.byref(p), 1, _ptr(df), None, _ptr(du), None) == E_ARG
    unchanged()
    # the device form
    goodt = torch.tensor(good, device="cuda")
    dft, dud = torch.tensor(df, device="cuda"), torch.empty(O, N, M, dtype=torch.float64, device="cuda")
    bdt = torch.tensor(bad_df, device="cuda")
    bda = torch.zeros(O, dtype=torch.float64, device="cuda"); bda[O - 1] = float("inf")
    torch.cuda.synchronize()
    for blk in (0, O - 1):
        for v in (float("nan"), -0.1):
            bt = goodt.clone(); bt[blk] = v
            torch.cuda.synchronize()
            rejected(E_ARG, s.unrolled_jvp_each_device, bt.data_ptr(), 1, 1, dft.data_ptr(), None, dud.data_ptr(), maxiter=20)
    rejected(E_ARG, s.unrolled_jvp_each_device, goodt.data_ptr(), 1, 1, bdt.data_ptr(), None, dud.data_ptr(), maxiter=20)
    rejected(E_ARG, s.unrolled_jvp_each_device, goodt.data_ptr(), 1, 1, dft.data_ptr(), bda.data_ptr(), dud.data_ptr(), maxiter=20)
    rejected(E_ARG, s.unrolled_jvp_each_device, goodt.data_ptr(), 1, 1, None, None, dud.data_ptr(), maxiter=20)
    rejected(E_ARG, s.unrolled_jvp_each_device, goodt.data_ptr(), 1, 1, dft.data_ptr(), None, dud.data_ptr(), ndir=0, maxiter=20)
    n = gpu_solver_cls(M, N, O)                # no dataset
    with pytest.raises(BpltvError) as e:
        n.unrolled_jvp_each(good, df=df, maxiter=5)
    assert e.value.code == E_NODATA
    n.close()
    s.close()


def test_two_shards_are_unsupported_and_one_is_forwarded(gpu_solver_cls):
    from bpldenoising_amd._lib import BpltvError
    name = "2x17x33"
    O, N, M = SHAPES[name]
    f, _, df = _data(name)
    alphas = _alphas("scalar", name)
    m = gpu_solver_cls(M, N, O, devices=[0, 0])
    m.set_data(f, f)
    u0 = m.denoise(0.07, maxiter=30)
    gap0 = m.duality_gap()
    for call, args, kw in ((m.unrolled_jvp_each, (alphas,), dict(df=df)), (m.unrolled_jvp_each_device, (1, 1, 1, 1, 1, 1), dict())):
        with pytest.raises(BpltvError) as e:     # (the device form is refused before any pointer is read)
            call(*args, maxiter=30, **kw)
        assert e.value.code == E_UNSUPPORTED
        assert _same(m.duality_gap(), gap0) and _same(m.denoise(0.07, maxiter=30), u0)
    m.close()
    one = gpu_solver_cls(M, N, O, ngpus=1)       # one shard holds everything: forwarded
    one.set_data(f, f)
    s, s32 = gpu_solver_cls(M, N, O), gpu_solver_cls(M, N, O, dtype=32)
    s.set_data(f, f)
    s32.set_data(f, f)
    da = np.ones(O)
    du0 = s.unrolled_jvp_each(alphas, df=df, dalphas=da, maxiter=30)
    assert _same(one.unrolled_jvp_each(alphas, df=df, dalphas=da, maxiter=30), du0)
    assert _same(s32.unrolled_jvp_each(alphas, df=df, dalphas=da, maxiter=30), du0)   # float handles sweep in Float64
    for h in (one, s, s32):
        h.close()
