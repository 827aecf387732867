"""GPU checks of the unrolled solve and reverse sweep with one parameter per image (bpltv_unrolled_denoise_each /
bpltv_unrolled_vjp_each and their device forms).

u is tied to bpltv_denoise_each bit for bit; image k of every result is bitwise a one-image handle's shared call, which catches
a parameter block handed to the wrong image (the per-image parameters differ strongly, and three images split 2 + 1 over two
launch chains); equal blocks reproduce the shared calls bit for bit; the gradients are held against the numpy twin
(tests/unrolled_each_ref.py, pinned on the CPU by tests/test_unrolled_each_abi.py); every plan gives the same bits; per-image
and shared calls never replay each other's graphs; and a rejected call leaves the handle as it was."""
import ctypes as C
import functools

import numpy as np
import pytest
from conftest import synth_batch

import unrolled_each_ref as ue
import unrolled_ref as ur

pytestmark = pytest.mark.gpu

E_ARG, E_NODATA, E_UNSUPPORTED = 1, 3, 6
_dp = C.POINTER(C.c_double)
SHAPES = {"3x40x48": (3, 40, 48), "2x17x33": (2, 17, 33), "1x1x9": (1, 1, 9), "1x9x1": (1, 9, 1), "2x70x72": (2, 70, 72)}
KINDS = ["scalar", "patch", "map"]


def _same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b))


def _ptr(a):
    return a.ctypes.data_as(_dp) if a is not None else None


def _one(alphas, k):
    """Block k as the one-image calls take it: a float, or an (n, m) array."""
    return float(alphas[k]) if alphas.ndim == 1 else alphas[k]


def _amn(alphas):
    return (1, 1) if alphas.ndim == 1 else (alphas.shape[2], alphas.shape[1])


@functools.lru_cache(maxsize=None)
def _data(name, seed=5):
    O, N, M = SHAPES[name]
    ub, f = synth_batch(O, N, M, seed=seed + M)
    gu = np.random.default_rng(seed + 100).standard_normal(f.shape)
    for a in (ub, f, gu):
        a.setflags(write=False)
    return ub, f, gu


def _alphas(kind, name):
    O, N, M = SHAPES[name]
    return ue.alphas_of(kind, O, N, M)


# ---- 1. u is bpltv_denoise_each's, bit for bit --------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_u_is_denoise_each_bitwise(gpu_solver_cls, name, kind):
    O, N, M = SHAPES[name]
    _, f, _ = _data(name)
    alphas = _alphas(kind, name)
    if O > 1:
        alphas[1] = 0.0        # one image with alpha = 0 (legal)
    s = gpu_solver_cls(M, N, O)
    s.set_data(f, f)
    for accel in (1, 0):
        for maxiter in (1, 7, 203):
            u0 = s.denoise_each(alphas, maxiter=maxiter, accel=accel)
            g0 = s.duality_gap()
            u1 = s.unrolled_denoise_each(alphas, maxiter=maxiter, accel=accel)
            assert _same(u1, u0), (accel, maxiter, float(np.abs(u1 - u0).max()))
            st = s.stats()
            assert st["iterations"] == maxiter and st["pdhg_variant"] == 0 and st["launches"] >= 1 and st["tiles"] >= O, st
            assert st["bytes_per_px_iter"] == (80.0 if kind == "map" and N * M > 1 else 72.0)
            assert s.unrolled_tape_doubles(maxiter=maxiter) == 2 * maxiter * M * N * O
            # the solve is the handle's last TV solve: its gap uses image k's own block, as after denoise_each
            assert _same(s.duality_gap(), g0)
    s.close()


# ---- 2. image k is a one-image handle's result ----------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_image_k_is_a_one_image_handle_s_result(gpu_solver_cls, name, kind):
    O, N, M = SHAPES[name]
    _, f, gu = _data(name)
    alphas = _alphas(kind, name)
    K = 50
    s = gpu_solver_cls(M, N, O)
    s.set_data(f, f)
    u = s.unrolled_denoise_each(alphas, maxiter=K)
    gf, ga = s.unrolled_vjp_each(alphas, gu, maxiter=K)
    assert ga.shape == alphas.shape
    s.close()
    one = gpu_solver_cls(M, N, 1)
    for k in range(O):
        one.set_data(f[k:k + 1], f[k:k + 1])
        u1 = one.unrolled_denoise(_one(alphas, k), maxiter=K)
        gf1, ga1 = one.unrolled_vjp(_one(alphas, k), gu[k:k + 1], maxiter=K)
        assert _same(u[k], u1[0]), (k, float(np.abs(u[k] - u1[0]).max()))
        assert _same(gf[k], gf1[0]), (k, float(np.abs(gf[k] - gf1[0]).max()))
        assert _same(ga[k], ga1), (k, ga[k], ga1)
    one.close()


# ---- 3. equal blocks reproduce the shared calls -----------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_equal_blocks_reproduce_the_shared_calls_bitwise(gpu_solver_cls, name, kind):
    O, N, M = SHAPES[name]
    _, f, gu = _data(name)
    alpha = _one(_alphas(kind, name), 0)
    alphas = np.stack([np.asarray(alpha, dtype=np.float64)] * O)
    K = 50
    s = gpu_solver_cls(M, N, O)
    s.set_data(f, f)
    u0 = s.unrolled_denoise(alpha, maxiter=K)
    gf0, ga0 = s.unrolled_vjp(alpha, gu, maxiter=K)
    u = s.unrolled_denoise_each(alphas, maxiter=K)
    gf, ga = s.unrolled_vjp_each(alphas, gu, maxiter=K)
    assert _same(u, u0) and _same(gf, gf0)
    tot = np.zeros(np.shape(ga[0]))
    for k in range(O):          # in image order: bpltv_vjp_each's contract
        tot = tot + ga[k]
    assert _same(tot, ga0), (tot, ga0)
    s.close()


# ---- 4. against the twin ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", ["3x40x48", "2x17x33", "1x1x9", "1x9x1"])
def test_gradients_match_the_twin(gpu_solver_cls, name, kind):
    """Bounds: tests/test_gpu_unrolled.py::_bounds with O = 1 per block -- 1e-11 * max|ref| for grad_f, 1e-11 * max|ref
    per-pixel term of the image| * pixels per entry for block k.  Measured on MI355X: grad_f at most
    1.5e-13 against bounds of 9.1e-12 and more, a block of grad_alpha at most 2.4e-13 against bounds of 9.9e-12 (map) ...
    8.0e-8 (scalar, 3x40x48), at most 3.9e-3 of its bound; the degenerate shapes stay at 1.2e-15 or below."""
    O, N, M = SHAPES[name]
    _, f, gu = _data(name)
    alphas = _alphas(kind, name)
    amaps = ue.stack_maps(alphas, M, N)
    s = gpu_solver_cls(M, N, O)
    s.set_data(f, f)
    for K in (50, 203):
        u0, tape, tab = ur.fwd_tape(f, amaps, K)
        gf0, ga0 = ur.reverse(gu, tape, tab, amaps)
        gae0 = ue.reduce_alpha_each(ga0, alphas)
        u = s.unrolled_denoise_each(alphas, maxiter=K)
        gf, ga = s.unrolled_vjp_each(alphas, gu, maxiter=K)
        st = s.stats()
        assert st["adjoint_method"] == "unrolled" and st["adjoint_ms"] > 0.0 and st["iterations"] == K, st
        bf = 1e-11 * float(np.abs(gf0).max())
        df = float(np.abs(gf - gf0).max())
        print("%s %s K %d: max|du| %.2e  grad_f %.2e (bound %.2e)" % (name, kind, K, float(np.abs(u - u0).max()), df, bf))
        assert df <= bf
        for k in range(O):
            ba = 1e-11 * float(np.abs(ga0[k]).max()) * ur.pixels_per_entry(_one(alphas, k), M, N)
            da = float(np.abs(ga[k] - gae0[k]).max())
            print("    block %d: grad_alpha %.2e (bound %.2e)" % (k, da, ba))
            assert da <= ba
    s.close()


# ---- 5. every plan gives the same bits ------------------------------------------------------------------------------------------
PLANS = [dict(), dict(tile_iters=4), dict(tile_iters=8), dict(chains=1), dict(chains=2), dict(use_graph=0),
         dict(chains=2, use_graph=0), dict(tile_iters=4, chains=2)]


@pytest.mark.parametrize("kind", ["scalar", "map"])
def test_results_do_not_depend_on_the_plan(gpu_solver_cls, kind):
    import torch
    name = "2x70x72"
    O, N, M = SHAPES[name]
    _, f, gu = _data(name)
    alphas = _alphas(kind, name)
    am, an = _amn(alphas)
    s = gpu_solver_cls(M, N, O)
    s.set_data(f, f)
    for K in (203, 200):   # 200 iterations at depth 8: the second chain runs half a launch out of phase
        u0 = s.unrolled_denoise_each(alphas, maxiter=K)
        gf0, ga0 = s.unrolled_vjp_each(alphas, gu, maxiter=K)
        assert _same(u0, s.denoise_each(alphas, maxiter=K))
        for kw in PLANS:
            u = s.unrolled_denoise_each(alphas, maxiter=K, **kw)
            if "chains" in kw:
                assert s.stats()["launch_chains"] == (kw["chains"] if kw.get("use_graph", 1) else 1)
            gf, ga = s.unrolled_vjp_each(alphas, gu, maxiter=K, **kw)
            assert _same(u, u0) and _same(gf, gf0) and _same(ga, ga0), kw
        # the device forms, on the handle's tape and on a caller's
        at, gt = torch.tensor(alphas, device="cuda"), torch.tensor(gu, device="cuda")
        out, gfd = torch.empty(O, N, M, dtype=torch.float64, device="cuda"), torch.empty(O, N, M, dtype=torch.float64, device="cuda")
        gad = torch.empty(alphas.shape, dtype=torch.float64, device="cuda")
        tape = torch.empty(s.unrolled_tape_doubles(maxiter=K), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        for tp in (None, tape.data_ptr(), tape.data_ptr()):   # (a repeated call replays the cached graphs)
            gfd.zero_(); gad.zero_(); torch.cuda.synchronize()
            s.unrolled_denoise_each_device(at.data_ptr(), am, an, tape_ptr=tp, maxiter=K)
            s.copy_u_device(out.data_ptr())
            s.unrolled_vjp_each_device(tp, at.data_ptr(), am, an, gt.data_ptr(), gfd.data_ptr(), gad.data_ptr(), maxiter=K)
            assert _same(out.cpu().numpy(), u0) and _same(gfd.cpu().numpy(), gf0)
            assert _same(gad.cpu().numpy(), ga0)
        # one output at a time
        assert _same(s.unrolled_vjp_each(alphas, gu, want_alpha=False, maxiter=K)[0], gf0)
        assert _same(s.unrolled_vjp_each(alphas, gu, want_f=False, maxiter=K)[1], ga0)
    s.close()


@pytest.mark.parametrize("kind", KINDS)
def test_two_chains_split_three_images(gpu_solver_cls, kind):
    """3 images over two launch chains: 2 + 1, so the second chain starts at image 2 and must read block 2."""
    name = "3x40x48"
    O, N, M = SHAPES[name]
    _, f, gu = _data(name)
    alphas = _alphas(kind, name)
    K = 57
    s = gpu_solver_cls(M, N, O)
    s.set_data(f, f)
    u0 = s.unrolled_denoise_each(alphas, maxiter=K, chains=1)
    gf0, ga0 = s.unrolled_vjp_each(alphas, gu, maxiter=K, chains=1)
    for kw in (dict(chains=2), dict(chains=2, tile_iters=4), dict(chains=2, use_graph=0)):
        u = s.unrolled_denoise_each(alphas, maxiter=K, **kw)
        if kw.get("use_graph", 1):
            assert s.stats()["launch_chains"] == 2
        gf, ga = s.unrolled_vjp_each(alphas, gu, maxiter=K, **kw)
        assert _same(u, u0) and _same(gf, gf0) and _same(ga, ga0), kw
    s.close()


# ---- 6. per-image and shared calls never replay each other's graphs -----------------------------------------------------------
@pytest.mark.parametrize("kind", ["scalar", "patch"])
def test_shared_and_per_image_calls_never_replay_each_other_s_graphs(gpu_solver_cls, kind):
    name = "3x40x48"
    O, N, M = SHAPES[name]
    _, f, gu = _data(name)
    alphas = _alphas(kind, name)
    alpha, K = _one(alphas, 0), 57      # the first block is the shared parameter: the staging buffers start alike

    def fresh(call):
        h = gpu_solver_cls(M, N, O)
        h.set_data(f, f)
        r = call(h)
        h.close()
        return r
    u_sh, g_sh = fresh(lambda h: (h.unrolled_denoise(alpha, maxiter=K), h.unrolled_vjp(alpha, gu, maxiter=K)))
    u_ea, g_ea = fresh(lambda h: (h.unrolled_denoise_each(alphas, maxiter=K), h.unrolled_vjp_each(alphas, gu, maxiter=K)))
    u_plain = fresh(lambda h: h.denoise(alpha, maxiter=K))
    assert _same(u_sh, u_plain) and not _same(u_ea, u_sh)
    h = gpu_solver_cls(M, N, O)
    h.set_data(f, f)
    for rnd in range(2):   # the second round replays what the first one cached
        assert _same(h.unrolled_denoise(alpha, maxiter=K), u_sh)
        gf, ga = h.unrolled_vjp(alpha, gu, maxiter=K)
        assert _same(gf, g_sh[0]) and _same(ga, g_sh[1])
        assert _same(h.unrolled_denoise_each(alphas, maxiter=K), u_ea)
        assert _same(h.denoise(alpha, maxiter=K), u_plain)
        gf, ga = h.unrolled_vjp_each(alphas, gu, maxiter=K)      # the per-image tape survives the plain solve
        assert _same(gf, g_ea[0]) and _same(ga, g_ea[1])
    h.close()


# ---- 7. the tape's contract ---------------------------------------------------------------------------------------------------
def test_the_handle_s_tape_remembers_how_it_was_recorded(gpu_solver_cls):
    from bpldenoising_amd._lib import BpltvError
    name = "2x17x33"
    O, N, M = SHAPES[name]
    _, f, gu = _data(name)
    alphas = _alphas("scalar", name)
    s = gpu_solver_cls(M, N, O)
    s.set_data(f, f)

    def refused(code, call, *a, **k):
        with pytest.raises(BpltvError) as e:
            call(*a, **k)
        assert e.value.code == code, (e.value.code, str(e.value))

    refused(E_NODATA, s.unrolled_vjp_each, alphas, gu, maxiter=20)       # no tape yet
    s.unrolled_denoise(0.08, maxiter=20)                                  # a shared tape
    refused(E_ARG, s.unrolled_vjp_each, alphas, gu, maxiter=20)
    s.unrolled_vjp(0.08, gu, maxiter=20)
    s.unrolled_denoise_each(alphas, maxiter=20)                           # a per-image tape
    refused(E_ARG, s.unrolled_vjp, 0.08, gu, maxiter=20)
    gf, ga = s.unrolled_vjp_each(alphas, gu, maxiter=20)
    assert gf.any() and ga.all()
    gfz, gaz = s.unrolled_vjp_each(alphas, np.zeros_like(gu), maxiter=20)
    assert not gfz.any() and not gaz.any()
    refused(E_ARG, s.unrolled_vjp_each, alphas, gu, maxiter=12)           # another maxiter
    for kw in (dict(accel=0), dict(tau0=4.0), dict(sigma0=0.1), dict(opnorm=2.5)):   # other steps than the tape's
        refused(E_ARG, s.unrolled_vjp_each, alphas, gu, maxiter=20, **kw)
    refused(E_ARG, s.unrolled_vjp_each, np.full((O, 2, 2), 0.08), gu, maxiter=20)    # another parameter shape
    assert _same(s.unrolled_vjp_each(alphas, gu, maxiter=20)[0], gf)
    n = gpu_solver_cls(M, N, O)                # no dataset
    refused(E_NODATA, n.unrolled_denoise_each, alphas, maxiter=5)
    n.close()
    s.close()


# ---- 8. rejections leave the handle as it was -------------------------------------------------------------------------------------
def test_rejections_leave_the_handle_as_it_was(gpu_solver_cls):
    import torch
    from bpldenoising_amd._lib import BpltvError
    name = "2x17x33"
    O, N, M = SHAPES[name]
    _, f, gu = _data(name)
    good = _alphas("scalar", name)
    maps = _alphas("map", name)
    s = gpu_solver_cls(M, N, O)
    s.set_data(f, f)
    s.unrolled_denoise_each(good, maxiter=20)
    gf0, ga0 = s.unrolled_vjp_each(good, gu, maxiter=20)
    u0 = s.denoise_each(maps, maxiter=57)           # the last solve: other parameters, another shape
    gap0 = s.duality_gap()

    def unchanged():
        assert _same(s.duality_gap(), gap0)
        assert _same(s.denoise_each(maps, maxiter=57), u0) and _same(s.duality_gap(), gap0)
        gf, ga = s.unrolled_vjp_each(good, gu, maxiter=20)      # ... and the tape is still the first solve's
        assert _same(gf, gf0) and _same(ga, ga0)
        assert _same(s.denoise_each(maps, maxiter=57), u0)

    def rejected(code, call, *a, **k):
        with pytest.raises(BpltvError) as e:
            call(*a, **k)
        assert e.value.code == code, (e.value.code, str(e.value))
        unchanged()

    bad_gu = gu.copy(); bad_gu[1, 3, 4] = np.inf
    bads = []
    for blk in (0, O - 1):                            # the first block and the last
        for v in (np.nan, -0.1):
            b = good.copy(); b[blk] = v
            bads.append(b)
        b = maps.copy(); b[blk, 2, 5] = np.nan
        bads.append(b)
        b = maps.copy(); b[blk, N - 1, M - 1] = -1e-3
        bads.append(b)
    for bad in bads:
        rejected(E_ARG, s.unrolled_denoise_each, bad, maxiter=20)
        rejected(E_ARG, s.unrolled_vjp_each, bad, gu, maxiter=20)
    rejected(E_ARG, s.unrolled_vjp_each, good, bad_gu, maxiter=20)
    rejected(E_ARG, s.unrolled_denoise_each, good, maxiter=0)
    for kw in (dict(rho=0.01), dict(init=1), dict(order=1)):
        rejected(E_UNSUPPORTED, s.unrolled_denoise_each, good, maxiter=20, **kw)
        rejected(E_UNSUPPORTED, s.unrolled_vjp_each, good, gu, maxiter=20, **kw)
    p = s.params(maxiter=20)
    rc = s._lib.bpltv_unrolled_vjp_each(s._h, _ptr(good), 1, 1, C.byref(p), _ptr(gu), None, None)   # both outputs NULL
    assert rc == E_ARG
    unchanged()
    # the device forms
    gt, gfd = torch.tensor(gu, device="cuda"), torch.empty(O, N, M, dtype=torch.float64, device="cuda")
    goodt = torch.tensor(good, device="cuda")
    torch.cuda.synchronize()
    for bad in bads[:2] + bads[4:6]:
        bt = torch.tensor(bad, device="cuda")
        torch.cuda.synchronize()
        rejected(E_ARG, s.unrolled_denoise_each_device, bt.data_ptr(), 1, 1, maxiter=20)
        rejected(E_ARG, s.unrolled_vjp_each_device, None, bt.data_ptr(), 1, 1, gt.data_ptr(), gfd.data_ptr(), None, maxiter=20)
    bgt = torch.tensor(bad_gu, device="cuda")
    torch.cuda.synchronize()
    rejected(E_ARG, s.unrolled_vjp_each_device, None, goodt.data_ptr(), 1, 1, bgt.data_ptr(), gfd.data_ptr(), None, maxiter=20)
    rejected(E_ARG, s.unrolled_vjp_each_device, None, goodt.data_ptr(), 1, 1, gt.data_ptr(), None, None, maxiter=20)
    s.close()


# ---- 9. shards and handle types ---------------------------------------------------------------------------------------------------
def test_two_shards_are_unsupported_and_one_is_forwarded(gpu_solver_cls):
    from bpldenoising_amd._lib import BpltvError
    name = "2x17x33"
    O, N, M = SHAPES[name]
    _, f, gu = _data(name)
    alphas = _alphas("scalar", name)
    m = gpu_solver_cls(M, N, O, devices=[0, 0])
    m.set_data(f, f)
    u0 = m.denoise(0.07, maxiter=30)
    gap0 = m.duality_gap()
    for call, args in ((m.unrolled_denoise_each, (alphas,)), (m.unrolled_vjp_each, (alphas, gu)),
                       (m.unrolled_denoise_each_device, (1, 1, 1)), (m.unrolled_vjp_each_device, (None, 1, 1, 1, 1, 1, 1))):
        with pytest.raises(BpltvError) as e:     # (the device forms are refused before any pointer is read)
            call(*args, maxiter=30)
        assert e.value.code == E_UNSUPPORTED
        assert _same(m.duality_gap(), gap0) and _same(m.denoise(0.07, maxiter=30), u0)
    m.close()
    one = gpu_solver_cls(M, N, O, ngpus=1)       # one shard holds everything: forwarded
    one.set_data(f, f)
    s = gpu_solver_cls(M, N, O)
    s.set_data(f, f)
    assert _same(one.unrolled_denoise_each(alphas, maxiter=30), s.unrolled_denoise_each(alphas, maxiter=30))
    a, b = one.unrolled_vjp_each(alphas, gu, maxiter=30), s.unrolled_vjp_each(alphas, gu, maxiter=30)
    assert _same(a[0], b[0]) and _same(a[1], b[1])
    one.close()
    s.close()


@pytest.mark.parametrize("kind", ["scalar", "map"])
def test_float_handles_run_the_per_image_solve_in_float64(gpu_solver_cls, kind):
    name = "2x17x33"
    O, N, M = SHAPES[name]
    _, f, gu = _data(name)
    alphas = _alphas(kind, name)
    s, s32 = gpu_solver_cls(M, N, O), gpu_solver_cls(M, N, O, dtype=32)
    for h in (s, s32):
        h.set_data(f, f)
    assert _same(s32.unrolled_denoise_each(alphas, maxiter=40), s.unrolled_denoise_each(alphas, maxiter=40))
    a, b = s32.unrolled_vjp_each(alphas, gu, maxiter=40), s.unrolled_vjp_each(alphas, gu, maxiter=40)
    assert _same(a[0], b[0]) and _same(a[1], b[1])
    s.close()
    s32.close()
