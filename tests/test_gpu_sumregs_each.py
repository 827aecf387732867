"""GPU checks of per-image sum-of-regularisers weights (bpltv_sumregs_denoise_each / _device,
bpltv_sumregs_vjp_each / _device).

Image k of the batch is solved with its own block alphas[k] of three slices: u[k] is bitwise the oracle's solve of
(f[k], alphas[k]) on both kernels, every chain count, replayed and eager; gap, early stop and the VJP use block k for
image k; the per-image gradients are image k's terms alone (their sum in image order is bpltv_sumregs_vjp's gradient
when the blocks are equal); per-image and shared solves on one handle never replay each other's graphs.  Every case
uses a different block per image, so a block index taken from the wrong image fails.  No tolerance is new: the bars are
those of test_gpu_sumregs.py (gap) and test_gpu_sumregs_vjp.py (gradients)."""
import functools
import os
import re
import subprocess

import numpy as np
import pytest
from conftest import ROOT, synth_batch

pytestmark = pytest.mark.gpu

IT = 53                                   # no multiple of any fusion depth
KINDS = ["vector", "patch23", "map"]
E_ARG, E_UNSUPPORTED = 1, 6
GRADF_TOL = 5e-6                          # test_gpu_sumregs_vjp.py: grad_f against the literal system, relative to max|p|
GAP_RTOL, GAP_ATOL = 1e-6, 2e-9           # test_gpu_sumregs.py, DESIGN 2.2


def _blocks(kind, O, N, M, seed=0, lo=0.02):
    """O blocks with entries in [lo, lo + 0.05]: (O, 3) vectors, (O, 3, 2, 3) non-square patches (a swapped am / an or
    a wrong slice distance reads the wrong entries) or (O, 3, N, M) maps."""
    rng = np.random.default_rng(seed)
    shape = {"vector": (O, 3), "patch23": (O, 3, 2, 3), "map": (O, 3, N, M)}[kind]
    return lo + 0.05 * rng.random(shape)


def _amn(a):
    return (1, 1) if a.ndim == 2 else (a.shape[3], a.shape[2])


def _oracle_each(oracle, f, blocks, maxiter, **kw):
    out = np.empty_like(f)
    for k in range(f.shape[0]):
        out[k] = oracle.sumregs_pdhg(f[k:k + 1], blocks[k], maxiter=maxiter, nthreads=4, **kw)[0]
    return out


def _solver(cls, ub, f, **kw):
    O, N, M = f.shape
    s = cls(M, N, O, **kw)
    s.set_data(ub, f)
    return s


def _same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b))


def _snapshot(s):
    import torch
    buf = torch.empty(s.O * s.N * s.M, dtype=torch.float64, device="cuda")
    s.copy_u_device(buf.data_ptr())
    return buf.cpu().numpy(), s.duality_gap()


def _sr_bytes_per_image(M, N):
    out = subprocess.run([os.path.join(ROOT, "tools", "_bin", "nd_host_check"), "bytes", str(M), str(N)],
                         capture_output=True, text=True, timeout=120).stdout
    return float(re.search(r"bytes_per_image sr (\d+)", out).group(1))


# ---- PDHG against the oracle -------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(3, 40, 33), (4, 256, 256)], ids=["tile", "strip"])
def test_each_matches_the_oracle_on_both_kernels(gpu_solver_cls, oracle, shape):
    """variant 1 (one pixel per thread), variant 2 (strips) and the automatic choice -- the one-pixel kernel on
    3 x 40 x 33, the strip kernel on 4 x 256^2 -- with chains 0 / 1 / 2, replayed from graphs and launched eagerly."""
    O, N, M = shape
    ub, f = synth_batch(O, N, M, seed=M + O)
    s = _solver(gpu_solver_cls, ub, f)
    auto_region = 32 if M <= 48 else 48
    for kind in KINDS:
        a = _blocks(kind, O, N, M, seed=len(kind))
        u0 = _oracle_each(oracle, f, a, IT)
        for variant in (0, 1, 2):
            for chains in (0, 1, 2):
                u = s.sumregs_denoise_each(a, maxiter=IT, variant=variant, chains=chains)
                st = s.stats()
                assert st["graph_used"] == 1
                assert st["region_i"] == ({1: 32, 2: 48}[variant] if variant else auto_region), (variant, st["region_i"])
                if chains:
                    assert st["launch_chains"] == chains
                assert _same(u, u0), (kind, variant, chains, np.abs(u - u0).max())
            u = s.sumregs_denoise_each(a, maxiter=IT, variant=variant, use_graph=0)
            assert s.stats()["graph_used"] == 0 and _same(u, u0), (kind, variant, "eager")
    s.close()


@pytest.mark.parametrize("variant", [1, 2])
def test_each_with_huber_smoothing(gpu_solver_cls, oracle, variant):
    """rho > 0 divides by image k's own entries."""
    O, N, M = 3, 40, 33
    ub, f = synth_batch(O, N, M, seed=21)
    s = _solver(gpu_solver_cls, ub, f)
    for kind in KINDS:
        a = _blocks(kind, O, N, M, seed=5 + len(kind))
        u = s.sumregs_denoise_each(a, maxiter=IT, rho=0.01, variant=variant)
        assert _same(u, _oracle_each(oracle, f, a, IT, rho=0.01)), kind
    s.close()


@pytest.mark.parametrize("kind", KINDS)
def test_duality_gap_and_early_stop_use_each_images_block(gpu_solver_cls, oracle, kind):
    O, N, M = 3, 48, 40
    ub, f = synth_batch(O, N, M, seed=71)
    blocks = _blocks(kind, O, N, M, seed=72)
    s = _solver(gpu_solver_cls, ub, f)
    gmax = None
    for it in (100, 400):
        u = s.sumregs_denoise_each(blocks, maxiter=it)
        g = s.duality_gap()
        for k in range(O):
            u0, y0 = oracle.sumregs_pdhg(f[k:k + 1], blocks[k], maxiter=it, nthreads=4, return_dual=True)
            assert _same(u[k], u0[0])
            g0 = oracle.sumregs_gap(u0, y0, f[k:k + 1], blocks[k])
            print("gap %s it=%d image %d: library %.6e oracle %.6e" % (kind, it, k, g[k], g0[0]))
            assert np.allclose(g[k], g0[0], rtol=GAP_RTOL, atol=GAP_ATOL), (it, k)
        gmax = float(g.max())
    u = s.sumregs_denoise_each(blocks, maxiter=5000, check_every=100, gap_tol=gmax * 1.0001)
    st = s.stats()
    assert st["iterations"] < 5000 and st["iterations"] % 100 == 0, st
    assert 0 <= st["last_gap"] <= gmax * 1.0001
    assert _same(u, _oracle_each(oracle, f, blocks, st["iterations"]))
    g = s.duality_gap()   # of the early-stopped iterate, block k for image k
    for k in range(O):
        u0, y0 = oracle.sumregs_pdhg(f[k:k + 1], blocks[k], maxiter=st["iterations"], nthreads=4, return_dual=True)
        assert np.allclose(g[k], oracle.sumregs_gap(u0, y0, f[k:k + 1], blocks[k])[0], rtol=GAP_RTOL, atol=GAP_ATOL), k
    s.close()


# ---- the VJP against the oracle --------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _vjp_case(O, N, M, kind):
    from bpldenoising_amd import TVSolver
    ub, f = synth_batch(O, N, M, seed=40 + M)
    a = _blocks(kind, O, N, M, seed=9)
    s = TVSolver(M, N, O)
    s.set_data(ub, f)
    u = s.sumregs_denoise_each(a, maxiter=300)
    s.close()
    return ub, f, a, u, np.random.default_rng(3).standard_normal(u.shape)


@pytest.mark.parametrize("reg", [0, 1])
@pytest.mark.parametrize("kind", KINDS)
def test_vjp_each_matches_the_oracle(gpu_solver_cls, oracle, kind, reg):
    """grad_alphas[k] == oracle.sumregs_gradient(alphas[k], u[k], (u - gu)[k]) relative to max|g0| (1e-6, reg = 1: 1e-7);
    grad_f[k] == +-p of the literal system of image k with block k (GRADF_TOL of max|p|)."""
    from oracle import np_twin_sumregs as TS
    O, N, M = 3, 48, 40
    ub, f, a, u, gu = _vjp_case(O, N, M, kind)
    s = gpu_solver_cls(M, N, O)
    gf, ga = s.sumregs_vjp_each(u, a, gu, reg=reg)
    st = s.stats()
    assert st["reg_gradient_used"] == reg and st["adjoint_residual"] <= 1e-6 and st["adjoint_chunks"] == 1, st
    s.close()
    assert ga.shape == a.shape and gf.shape == u.shape
    for k in range(O):
        g0 = oracle.sumregs_gradient(a[k], u[k:k + 1], (u - gu)[k:k + 1], reg=bool(reg))
        scale = np.abs(g0).max()
        ea = np.abs(ga[k] - g0).max() / scale
        if reg:
            p = -TS.gradient_reg_image(a[k], u[k], u[k] - gu[k])[1]
        else:
            p = TS.gradient_image(a[k], u[k], u[k] - gu[k])[1]
        p = p.reshape(N, M)
        ef = np.abs(gf[k] - p).max() / np.abs(p).max()
        print("vjp_each %s reg=%d image %d: grad_alphas %.3e of max|g0|, grad_f %.3e of max|p|" % (kind, reg, k, ea, ef))
        assert ea <= (1e-7 if reg else 1e-6), (k, ea)
        assert ef <= GRADF_TOL, (k, ef)


# ---- bitwise properties ------------------------------------------------------------------------------------------------
def _shared_alpha(kind, N, M):
    return _blocks(kind, 1, N, M, seed=2)[0]


@pytest.mark.parametrize("kind", KINDS)
def test_equal_blocks_give_the_shared_result_bitwise(gpu_solver_cls, kind):
    O, N, M = 4, 48, 40
    ub, f = synth_batch(O, N, M, seed=31)
    s = _solver(gpu_solver_cls, ub, f)
    alpha = _shared_alpha(kind, N, M)
    stack = np.stack([alpha] * O)
    u = s.sumregs_denoise(alpha, maxiter=300)
    assert _same(s.sumregs_denoise_each(stack, maxiter=300), u)
    gu = np.random.default_rng(4).standard_normal(u.shape)
    for reg in (0, 1):
        gf, ga = s.sumregs_vjp(u, alpha, gu, reg=reg)
        ef, ea = s.sumregs_vjp_each(u, stack, gu, reg=reg)
        assert ea.shape == stack.shape and _same(ef, gf)
        acc = np.zeros(np.shape(alpha))
        for k in range(O):   # sum_final_kernel / map_sum_kernel add the images in this order, from 0.0
            acc = acc + ea[k]
        assert _same(acc, ga), reg
    s.close()


@pytest.mark.parametrize("kind", KINDS)
def test_changing_one_block_leaves_the_other_images_bit_identical(gpu_solver_cls, kind):
    O, N, M = 3, 48, 40
    ub, f, a, u, gu = _vjp_case(O, N, M, kind)
    j = 1
    b = a.copy()
    b[j] = 1.5 * a[j][::-1]   # the three slices swapped end to end and scaled: every entry of block j differs
    s = _solver(gpu_solver_cls, ub, f)
    ua, ub_ = s.sumregs_denoise_each(a, maxiter=IT), s.sumregs_denoise_each(b, maxiter=IT)
    assert not _same(ua[j], ub_[j])
    for reg in (0, 1):
        fa, ga = s.sumregs_vjp_each(u, a, gu, reg=reg)
        fb, gb = s.sumregs_vjp_each(u, b, gu, reg=reg)
        assert not _same(fa[j], fb[j]) and not _same(ga[j], gb[j])
        for k in range(O):
            if k != j:
                assert _same(ua[k], ub_[k]) and _same(fa[k], fb[k]) and _same(ga[k], gb[k]), (k, reg)
    s.close()


@pytest.mark.parametrize("reg", [0, 1])
@pytest.mark.parametrize("kind", KINDS)
def test_image_groups_and_device_forms_give_the_same_bits(gpu_solver_cls, kind, reg):
    import torch
    O, N, M = 3, 48, 40
    ub, f, a, u, gu = _vjp_case(O, N, M, kind)
    s = gpu_solver_cls(M, N, O)
    gf, ga = s.sumregs_vjp_each(u, a, gu, reg=reg)
    assert s.stats()["adjoint_chunks"] == 1
    assert _same(s.sumregs_vjp_each(u, a, gu, reg=reg, want_f=False)[1], ga)
    assert _same(s.sumregs_vjp_each(u, a, gu, reg=reg, want_alpha=False)[0], gf)
    am, an = _amn(a)
    dev = torch.device("cuda", 0)
    tu, tg, ta = (torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (u, gu, a))
    tf, tga = torch.empty_like(tu), torch.empty_like(ta)
    torch.cuda.synchronize()
    s.sumregs_vjp_each_device(tu.data_ptr(), ta.data_ptr(), am, an, tg.data_ptr(), tf.data_ptr(), tga.data_ptr(), reg=reg)
    assert _same(tf.cpu().numpy(), gf) and _same(tga.cpu().numpy(), ga)
    tf2, tga2 = torch.zeros_like(tu), torch.zeros_like(ta)
    s.sumregs_vjp_each_device(tu.data_ptr(), ta.data_ptr(), am, an, tg.data_ptr(), tf2.data_ptr(), None, reg=reg)
    s.sumregs_vjp_each_device(tu.data_ptr(), ta.data_ptr(), am, an, tg.data_ptr(), None, tga2.data_ptr(), reg=reg)
    assert _same(tf2.cpu().numpy(), gf) and _same(tga2.cpu().numpy(), ga)
    s.close()
    # image groups: a budget of 2.5 images' nested-dissection workspace -- the second group starts at image 2 (the LU
    # variant's workspace is larger: more groups), and a group offset that is not applied to the blocks fails
    sg = gpu_solver_cls(M, N, O)
    sg.set_option("adjoint_budget_mb", 2.5 * _sr_bytes_per_image(M, N) / 1e6)
    gfg, gag = sg.sumregs_vjp_each(u, a, gu, reg=reg)
    assert sg.stats()["adjoint_chunks"] > 1
    assert _same(gfg, gf) and _same(gag, ga)
    sg.close()
    # the forward solve: host and device forms, float handles too (the model is Float64 there)
    for dtype in (64, 32):
        s = _solver(gpu_solver_cls, ub, f, dtype=dtype)
        uh = s.sumregs_denoise_each(a, maxiter=IT)
        torch.cuda.synchronize()
        s.sumregs_denoise_each_device(ta.data_ptr(), am, an, maxiter=IT)
        assert _same(_snapshot(s)[0], uh.ravel()), dtype
        s.close()


@pytest.mark.parametrize("kind", KINDS)
def test_float_handles_give_the_double_handles_results(gpu_solver_cls, kind):
    O, N, M = 3, 48, 40
    ub, f, a, u, gu = _vjp_case(O, N, M, kind)
    s64, s32 = _solver(gpu_solver_cls, ub, f), _solver(gpu_solver_cls, ub, f, dtype=32)
    assert _same(s32.sumregs_denoise_each(a, maxiter=IT), s64.sumregs_denoise_each(a, maxiter=IT))
    assert _same(s32.duality_gap(), s64.duality_gap())
    for reg in (0, 1):
        f64, a64 = s64.sumregs_vjp_each(u, a, gu, reg=reg)
        f32, a32 = s32.sumregs_vjp_each(u, a, gu, reg=reg)
        assert _same(f32, f64) and _same(a32, a64), reg
    s32.close()
    s64.close()


@pytest.mark.parametrize("kind", KINDS)
def test_shared_and_per_image_solves_never_replay_each_other(gpu_solver_cls, oracle, kind):
    """shared -> per-image -> shared -> per-image on one handle, graphs on, one maxiter: every result bitwise a fresh
    handle's (a GraphKey without the block stride would replay the shared graph, block 0 for every image)."""
    O, N, M = 3, 40, 33
    ub, f = synth_batch(O, N, M, seed=61)
    blocks = _blocks(kind, O, N, M, seed=62)
    alpha = blocks[0].copy()   # the shared parameter IS block 0: the same bytes at d_alpha + 0 in both modes
    fresh = {}
    for name, call in (("shared", lambda s: s.sumregs_denoise(alpha, maxiter=IT)),
                       ("each", lambda s: s.sumregs_denoise_each(blocks, maxiter=IT))):
        s = _solver(gpu_solver_cls, ub, f)
        fresh[name] = (call(s), s.duality_gap())
        s.close()
    assert not _same(fresh["shared"][0][1:], fresh["each"][0][1:])
    s = _solver(gpu_solver_cls, ub, f)
    for name in ("shared", "each", "shared", "each"):
        u = s.sumregs_denoise(alpha, maxiter=IT) if name == "shared" else s.sumregs_denoise_each(blocks, maxiter=IT)
        assert s.stats()["graph_used"] == 1
        assert _same(u, fresh[name][0]), name
        snap = _snapshot(s)
        assert _same(snap[0], fresh[name][0].ravel()) and _same(snap[1], fresh[name][1]), name
    s.close()
    assert _same(fresh["each"][0], _oracle_each(oracle, f, blocks, IT))


@pytest.mark.parametrize("kind", KINDS)
def test_sharded_handles_match_a_single_handle(gpu_solver_cls, kind):
    """bpltv_create_sharded with a repeated device: shard k takes the blocks [lo_k, hi_k) and writes its gradient blocks
    in place; the host forms are bitwise a single handle's; the device forms are refused beyond one shard."""
    import torch
    from bpldenoising_amd._lib import BpltvError
    O, N, M = 3, 48, 40
    ub, f, a, u, gu = _vjp_case(O, N, M, kind)
    s = _solver(gpu_solver_cls, ub, f)
    m = _solver(gpu_solver_cls, ub, f, devices=[0, 0])
    assert _same(m.sumregs_denoise_each(a, maxiter=IT), s.sumregs_denoise_each(a, maxiter=IT))
    assert _same(m.duality_gap(), s.duality_gap())
    for reg in (0, 1):
        mf, ma = m.sumregs_vjp_each(u, a, gu, reg=reg)
        sf, sa = s.sumregs_vjp_each(u, a, gu, reg=reg)
        assert _same(mf, sf) and _same(ma, sa), reg
    assert m.stats()["shards"] == 2
    am, an = _amn(a)
    tu, ta = torch.from_numpy(u).cuda(), torch.from_numpy(np.ascontiguousarray(a)).cuda()
    tf = torch.empty_like(tu)
    torch.cuda.synchronize()
    for call in (lambda: m.sumregs_denoise_each_device(ta.data_ptr(), am, an, maxiter=IT),
                 lambda: m.sumregs_vjp_each_device(tu.data_ptr(), ta.data_ptr(), am, an, tu.data_ptr(), tf.data_ptr(), None)):
        with pytest.raises(BpltvError) as e:
            call()
        assert e.value.code == E_UNSUPPORTED
    m.close()
    s.close()


# ---- rejections ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("last", ["each", "shared"])
def test_rejected_calls_change_nothing(gpu_solver_cls, last):
    """A NaN, a negative entry, a zero under rho != 0, a zero under reg = 1 with a patch parameter -- each in ONE block
    of the batch -- a non-finite gu, reserved[4] = 2 and init / order: each returns its code, host and device forms, and
    the last solve (per-image or shared), its duality gap and the next solve are bit for bit those of a handle that
    never saw the rejected calls."""
    import torch
    from bpldenoising_amd._lib import BpltvError
    from bpldenoising_amd.learning_function import _ptr
    O, N, M = 3, 48, 40
    ub, f = synth_batch(O, N, M, seed=81)
    good = _blocks("patch23", O, N, M, seed=82)
    shared = good[1].copy()

    def solve(s):
        return s.sumregs_denoise_each(good, maxiter=200) if last == "each" else s.sumregs_denoise(shared, maxiter=200)

    clean = _solver(gpu_solver_cls, ub, f)   # never sees a rejected call
    u0 = solve(clean)
    snap0 = _snapshot(clean)
    gu = np.random.default_rng(83).standard_normal(u0.shape)
    ref = clean.sumregs_vjp_each(u0, good, gu, reg=1)
    again0 = solve(clean)
    snap1 = _snapshot(clean)
    clean.close()

    s = _solver(gpu_solver_cls, ub, f)
    assert _same(solve(s), u0)
    nan_last, neg_mid, zero_one = good.copy(), good.copy(), good.copy()
    nan_last[2, 2, 1, 2] = np.nan
    neg_mid[1, 0, 0, 0] = -0.01
    zero_one[2, 1, 0, 1] = 0.0
    vec_inf = np.array([[0.03, 0.02, 0.05], [0.03, 0.02, 0.05], [0.03, np.inf, 0.05]])
    vec_zero = np.array([[0.03, 0.02, 0.05], [0.03, 0.0, 0.05], [0.03, 0.02, 0.05]])
    bad_gu = gu.copy()
    bad_gu[2, 7, 5] = np.nan
    for blocks, kw in ((nan_last, {}), (neg_mid, {}), (vec_inf, {}), (zero_one, dict(rho=0.01)), (vec_zero, dict(rho=0.01))):
        with pytest.raises(BpltvError) as e:
            s.sumregs_denoise_each(blocks, maxiter=200, **kw)
        assert e.value.code == E_ARG, kw
    for kw in (dict(init=1), dict(order=1)):
        with pytest.raises(BpltvError) as e:
            s.sumregs_denoise_each(good, maxiter=200, **kw)
        assert e.value.code == E_UNSUPPORTED, kw
    for blocks, g, reg in ((nan_last, gu, 0), (neg_mid, gu, 1), (zero_one, gu, 1), (good, bad_gu, 0), (good, bad_gu, 1)):
        with pytest.raises(BpltvError) as e:
            s.sumregs_vjp_each(u0, blocks, g, reg=reg)
        assert e.value.code == E_ARG, reg
    with pytest.raises(BpltvError) as e:
        s.sumregs_vjp_each(u0, good, gu, adjoint_method="bcr")
    assert e.value.code == E_UNSUPPORTED
    s.sumregs_vjp_each(u0, zero_one, gu, reg=0)   # a zero entry is fine for sumregs_gradient (reg = 0)
    # a bad shape (an am larger than the image) straight through the ABI
    big = np.ascontiguousarray(np.full(3 * 3 * 41 * 2, 0.1))
    assert s._lib.bpltv_sumregs_denoise_each(s._h, _ptr(big), 41, 2, None, None) == E_ARG
    assert s._lib.bpltv_sumregs_vjp_each(s._h, _ptr(u0), _ptr(big), 41, 2, 0, None, _ptr(gu), None, _ptr(big)) == E_ARG
    # device forms: every block and the cotangent checked on the device
    tu, tg, tbad = (torch.from_numpy(x).cuda() for x in (u0, gu, bad_gu))
    tf = torch.empty_like(tu)
    tgood = torch.from_numpy(np.ascontiguousarray(good)).cuda()
    for blocks in (nan_last, neg_mid):
        tb = torch.from_numpy(np.ascontiguousarray(blocks)).cuda()
        torch.cuda.synchronize()
        with pytest.raises(BpltvError) as e:
            s.sumregs_denoise_each_device(tb.data_ptr(), 3, 2, maxiter=200)
        assert e.value.code == E_ARG
        with pytest.raises(BpltvError) as e:
            s.sumregs_vjp_each_device(tu.data_ptr(), tb.data_ptr(), 3, 2, tg.data_ptr(), tf.data_ptr(), None)
        assert e.value.code == E_ARG
    tz = torch.from_numpy(np.ascontiguousarray(zero_one)).cuda()
    torch.cuda.synchronize()
    with pytest.raises(BpltvError) as e:
        s.sumregs_denoise_each_device(tz.data_ptr(), 3, 2, maxiter=200, rho=0.01)
    assert e.value.code == E_ARG
    with pytest.raises(BpltvError) as e:
        s.sumregs_vjp_each_device(tu.data_ptr(), tz.data_ptr(), 3, 2, tg.data_ptr(), tf.data_ptr(), None, reg=1)
    assert e.value.code == E_ARG
    with pytest.raises(BpltvError) as e:
        s.sumregs_vjp_each_device(tu.data_ptr(), tgood.data_ptr(), 3, 2, tbad.data_ptr(), tf.data_ptr(), None)
    assert e.value.code == E_ARG
    with pytest.raises(BpltvError) as e:
        s.sumregs_vjp_each_device(tu.data_ptr(), tgood.data_ptr(), 3, 2, tg.data_ptr(), tf.data_ptr(), None,
                                  adjoint_method="bcr")
    assert e.value.code == E_UNSUPPORTED
    now = _snapshot(s)
    assert _same(now[0], snap0[0]) and _same(now[1], snap0[1])
    got = s.sumregs_vjp_each(u0, good, gu, reg=1)
    assert _same(got[0], ref[0]) and _same(got[1], ref[1])
    assert _same(solve(s), again0)
    now = _snapshot(s)
    assert _same(now[0], snap1[0]) and _same(now[1], snap1[1])
    s.close()


def test_a_sharded_handle_rejects_before_any_shard_solves(gpu_solver_cls):
    from bpldenoising_amd._lib import BpltvError
    O, N, M = 3, 48, 40
    ub, f = synth_batch(O, N, M, seed=81)
    good = _blocks("patch23", O, N, M, seed=82)
    nan_last = good.copy()
    nan_last[2, 2, 1, 2] = np.nan   # a block only the second shard holds
    m = _solver(gpu_solver_cls, ub, f, devices=[0, 0])
    m.sumregs_denoise_each(good, maxiter=200)
    gap = m.duality_gap()
    with pytest.raises(BpltvError) as e:
        m.sumregs_denoise_each(nan_last, maxiter=200)
    assert e.value.code == E_ARG
    assert _same(m.duality_gap(), gap)
    m.close()
