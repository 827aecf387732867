"""GPU checks of one parameter per image (bpltv_denoise_each / _device, bpltv_vjp_each / _device).

Image k of the batch is solved with its own parameter block alphas[k]: u[k] is bitwise the oracle's solve of
(f[k], alphas[k]) on every kernel plan, the VJP's per-image gradients are image k's terms alone (their sum in image
order is bpltv_vjp's gradient when the blocks are equal), and per-image and shared solves on one handle never replay
each other's graphs.  Every case uses a different parameter per image, so a block index taken from the wrong image
fails."""
import functools

import numpy as np
import pytest
from conftest import synth_batch

pytestmark = pytest.mark.gpu

IT = 53                                   # no multiple of any fusion depth the plans pick
KINDS = ["scalar", "patch23", "map"]
E_ARG, E_UNSUPPORTED = 1, 6


def _blocks(kind, O, N, M, seed=0, lo=0.02):
    """O parameter blocks with entries in [lo, lo + 0.15]: (O,) scalars, (O, 2, 3) non-square patches (a swapped
    am / an reads the wrong entries) or (O, N, M) maps."""
    rng = np.random.default_rng(seed)
    shape = {"scalar": (O,), "patch23": (O, 2, 3), "map": (O, N, M)}[kind]
    return lo + 0.15 * rng.random(shape)


def _oracle_each(oracle, f, blocks, maxiter, dtype=64, **kw):
    out = np.empty_like(f)
    for k in range(f.shape[0]):
        if dtype == 32:
            out[k] = oracle.pdhg_f32(f[k:k + 1], blocks[k], maxiter=maxiter, **kw)[0]
        elif kw.get("init") or kw.get("order"):
            out[k] = oracle.pdhg_opts(f[k:k + 1], blocks[k], maxiter=maxiter, **kw)[0]
        else:
            out[k] = oracle.pdhg(f[k:k + 1], blocks[k], maxiter=maxiter, **kw)[0]
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


# ---- PDHG against the oracle -------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [64, 32])
@pytest.mark.parametrize("shape", [(3, 40, 33), (2, 290, 270)], ids=["tile", "rows"])
def test_each_matches_the_oracle_auto_and_two_chains(gpu_solver_cls, oracle, shape, dtype):
    O, N, M = shape
    ub, f = synth_batch(O, N, M, seed=M + O)
    s = _solver(gpu_solver_cls, ub, f, dtype=dtype)
    for kind in KINDS:
        a = _blocks(kind, O, N, M, seed=len(kind))
        u0 = _oracle_each(oracle, f, a, IT, dtype)
        for chains in (0, 2):
            u = s.denoise_each(a, maxiter=IT, chains=chains)
            assert _same(u, u0), (kind, chains)
            if chains == 2:
                assert s.stats()["launch_chains"] == 2
        assert _same(s.denoise_each(a, maxiter=IT, use_graph=0), u0), kind
    s.close()


@pytest.mark.parametrize("dtype", [64, 32])
def test_each_on_every_kernel_variant(gpu_solver_cls, oracle, dtype):
    """Variants 1-36 forced on one shape every variant's min_image admits (tile, wave, rows, rows2, stream, rowsw)."""
    O, N, M = 3, 150, 140
    ub, f = synth_batch(O, N, M, seed=3)
    s = _solver(gpu_solver_cls, ub, f, dtype=dtype)
    for kind in KINDS:
        a = _blocks(kind, O, N, M, seed=11 + len(kind))
        u0 = _oracle_each(oracle, f, a, IT, dtype)
        for variant in range(1, 37):
            for chains in (1, 2):
                u = s.denoise_each(a, maxiter=IT, variant=variant, chains=chains)
                assert s.stats()["pdhg_variant"] == variant
                assert _same(u, u0), (kind, variant, chains, np.abs(u - u0).max())
    s.close()


def test_each_init_order_and_huber(gpu_solver_cls, oracle):
    """pdhg_init_kernel reads image k's block on the dual-first start; rho > 0 divides by image k's entries."""
    O, N, M = 3, 40, 33
    ub, f = synth_batch(O, N, M, seed=21)
    s = _solver(gpu_solver_cls, ub, f)
    for kind in ("patch23", "map"):
        a = _blocks(kind, O, N, M, seed=5 + len(kind))
        u = s.denoise_each(a, maxiter=IT, init=1, order=1)
        assert _same(u, _oracle_each(oracle, f, a, IT, init=1, order=1)), kind
        u = s.denoise_each(a, maxiter=IT, order=1)
        assert _same(u, _oracle_each(oracle, f, a, IT, order=1)), kind
        u = s.denoise_each(a, maxiter=IT, rho=0.01)
        assert _same(u, _oracle_each(oracle, f, a, IT, rho=0.01)), kind
    s.close()


# ---- equal blocks give the shared result -------------------------------------------------------------------------
def _shared_alpha(kind, N, M):
    return {"scalar": 0.08, "patch23": _blocks("patch23", 1, N, M, seed=2)[0], "map": _blocks("map", 1, N, M, seed=3)[0]}[kind]


@pytest.mark.parametrize("kind", KINDS)
def test_equal_blocks_give_the_shared_result_bitwise(gpu_solver_cls, kind):
    O, N, M = 4, 48, 40
    ub, f = synth_batch(O, N, M, seed=31)
    s = _solver(gpu_solver_cls, ub, f)
    alpha = _shared_alpha(kind, N, M)
    stack = np.stack([np.asarray(alpha, dtype=np.float64)] * O)
    u = s.denoise(alpha, maxiter=300)
    assert _same(s.denoise_each(stack, maxiter=300), u)
    gu = np.random.default_rng(4).standard_normal(u.shape)
    for reg in (0, 1):
        gf, ga = s.vjp(u, alpha, gu, reg=reg)
        ef, ea = s.vjp_each(u, stack, gu, reg=reg)
        assert ea.shape == stack.shape and _same(ef, gf)
        acc = np.zeros(np.shape(alpha))
        for k in range(O):   # sum_final_kernel / map_sum_kernel add the images in this order, from 0.0
            acc = acc + ea[k]
        assert _same(acc, ga), reg
    s.close()


# ---- distinct blocks against the oracle gradient --------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _vjp_case(O, N, M, kind):
    from bpldenoising_amd import TVSolver
    ub, f = synth_batch(O, N, M, seed=40 + M)
    a = _blocks(kind, O, N, M, seed=9, lo=0.04)
    s = TVSolver(M, N, O)
    s.set_data(ub, f)
    u = s.denoise_each(a, maxiter=300)
    s.close()
    return ub, f, a, u, np.random.default_rng(3).standard_normal(u.shape)


@pytest.mark.parametrize("reg", [0, 1])
@pytest.mark.parametrize("kind", KINDS)
def test_vjp_each_matches_the_oracle_and_one_image_handles(gpu_solver_cls, oracle, kind, reg):
    O, N, M = 3, 48, 40
    ub, f, a, u, gu = _vjp_case(O, N, M, kind)
    s = gpu_solver_cls(M, N, O)
    gf, ga = s.vjp_each(u, a, gu, reg=reg)
    st = s.stats()
    assert st["reg_gradient_used"] == reg and st["adjoint_residual"] <= 1e-6, st
    s.close()
    assert ga.shape == a.shape and gf.shape == u.shape
    patch = kind != "scalar"
    one = gpu_solver_cls(M, N, 1)
    for k in range(O):
        amap = oracle.patch_upsample(a[k], M, N)
        _, p, _ = oracle.gradient_image(u[k], u[k] - gu[k], amap, patch=patch, reg=bool(reg))
        want = -p if reg else p
        assert np.allclose(gf[k], want, rtol=1e-6, atol=1e-8 * np.abs(p).max()), k
        g0 = oracle.gradient(a[k], u[k:k + 1], u[k:k + 1] - gu[k:k + 1], reg=bool(reg))
        assert np.allclose(ga[k], g0, rtol=1e-6, atol=1e-8 * np.abs(g0).max()), k
        # one-image handle: the same system, a nested-dissection kernel choice that depends on the batch size
        of, oa = one.vjp(u[k:k + 1], a[k] if patch else float(a[k]), gu[k:k + 1], reg=reg)
        assert np.allclose(gf[k], of[0], rtol=1e-9, atol=1e-9 * np.abs(of).max()), k
        assert np.allclose(ga[k], oa, rtol=1e-9, atol=1e-9 * np.abs(oa).max()), k
    one.close()


# ---- solve contexts do not mix ------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [64, 32])
@pytest.mark.parametrize("kind", KINDS)
def test_shared_and_per_image_solves_never_replay_each_other(gpu_solver_cls, oracle, kind, dtype):
    """shared -> per-image -> sweep -> shared -> per-image on one handle with graphs on: every result bitwise a fresh
    handle's (a GraphKey without the addressing would replay the shared graph, block 0 for every image)."""
    O, N, M = 3, 40, 33
    ub, f = synth_batch(O, N, M, seed=61)
    alpha = _shared_alpha(kind, N, M)
    blocks = _blocks(kind, O, N, M, seed=62)
    fresh = {}
    for name, call in (("shared", lambda s: s.denoise(alpha, maxiter=IT)), ("each", lambda s: s.denoise_each(blocks, maxiter=IT))):
        s = _solver(gpu_solver_cls, ub, f, dtype=dtype)
        fresh[name] = call(s)
        s.close()
    s = _solver(gpu_solver_cls, ub, f, dtype=dtype)
    assert _same(s.denoise(alpha, maxiter=IT), fresh["shared"])
    assert _same(s.denoise_each(blocks, maxiter=IT), fresh["each"]) and s.stats()["graph_used"] == 1
    s.sweep(blocks[:2], maxiter=IT)
    assert _same(s.denoise(alpha, maxiter=IT), fresh["shared"])
    assert _same(s.denoise_each(blocks, maxiter=IT), fresh["each"])
    assert _same(_snapshot(s)[0], fresh["each"].ravel())
    assert _same(s.denoise(alpha, maxiter=IT), fresh["shared"])
    s.close()
    assert _same(fresh["each"], _oracle_each(oracle, f, blocks, IT, dtype))


@pytest.mark.parametrize("kind", KINDS)
def test_duality_gap_and_early_stop_use_each_images_block(gpu_solver_cls, oracle, kind):
    O, N, M = 3, 48, 40
    ub, f = synth_batch(O, N, M, seed=71)
    blocks = _blocks(kind, O, N, M, seed=72)
    s = _solver(gpu_solver_cls, ub, f)
    gmax = None
    for it in (100, 400):
        u = s.denoise_each(blocks, maxiter=it)
        g = s.duality_gap()
        for k in range(O):
            u0, y1, y2 = oracle.pdhg(f[k:k + 1], blocks[k], maxiter=it, return_dual=True)
            assert _same(u[k], u0[0])
            assert np.allclose(g[k], oracle.gap(u0, y1, y2, f[k:k + 1], blocks[k]), rtol=1e-6, atol=2e-9), (it, k)
        gmax = float(g.max())
    u = s.denoise_each(blocks, maxiter=5000, check_every=100, gap_tol=gmax * 1.0001)
    st = s.stats()
    assert st["iterations"] < 5000 and st["iterations"] % 100 == 0, st
    assert st["last_gap"] <= gmax * 1.0001
    assert _same(u, _oracle_each(oracle, f, blocks, st["iterations"]))
    s.close()


# ---- image groups, host and device forms, shards -------------------------------------------------------------------
def _nd_bytes_per_image(M, N):
    import os, re, subprocess
    from conftest import ROOT
    exe = os.path.join(ROOT, "tools", "_bin", "nd_host_check")
    out = subprocess.run([exe, "bytes", str(M), str(N)], capture_output=True, text=True, timeout=120).stdout
    return float(re.search(r"bytes_per_image tv (\d+)", out).group(1))


@pytest.mark.parametrize("reg", [0, 1])
@pytest.mark.parametrize("kind", KINDS)
def test_image_groups_and_device_forms_give_the_same_bits(gpu_solver_cls, kind, reg):
    import torch
    O, N, M = 3, 48, 40
    ub, f, a, u, gu = _vjp_case(O, N, M, kind)
    s = gpu_solver_cls(M, N, O)
    gf, ga = s.vjp_each(u, a, gu, reg=reg)
    assert s.stats()["adjoint_chunks"] == 1
    assert _same(s.vjp_each(u, a, gu, reg=reg, want_f=False)[1], ga)
    assert _same(s.vjp_each(u, a, gu, reg=reg, want_alpha=False)[0], gf)
    am, an = (1, 1) if kind == "scalar" else (a.shape[2], a.shape[1])
    dev = torch.device("cuda", 0)
    tu, tg, ta = (torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (u, gu, a))
    tf, tga = torch.empty_like(tu), torch.empty_like(ta)
    torch.cuda.synchronize()
    s.vjp_each_device(tu.data_ptr(), ta.data_ptr(), am, an, tg.data_ptr(), tf.data_ptr(), tga.data_ptr(), reg=reg)
    assert _same(tf.cpu().numpy(), gf) and _same(tga.cpu().numpy(), ga)
    s.close()
    sg = gpu_solver_cls(M, N, O)
    sg.set_option("adjoint_budget_mb", 1.5 * _nd_bytes_per_image(M, N) / 1e6)
    gfg, gag = sg.vjp_each(u, a, gu, reg=reg)
    assert sg.stats()["adjoint_chunks"] > 1
    assert _same(gfg, gf) and _same(gag, ga)
    sg.close()
    # the forward solve: host and device forms, float handles too
    for dtype in (64, 32):
        s = _solver(gpu_solver_cls, ub, f, dtype=dtype)
        uh = s.denoise_each(a, maxiter=IT)
        torch.cuda.synchronize()
        s.denoise_each_device(ta.data_ptr(), am, an, maxiter=IT)
        assert _same(_snapshot(s)[0], uh.ravel()), dtype
        s.close()


@pytest.mark.parametrize("kind", KINDS)
def test_sharded_handles_match_a_single_handle(gpu_solver_cls, kind):
    """bpltv_create_sharded with a repeated device: shard k takes the blocks [lo_k, hi_k); the host forms are bitwise a
    single handle's; the device forms are refused beyond one shard."""
    import torch
    from bpldenoising_amd._lib import BpltvError
    O, N, M = 3, 48, 40
    ub, f, a, u, gu = _vjp_case(O, N, M, kind)
    s = _solver(gpu_solver_cls, ub, f)
    m = _solver(gpu_solver_cls, ub, f, devices=[0, 0])
    assert _same(m.denoise_each(a, maxiter=IT), s.denoise_each(a, maxiter=IT))
    assert _same(m.duality_gap(), s.duality_gap())
    for reg in (0, 1):
        mf, ma = m.vjp_each(u, a, gu, reg=reg)
        sf, sa = s.vjp_each(u, a, gu, reg=reg)
        assert _same(mf, sf) and _same(ma, sa), reg
    assert m.stats()["shards"] == 2
    am, an = (1, 1) if kind == "scalar" else (a.shape[2], a.shape[1])
    tu, ta = torch.from_numpy(u).cuda(), torch.from_numpy(np.ascontiguousarray(a)).cuda()
    tf = torch.empty_like(tu)
    torch.cuda.synchronize()
    for call in (lambda: m.denoise_each_device(ta.data_ptr(), am, an, maxiter=IT),
                 lambda: m.vjp_each_device(tu.data_ptr(), ta.data_ptr(), am, an, tu.data_ptr(), tf.data_ptr(), None)):
        with pytest.raises(BpltvError) as e:
            call()
        assert e.value.code == E_UNSUPPORTED
    m.close()
    s.close()


# ---- rejections ---------------------------------------------------------------------------------------------------
def test_rejected_calls_change_nothing(gpu_solver_cls):
    import torch
    from bpldenoising_amd._lib import BpltvError
    from bpldenoising_amd.learning_function import _ptr
    O, N, M = 3, 48, 40
    ub, f = synth_batch(O, N, M, seed=81)
    good = _blocks("patch23", O, N, M, seed=82)
    s = _solver(gpu_solver_cls, ub, f)
    u0 = s.denoise_each(good, maxiter=200)
    snap = _snapshot(s)
    gu = np.random.default_rng(83).standard_normal(u0.shape)
    ref = s.vjp_each(u0, good, gu)
    nan_last, neg_mid, zero_one = good.copy(), good.copy(), good.copy()
    nan_last[2, 1, 2] = np.nan
    neg_mid[1, 0, 0] = -0.01
    zero_one[2, 0, 1] = 0.0
    scal = np.array([0.1, 0.2, np.inf])
    for blocks, kw in ((nan_last, {}), (neg_mid, {}), (scal, {}), (zero_one, dict(rho=0.01)),
                       (np.array([0.1, 0.0, 0.2]), dict(rho=0.01))):
        with pytest.raises(BpltvError) as e:
            s.denoise_each(blocks, maxiter=200, **kw)
        assert e.value.code == E_ARG, kw
    for blocks, reg in ((nan_last, 0), (neg_mid, 1), (zero_one, 1)):
        with pytest.raises(BpltvError) as e:
            s.vjp_each(u0, blocks, gu, reg=reg)
        assert e.value.code == E_ARG, reg
    # a bad shape (an am larger than the image) straight through the ABI
    a = np.ascontiguousarray(np.full(3 * 41 * 2, 0.1))
    assert s._lib.bpltv_denoise_each(s._h, _ptr(a), 41, 2, None, None) == E_ARG
    # device forms: every block checked on the device
    tu, tg = torch.from_numpy(u0).cuda(), torch.from_numpy(gu).cuda()
    tf = torch.empty_like(tu)
    for blocks in (nan_last, neg_mid):
        tb = torch.from_numpy(np.ascontiguousarray(blocks)).cuda()
        torch.cuda.synchronize()
        with pytest.raises(BpltvError) as e:
            s.denoise_each_device(tb.data_ptr(), 3, 2, maxiter=200)
        assert e.value.code == E_ARG
        with pytest.raises(BpltvError) as e:
            s.vjp_each_device(tu.data_ptr(), tb.data_ptr(), 3, 2, tg.data_ptr(), tf.data_ptr(), None)
        assert e.value.code == E_ARG
    tz = torch.from_numpy(np.ascontiguousarray(zero_one)).cuda()
    torch.cuda.synchronize()
    with pytest.raises(BpltvError) as e:
        s.denoise_each_device(tz.data_ptr(), 3, 2, maxiter=200, rho=0.01)
    assert e.value.code == E_ARG
    now = _snapshot(s)
    assert _same(now[0], snap[0]) and _same(now[1], snap[1])
    again = s.vjp_each(u0, good, gu)
    assert _same(again[0], ref[0]) and _same(again[1], ref[1])
    assert _same(s.denoise_each(good, maxiter=200), u0)
    s.close()
    # a sharded handle rejects a block only its second shard holds before either shard solves
    m = _solver(gpu_solver_cls, ub, f, devices=[0, 0])
    mu = m.denoise_each(good, maxiter=200)
    gap = m.duality_gap()
    with pytest.raises(BpltvError) as e:
        m.denoise_each(nan_last, maxiter=200)
    assert e.value.code == E_ARG
    assert _same(m.duality_gap(), gap) and _same(mu, u0)
    m.close()
