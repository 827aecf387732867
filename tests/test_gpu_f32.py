"""Opt-in single-precision PDHG (bpltv_create(dtype = 32)): the kernel's float instantiation against the oracle's
"spec v2f" restatement (bit for bit), and against the Float64 result (how much narrower it is).  The reference is
Float64 only (src/TVLearningFunctionVec.jl:8-9): nothing here is a parity claim with it.
Pinned bit for bit like the Float64 path: all 36 float kernel instantiations (fusion depths, launch chains, eager and graph
launches), awkward shapes, the three parameter forms, the Huber term, accel = 0, chunked solves, sweeps, the multi-device
handle, subnormal parameters; the gap and the gradient against the oracle's of the same float state."""
import numpy as np
import pytest

from conftest import DATASETS_NPZ, synth_batch
from oracle import np_twin as T

pytestmark = pytest.mark.gpu

P22 = np.array([[0.05, 0.1], [0.2, 0.08]])


@pytest.mark.parametrize("amode", ["scalar", "patch", "map"])
def test_f32_matches_oracle_f32_bitwise(gpu_solver_cls, oracle, amode):
    ub, f = T.load_dataset(DATASETS_NPZ, "faces_train_128_10")
    O, N, M = f.shape
    rng = np.random.default_rng(5)
    alpha = {"scalar": 0.1, "patch": np.array([[0.05, 0.12], [0.2, 0.08]]),
             "map": 0.02 + 0.18 * rng.random((N, M))}[amode]
    s = gpu_solver_cls(M, N, O, dtype=32)
    s.set_data(ub, f)
    for variant in (0, 2, 13, 19, 24):   # the automatic plan, a 4-pixel-per-thread tile, the wide-image tile, 64-lane rows
        u = s.denoise(alpha, maxiter=200, variant=variant)
        ref = oracle.pdhg_f32(f, alpha, maxiter=200)
        assert np.array_equal(u, ref), (amode, variant, np.abs(u - ref).max())
    st = s.stats()
    assert st["bytes_per_px_iter"] in (28.0, 32.0)
    s.close()


def test_f32_close_to_f64_and_evaluate_runs(gpu_solver_cls, oracle):
    """5000 iterations: the float iterate stays within 1e-4 of the Float64 one (measured 1.5e-5 max, ~2e-7 typical),
    the loss within 1e-5 relative.  The adjoint gradient (computed in Float64 from the widened u) moves by about 1 %
    (bound here: 5 %): the reference's active set is |grad u| < 1e-12 (src/TVLearningFunctionVec.jl:110), and float
    noise of ~1e-7 in the flat regions of u empties it -- the reason this mode is opt-in and not a parity claim."""
    ub, f = T.load_dataset(DATASETS_NPZ, "faces_train_128_10")
    O, N, M = f.shape
    s64 = gpu_solver_cls(M, N, O)
    s32 = gpu_solver_cls(M, N, O, dtype=32)
    for s in (s64, s32):
        s.set_data(ub, f)
    u64, c64, g64 = s64.evaluate(0.1, 0.1)
    u32, c32, g32 = s32.evaluate(0.1, 0.1)
    assert np.abs(u32 - u64).max() < 1e-4
    assert abs(c32 - c64) <= 1e-5 * abs(c64)
    assert abs(g32 - g64) <= 5e-2 * abs(g64)
    assert s32.stats()["adjoint_residual"] <= 1e-8
    # the gap certificate works on the widened state (chunked solve with early stop)
    s32.denoise(0.1, maxiter=600, check_every=200, gap_tol=1e30)
    assert s32.stats()["iterations"] == 200 and np.all(np.isfinite(s32.duality_gap()))
    s64.close(); s32.close()


def test_f32_sweep_and_alpha_zero(gpu_solver_cls, oracle):
    ub, f = synth_batch(3, 64, 48, seed=2)
    O, N, M = f.shape
    s = gpu_solver_cls(M, N, O, dtype=32)
    s.set_data(ub, f)
    u0 = s.denoise(0.0, maxiter=50)
    assert np.array_equal(u0, oracle.pdhg_f32(f, 0.0, maxiter=50)) and np.abs(u0 - f).max() < 1e-6   # alpha = 0: u = f
    alphas = [0.05, 0.1, 0.2]
    costs = s.sweep(alphas, maxiter=150)
    for a, c in zip(alphas, costs):
        u = oracle.pdhg_f32(f, a, maxiter=150)
        assert np.isclose(c, 0.5 * np.sum((u - ub) ** 2), rtol=1e-12)
    s.close()


def test_dtype_is_validated(gpu_solver_cls):
    from bpldenoising_amd import _lib
    with pytest.raises(_lib.BpltvError):
        gpu_solver_cls(8, 8, 1, dtype=16)


def test_f32_every_kernel_variant_and_fusion_depth_is_bit_identical(gpu_solver_cls, oracle):
    """The float instantiation of every kernel variant (register-tile waves 16-18 with the split float rsqrt, rows 19-29,
    rows2 30 / 31, the streaming pipeline 32 / 33, the 128-pixel rows 34-36 with the float fill shifts), every fusion depth,
    one and two launch chains, eager launches (V.launch32 with its own LDS size) and the hipGraph: the oracle's bits."""
    O, N, M = 2, 150, 140
    ub, f = synth_batch(O, N, M, seed=3)
    u0 = oracle.pdhg_f32(f, 0.08, maxiter=97)
    s = gpu_solver_cls(M, N, O, dtype=32)
    s.set_data(ub, f)
    for variant in range(1, 37):
        for T_ in (1, 2, 5, 8):
            for chains in (1, 2):
                for graph in (0, 1):
                    u = s.denoise(0.08, maxiter=97, variant=variant, tile_iters=T_, chains=chains, use_graph=graph)
                    assert np.array_equal(u, u0), (variant, T_, chains, graph, np.abs(u - u0).max())
                    assert s.stats()["pdhg_variant"] == variant
    s.close()


@pytest.mark.parametrize("shape", [(3, 70, 50), (1, 33, 31), (2, 128, 128), (1, 1, 1), (2, 5, 200), (1, 130, 40)])
@pytest.mark.parametrize("amode", ["scalar", "patch", "map"])
def test_f32_bit_exact_vs_oracle_shapes(gpu_solver_cls, oracle, shape, amode):
    O, N, M = shape
    ub, f = synth_batch(O, N, M, seed=40 + M)
    if amode == "scalar":
        alpha = 0.1
    elif amode == "patch":
        alpha = P22 if (M >= 2 and N >= 2) else np.array([[0.07]])
    else:
        alpha = 0.05 + 0.1 * np.random.default_rng(2).random((N, M))
    s = gpu_solver_cls(M, N, O, dtype=32)
    s.set_data(ub, f)
    for maxiter in (1, 7, 203):                       # not multiples of the fusion depth
        u = s.denoise(alpha, maxiter=maxiter)
        u0 = oracle.pdhg_f32(f, alpha, maxiter=maxiter)
        assert np.array_equal(u, u0), (maxiter, np.abs(u - u0).max())
    s.close()


@pytest.mark.parametrize("amode", ["scalar", "patch", "map"])
def test_f32_rows_kernels_alpha_modes_and_huber(gpu_solver_cls, oracle, amode):
    """The float row kernels (19-29), rows2's ping-pong (30 / 31, odd iteration count), the stream kernel (32 / 33) and the
    float fill shifts of the 128-pixel rows (34-36) on a shape that is no multiple of anything, every parameter form,
    with and without the Huber term.  Images narrower than a region are refused for dtype 32 as for dtype 64."""
    O, N, M = 2, 131, 203
    ub, f = synth_batch(O, N, M, seed=31)
    alpha = {"scalar": 0.09, "patch": np.array([[0.05, 0.12, 0.07], [0.2, 0.08, 0.1]]),
             "map": 0.03 + 0.15 * np.random.default_rng(6).random((N, M))}[amode]
    s = gpu_solver_cls(M, N, O, dtype=32)
    s.set_data(ub, f)
    for rho in (0.0, 0.3):
        u0 = oracle.pdhg_f32(f, alpha, maxiter=53, rho=rho)
        for variant, T_ in ((19, 8), (19, 3), (20, 8), (21, 8), (21, 11), (22, 8), (23, 8), (24, 8), (24, 5), (25, 8),
                            (26, 8), (27, 8), (28, 8), (29, 8), (30, 8), (30, 5), (31, 8), (31, 3), (32, 8), (32, 5),
                            (33, 8), (33, 3), (34, 8), (34, 3), (35, 8), (35, 5), (36, 8), (36, 11)):
            u = s.denoise(alpha, maxiter=53, rho=rho, variant=variant, tile_iters=T_)
            assert np.array_equal(u, u0), (amode, rho, variant, T_, np.abs(u - u0).max())
    s.close()
    s = gpu_solver_cls(60, 300, 1, dtype=32)
    s.set_data(*synth_batch(1, 300, 60, seed=2))
    with pytest.raises(RuntimeError, match="at least 64x64"):
        s.denoise(0.1, maxiter=8, variant=19)
    u = s.denoise(0.1, maxiter=8)                          # automatic plan: the 48x48 tile kernel
    assert s.stats()["region_i"] == 48
    s.close()


def test_f32_rho_and_no_accel(gpu_solver_cls, oracle):
    ub, f = synth_batch(2, 40, 36, seed=5)
    s = gpu_solver_cls(36, 40, 2, dtype=32)
    s.set_data(ub, f)
    for kw in (dict(rho=0.05), dict(accel=0), dict(rho=0.01, accel=0, tau0=3.0, sigma0=0.25)):
        u = s.denoise(0.1, maxiter=150, **kw)
        ok = dict(kw)
        if "accel" in ok:
            ok["accel"] = bool(ok["accel"])
        assert np.array_equal(u, oracle.pdhg_f32(f, 0.1, maxiter=150, **ok)), kw
    s.close()


def test_f32_launch_chains_out_of_phase(gpu_solver_cls, oracle):
    """12 x 128^2, an iteration count that is a multiple of T and >= 64 T: two launch chains, the second half a launch out
    of phase.  The same bits with one chain, with the default plan and with the XCD-aware tile order."""
    O, N, M = 12, 128, 128
    ub, f = synth_batch(O, N, M, seed=8)
    s = gpu_solver_cls(M, N, O, dtype=32)
    s.set_data(ub, f)
    maxiter, T_ = 512, 8
    u0 = oracle.pdhg_f32(f, 0.08, maxiter=maxiter)
    u2 = s.denoise(0.08, maxiter=maxiter, tile_iters=T_, chains=2)
    assert s.stats()["launches"] == 2 * (maxiter // T_) + 1, s.stats()
    assert np.array_equal(u2, u0)
    assert np.array_equal(s.denoise(0.08, maxiter=maxiter, tile_iters=T_, chains=1), u0)
    assert np.array_equal(s.denoise(0.08, maxiter=maxiter), u0)
    assert np.array_equal(s.denoise(0.08, maxiter=maxiter, xcd=True), u0)
    s.close()


def test_f32_full_size_matches_oracle_1024(gpu_solver_cls, oracle):
    """2 x 1024^2, a pixel map, 32 iterations: the automatic plan (rows), the 64x64 / 4 px tile, the 48x48 tile and the
    128-pixel rows against the oracle (single-threaded C: ~6.7e7 pixel-iterations)."""
    O, N, M = 2, 1024, 1024
    ub, f = synth_batch(O, N, M, seed=10)
    jj, ii = np.meshgrid(np.arange(N), np.arange(M), indexing="ij")
    amap = 0.11 + 0.09 * np.sin(2 * np.pi * ii / M) * np.cos(2 * np.pi * jj / N)
    u0 = oracle.pdhg_f32(f, amap, maxiter=32)
    s = gpu_solver_cls(M, N, O, dtype=32)
    s.set_data(ub, f)
    u = s.denoise(amap, maxiter=32)
    assert s.stats()["region_i"] == 64 and s.stats()["bytes_per_px_iter"] == 32.0
    assert np.array_equal(u, u0)
    for variant in (2, 13, 34):
        assert np.array_equal(s.denoise(amap, maxiter=32, variant=variant), u0), variant
    s.close()


def test_f32_chunked_solve_gap_and_early_stop(gpu_solver_cls, oracle):
    """The chunked solve widens the float state into the double buffers after every chunk (the gap kernels read it): the
    same bits as one sequence; the gap the library reports is the oracle's gap of the widened float state."""
    ub, f = synth_batch(3, 96, 80, seed=9)
    s = gpu_solver_cls(80, 96, 3, dtype=32)
    s.set_data(ub, f)
    u_plain = s.denoise(0.1, maxiter=600)
    u_chunk = s.denoise(0.1, maxiter=600, check_every=200, gap_tol=0)
    assert s.stats()["iterations"] == 600
    assert np.array_equal(u_chunk, u_plain)
    assert np.array_equal(u_plain, oracle.pdhg_f32(f, 0.1, maxiter=600))
    prev = None
    for it in (100, 400):
        u = s.denoise(0.1, maxiter=it)
        g = s.duality_gap()
        u0, y1, y2 = oracle.pdhg_f32(f, 0.1, maxiter=it, return_dual=True)
        assert np.array_equal(u, u0)
        assert np.allclose(g, oracle.gap(u0, y1, y2, f, 0.1), rtol=1e-6, atol=2e-9), it
        assert np.all(g >= -2e-9)
        if prev is not None:
            assert np.all(g < prev)
        prev = g
    u = s.denoise(0.1, maxiter=5000, check_every=100, gap_tol=float(prev.max()) * 1.0001)
    st = s.stats()
    assert st["iterations"] < 5000 and st["iterations"] % 100 == 0, st
    assert st["last_gap"] <= float(prev.max()) * 1.0001
    assert np.array_equal(u, oracle.pdhg_f32(f, 0.1, maxiter=st["iterations"]))
    s.close()


@pytest.mark.parametrize("alpha", [0.1, P22, "map"], ids=["scalar", "patch22", "map"])
def test_f32_evaluate_matches_oracle_on_the_same_u(gpu_solver_cls, oracle, alpha):
    """evaluate on an f32 handle: u is spec v2f's; the loss and the adjoint gradient (Float64, from the widened u) are the
    oracle's for that u, with the tolerances of the Float64 path (tests/test_gpu_evaluate.py)."""
    ub, f = synth_batch(3, 64, 48, seed=20)
    if isinstance(alpha, str):
        alpha = 0.05 + 0.1 * np.random.default_rng(3).random((64, 48))
    s = gpu_solver_cls(48, 64, 3, dtype=32)
    s.set_data(ub, f)
    u, cost, grad = s.evaluate(alpha, 0.1, maxiter=800)
    u0 = oracle.pdhg_f32(f, alpha, maxiter=800)
    assert np.array_equal(u, u0)
    assert np.isclose(cost, oracle.cost(u0, ub), rtol=1e-13)
    g0 = oracle.gradient(alpha, u0, ub)
    assert np.shape(grad) == np.shape(g0)
    assert np.allclose(grad, g0, rtol=1e-6, atol=1e-10), np.abs(np.asarray(grad) - g0).max()
    st = s.stats()
    assert st["reg_gradient_used"] == 0 and st["adjoint_residual"] <= 1e-8, st
    if np.size(alpha) < 48 * 64:
        rows = s.per_image()
        assert np.isclose(rows[:, 0].sum(), cost, rtol=1e-14)
        assert np.allclose(rows[:, 1:].sum(axis=0), np.ravel(grad), rtol=1e-12, atol=1e-15)
    u, cost, greg = s.evaluate(alpha, 1e-7, maxiter=800)      # Delta <= Delta_t: the gradient_reg branch
    assert s.stats()["reg_gradient_used"] == 1 and np.array_equal(u, u0)
    gr0 = oracle.gradient(alpha, u0, ub, reg=True)
    # a pixel map: the Float64 path's bound for it (test_gpu_evaluate.py, both adjoint factorisations).  Measured on this
    # case: max|greg - oracle| 3.1e-10 for the f32 handle, 2.5e-10 for a Float64 handle (|greg| up to 0.32): the float u
    # leaves the adjoint as well conditioned as the Float64 one; rtol 1e-8 fails on both.
    if np.ndim(gr0) == 2 and gr0.shape == (64, 48):
        assert np.allclose(greg, gr0, rtol=1e-6, atol=1e-8 * np.abs(gr0).max()), np.abs(greg - gr0).max()
    else:
        assert np.allclose(greg, gr0, rtol=1e-8, atol=1e-12)
    s.close()


def test_f32_sweep_with_parameter_matrices(gpu_solver_cls, oracle):
    """A sweep grows the float state for K problems per image: patch matrices, then pixel maps; costs and u against the
    oracle, and a plain solve on the same handle afterwards finds no stale graph or parameter."""
    O, N, M = 2, 64, 48
    ub, f = synth_batch(O, N, M, seed=21)
    s = gpu_solver_cls(M, N, O, dtype=32)
    s.set_data(ub, f)
    rng = np.random.default_rng(9)
    for alphas in (0.03 + 0.15 * rng.random((3, 2, 3)), 0.03 + 0.15 * rng.random((2, N, M))):
        costs = s.sweep(alphas, maxiter=150)
        costs_u, us = s.sweep(alphas, fetch_u=True, maxiter=150)
        assert np.array_equal(costs, costs_u)
        for k, a in enumerate(alphas):
            u0 = oracle.pdhg_f32(f, a, maxiter=150)
            assert np.isclose(costs[k], 0.5 * np.sum((u0 - ub) ** 2), rtol=1e-12), k
            assert np.array_equal(us[k], u0), k
    assert np.array_equal(s.denoise(P22, maxiter=77), oracle.pdhg_f32(f, P22, maxiter=77))
    s.close()


def _f32_single(gpu_solver_cls, ub, f, alpha, delta=0.1, **kw):
    O, N, M = f.shape
    s = gpu_solver_cls(M, N, O, dtype=32)
    s.set_data(ub, f)
    out = s.evaluate(alpha, delta, **kw)
    rows = s.per_image()
    u_d = s.denoise(alpha, maxiter=123)
    alphas = np.linspace(0.02, 0.2, 5)
    sw = s.sweep(alphas, fetch_u=True, maxiter=200)
    s.close()
    return out, rows, u_d, alphas, sw


@pytest.mark.parametrize("nshards", [2, 3])
@pytest.mark.parametrize("alpha", [0.1, P22], ids=["scalar", "patch22"])
def test_f32_shards_on_one_device_match_a_single_handle(gpu_solver_cls, alpha, nshards):
    """The handle bench.py --f32 --gpus N builds (bpltv_create_sharded with dtype 32), rehearsed with a repeated device:
    evaluate, denoise and sweep have the bits of one single-device f32 handle; deterministic totals too."""
    ub, f = synth_batch(5, 48, 40, seed=32)
    (u0, c0, g0), rows0, ud0, alphas, (cs0, us0) = _f32_single(gpu_solver_cls, ub, f, alpha, maxiter=400)
    s = gpu_solver_cls(40, 48, 5, devices=[0] * nshards, dtype=32)
    s.set_data(ub, f)
    u, c, g = s.evaluate(alpha, 0.1, maxiter=400, deterministic=1)
    st = s.stats()
    assert st["shards"] == nshards and st["collective"] == "host sum"
    assert np.array_equal(u, u0)
    assert c == c0 and np.array_equal(np.asarray(g), np.asarray(g0))
    assert np.array_equal(s.per_image(), rows0)
    u, c, g = s.evaluate(alpha, 0.1, maxiter=400)
    assert np.array_equal(u, u0)
    assert np.isclose(c, c0, rtol=1e-14) and np.allclose(g, g0, rtol=1e-12)
    assert np.array_equal(s.denoise(alpha, maxiter=123), ud0)
    s.set_option("sweep_split", 2)                       # replicas of the dataset: each problem on one device
    cs, us = s.sweep(alphas, fetch_u=True, maxiter=200)
    assert s.stats()["sweep_shards"] == nshards
    assert np.array_equal(us, us0) and np.array_equal(cs, cs0)
    s.set_option("sweep_split", 1)                       # image shards: host sum of the shards' partial costs
    cs, us = s.sweep(alphas, fetch_u=True, maxiter=200)
    assert s.stats()["sweep_shards"] == 0
    assert np.array_equal(us, us0) and np.allclose(cs, cs0, rtol=1e-14)
    s.close()


def test_f32_handle_keeps_float64_where_promised(gpu_solver_cls, oracle):
    """include/bpltv.h (bpltv_create): the sum-of-regularisers model stays Float64 on a dtype 32 handle, and maxiter = 0
    returns f itself (not f rounded to float)."""
    ub, f = synth_batch(2, 48, 40, seed=23)
    s = gpu_solver_cls(40, 48, 2, dtype=32)
    s.set_data(ub, f)
    a3 = np.array([0.03, 0.02, 0.05])
    assert np.array_equal(s.sumregs_denoise(a3, maxiter=120), oracle.sumregs_pdhg(f, a3, maxiter=120))
    assert np.array_equal(s.denoise(0.1, maxiter=0), f)
    assert np.array_equal(s.denoise(0.1, maxiter=40), oracle.pdhg_f32(f, 0.1, maxiter=40))   # and back to the float path
    s.close()


def test_f32_subnormal_parameter(gpu_solver_cls, oracle):
    """alpha = 8e-20 on data of ~1e-19: alpha^2 (6.4e-39) and most |y|^2 are float subnormals, so the projection test
    n2 > a*a compares subnormals.  The oracle keeps them (C float arithmetic); so must the kernels (float denormals on).
    Not smaller: spec v2f's rsqrt seed (0x5F375A86 - bits/2) is meant for normal floats, and its three Newton steps
    overflow for n2 below ~3e-39 (measured on the oracle: inf / NaN in u at alpha = 1e-20), so the float
    mode is defined for alpha >= ~5.5e-20."""
    ub, f = synth_batch(2, 64, 130, seed=24)
    f = f * 1e-19
    ub = ub * 1e-19
    a = 8e-20
    assert 0 < np.float32(a) * np.float32(a) < np.finfo(np.float32).tiny
    u0, y1, y2 = oracle.pdhg_f32(f, a, maxiter=60, return_dual=True)
    assert np.all(np.isfinite(u0))
    n2 = y1.astype(np.float32) ** 2 + y2.astype(np.float32) ** 2
    assert np.count_nonzero((n2 > 0) & (n2 < np.finfo(np.float32).tiny)) > 1000           # subnormal |y|^2
    nrm = np.sqrt(y1 ** 2 + y2 ** 2)
    assert nrm.max() > 0.999 * a and np.count_nonzero(nrm > 0.999 * a) > 1000            # the projection is active
    assert np.abs(u0 - f).max() > 1e-20                                                  # and u moved away from f
    s = gpu_solver_cls(130, 64, 2, dtype=32)
    s.set_data(ub, f)
    for variant in (0, 2, 13, 16, 19, 30, 32, 34):
        u = s.denoise(a, maxiter=60, variant=variant)
        assert np.array_equal(u, u0), (variant, np.abs(u - u0).max())
    s.close()
