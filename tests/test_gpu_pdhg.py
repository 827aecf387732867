"""GPU parity of the PDHG hot path (through the C ABI) against the oracle.

Stated bar: Float64; the HIP kernels reproduce the oracle's "spec v2" arithmetic BIT FOR BIT at equal
iteration count (tolerance SURVEY.md asks for: max|du| <= 1e-9).  Size-independent properties at
BASELINE's full sizes: results are bitwise independent of tiling / fusion depth / launch chains,
duality gap >= 0 and decreasing, closed-form limits.
"""
import zlib
import numpy as np
import pytest
from oracle import np_twin as T
from conftest import DATASETS_NPZ, synth_batch

pytestmark = pytest.mark.gpu

P22 = np.array([[0.05, 0.1], [0.2, 0.08]])


@pytest.mark.parametrize("shape", [(3, 70, 50), (1, 33, 31), (2, 128, 128), (1, 1, 1), (2, 5, 200), (1, 130, 40)])
@pytest.mark.parametrize("amode", ["scalar", "patch", "map"])
def test_bit_exact_vs_oracle(gpu_solver_cls, oracle, shape, amode):
    O, N, M = shape
    ub, f = synth_batch(O, N, M, seed=40 + M)
    if amode == "scalar":
        alpha = 0.1
    elif amode == "patch":
        alpha = P22 if (M >= 2 and N >= 2) else np.array([[0.07]])
    else:
        alpha = 0.05 + 0.1 * np.random.default_rng(2).random((N, M))
    s = gpu_solver_cls(M, N, O)
    s.set_data(ub, f)
    for maxiter in (1, 7, 203):                       # not multiples of the fusion depth
        u = s.denoise(alpha, maxiter=maxiter)
        u0 = oracle.pdhg(f, alpha, maxiter=maxiter)
        assert np.abs(u - u0).max() <= 1e-9           # the stated tolerance
        assert np.array_equal(u, u0)                  # and in fact bit exact
    s.close()


def test_every_kernel_variant_and_fusion_depth_is_bit_identical(gpu_solver_cls, oracle):
    O, N, M = 2, 150, 140
    ub, f = synth_batch(O, N, M, seed=3)
    u0 = oracle.pdhg(f, 0.08, maxiter=97)
    s = gpu_solver_cls(M, N, O)
    s.set_data(ub, f)
    for variant in range(1, 37):
        for T_ in (1, 2, 5, 8):
            for chains in (1, 2):
                for graph in (0, 1):
                    u = s.denoise(0.08, maxiter=97, variant=variant, tile_iters=T_, chains=chains, use_graph=graph)
                    assert np.array_equal(u, u0), (variant, T_, chains, graph)
    s.close()


def test_launch_chains_out_of_phase_are_bit_identical(gpu_solver_cls, oracle):
    """Two launch chains (image groups on two streams), the second half a launch out of phase: its first launch fuses
    T/2 iterations and writes the other state set (only when that leaves every chain in the same set: iteration counts
    that are multiples of T, e.g. the reference's 5000).  Same bits as one chain and as the oracle; explicit and default
    (a batch beyond 1.5 workgroups per CU), the tile and the rows kernel, also for the sum of regularisers."""
    O, N, M = 12, 128, 128
    ub, f = synth_batch(O, N, M, seed=8)
    s = gpu_solver_cls(M, N, O)
    s.set_data(ub, f)
    for maxiter, T_ in ((96, 8), (200, 8), (120, 6), (97, 8)):
        u0 = oracle.pdhg(f, 0.08, maxiter=maxiter, nthreads=8)
        for chains in (0, 1, 2):
            u = s.denoise(0.08, maxiter=maxiter, tile_iters=T_, chains=chains)
            st = s.stats()
            assert np.array_equal(u, u0), (maxiter, T_, chains)
            nl = -(-maxiter // T_)
            if chains != 1:
                assert st["launches"] in (2 * nl, 2 * nl + 1), st       # two chains; + 1 launch when out of phase
                assert (st["launches"] == 2 * nl + 1) == (maxiter % T_ == 0)
    for init, order in ((1, 0), (0, 1), (1, 1)):      # prepared starts: two chains in phase (they begin in state set 1)
        u = s.denoise(0.08, maxiter=96, tile_iters=8, init=init, order=order)
        assert np.array_equal(u, oracle.pdhg_opts(f, 0.08, maxiter=96, init=init, order=order)), (init, order)
    a3 = np.array([0.03, 0.02, 0.05])
    us = s.sumregs_denoise(a3, maxiter=96, variant=1)                 # 588 tiles of 32 x 32: two chains
    assert s.stats()["launches"] == 2 * 24 + 1
    assert np.array_equal(us, s.sumregs_denoise(a3, maxiter=96, variant=1, chains=1))
    s.close()
    O, N, M = 6, 300, 260                     # rows kernel, 2 x 150 tiles
    ub, f = synth_batch(O, N, M, seed=9)
    s = gpu_solver_cls(M, N, O)
    s.set_data(ub, f)
    u1 = s.denoise(0.1, maxiter=64, chains=1)
    u2 = s.denoise(0.1, maxiter=64, chains=2)
    assert s.stats()["pdhg_variant"] in (19, 20) and s.stats()["launches"] == 2 * 8 + 1
    assert np.array_equal(u1, u2) and np.array_equal(u1, oracle.pdhg(f, 0.1, maxiter=64, nthreads=8))
    s.close()


@pytest.mark.parametrize("ds,lo,hi,alpha,maxiter,name", [
    ("faces_train_128_10", 0, 10, 0.07, 5000, "faces_train_scalar"),
    ("cameraman_128_10", 0, 1, P22 * 0 + np.array([[0.08, 0.12], [0.1, 0.05]]), 5000, "cameraman10_patch22"),
    ("cameraman_128_5", 0, 1, 0.05, 10000, "cameraman5_scalar_tvdenoise"),
    ("circle_128_10", 0, 1, 0.1, 5000, "circle_scalar"),
])
def test_reference_datasets_match_golden(gpu_solver_cls, golden, ds, lo, hi, alpha, maxiter, name):
    """BASELINE configs 1-4 on the reference's own images: u bit-identical to the golden vectors."""
    z, meta = golden
    ub, f = T.load_dataset(DATASETS_NPZ, ds)
    ub, f = ub[lo:hi], f[lo:hi]
    s = gpu_solver_cls(128, 128, hi - lo)
    s.set_data(ub, f)
    u = s.denoise(alpha, maxiter=maxiter)
    assert zlib.crc32(np.ascontiguousarray(u).tobytes()) == int(z[name + "/u_crc32"])
    if name + "/u" in z:
        assert np.array_equal(u, z[name + "/u"])
    gap = s.duality_gap()
    # the gap is a difference of energies of size ~1e2: different summation orders -> ~1e-10 absolute
    assert np.allclose(gap, z[name + "/gap"], rtol=1e-6, atol=2e-9)
    assert s.stats()["iterations"] == maxiter
    s.close()


def test_rho_and_no_accel(gpu_solver_cls, oracle):
    ub, f = synth_batch(2, 40, 36, seed=5)
    s = gpu_solver_cls(36, 40, 2)
    s.set_data(ub, f)
    for kw in (dict(rho=0.05), dict(accel=0), dict(rho=0.01, accel=0, tau0=3.0, sigma0=0.25)):
        u = s.denoise(0.1, maxiter=150, **kw)
        ok = dict(kw)
        if "accel" in ok:
            ok["accel"] = bool(ok["accel"])
        assert np.array_equal(u, oracle.pdhg(f, 0.1, maxiter=150, **ok)), kw
    s.close()


def test_closed_form_cases(gpu_solver_cls):
    ub, f = synth_batch(2, 64, 64, seed=6)
    s = gpu_solver_cls(64, 64, 2)
    s.set_data(ub, f)
    assert np.abs(s.denoise(0.0, maxiter=64) - f).max() < 1e-15        # alpha = 0 => u = f
    assert np.array_equal(s.denoise(0.1, maxiter=0), f)                # maxiter = 0
    c = np.full((2, 64, 64), 0.37)
    s.set_data(c, c)
    assert np.abs(s.denoise(0.2, maxiter=300) - c).max() < 1e-15       # constant f => u = f
    s.close()
    ub, f = synth_batch(1, 16, 16, seed=7)
    s = gpu_solver_cls(16, 16, 1)
    s.set_data(ub, f)
    assert np.abs(s.denoise(50.0, maxiter=4000) - f.mean()).max() < 1e-6   # alpha large => mean(f)
    s.close()


def test_transposition_equivariance(gpu_solver_cls):
    ub, f = synth_batch(1, 96, 80, seed=8)
    s = gpu_solver_cls(80, 96, 1)
    s.set_data(ub, f)
    u = s.denoise(0.1, maxiter=300)
    s.close()
    ft = np.ascontiguousarray(f.transpose(0, 2, 1))
    s = gpu_solver_cls(96, 80, 1)
    s.set_data(ft, ft)
    ut = s.denoise(0.1, maxiter=300)
    s.close()
    assert np.abs(u - ut.transpose(0, 2, 1)).max() < 1e-12


def test_gap_certificate_and_early_stop(gpu_solver_cls, oracle):
    ub, f = synth_batch(4, 128, 128, seed=9)
    s = gpu_solver_cls(128, 128, 4)
    s.set_data(ub, f)
    prev = None
    for it in (100, 400, 1600):
        u = s.denoise(0.1, maxiter=it)
        g = s.duality_gap()
        u0, y1, y2 = oracle.pdhg(f, 0.1, maxiter=it, return_dual=True, nthreads=4)
        assert np.allclose(g, oracle.gap(u0, y1, y2, f, 0.1), rtol=1e-6, atol=2e-9)
        assert np.all(g >= -2e-9)
        if prev is not None:
            assert np.all(g < prev)
        prev = g
    # early stop on the gap: stops at a multiple of check_every, well before maxiter
    u = s.denoise(0.1, maxiter=5000, check_every=100, gap_tol=float(prev.max()) * 1.0001)
    st = s.stats()
    assert st["iterations"] <= 1600 and st["iterations"] % 100 == 0
    assert st["last_gap"] <= float(prev.max()) * 1.0001
    assert np.array_equal(u, oracle.pdhg(f, 0.1, maxiter=st["iterations"], nthreads=4))
    s.close()


def test_full_size_properties_1024(gpu_solver_cls):
    """BASELINE config 5 shape (per-GPU share: 8 x 1024 x 1024, spatially varying alpha): properties
    that need no oracle run -- tiling/fusion independence, gap >= 0 and decreasing, alpha = 0."""
    O, N, M = 8, 1024, 1024
    ub, f = synth_batch(O, N, M, seed=10)
    jj, ii = np.meshgrid(np.arange(N), np.arange(M), indexing="ij")
    amap = 0.11 + 0.09 * np.sin(2 * np.pi * ii / M) * np.cos(2 * np.pi * jj / N)
    s = gpu_solver_cls(M, N, O)
    s.set_data(ub, f)
    u_a = s.denoise(amap, maxiter=64, variant=2, tile_iters=8)
    g64 = s.duality_gap()
    assert s.stats()["bytes_per_px_iter"] == 64.0
    u_b = s.denoise(amap, maxiter=64, variant=1, tile_iters=4)
    u_c = s.denoise(amap, maxiter=64, variant=6, tile_iters=3, use_graph=0)
    u_d = s.denoise(amap, maxiter=64)                      # automatic plan: 64-lane rows, 64x64 regions (variant 19)
    st = s.stats()
    assert (st["region_i"], st["region_j"], st["tile_iters"], st["tiles"]) == (64, 64, 8, 8 * 21 * 21)
    u_e = s.denoise(amap, maxiter=64, variant=13)          # the 48x48 tile kernel
    assert s.stats()["tiles"] == 8 * 32 * 32
    assert np.array_equal(u_a, u_b) and np.array_equal(u_a, u_c) and np.array_equal(u_a, u_d) and np.array_equal(u_a, u_e)
    s.denoise(amap, maxiter=256, fetch=False)
    g256 = s.duality_gap()
    assert np.all(g64 >= 0) and np.all(g256 >= 0) and np.all(g256 < g64)
    assert np.abs(s.denoise(0.0, maxiter=16) - f).max() < 1e-15
    s.close()


def test_full_size_matches_oracle_1024(gpu_solver_cls, oracle):
    """BASELINE config 5 at full image size against the C oracle: 2 x 1024 x 1024, the spatially varying alpha
    of SURVEY 8(d), 32 iterations (the oracle does this in well under a second on the host).  Bit-exact for
    the automatic plan (64-lane rows, 64x64 regions, variant 19), the 48x48 tile kernel and the 64x64 / 4 px variant."""
    O, N, M = 2, 1024, 1024
    ub, f = synth_batch(O, N, M, seed=10)
    jj, ii = np.meshgrid(np.arange(N), np.arange(M), indexing="ij")
    amap = 0.11 + 0.09 * np.sin(2 * np.pi * ii / M) * np.cos(2 * np.pi * jj / N)
    u0 = oracle.pdhg(f, amap, maxiter=32, nthreads=8)
    s = gpu_solver_cls(M, N, O)
    s.set_data(ub, f)
    u_auto = s.denoise(amap, maxiter=32)
    st = s.stats()
    assert st["tiles"] == O * 21 * 21 and st["region_i"] == 64 and st["bytes_per_px_iter"] == 64.0     # 64x64 regions, T = 8
    assert np.array_equal(u_auto, u0)
    assert np.array_equal(s.denoise(amap, maxiter=32, variant=2), u0)
    assert np.array_equal(s.denoise(amap, maxiter=32, variant=13), u0)
    assert np.array_equal(s.denoise(0.1, maxiter=32), oracle.pdhg(f, 0.1, maxiter=32, nthreads=8))   # scalar alpha
    s.close()


@pytest.mark.parametrize("amode", ["scalar", "patch", "map"])
def test_rows_kernel_alpha_modes_and_huber(gpu_solver_cls, oracle, amode):
    """pdhg_rows_kernel (64-lane rows, i-neighbours by lane shifts, j-strips in registers, halo rows that stop early) on a
    shape that is no multiple of anything, every parameter form, with and without the Huber term, several fusion depths
    and region heights, f and alpha in registers or in LDS, and the re-cut with several dual chains in flight
    (pdhg_rows2_kernel, variants 30 / 31; an odd iteration count exercises its ping-pong of x), and the streaming pipeline of
    waves (pdhg_stream_kernel, variants 32 / 33: one wave per fused iteration, LDS rings, no workgroup barrier), and the rows of
    128 pixels (pdhg_rowsw_kernel, variants 34 / 35 / 36: two waves side by side that exchange one column per step): bit-exact
    against the oracle.  Images narrower than a region
    are refused for these variants (the automatic plan then keeps the tile kernel)."""
    O, N, M = 2, 131, 203
    ub, f = synth_batch(O, N, M, seed=31)
    alpha = {"scalar": 0.09, "patch": np.array([[0.05, 0.12, 0.07], [0.2, 0.08, 0.1]]),
             "map": 0.03 + 0.15 * np.random.default_rng(6).random((N, M))}[amode]
    s = gpu_solver_cls(M, N, O)
    s.set_data(ub, f)
    for rho in (0.0, 0.3):
        u0 = oracle.pdhg(f, alpha, maxiter=53, rho=rho, nthreads=4)
        for variant, T_ in ((19, 8), (19, 3), (20, 8), (21, 8), (21, 11), (24, 8), (24, 5), (29, 8), (30, 8), (30, 5), (31, 8), (31, 3), (32, 8), (32, 5), (33, 8), (33, 3),
                            (34, 8), (34, 3), (35, 8), (35, 5), (36, 8), (36, 11)):
            u = s.denoise(alpha, maxiter=53, rho=rho, variant=variant, tile_iters=T_)
            assert np.array_equal(u, u0), (amode, rho, variant, T_)
    s.close()
    s = gpu_solver_cls(60, 300, 1)
    ub, f = synth_batch(1, 300, 60, seed=2)
    s.set_data(ub, f)
    with pytest.raises(RuntimeError, match="at least 64x64"):
        s.denoise(0.1, maxiter=8, variant=19)
    u = s.denoise(0.1, maxiter=8)                          # automatic plan: the 48x48 tile kernel
    assert s.stats()["region_i"] == 48
    assert np.array_equal(u, oracle.pdhg(f, 0.1, maxiter=8))
    s.close()


def test_operators_match_oracle(gpu_solver_cls, oracle):
    rng = np.random.default_rng(11)
    N, M = 37, 29
    s = gpu_solver_cls(M, N, 1)
    x = rng.standard_normal((N, M)); y1 = rng.standard_normal((N, M)); y2 = rng.standard_normal((N, M))
    d1, d2 = s.grad_fwd(x)
    o1, o2 = oracle.grad_fwd(x)
    assert np.array_equal(d1, o1) and np.array_equal(d2, o2)
    gt = s.grad_fwd_adjoint(y1, y2)
    assert np.array_equal(gt, oracle.grad_fwd_T(y1, y2))
    assert abs(np.sum(d1 * y1 + d2 * y2) - np.sum(x * gt)) < 1e-11       # <Gx, y> = <x, G^T y>
    s.close()


@pytest.mark.parametrize("init,order,L", [(1, 0, None), (0, 1, None), (1, 1, None), (0, 0, 2 * np.sqrt(2) * (1 - 1 / 64)),
                                          (1, 1, 2.5)])
@pytest.mark.parametrize("amode", ["scalar", "map"])
def test_run_time_choices_of_the_unpinned_recurrence_are_bit_exact(gpu_solver_cls, oracle, init, order, L, amode):
    """bpltv_params.init / order / opnorm (x0 = 0, dual step first, another operator-norm estimate: what
    op_denoise_pdps may do differently, /root/reference/src/TVLearningFunctionVec.jl:33-43,52) against the oracle's
    bplo_pdhg_opts -- same arithmetic, bit for bit, eager and from the hipGraph, with and without gap checks."""
    O, N, M = 3, 70, 64
    ub, f = synth_batch(O, N, M, seed=11)
    alpha = 0.09 if amode == "scalar" else 0.05 + 0.1 * np.random.default_rng(4).random((N, M))
    s = gpu_solver_cls(M, N, O)
    s.set_data(ub, f)
    kw = dict(init=init, order=order)
    if L is not None:
        kw["opnorm"] = L
    for maxiter in (0, 1, 2, 9, 150):
        u0, y10, y20 = oracle.pdhg_opts(f, alpha, maxiter=maxiter, init=init, order=order, L=L, return_dual=True)
        for graph in (1, 0):
            u = s.denoise(alpha, maxiter=maxiter, use_graph=graph, **kw)
            assert np.array_equal(u, u0), (maxiter, graph)
        if maxiter:
            # the dual the library holds is the oracle's too: same duality gap
            g = s.duality_gap()
            assert np.allclose(g, oracle.gap(u0, y10, y20, f, alpha), rtol=1e-6, atol=2e-9)
    u = s.denoise(alpha, maxiter=150, check_every=40, **kw)       # chunked launch sequence with gap checks
    assert np.array_equal(u, oracle.pdhg_opts(f, alpha, maxiter=150, init=init, order=order, L=L))
    # defaults restored: the restatement every parity claim refers to
    assert np.array_equal(s.denoise(alpha, maxiter=9), oracle.pdhg(f, alpha, maxiter=9))
    s.close()


def test_run_time_choices_and_gap_checks_on_a_large_image(gpu_solver_cls, oracle):
    """The same switches, the chunked launch sequence with duality-gap checks and a parameter sweep on an image above
    256 px, where the automatic plan is pdhg_rows_kernel (starts from a prepared state, several problems per image)."""
    O, N, M = 2, 290, 270
    ub, f = synth_batch(O, N, M, seed=12)
    alpha = 0.05 + 0.1 * np.random.default_rng(4).random((N, M))
    s = gpu_solver_cls(M, N, O)
    s.set_data(ub, f)
    for init, order in ((1, 0), (0, 1), (1, 1)):
        for maxiter in (1, 9, 70):
            u = s.denoise(alpha, maxiter=maxiter, init=init, order=order)
            assert s.stats()["region_i"] == 64 and s.stats()["pdhg_variant"] in (19, 20)
            assert np.array_equal(u, oracle.pdhg_opts(f, alpha, maxiter=maxiter, init=init, order=order)), (init, order, maxiter)
    u = s.denoise(alpha, maxiter=70, check_every=24)
    assert np.array_equal(u, oracle.pdhg(f, alpha, maxiter=70, nthreads=4))
    alphas = [0.03, 0.08, 0.2]
    costs, us = s.sweep(alphas, fetch_u=True, maxiter=40)
    for k, a in enumerate(alphas):
        u0 = oracle.pdhg(f, a, maxiter=40, nthreads=4)
        assert np.array_equal(us[k], u0) and np.isclose(costs[k], oracle.cost(u0, ub), rtol=1e-12), a
    s.close()


def test_prepared_start_with_two_threaded_launch_chains_1024(gpu_solver_cls, oracle):
    """A prepared start (params.init / order) on a batch that runs as TWO launch chains with >= 128 launches each, so that
    chain 1 is launched from the handle's launcher thread while pdhg_init_kernel may still be running on the handle's
    stream: the chains fork behind the init kernel (fork event), not behind the timing event in front of it.
    2 x 1024^2, pixel map, 1040 iterations = 130 launches at T = 8; chain 1 owns the image the init kernel writes last."""
    O, N, M = 2, 1024, 1024
    ub, f = synth_batch(O, N, M, seed=31)
    jj, ii = np.meshgrid(np.arange(N), np.arange(M), indexing="ij")
    alpha = 0.11 + 0.09 * np.sin(2 * np.pi * ii / M) * np.cos(2 * np.pi * jj / N)
    s = gpu_solver_cls(M, N, O)
    s.set_data(ub, f)
    u = s.denoise(alpha, maxiter=1040, init=1, order=1, chains=2)
    st = s.stats()
    assert st["graph_used"] == 1 and st["launches"] >= 2 * 128, st
    assert np.array_equal(u, oracle.pdhg_opts(f, alpha, maxiter=1040, init=1, order=1))
    s.close()


def test_run_time_choices_are_rejected_where_unsupported(gpu_solver_cls):
    from bpldenoising_amd._lib import BpltvError
    ub, f = synth_batch(1, 32, 32, seed=2)
    s = gpu_solver_cls(32, 32, 1, dtype=32)
    s.set_data(ub, f)
    with pytest.raises(BpltvError) as e:
        s.denoise(0.1, maxiter=5, order=1)
    assert e.value.code == 6
    s.close()
    s = gpu_solver_cls(32, 32, 1)
    s.set_data(ub, f)
    for bad in (dict(init=2), dict(order=-1), dict(opnorm=-1.0)):
        with pytest.raises(BpltvError) as e:
            s.denoise(0.1, maxiter=5, **bad)
        assert e.value.code == 1
    with pytest.raises(BpltvError) as e:
        s.sumregs_denoise(np.array([0.03, 0.02, 0.05]), maxiter=5, init=1)
    assert e.value.code == 6
    s.close()


def test_a_second_handle_runs_at_the_speed_of_the_first(gpu_solver_cls):
    """The reference's workflow keeps a training set and a validation set (src/BPLDenoising.jl:316-336, :113-131): two
    handles alive in one process.  The handles of a device share its main stream and chain streams (csrc/bpltv.hip,
    DeviceStreams): with a stream pair per handle the second handle's two launch chains could land on one hardware queue
    and run one after the other (measured before the change: 5.8 -> 11.1 ms for the reference batch).  Same bits, and
    the second handle's solve is not slower than 1.5 x the first's."""
    O, N, M = 10, 128, 128
    ub, f = synth_batch(O, N, M, seed=77)
    a = gpu_solver_cls(M, N, O)
    a.set_data(ub, f)
    for _ in range(2):
        ua = a.denoise(0.1, maxiter=5000)
    ta = min(a.stats()["pdhg_ms"] for _ in range(1))
    b = gpu_solver_cls(M, N, O)              # created while `a` is alive and has run
    b.set_data(ub, f)
    tb = []
    for _ in range(3):
        ubb = b.denoise(0.1, maxiter=5000)
        tb.append(b.stats()["pdhg_ms"])
    assert np.array_equal(ua, ubb)
    assert a.stats()["launch_chains"] == 2 and b.stats()["launch_chains"] == 2
    assert min(tb) < 1.5 * ta, (ta, tb)
    c = gpu_solver_cls(M, N, O)              # and a third one; `a` goes away first: the shared streams stay
    c.set_data(ub, f)
    a.close()
    assert np.array_equal(c.denoise(0.1, maxiter=5000), ubb) and c.stats()["pdhg_ms"] < 1.5 * ta
    b.close()
    assert np.array_equal(c.denoise(0.1, maxiter=300), c.denoise(0.1, maxiter=300))
    c.close()


def test_parameter_resident_in_hbm_and_handle_options(gpu_solver_cls):
    """bpltv_denoise_device: the parameter map handed over as a device pointer (checked on the device: finite, >= 0), the
    result left in HBM -- the same bits as bpltv_denoise from host arrays.  bpltv_set_option: unknown names and bad
    values are BPLTV_E_ARG."""
    import torch
    from bpldenoising_amd._lib import BpltvError
    O, N, M = 2, 96, 80
    ub, f = synth_batch(O, N, M, seed=51)
    amap = 0.03 + 0.15 * np.random.default_rng(7).random((N, M))
    s = gpu_solver_cls(M, N, O)
    s.set_data(ub, f)
    u0 = s.denoise(amap, maxiter=77)
    t_a = torch.from_numpy(amap).cuda()
    out = torch.empty(O * N * M, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    s.denoise_device(t_a.data_ptr(), M, N, maxiter=77)
    s.copy_u_device(out.data_ptr())
    assert np.array_equal(out.cpu().numpy().reshape(O, N, M), u0)
    t_s = torch.tensor([0.09], dtype=torch.float64, device="cuda")          # a scalar parameter the same way
    s.denoise_device(t_s.data_ptr(), 1, 1, maxiter=40)
    s.copy_u_device(out.data_ptr())
    assert np.array_equal(out.cpu().numpy().reshape(O, N, M), s.denoise(0.09, maxiter=40))
    for bad in (-0.1, float("nan"), float("inf")):
        t_b = t_a.clone(); t_b[3, 5] = bad
        torch.cuda.synchronize()
        with pytest.raises(BpltvError) as e:
            s.denoise_device(t_b.data_ptr(), M, N, maxiter=5)
        assert e.value.code == 1 and "finite" in str(e.value)
    for name, val in (("no_such_option", 1), ("hb_sync", 7), ("hb_rw", 64), ("adjoint_budget_mb", -1), ("nd_leaf", 99999)):
        with pytest.raises(BpltvError) as e:
            s.set_option(name, val)
        assert e.value.code == 1, name
    s.set_option("nd_leaf", 16)                                              # another elimination tree, the same gradient
    _, _, g16 = s.evaluate(0.1, 0.1, maxiter=150)
    s.set_option("nd_leaf", 0)
    _, _, g32 = s.evaluate(0.1, 0.1, maxiter=150)
    assert np.isclose(g16, g32, rtol=1e-7)
    s.set_option("nd_wave", 0)                                               # small fronts by the workgroup-per-front kernel
    _, _, gwg = s.evaluate(0.1, 0.1, maxiter=150)
    s.set_option("nd_wave", 1)
    assert np.isclose(gwg, g32, rtol=1e-9) and s.evaluate(0.1, 0.1, maxiter=150)[2] == g32
    s.set_option("nd_staged", 0)                                             # column-loop substitutions: the same bits
    assert s.evaluate(0.1, 0.1, maxiter=150)[2] == g32
    s.set_option("nd_staged", 1)
    s.set_option("nd_skinny", 0)                                             # skinny fronts by the older kernels
    _, _, gsk = s.evaluate(0.1, 0.1, maxiter=150)
    s.set_option("nd_skinny", 1)
    assert np.isclose(gsk, g32, rtol=1e-9) and s.evaluate(0.1, 0.1, maxiter=150)[2] == g32
    s.close()



@pytest.mark.parametrize("dtype", [64, 32])
@pytest.mark.parametrize("first", ["scalar", "map"])
@pytest.mark.parametrize("bad", ["nan", "negative"])
def test_rejected_device_parameter_leaves_the_handle_as_it_was(gpu_solver_cls, dtype, first, bad):
    """bpltv_denoise_device checks the caller's array before anything of the handle changes: after a rejected parameter
    (one NaN or one negative entry; BPLTV_E_ARG) the resident parameter, its shape and minimum are those of the last
    solve, so duality_gap() -- which reads them -- returns the same bits.  A scalar first (the map would reallocate the
    parameter buffer) and a device map first (same shape: the copy would overwrite it in place)."""
    import torch
    from bpldenoising_amd._lib import BpltvError
    O, N, M = 2, 70, 64
    ub, f = synth_batch(O, N, M, seed=52)
    amap = 0.03 + 0.15 * np.random.default_rng(8).random((N, M))
    s = gpu_solver_cls(M, N, O, dtype=dtype)
    s.set_data(ub, f)
    t_a = torch.from_numpy(amap).cuda()
    if first == "scalar":
        s.denoise(0.1, maxiter=60, fetch=False)
    else:
        torch.cuda.synchronize()
        s.denoise_device(t_a.data_ptr(), M, N, maxiter=60)
    g0 = s.duality_gap()
    assert np.all(np.isfinite(g0)) and np.all(g0 > 0)
    t_b = t_a.clone()
    t_b[0, 0] = float("nan") if bad == "nan" else -0.25    # the entry a scalar parameter would be read from
    t_b[7, 9] = float("nan") if bad == "nan" else -0.5
    torch.cuda.synchronize()
    with pytest.raises(BpltvError) as e:
        s.denoise_device(t_b.data_ptr(), M, N, maxiter=5)
    assert e.value.code == 1 and "finite" in str(e.value)
    g1 = s.duality_gap()
    assert np.array_equal(g1, g0), (g0, g1)
    assert s.stats()["iterations"] == 60
    # and the handle still solves: the accepted map after the rejected one
    torch.cuda.synchronize()
    s.denoise_device(t_a.data_ptr(), M, N, maxiter=60)
    u = torch.empty(O * N * M, dtype=torch.float64, device="cuda")
    s.copy_u_device(u.data_ptr())
    assert np.array_equal(u.cpu().numpy().reshape(O, N, M), s.denoise(amap, maxiter=60))
    s.close()
