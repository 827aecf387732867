"""The step rows of a launch of pdhg_tile_kernel come from LDS: threads tid < nit * TAB_STRIDE copy
the rows [it0, it0 + nit) of the step table into a static LDS array together with the state loads, and every iteration
reads its row from there instead of fetching it by scalar loads.  The values are the same words of the same table, so
every result stays BIT FOR BIT the oracle's: at every fusion depth (the depth is the number of rows a launch copies),
for launches shorter than the depth (the last launch of a sequence, the half-depth first launch of the second chain),
with one and two launch chains, both grid forms, a scalar parameter and a pixel map, in Float64 and Float32.  The array
holds PDHG_MAX_T = 32 rows: that depth runs, one more is refused."""
import numpy as np
import pytest
from conftest import synth_batch

pytestmark = pytest.mark.gpu

DEPTHS = tuple(range(2, 13))
MAX_T = 32   # PDHG_MAX_T of csrc/pdhg_kernels.hpp


@pytest.mark.parametrize("O", [1, 5, 10])
def test_128_batches_every_depth_bit_identical(gpu_solver_cls, oracle, O):
    """1, 5 and 10 images of 128 x 128, the default plan and depths 2 ... 12, at iteration counts that are no multiples
    of the depth: 1 (one launch of one row), 7, 203 and 4996 (default plan: long enough for the phase gate of two chains;
    a sequence whose second chain cannot run out of phase)."""
    N = M = 128
    ub, f = synth_batch(O, N, M, seed=80 + O)
    s = gpu_solver_cls(M, N, O)
    s.set_data(ub, f)
    for maxiter in (1, 7, 203, 4996):
        u0 = oracle.pdhg(f, 0.08, maxiter=maxiter, nthreads=8)
        u = s.denoise(0.08, maxiter=maxiter)
        st = s.stats()
        assert np.array_equal(u, u0), ("default plan", maxiter, st["pdhg_variant"], st["tile_iters"], st["launch_chains"])
        if maxiter == 4996:
            continue
        for T_ in DEPTHS:
            for chains in (1, 2) if O > 1 else (1,):
                u = s.denoise(0.08, maxiter=maxiter, tile_iters=T_, chains=chains)
                st = s.stats()
                assert st["pdhg_variant"] == 1 and st["tile_iters"] == T_ and st["launch_chains"] == chains, st
                assert np.array_equal(u, u0), (maxiter, T_, chains)
    s.close()


@pytest.mark.parametrize("shape", [(100, 70), (70, 100), (30, 100)])
@pytest.mark.parametrize("dtype", [64, 32])
@pytest.mark.parametrize("amode", ["scalar", "map"])
def test_non_square_borders_chains_and_dtypes_bit_identical(gpu_solver_cls, oracle, shape, dtype, amode):
    """(N, M), j over N: tiles with and without image borders, a last tile shifted back onto the image, one tile row
    (N = 30); iteration counts 203 and 7 (a short last launch at every depth; at 7 most depths give one short launch)."""
    N, M = shape
    O = 3
    ub, f = synth_batch(O, N, M, seed=17 + N)
    alpha = 0.09 if amode == "scalar" else 0.05 + 0.1 * np.random.default_rng(5).random((N, M))
    ref = oracle.pdhg if dtype == 64 else oracle.pdhg_f32
    s = gpu_solver_cls(M, N, O, dtype=dtype)
    s.set_data(ub, f)
    for maxiter in (203, 7, 1):
        u0 = ref(f, alpha, maxiter=maxiter)
        for chains in (1, 2):
            for T_ in (0,) + DEPTHS:      # 0: the planner's depth
                u = s.denoise(alpha, maxiter=maxiter, variant=1, tile_iters=T_, chains=chains)
                st = s.stats()
                assert st["pdhg_variant"] == 1 and st["launch_chains"] == chains, st
                assert np.array_equal(u, u0), (maxiter, chains, T_, st["tile_iters"])
    s.close()


@pytest.mark.parametrize("dtype", [64, 32])
def test_both_grid_forms_and_the_eager_path_bit_identical(gpu_solver_cls, oracle, dtype):
    """The tile kernels are compiled once per grid form.  The 1-D form runs with the XCD-aware tile order (xcd = 1); the
    eager launch path (use_graph = 0) picks its instantiation on its own."""
    O, N, M = 4, 100, 128
    ub, f = synth_batch(O, N, M, seed=3)
    ref = oracle.pdhg if dtype == 64 else oracle.pdhg_f32
    s = gpu_solver_cls(M, N, O, dtype=dtype)
    s.set_data(ub, f)
    u0 = ref(f, 0.08, maxiter=203)
    for variant in (1, 3, 4, 11):
        for graph in (1, 0):
            for xcd in (0, 1):
                u = s.denoise(0.08, maxiter=203, variant=variant, tile_iters=5, use_graph=graph, xcd=xcd)
                assert np.array_equal(u, u0), (variant, graph, xcd)
    s.close()


@pytest.mark.parametrize("dtype", [64, 32])
def test_deepest_launch_runs_and_one_more_is_refused(gpu_solver_cls, oracle, dtype):
    """An image that fits one region has no halo, so nothing but the LDS array of step rows caps the depth: 32 rows
    (one launch of 32 iterations, then a short one) run bit-exactly on every tile variant's thread count class; 33 is
    BPLTV_E_ARG and leaves the handle usable.  Images larger than a region: the deepest plan their halo allows."""
    from bpldenoising_amd._lib import BpltvError
    O, N, M = 2, 16, 16     # fits the smallest region (16 x 16, 256 threads: one thread per word of the 32 rows)
    ub, f = synth_batch(O, N, M, seed=9)
    ref = oracle.pdhg if dtype == 64 else oracle.pdhg_f32
    s = gpu_solver_cls(M, N, O, dtype=dtype)
    s.set_data(ub, f)
    u0 = ref(f, 0.1, maxiter=45)
    for variant in (1, 2, 3, 4, 12, 13):
        u = s.denoise(0.1, maxiter=45, variant=variant, tile_iters=MAX_T)
        st = s.stats()
        assert st["tile_iters"] == MAX_T and st["pdhg_variant"] == variant, st
        assert np.array_equal(u, u0), variant
        with pytest.raises(BpltvError) as e:
            s.denoise(0.1, maxiter=45, variant=variant, tile_iters=MAX_T + 1)
        assert e.value.code == 1 and "at most 32" in str(e.value), str(e.value)
        assert np.array_equal(s.denoise(0.1, maxiter=45, variant=variant, tile_iters=MAX_T), u0)
    s.close()
    # larger than the region: the halo caps the depth (tile_iters beyond it is clamped, as before)
    O, N, M = 2, 100, 128
    ub, f = synth_batch(O, N, M, seed=10)
    s = gpu_solver_cls(M, N, O, dtype=dtype)
    s.set_data(ub, f)
    u0 = ref(f, 0.1, maxiter=77)
    for variant, cap in ((1, 15), (2, 31), (3, 7)):
        u = s.denoise(0.1, maxiter=77, variant=variant, tile_iters=40)
        assert s.stats()["tile_iters"] == cap, s.stats()
        assert np.array_equal(u, u0), variant
    s.close()
