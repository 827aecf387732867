"""Spent halo waves of the 32x32 / 1 px PDHG kernel stop computing (pdhg_tile_kernel): a wave whose
pixel rows lie in the halo along j runs only the iterations somebody still reads and then keeps the barriers company.
What it no longer computes was never read, so every result stays BIT FOR BIT the oracle's -- at every fusion depth
(the depth sets which waves stop, and when), with one and two launch chains, on tiles with and without image borders
along j, for a scalar parameter and a pixel map, in Float64 and in the opt-in Float32 mode."""
import numpy as np
import pytest
from conftest import synth_batch

pytestmark = pytest.mark.gpu

DEPTHS = tuple(range(2, 13))


@pytest.mark.parametrize("O", [1, 5, 10])
def test_128_batches_every_depth_bit_identical(gpu_solver_cls, oracle, O):
    """1, 5 and 10 images of 128 x 128: the default plan (long enough for the phase gate of two chains: >= 64 launches)
    and explicit depths 2 ... 12, at an iteration count that is a multiple of most depths (the second chain then runs
    half a launch out of phase) and at one that is of none (a short last launch)."""
    N = M = 128
    ub, f = synth_batch(O, N, M, seed=60 + O)
    s = gpu_solver_cls(M, N, O)
    s.set_data(ub, f)
    for maxiter in (120, 97, 520):
        u0 = oracle.pdhg(f, 0.08, maxiter=maxiter, nthreads=8)
        u = s.denoise(0.08, maxiter=maxiter)
        st = s.stats()
        assert np.array_equal(u, u0), ("default plan", maxiter, st["pdhg_variant"], st["tile_iters"], st["launch_chains"])
        if maxiter == 520:
            continue
        for T_ in DEPTHS:
            u = s.denoise(0.08, maxiter=maxiter, tile_iters=T_)
            st = s.stats()
            assert st["pdhg_variant"] == 1 and st["tile_iters"] == T_, st
            assert np.array_equal(u, u0), (maxiter, T_, st["launch_chains"])
    s.close()


# (N, M): j runs over N.  100 and 70 are no multiples of a tile stride 32 - 2 T: the last tile is shifted back onto the
# image and overlaps its neighbour by more than the halo.  N = 100 / 70: tile rows with the near border, with none and
# with the far border along j; N = 30 <= 32: one tile row holding both borders (no halo along j at all).
@pytest.mark.parametrize("shape", [(100, 70), (70, 100), (30, 100)])
@pytest.mark.parametrize("dtype", [64, 32])
@pytest.mark.parametrize("amode", ["scalar", "map"])
def test_non_square_borders_chains_and_dtypes_bit_identical(gpu_solver_cls, oracle, shape, dtype, amode):
    N, M = shape
    O = 3
    ub, f = synth_batch(O, N, M, seed=7 + N)
    alpha = 0.09 if amode == "scalar" else 0.05 + 0.1 * np.random.default_rng(5).random((N, M))
    ref = oracle.pdhg if dtype == 64 else oracle.pdhg_f32
    s = gpu_solver_cls(M, N, O, dtype=dtype)
    s.set_data(ub, f)
    for maxiter in (96, 61):
        u0 = ref(f, alpha, maxiter=maxiter)
        for chains in (1, 2):
            for T_ in (0,) + DEPTHS:      # 0: the planner's depth
                u = s.denoise(alpha, maxiter=maxiter, variant=1, tile_iters=T_, chains=chains)
                st = s.stats()
                assert st["pdhg_variant"] == 1 and st["launch_chains"] == chains, st
                assert np.array_equal(u, u0), (maxiter, chains, T_, st["tile_iters"])
    s.close()
