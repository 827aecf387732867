"""The prologue and the tail of pdhg_tile_kernel ("One argument round trip"): every argument word
is fetched in the entry block, the launch-invariant arithmetic (M * N, the first image's offset, R - 2T, the form of
alpha, sweep or not) arrives as argument words from the host, the common solve (no sweep, rho = 0, scalar or full-map
alpha) runs an instantiation of its own with 32-bit indices and no branch in front of its loads (in a first launch it
issues the state loads too, from the set the launch does not write), and the last fused iteration of a launch of the
1 px kernels skips the LDS write of y and barrier #2 and stores x behind its primal step.  None of this touches the arithmetic: every
result stays BIT FOR BIT the oracle's, on every tiling path (one tile, tiles in one dimension only, interior tiles, a
last tile pulled back), at every fusion depth and for launches shorter than it, for every form of alpha, with rho, in
f64 and f32, one and two chains, both grid forms, graph and eager launches, a prepared start -- and a cached graph never
carries another handle's launch-invariant words."""
import numpy as np
import pytest
from conftest import synth_batch

pytestmark = pytest.mark.gpu

# (M, N): inside one 32 x 32 region; larger in one dimension only; two tiles per dimension; three (an interior tile);
# a last tile that is pulled back onto the image in both dimensions
SHAPES = [(20, 20), (40, 20), (20, 40), (40, 40), (60, 60), (50, 37)]
DEPTHS = (1, 2, 8, 0)      # 0: the planner's depth
ITERS = (1, 7, 203)        # the last launch is shorter than the depth; nit = 1 runs the peeled tail alone


def _ref(oracle, dtype):
    return oracle.pdhg if dtype == 64 else oracle.pdhg_f32


@pytest.mark.parametrize("shape", SHAPES)
def test_tiling_paths_depths_and_short_launches_bit_identical(gpu_solver_cls, oracle, shape):
    M, N = shape
    O = 3
    ub, f = synth_batch(O, N, M, seed=M + 3 * N)
    amap = 0.05 + 0.1 * np.random.default_rng(M * N).random((N, M))
    s = gpu_solver_cls(M, N, O)
    s.set_data(ub, f)
    for alpha in (0.08, amap):
        for maxiter in ITERS:
            u0 = oracle.pdhg(f, alpha, maxiter=maxiter)
            for T_ in DEPTHS:
                for chains in (1, 2):
                    u = s.denoise(alpha, maxiter=maxiter, variant=1, tile_iters=T_, chains=chains)
                    st = s.stats()
                    assert st["pdhg_variant"] == 1 and st["launch_chains"] == chains, st
                    assert np.array_equal(u, u0), (np.ndim(alpha), maxiter, T_, chains, st["tile_iters"])
    s.close()


@pytest.mark.parametrize("dtype", [64, 32])
def test_alpha_forms_bit_identical(gpu_solver_cls, oracle, dtype):
    """Scalar, full map, a 3 x 2 patch map over 40 x 60 (the division block), per-image parameters (scalars and maps:
    the parameter block of image k), and a sweep of 2 parameters x 3 images (image % Odata, block image / Odata)."""
    M, N, O = 40, 60, 3
    ref = _ref(oracle, dtype)
    ub, f = synth_batch(O, N, M, seed=11)
    rng = np.random.default_rng(12)
    s = gpu_solver_cls(M, N, O, dtype=dtype)
    s.set_data(ub, f)
    patch = 0.04 + 0.1 * rng.random((2, 3))          # (an, am) = (2, 3): 3 x 2 over 40 x 60
    amap = 0.04 + 0.1 * rng.random((N, M))
    for maxiter, T_ in ((53, 8), (7, 2), (1, 8), (203, 0)):
        kw = dict(maxiter=maxiter, variant=1, tile_iters=T_)
        for alpha in (0.07, amap, patch):
            assert np.array_equal(s.denoise(alpha, **kw), ref(f, alpha, maxiter=maxiter)), (maxiter, T_, np.shape(alpha))
        each = np.array([0.05, 0.09, 0.13])
        u = s.denoise_each(each, **kw)
        for k in range(O):
            assert np.array_equal(u[k], ref(f[k], each[k], maxiter=maxiter)), ("each scalar", maxiter, k)
        maps = 0.04 + 0.1 * rng.random((O, N, M))
        u = s.denoise_each(maps, **kw)
        for k in range(O):
            assert np.array_equal(u[k], ref(f[k], maps[k], maxiter=maxiter)), ("each map", maxiter, k)
    s.close()


def test_sweep_takes_the_division_path_bit_identical(gpu_solver_cls, oracle):
    M, N, O = 40, 60, 3
    ub, f = synth_batch(O, N, M, seed=21)
    s = gpu_solver_cls(M, N, O)
    s.set_data(ub, f)
    alphas = np.array([0.06, 0.11])
    patches = 0.04 + 0.1 * np.random.default_rng(22).random((2, 2, 3))
    for maxiter, T_ in ((53, 8), (7, 0)):
        for par in (alphas, patches):
            costs, u = s.sweep(par, fetch_u=True, maxiter=maxiter, variant=1, tile_iters=T_)
            for k in range(2):
                assert np.array_equal(u[k], oracle.pdhg(f, par[k], maxiter=maxiter)), (maxiter, T_, par.ndim, k)
    # the dataset context afterwards: a sweep's graphs and argument words are not replayed for it
    assert np.array_equal(s.denoise(0.06, maxiter=53, variant=1, tile_iters=8), oracle.pdhg(f, 0.06, maxiter=53))
    s.close()


@pytest.mark.parametrize("dtype", [64, 32])
def test_solver_options_bit_identical(gpu_solver_cls, oracle, dtype):
    """rho > 0 (the general instantiation; rho = 0 beside it on the same handle), both grid forms (xcd = 1: the 1-D grid),
    graph and eager launches, one and two chains, at 50 x 37 (a pulled-back last tile in both dimensions)."""
    M, N, O = 50, 37, 4
    ref = _ref(oracle, dtype)
    ub, f = synth_batch(O, N, M, seed=31)
    amap = 0.05 + 0.1 * np.random.default_rng(32).random((N, M))
    s = gpu_solver_cls(M, N, O, dtype=dtype)
    s.set_data(ub, f)
    for alpha in (0.08, amap):
        for rho in (0.0, 0.05):
            for maxiter, T_ in ((203, 8), (7, 8), (1, 1)):
                u0 = ref(f, alpha, maxiter=maxiter, rho=rho)
                for graph in (1, 0):
                    for xcd in (0, 1):
                        for chains in (1, 2):
                            u = s.denoise(alpha, maxiter=maxiter, rho=rho, variant=1, tile_iters=T_, use_graph=graph, xcd=xcd,
                                          chains=chains)
                            assert np.array_equal(u, u0), (np.ndim(alpha), rho, maxiter, T_, graph, xcd, chains)
    s.close()


def test_prepared_start_bit_identical(gpu_solver_cls, oracle):
    """init / order: the sequence starts from a prepared state in set 1 (no launch with first = 1)."""
    M, N, O = 60, 60, 3
    ub, f = synth_batch(O, N, M, seed=41)
    s = gpu_solver_cls(M, N, O)
    s.set_data(ub, f)
    for init, order in ((1, 0), (0, 1), (1, 1)):
        for maxiter, T_ in ((96, 8), (7, 2), (1, 8)):
            for chains in (1, 2):
                u = s.denoise(0.08, maxiter=maxiter, variant=1, tile_iters=T_, init=init, order=order, chains=chains)
                assert np.array_equal(u, oracle.pdhg_opts(f, 0.08, maxiter=maxiter, init=init, order=order)), (init, order, maxiter, chains)
    s.close()


def test_cached_graphs_keep_their_own_launch_invariant_words(gpu_solver_cls, oracle):
    """Two image sizes on handles alive in one process, then the first again: M * N, the image offsets and R - 2T of a
    cached graph are its own handle's."""
    shapes = [(60, 60, 4), (50, 37, 3)]
    hs, fs, refs = [], [], []
    for M, N, O in shapes:
        ub, f = synth_batch(O, N, M, seed=M)
        s = gpu_solver_cls(M, N, O)
        s.set_data(ub, f)
        hs.append(s); fs.append(f)
        refs.append({(mi, ch): None for mi in (203, 7) for ch in (1, 2)})
    for rnd in range(3):
        for s, f, r in zip(hs, fs, refs):
            for mi, ch in r:
                if r[(mi, ch)] is None:
                    r[(mi, ch)] = oracle.pdhg(f, 0.08, maxiter=mi)
                u = s.denoise(0.08, maxiter=mi, variant=1, tile_iters=8, chains=ch)
                assert np.array_equal(u, r[(mi, ch)]), (rnd, s.M, s.N, mi, ch)
    for s in hs:
        s.close()
