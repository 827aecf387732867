"""GPU checks of the batched sum-of-regularisers sweep (bpltv_sumregs_sweep): the reference's generate_cost with
denoise_function = sumregs_denoise (the reference's src/BPLDenoising.jl:92-158, src/SumRegsLearningFunction.jl:38-85)
as one batch of K*O problems.  Every problem is bit-exact to oracle/sumregs_oracle.c, whatever the kernel, the fusion
depth, the grouping of the parameter blocks or the device split; the sweep never touches the dataset context."""
import numpy as np
import pytest
from conftest import DATASETS_NPZ, synth_batch

pytestmark = pytest.mark.gpu

A3 = np.array([0.03, 0.02, 0.05])
P3 = np.stack([np.array([[0.03, 0.05], [0.02, 0.04]]), np.array([[0.02, 0.03], [0.05, 0.02]]), np.array([[0.04, 0.02], [0.03, 0.06]])])


def _blocks(kind, K, N, M, seed=0):
    """K parameter blocks of one kind: (K, 3) triples, (K, 3, 2, 2) patches or (K, 3, N, M) pixel maps."""
    rng = np.random.default_rng(seed)
    if kind == "vector":
        return A3[None] * (0.5 + rng.random((K, 3)))
    if kind == "patch22":
        return P3[None] * (0.5 + rng.random((K, 3, 1, 1)))
    return 0.02 + 0.05 * rng.random((K, 3, N, M))


def _check_oracle(oracle, f, ub, blocks, costs, us, maxiter, ks=None):
    for k in (range(len(blocks)) if ks is None else ks):
        u0 = oracle.sumregs_pdhg(f, blocks[k], maxiter=maxiter, nthreads=4)
        assert np.array_equal(us[k], u0.reshape(us[k].shape)), k
        c0 = oracle.cost(us[k], ub)
        assert abs(costs[k] - c0) <= 1e-13 * abs(c0), (k, costs[k], c0)


@pytest.mark.parametrize("shape", [(2, 40, 33), (3, 70, 96), (1, 20, 150), (1, 128, 128)], ids=["40x33", "70x96", "20x150", "128"])
@pytest.mark.parametrize("kind", ["vector", "patch22", "map"])
@pytest.mark.parametrize("K", [1, 3, 5])
def test_sweep_bit_exact(gpu_solver_cls, oracle, shape, kind, K):
    O, N, M = shape
    ub, f = synth_batch(O, N, M, seed=11 + M)
    blocks = _blocks(kind, K, N, M, seed=K)
    s = gpu_solver_cls(M, N, O)
    s.set_data(ub, f)
    for it, T_, var in ((37, 0, 0), (64, 1, 2), (50, 4, 2), (37, 2, 1)):   # both kernels, several fusion depths
        costs, us = s.sumregs_sweep(blocks, fetch_u=True, maxiter=it, tile_iters=T_, variant=var)
        assert us.shape == (K, O, N, M)
        st = s.stats()
        assert st["iterations"] == it and st["sweep_groups"] == 1
        if var:
            assert st["region_i"] == {1: 32, 2: 48}[var]
        _check_oracle(oracle, f, ub, blocks, costs, us, it)
    s.close()


def test_large_single_image_sweep_takes_the_strip_kernel(gpu_solver_cls, oracle):
    """1 x 128^2 with K = 48: 48 problems, past the ~40 images where the 48 x 48 strip kernel takes over."""
    ub, f = synth_batch(1, 128, 128, seed=48)
    blocks = _blocks("vector", 48, 128, 128, seed=48)
    s = gpu_solver_cls(128, 128, 1)
    s.set_data(ub, f)
    costs, us = s.sumregs_sweep(blocks, fetch_u=True, maxiter=40)
    assert s.stats()["region_i"] == 48
    _check_oracle(oracle, f, ub, blocks, costs, us, 40)
    s.close()


def test_sweep_and_dataset_contexts_do_not_mix(gpu_solver_cls, oracle):
    """denoise -> sweep -> denoise -> evaluate with the same maxiter: each result is the oracle's; a sweep leaves the last
    solve's result (u_device, duality gap) as it was, and a TV sweep in between changes nothing."""
    O, N, M = 2, 48, 40
    ub, f = synth_batch(O, N, M, seed=21)
    it = 60
    blocks = _blocks("vector", 3, N, M, seed=3)
    s = gpu_solver_cls(M, N, O)
    s.set_data(ub, f)
    u0 = oracle.sumregs_pdhg(f, A3, maxiter=it, nthreads=4)
    assert np.array_equal(s.sumregs_denoise(A3, maxiter=it), u0)
    gap0 = s.duality_gap()
    costs, us = s.sumregs_sweep(blocks, fetch_u=True, maxiter=it)
    _check_oracle(oracle, f, ub, blocks, costs, us, it)
    assert np.array_equal(s.duality_gap(), gap0)           # the dataset context still holds the denoise
    assert np.array_equal(s.sumregs_denoise(A3, maxiter=it), u0)
    costs_tv = s.sweep(np.array([0.05, 0.1]), maxiter=it)
    c2, us2 = s.sumregs_sweep(blocks, fetch_u=True, maxiter=it)
    assert np.array_equal(us2, us) and np.array_equal(c2, costs)
    assert np.array_equal(s.sweep(np.array([0.05, 0.1]), maxiter=it), costs_tv)
    u, cost, _ = s.sumregs_evaluate(P3, 0.1, maxiter=it)
    assert np.array_equal(u, oracle.sumregs_pdhg(f, P3, maxiter=it, nthreads=4))
    assert np.array_equal(s.sumregs_sweep(blocks, maxiter=it), costs)
    s.close()


def test_groups_give_bitwise_the_same_result(gpu_solver_cls, oracle):
    O, N, M = 2, 40, 33
    ub, f = synth_batch(O, N, M, seed=31)
    blocks = _blocks("patch22", 5, N, M, seed=31)
    s = gpu_solver_cls(M, N, O)
    s.set_data(ub, f)
    costs, us = s.sumregs_sweep(blocks, fetch_u=True, maxiter=50)
    assert s.stats()["sweep_groups"] == 1
    per_block = O * 14 * N * M * 8 / 1e6            # MB of state per parameter block
    for nfit, groups in ((2, 3), (1, 5), (4, 2)):
        s.set_option("sr_sweep_budget_mb", nfit * per_block * 1.01)
        c, u = s.sumregs_sweep(blocks, fetch_u=True, maxiter=50)
        assert s.stats()["sweep_groups"] == groups
        assert np.array_equal(u, us) and np.array_equal(c, costs)
    s.set_option("sr_sweep_budget_mb", 0.5 * per_block)   # not even one block fits
    from bpldenoising_amd._lib import BpltvError
    with pytest.raises(BpltvError) as e:
        s.sumregs_sweep(blocks, maxiter=50)
    assert e.value.code == 5                              # BPLTV_E_NOMEM
    s.set_option("sr_sweep_budget_mb", 0)
    assert np.array_equal(s.sumregs_sweep(blocks, maxiter=50), costs)
    _check_oracle(oracle, f, ub, blocks, costs, us, 50, ks=[0, 4])
    s.close()


def test_more_than_65535_problems_run_in_groups(gpu_solver_cls, oracle):
    O, N, M, K = 2, 8, 8, 32769                     # 65538 problems: one more than a grid dimension holds
    ub, f = synth_batch(O, N, M, seed=41)
    blocks = _blocks("vector", K, N, M, seed=41)
    s = gpu_solver_cls(M, N, O)
    s.set_data(ub, f)
    costs, us = s.sumregs_sweep(blocks, fetch_u=True, maxiter=20)
    assert s.stats()["sweep_groups"] == 2
    _check_oracle(oracle, f, ub, blocks, costs, us, 20, ks=[0, 1, 16384, 16385, K - 1])
    s.close()


def test_edge_cases(gpu_solver_cls, oracle):
    from bpldenoising_amd._lib import BpltvError
    O, N, M = 2, 36, 30
    ub, f = synth_batch(O, N, M, seed=51)
    blocks = _blocks("vector", 3, N, M, seed=51)
    s = gpu_solver_cls(M, N, O)
    s.set_data(ub, f)
    costs, us = s.sumregs_sweep(blocks, fetch_u=True, maxiter=0)          # u = f for every block
    assert all(np.array_equal(us[k], f) for k in range(3))
    c0 = oracle.cost(f, ub)
    assert np.allclose(costs, c0, rtol=1e-13)
    costs, us = s.sumregs_sweep(blocks, fetch_u=True, maxiter=45, check_every=5, gap_tol=1e3)   # no early stop
    assert s.stats()["iterations"] == 45
    _check_oracle(oracle, f, ub, blocks, costs, us, 45)
    u_ref = oracle.sumregs_pdhg(f, A3, maxiter=30, nthreads=4)
    assert np.array_equal(s.sumregs_denoise(A3, maxiter=30), u_ref)
    gap0 = s.duality_gap()
    bad = [(np.array([[0.1, np.nan, 0.1]]), {}), (np.array([[0.1, -0.01, 0.1]]), {}), (np.zeros((0, 3)), {}),
           (0.05 * np.ones((1, 3, N + 1, M)), {}), (np.array([[0.1, 0.0, 0.1]]), {"rho": 0.5})]
    for a, kw in bad:
        with pytest.raises(BpltvError) as e:
            s.sumregs_sweep(a, maxiter=30, **kw)
        assert e.value.code == 1, (a.shape, kw)
        assert np.array_equal(s.duality_gap(), gap0)
    with pytest.raises(ValueError):
        s.sumregs_sweep(np.ones((2, 4)), maxiter=30)
    assert np.array_equal(s.sumregs_denoise(A3, maxiter=30), u_ref)
    s.close()


def test_multi_handle_replicas_and_image_split(gpu_solver_cls):
    """Rehearsed with a repeated device: O = 1 splits the K blocks over replicas (bitwise a single handle); O = 4 with
    the image split requested adds per-shard costs on the host (rounding) and writes u in place (bitwise)."""
    N, M = 48, 40
    ub, f = synth_batch(1, N, M, seed=61)
    blocks = _blocks("vector", 7, N, M, seed=61)
    s1 = gpu_solver_cls(M, N, 1)
    s1.set_data(ub, f)
    c1, u1 = s1.sumregs_sweep(blocks, fetch_u=True, maxiter=80)
    s = gpu_solver_cls(M, N, 1, devices=[0] * 3)
    s.set_data(ub, f)
    c, u = s.sumregs_sweep(blocks, fetch_u=True, maxiter=80)
    assert s.stats()["sweep_shards"] == 3
    assert np.array_equal(u, u1) and np.array_equal(c, c1)
    s.close(); s1.close()

    ub, f = synth_batch(4, N, M, seed=62)
    blocks = _blocks("patch22", 3, N, M, seed=62)
    s1 = gpu_solver_cls(M, N, 4)
    s1.set_data(ub, f)
    c1, u1 = s1.sumregs_sweep(blocks, fetch_u=True, maxiter=80)
    s = gpu_solver_cls(M, N, 4, devices=[0] * 3)
    s.set_data(ub, f)
    s.set_option("sweep_split", 1)
    c, u = s.sumregs_sweep(blocks, fetch_u=True, maxiter=80)
    assert s.stats()["sweep_shards"] == 0
    assert np.array_equal(u, u1) and np.allclose(c, c1, rtol=1e-14)
    s.close(); s1.close()


def test_python_generate_cost_and_experiment_driver(gpu_solver_cls, tmp_path):
    from bpldenoising_amd import experiments as E
    from bpldenoising_amd.learning_function import clear_cache, generate_cost, sumregs_denoise
    ub, f = E.testdataset("cameraman_128_5", npz=DATASETS_NPZ)
    P = _blocks("vector", 4, 0, 0, seed=71)
    c = generate_cost((ub, f), P, denoise_function=sumregs_denoise, maxiter=30)
    O = 1 if np.ndim(f) == 2 else f.shape[0]
    N, M = np.shape(f)[-2:]
    s = gpu_solver_cls(M, N, O)
    s.set_data(ub, f)
    assert np.array_equal(c, s.sumregs_sweep(P, maxiter=30))
    costs = E.generate_sumregs_cost("cameraman_128_5", P, npz=DATASETS_NPZ, out_root=str(tmp_path), maxiter=30)
    full = E._full("cameraman_128_5")
    z = np.load(tmp_path / full / (full + "_sumregs_cost.npz"))
    assert np.array_equal(z["costs"], costs) and np.array_equal(z["parameters"], P)
    assert costs.shape == (4,) and np.all(np.isfinite(costs))
    s.close()
    clear_cache()
