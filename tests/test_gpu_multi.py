"""The single-process multi-device handle (bpltv_create_multi / bpltv_create_sharded, csrc/multi_gpu.hpp).

What can be proven on a one-GPU box: (i) with ngpus = 1 the RCCL communicator (ncclCommInitAll, one rank) is
created and the evaluate's collective really is ncclAllReduce / ncclAllGather; (ii) with several shards placed
on device 0 (RCCL cannot hold two ranks on one device, the same reduction then runs on the host) every entry
point shards the images, fans out to the worker threads and reassembles whole-batch results:
`deterministic` totals are BITWISE those of one single-device handle over the whole batch, the plain sum
agrees to rounding.  The N > 1 RCCL path itself runs only on the driver's 8-GPU node.
"""
import numpy as np
import pytest
from conftest import synth_batch

pytestmark = pytest.mark.gpu

P22 = np.array([[0.08, 0.12], [0.1, 0.05]])


def _single(gpu_solver_cls, ub, f, alpha, delta=0.1, **kw):
    O, N, M = f.shape
    s = gpu_solver_cls(M, N, O)
    s.set_data(ub, f)
    out = s.evaluate(alpha, delta, **kw)
    rows = s.per_image() if np.size(alpha) < M * N else None
    s.close()
    return out, rows


@pytest.mark.parametrize("alpha", [0.1, P22], ids=["scalar", "patch22"])
def test_multi_handle_one_gpu_runs_rccl(gpu_solver_cls, alpha):
    ub, f = synth_batch(3, 48, 40, seed=31)
    (u0, c0, g0), rows0 = _single(gpu_solver_cls, ub, f, alpha, maxiter=400)
    s = gpu_solver_cls(40, 48, 3, ngpus=1)
    s.set_data(ub, f)
    u, c, g = s.evaluate(alpha, 0.1, maxiter=400)
    st = s.stats()
    assert st["ngpus"] == 1 and st["shards"] == 1 and st["collective"] == "ncclAllReduce"
    assert np.array_equal(u, u0) and c == c0 and np.array_equal(np.asarray(g), np.asarray(g0))
    u, c, g = s.evaluate(alpha, 0.1, maxiter=400, deterministic=1)
    assert s.stats()["collective"] == "ncclAllGather+ordered sum"
    assert np.array_equal(u, u0) and c == c0 and np.array_equal(np.asarray(g), np.asarray(g0))
    assert np.array_equal(s.per_image(), rows0)
    s.close()


def test_multi_handle_one_gpu_all_reduces_a_pixel_map_gradient(gpu_solver_cls):
    """The 1 + M*N-double payload of SURVEY 8(e) (a whole gradient image: 513 KiB here, 8 MiB for 1024^2) through the
    one-rank RCCL communicator: ncclAllReduce in place on the shard's partial vector, copied out behind it."""
    O, N, M = 2, 256, 256
    ub, f = synth_batch(O, N, M, seed=39)
    jj, ii = np.meshgrid(np.arange(N), np.arange(M), indexing="ij")
    amap = 0.11 + 0.09 * np.sin(2 * np.pi * ii / M) * np.cos(2 * np.pi * jj / N)
    (u0, c0, g0), _ = _single(gpu_solver_cls, ub, f, amap, maxiter=200)
    s = gpu_solver_cls(M, N, O, ngpus=1)
    s.set_data(ub, f)
    u, c, g = s.evaluate(amap, 0.1, maxiter=200)
    st = s.stats()
    assert st["collective"] == "ncclAllReduce" and st["nccl_ranks"] == 1 and st["shards"] == 1, st
    assert g.shape == (N, M) and np.array_equal(u, u0) and c == c0 and np.array_equal(g, g0)
    s.close()


@pytest.mark.parametrize("nshards", [2, 3])
@pytest.mark.parametrize("alpha", [0.1, P22], ids=["scalar", "patch22"])
def test_shards_on_one_device_match_a_single_handle(gpu_solver_cls, alpha, nshards):
    ub, f = synth_batch(5, 48, 40, seed=32)
    (u0, c0, g0), rows0 = _single(gpu_solver_cls, ub, f, alpha, maxiter=400)
    s = gpu_solver_cls(40, 48, 5, devices=[0] * nshards)
    s.set_data(ub, f)
    u, c, g = s.evaluate(alpha, 0.1, maxiter=400, deterministic=1)
    st = s.stats()
    assert st["shards"] == nshards and st["ngpus"] == 1 and st["collective"] == "host sum"
    assert np.array_equal(u, u0)                         # u shards land in the caller's slices
    assert c == c0 and np.array_equal(np.asarray(g), np.asarray(g0))   # bitwise: rows added in image order
    assert np.array_equal(s.per_image(), rows0)
    u, c, g = s.evaluate(alpha, 0.1, maxiter=400)        # plain sum of the per-shard partial vectors
    assert np.array_equal(u, u0)
    assert np.isclose(c, c0, rtol=1e-14) and np.allclose(g, g0, rtol=1e-12)
    # gradient_reg branch, denoise, duality gap, stand-alone gradient and sweep through the same handle
    _, _, greg = s.evaluate(alpha, 0.0, maxiter=400, deterministic=1)
    (_, _, greg0), _ = _single(gpu_solver_cls, ub, f, alpha, delta=0.0, maxiter=400)
    assert np.array_equal(np.asarray(greg), np.asarray(greg0))
    assert np.array_equal(s.denoise(alpha, maxiter=123), _denoise1(gpu_solver_cls, ub, f, alpha, 123))
    gap = s.duality_gap()
    assert gap.shape == (5,) and (gap >= -1e-12).all()
    assert np.allclose(s.gradient(u0, ub, alpha), g0, rtol=1e-9)
    s.close()


def _denoise1(gpu_solver_cls, ub, f, alpha, it):
    O, N, M = f.shape
    s = gpu_solver_cls(M, N, O)
    s.set_data(ub, f)
    u = s.denoise(alpha, maxiter=it)
    s.close()
    return u


def test_sharded_pixel_map_and_sweep(gpu_solver_cls):
    ub, f = synth_batch(4, 40, 36, seed=33)
    amap = 0.05 + 0.1 * np.random.default_rng(5).random((40, 36))
    (u0, c0, g0), _ = _single(gpu_solver_cls, ub, f, amap, maxiter=300)
    s = gpu_solver_cls(36, 40, 4, devices=[0, 0])
    s.set_data(ub, f)
    u, c, g = s.evaluate(amap, 0.1, maxiter=300)
    assert np.array_equal(u, u0) and np.isclose(c, c0, rtol=1e-14)
    assert g.shape == (40, 36) and np.allclose(g, g0, rtol=1e-9, atol=1e-12 * np.abs(g0).max())
    alphas = np.linspace(0.02, 0.2, 7)
    costs, us = s.sweep(alphas, fetch_u=True, maxiter=200)
    s1 = gpu_solver_cls(36, 40, 4)
    s1.set_data(ub, f)
    costs1, us1 = s1.sweep(alphas, fetch_u=True, maxiter=200)
    s1.close()
    assert np.array_equal(us, us1) and np.allclose(costs, costs1, rtol=1e-14)
    # more shards than images: no empty shard is created
    s2 = gpu_solver_cls(36, 40, 2, devices=[0, 0, 0, 0])
    assert s2.stats()["shards"] == 2
    s2.close()
    # device-pointer entry points are ambiguous over several shards
    from bpldenoising_amd._lib import BpltvError
    with pytest.raises(BpltvError) as e:
        s.u_device_ptr()
    assert e.value.code == 6
    s.close()


@pytest.mark.parametrize("O,K,ndev", [(1, 7, 3), (1, 2, 3), (2, 5, 3), (1, 8, 8)], ids=["1img_K7_n3", "1img_K2_n3", "2img_K5_n3", "1img_K8_n8"])
def test_sweep_splits_the_parameter_blocks_over_replicas(gpu_solver_cls, O, K, ndev):
    """The second data-parallel axis: a dataset with fewer images than devices -- the reference's default
    num_samples = 1 (/root/reference/src/BPLDenoising.jl:313), cameraman_128_10's one pair -- sweeps its K parameters over
    REPLICAS of the dataset, shard_range(K, n) blocks per device.  Rehearsed with a repeated device: bitwise equal to one
    single-device handle's sweep, for K not divisible by n and K < n; scalar and patch parameters; new data reaches the
    replicas; the image shards still serve evaluate."""
    N, M = 48, 40
    ub, f = synth_batch(O, N, M, seed=36)
    alphas = np.linspace(0.02, 0.2, K)
    s1 = gpu_solver_cls(M, N, O)
    s1.set_data(ub, f)
    costs1, us1 = s1.sweep(alphas, fetch_u=True, maxiter=200)
    s = gpu_solver_cls(M, N, O, devices=[0] * ndev)
    s.set_data(ub, f)
    assert s.stats()["shards"] == min(ndev, O)
    costs, us = s.sweep(alphas, fetch_u=True, maxiter=200)
    st = s.stats()
    assert st["sweep_shards"] == min(ndev, K) and st["iterations"] == 200, st
    assert np.array_equal(us, us1) and np.array_equal(costs, costs1)
    # 2 x 1 patch blocks (generate_2d_cost, src/BPLDenoising.jl:136-158)
    blocks = np.array([[[a, b]] for a in (0.05, 0.1, 0.2) for b in (0.03, 0.12)])[:max(2, K - 1)]
    c2 = s.sweep(blocks, maxiter=150)
    nrep = min(ndev, len(blocks))
    by_par = -(-len(blocks) // nrep) * O < len(blocks) * -(-O // min(ndev, O))     # the smaller largest share; ties: images
    assert s.stats()["sweep_shards"] == (nrep if by_par else 0)
    c2s = s1.sweep(blocks, maxiter=150)
    assert np.array_equal(c2, c2s) if by_par else np.allclose(c2, c2s, rtol=1e-14)
    # the image split on request: same numbers, no replica involved
    s.set_option("sweep_split", 1)
    costs_i, us_i = s.sweep(alphas, fetch_u=True, maxiter=200)
    assert s.stats()["sweep_shards"] == 0
    assert np.array_equal(us_i, us1) and np.allclose(costs_i, costs1, rtol=1e-14)
    s.set_option("sweep_split", 0)
    # a new dataset reaches shards and replicas alike
    ub2, f2 = synth_batch(O, N, M, seed=37)
    s.set_data(ub2, f2); s1.set_data(ub2, f2)
    assert np.array_equal(s.sweep(alphas, maxiter=120), s1.sweep(alphas, maxiter=120))
    assert s.stats()["sweep_shards"] == min(ndev, K)
    u, c, g = s.evaluate(0.1, 0.1, maxiter=150, deterministic=1)
    u0, c0, g0 = s1.evaluate(0.1, 0.1, maxiter=150)
    assert np.array_equal(u, u0) and c == c0 and g == g0
    from bpldenoising_amd._lib import BpltvError
    with pytest.raises(BpltvError) as e:
        s.set_option("sweep_split", 3)
    assert e.value.code == 1
    s.close(); s1.close()


def test_sweep_axis_is_chosen_by_the_largest_share(gpu_solver_cls):
    """Automatic choice: the axis whose largest per-device share is smaller; ties keep the image split."""
    ub, f = synth_batch(4, 40, 36, seed=38)
    s = gpu_solver_cls(36, 40, 4, devices=[0, 0, 0])          # images 2,1,1
    s.set_data(ub, f)
    s.sweep(np.linspace(0.05, 0.2, 2), maxiter=20)             # images: 2 x 2 = 4 problems at most; parameters: 1 x 4 = 4 -> images
    assert s.stats()["sweep_shards"] == 0
    s.sweep(np.linspace(0.05, 0.2, 6), maxiter=20)             # images: 6 x 2 = 12; parameters: 2 x 4 = 8 -> parameters
    assert s.stats()["sweep_shards"] == 3
    s.close()


def test_multi_handle_reports_shard_errors(gpu_solver_cls):
    from bpldenoising_amd._lib import BpltvError
    s = gpu_solver_cls(32, 32, 2, devices=[0, 0])
    with pytest.raises(BpltvError) as e:
        s.denoise(0.1, maxiter=5)                      # no data yet
    assert e.value.code == 3 and "shard" in str(e.value)
    with pytest.raises(BpltvError):
        gpu_solver_cls(32, 32, 2, ngpus=99)            # more devices than visible
    s.close()


# ---------------------------------------------------------------------------------------------------------------
# The n > 1 RCCL path itself.  These tests switch themselves on when the box shows at least n devices (the driver's
# 8-GPU node; a one-GPU box skips them), so the first multi-GPU lease validates ncclCommInitAll over n ranks, the
# grouped single-thread ncclAllReduce / ncclAllGather and the ordered sum -- on the workload north_star names:
# faces_train_128_10 sharded over the GPUs (/root/reference/src/TVLearningFunctionVec.jl:20,76-82,168-173).
# ---------------------------------------------------------------------------------------------------------------
def _ndev():
    import torch
    return torch.cuda.device_count()


@pytest.mark.parametrize("n", [2, 3, 4, 8])
@pytest.mark.parametrize("alpha", [0.1, P22], ids=["scalar", "patch22"])
def test_rccl_handle_over_n_devices_matches_a_single_handle(gpu_solver_cls, n, alpha):
    if _ndev() < n:
        pytest.skip("needs %d visible devices (this box shows %d)" % (n, _ndev()))
    from oracle import np_twin as T
    from conftest import DATASETS_NPZ
    ub, f = T.load_dataset(DATASETS_NPZ, "faces_train_128_10")
    (u0, c0, g0), rows0 = _single(gpu_solver_cls, ub, f, alpha, maxiter=600)
    s = gpu_solver_cls(128, 128, 10, ngpus=n)
    s.set_data(ub, f)
    u, c, g = s.evaluate(alpha, 0.1, maxiter=600, deterministic=1)
    st = s.stats()
    assert st["ngpus"] == n and st["shards"] == n and st["nccl_ranks"] == n        # what RCCL itself reports
    assert st["collective"] == "ncclAllGather+ordered sum"
    assert np.array_equal(u, u0)                                                   # every shard's slice landed
    assert c == c0 and np.array_equal(np.asarray(g), np.asarray(g0))               # bitwise: rows added in image order
    assert np.array_equal(s.per_image(), rows0)
    u, c, g = s.evaluate(alpha, 0.1, maxiter=600)                                  # ONE ncclAllReduce(sum, f64) over xGMI
    st = s.stats()
    assert st["collective"] == "ncclAllReduce" and st["nccl_ranks"] == n
    assert np.array_equal(u, u0)
    assert np.isclose(c, c0, rtol=1e-13, atol=0) and np.allclose(g, g0, rtol=1e-12, atol=0)
    # gradient_reg branch and the forward-only entry points through the same communicator-backed handle
    _, _, greg = s.evaluate(alpha, 0.0, maxiter=600, deterministic=1)
    (_, _, greg0), _ = _single(gpu_solver_cls, ub, f, alpha, delta=0.0, maxiter=600)
    assert np.array_equal(np.asarray(greg), np.asarray(greg0))
    assert np.array_equal(s.denoise(alpha, maxiter=77), _denoise1(gpu_solver_cls, ub, f, alpha, 77))
    s.close()


def test_rccl_handle_pixel_map_all_reduce_of_a_whole_gradient_image(gpu_solver_cls):
    """The one payload of section 8(e) that is not latency-bound: 1 + M*N doubles per evaluation."""
    if _ndev() < 2:
        pytest.skip("needs 2 visible devices (this box shows %d)" % _ndev())
    n = min(_ndev(), 4)
    ub, f = synth_batch(6, 64, 64, seed=35)
    amap = 0.05 + 0.1 * np.random.default_rng(6).random((64, 64))
    (u0, c0, g0), _ = _single(gpu_solver_cls, ub, f, amap, maxiter=300)
    s = gpu_solver_cls(64, 64, 6, ngpus=n)
    s.set_data(ub, f)
    u, c, g = s.evaluate(amap, 0.1, maxiter=300)
    assert s.stats()["collective"] == "ncclAllReduce" and s.stats()["nccl_ranks"] == n
    assert np.array_equal(u, u0) and np.isclose(c, c0, rtol=1e-13)
    assert np.allclose(g, g0, rtol=1e-9, atol=1e-12 * np.abs(g0).max())
    s.close()


@pytest.mark.parametrize("n", [2, 4, 8])
def test_one_image_sweep_uses_n_devices(gpu_solver_cls, n):
    """VERDICT r3 item 2, on real devices: 100 parameters x the ONE image of cameraman_128_10 x 10000 iterations
    (generate_cost, /root/reference/src/BPLDenoising.jl:92-111) run as ceil(100 / n) problems per device."""
    if _ndev() < n:
        pytest.skip("needs %d visible devices (this box shows %d)" % (n, _ndev()))
    from oracle import np_twin as T
    from conftest import DATASETS_NPZ
    ub, f = T.load_dataset(DATASETS_NPZ, "cameraman_128_10")
    alphas = np.linspace(0.005, 0.5, 100)
    s1 = gpu_solver_cls(128, 128, 1)
    s1.set_data(ub, f)
    costs1 = s1.sweep(alphas, maxiter=10000)
    s1.close()
    s = gpu_solver_cls(128, 128, 1, ngpus=n)
    s.set_data(ub, f)
    costs = s.sweep(alphas, maxiter=10000)
    st = s.stats()
    assert st["sweep_shards"] == n and st["ngpus"] == n and st["shards"] == 1, st
    assert np.array_equal(costs, costs1)
    s.close()


@pytest.mark.parametrize("mode", ["ranks", "multi-handle"])
def test_bench_multi_gpu_line(mode):
    """bench.py at N = 2 in both forms (one process per GPU over torch.distributed/RCCL; one in-library handle): the
    line says strong scaling of ONE batch, carries the rank count the collective library reports and the per-rank
    shards, and keeps the replica figure out of `value`."""
    if _ndev() < 2:
        pytest.skip("needs 2 visible devices (this box shows %d)" % _ndev())
    import json, os, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cmd = [sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1", "--iters", "400",
           "--full", "--no-cpu-baseline"] + (["--multi-handle", "--evaluate"] if mode == "multi-handle" else [])
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=root)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert line["n_gpus"] == 2 and line["scaling"] == "strong" and line["value"] > 0
    if mode == "ranks":
        assert line["comm"]["world_size"] == 2 and line["comm"]["backend"] == "nccl"
        assert [r_["images"] for r_ in line["ranks"]] == [[0, 5], [5, 10]]
        assert line["weak_value"] > 0 and "weak" in line["weak_note"]
    else:
        mh = line["multi_handle"]
        assert mh["nccl_ranks_reported_by_rccl"] == 2 and mh["collective"] == "ncclAllReduce" and mh["shard_ranges"] == [[0, 5], [5, 10]]


def _bench_mod():
    import importlib.util, os
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bench.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _bench_line(extra, timeout=900):
    import json, os, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py")] + extra, capture_output=True, text=True, timeout=timeout, cwd=root, env=env)
    assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-3000:]
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])


def test_bench_two_ranks_rehearsed_on_one_device(tmp_path, oracle):
    """bench.py's N > 1 code under the one-GPU suite: two ranks launched by torch.distributed.run on device 0 (gloo --
    RCCL cannot hold two ranks on one device), ONE faces_train_128_10 batch sharded 5 + 5, the replica figure kept out
    of `value`; the line carries comm / ranks / weak_value as a multi-GPU run will.  --dump-outputs: each
    rank writes its shard of u, together the oracle's PDHG of the batch."""
    line = _bench_line(["--gpus", "2", "--one-device", "--backend", "gloo", "--steps", "2", "--warmup", "1", "--iters", "400", "--full",
                        "--no-cpu-baseline", "--dump-outputs", str(tmp_path)])
    assert line["n_gpus"] == 2 and line["scaling"] == "strong" and line["value"] > 0
    assert line["comm"]["world_size"] == 2 and line["comm"]["backend"] == "gloo"
    assert [r_["images"] for r_ in line["ranks"]] == [[0, 5], [5, 10]] and all(r_["device"] == 0 for r_ in line["ranks"])
    assert line["weak_value"] > 0 and "NOT `value`" in line["weak_note"]
    assert line["config"]["images_per_gpu"] == 5 and 0 < line["roofline"]["frac"] <= 1.0
    u = np.concatenate([np.load(tmp_path / ("u_rank%d.npy" % r)) for r in (0, 1)])
    _, f, _ = _bench_mod().load_batch("auto", 10, 128, 128, 20211004)
    assert np.array_equal(u, oracle.pdhg(f, 0.1, maxiter=400))


def test_bench_multi_handle_and_sweep_rehearsed_on_one_device(tmp_path, oracle):
    """The in-library form (`--multi-handle --evaluate`: two shards on device 0, host sum in place of the collective) and
    the parameter sweep over replicas (`--sweep`: 7 parameters x 1 image on three devices = 3, 2, 2); --dump-outputs
    writes the [cost, grad] of the last evaluation, the oracle's to the tolerances of smoke()."""
    line = _bench_line(["--gpus", "2", "--multi-handle", "--one-device", "--evaluate", "--steps", "2", "--warmup", "1", "--iters", "400",
                        "--full", "--no-cpu-baseline", "--dump-outputs", str(tmp_path)])
    mh = line["multi_handle"]
    assert line["n_gpus"] == 2 and mh["shards"] == 2 and mh["shard_ranges"] == [[0, 5], [5, 10]]
    assert mh["collective"] == "host sum" and mh["nccl_ranks_reported_by_rccl"] == 0
    assert "evaluate" in line["config"]["workload"] and 0 < line["roofline"]["frac"] <= 1.0
    cg = np.load(tmp_path / "cost_grad.npy")
    ub, f, _ = _bench_mod().load_batch("auto", 10, 128, 128, 20211004)
    u0 = oracle.pdhg(f, 0.1, maxiter=400)
    c0, g0 = oracle.cost(u0, ub), oracle.gradient(0.1, u0, ub)
    assert cg.shape == (2,) and abs(cg[0] - c0) <= 1e-10 * abs(c0) and np.allclose(cg[1], g0, rtol=1e-5, atol=1e-8), (cg, c0, g0)
    line = _bench_line(["--gpus", "3", "--one-device", "--sweep", "7", "--iters", "300", "--steps", "1", "--warmup", "1"])
    sw = line["sweep"]
    assert sw["sweep_shards"] == 3 and sw["parameter_ranges_per_device"] == [[0, 3], [3, 5], [5, 7]] and sw["image_shards"] == 1
    assert line["value"] > 0 and "cameraman_128_10" in line["data"]

