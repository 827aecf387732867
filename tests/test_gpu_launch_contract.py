"""The launch-count contract of the shared launch driver (run_chains), for the three models it serves: TV
(bpltv_denoise), sum of regularisers (bpltv_sumregs_denoise) and the weighted model (bpltv_weighted_denoise).

maxiter iterations at depth T are nl = ceil(maxiter / T) launches per chain; with two chains the odd one runs half a
launch out of phase -- one launch more -- exactly when tiling.hpp's chain_out_of_phase allows it (T >= 2, at least 8
launches, the out-of-phase chain ends in the same state set, and the sequence does not start from a prepared state).
However the iterations are cut into launches and chains, the result has the same bits."""
import numpy as np
import pytest
from conftest import synth_batch

pytestmark = pytest.mark.gpu

A3 = np.array([0.03, 0.02, 0.05])
ALPHA = 0.1
# multiples of T and not, both parities of the out-of-phase chain's launch count, fewer than 8 launches, T = 1
CASES = [(40, 4), (43, 4), (38, 4), (39, 3), (38, 3), (20, 4), (12, 1)]


def _out_of_phase(it, T):
    """chain_out_of_phase(it, T, from_state = false), restated"""
    nl = -(-it // T)
    h0 = max(1, T // 2)
    return int(T >= 2 and nl >= 8 and ((1 + -(-(it - h0) // T)) - nl) % 2 == 1)


def _batch():
    return synth_batch(3, 50, 44, seed=81)


def _check_stats(st, chains, nl, s, what):
    assert st["launch_chains"] == chains and st["graph_used"] == 1, (what, st)
    assert st["launches"] == chains * nl + s, (what, chains, nl, s, st["launches"])


@pytest.mark.parametrize("case", CASES, ids=["%dx%d" % c for c in CASES])
def test_launch_counts_and_bits_of_the_three_models(gpu_solver_cls, oracle, case):
    it, T = case
    ub, f = _batch()
    O, N, M = f.shape
    w = np.ones((N, M))
    nl = -(-it // T)
    s = gpu_solver_cls(M, N, O)
    s.set_data(ub, f)
    # no graph: one chain, launched eagerly
    u_tv = s.denoise(ALPHA, maxiter=it, tile_iters=T, variant=1, use_graph=0)
    st = s.stats()
    assert st["graph_used"] == 0 and st["launches"] == nl, st
    u_w = s.weighted_denoise(ALPHA, w, maxiter=it, tile_iters=T, use_graph=0)
    st = s.stats()
    assert st["graph_used"] == 0 and st["launches"] == nl, st
    assert np.array_equal(u_w, u_tv)
    u_sr = oracle.sumregs_pdhg(f, A3, maxiter=it, nthreads=4)
    for chains in (1, 2):
        extra = _out_of_phase(it, T) if chains == 2 else 0
        u = s.denoise(ALPHA, maxiter=it, tile_iters=T, variant=1, chains=chains)
        _check_stats(s.stats(), chains, nl, extra, "tv")
        assert np.array_equal(u, u_tv), (it, T, chains)
        u = s.weighted_denoise(ALPHA, w, maxiter=it, tile_iters=T, chains=chains)
        _check_stats(s.stats(), chains, nl, extra, "weighted")
        assert np.array_equal(u, u_tv), (it, T, chains)
        u = s.sumregs_denoise(A3, maxiter=it, tile_iters=T, variant=1, chains=chains)
        _check_stats(s.stats(), chains, nl, extra, "sumregs")
        assert np.array_equal(u, u_sr), (it, T, chains)
    s.close()


def test_prepared_start_keeps_two_chains_in_phase(gpu_solver_cls, oracle):
    """params.init = 1: the sequence starts from a prepared state in set 1, so the odd chain is not moved out of phase
    although 40 iterations at depth 4 would allow it."""
    it, T = 40, 4
    assert _out_of_phase(it, T) == 1
    ub, f = _batch()
    O, N, M = f.shape
    s = gpu_solver_cls(M, N, O)
    s.set_data(ub, f)
    u = s.denoise(ALPHA, maxiter=it, tile_iters=T, variant=1, chains=2, init=1)
    _check_stats(s.stats(), 2, it // T, 0, "tv, init = 1")
    assert np.array_equal(u, oracle.pdhg_opts(f, ALPHA, maxiter=it, init=1, order=0))
    s.close()
