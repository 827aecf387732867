"""CPU check of the cases tests/test_gpu_tile_depths.py holds against the numpy twins: every projection decision of every
twin stays at least 1e-9 (relative to alpha^2) away from its threshold, the condition tests/test_color_abi.py sets -- so the
HIP kernels, whose roundings differ from numpy's in the last bits, take the same decisions and the twin's bounds apply.

One tape of 203 iterations per case covers the shorter solves: the step tables do not depend on the iteration count, so the
first K iterations of a longer solve are the solve of K iterations."""
import numpy as np
import pytest

import tile_depth_ref as td
import weighted_ref as wr
from oracle import np_twin as tw


def test_a_longer_solve_starts_with_the_shorter_one():
    kmax = max(td.KS)
    for K in td.KS:
        assert np.array_equal(tw.step_table(kmax)[:K], tw.step_table(K))
        assert np.array_equal(wr.step_table(kmax, 0.25)[:K], wr.step_table(K, 0.25))
    shape = (1, 33, 32)
    for fam in td.FAMILIES:           # (the sum of regularisers builds its table inside the loop)
        _, t7, tab7, _ = td.forward(fam, shape, "patch", 7)
        _, t50, tab50, _ = td.forward(fam, shape, "patch", 50)
        assert np.array_equal(t50[:7], t7) and np.array_equal(tab50[:7], tab7), fam


def test_the_cases_are_the_ones_the_geometry_asks_for():
    import tiling_ref as tr
    assert td.SHAPES == [(2, 70, 72), (2, 32, 32), (1, 33, 32), (1, 32, 33), (1, 49, 33)]
    assert td.COLOR_SHAPES == [(2, 3, 70, 72), (1, 2, 49, 33), (1, 4, 70, 33), (2, 2, 32, 32)]
    assert sorted(sh[1] for sh in td.COLOR_SHAPES) == [2, 2, 3, 4]
    for fam, sh in td.CASES:
        N, M = sh[-2:]
        f, gu, df = td.data(fam, sh)
        assert f.shape == gu.shape == df.shape == (int(np.prod(sh[:-2])), N, M)
        assert tr.depth_cap(td.model_of(fam, sh), N, M) == ((7 if fam == "sumregs" else 32) if max(N, M) <= 32 else (7 if fam == "sumregs" else 15))
    # colour: 70 rows have a middle tile along j at every depth, the reverse depths 3, 4 and 6 included; 49 rows at the default
    for B, Cc, N, M in td.COLOR_SHAPES[:-1]:
        assert all(tr.interior(N, T) >= 1 for T in (range(1, 16) if N == 70 else (8,))), (N, M)


@pytest.mark.parametrize("kind", td.KINDS)
@pytest.mark.parametrize("case", td.CASES, ids=td.case_id)
def test_the_twin_s_decisions_stay_clear_of_the_threshold(case, kind):
    fam, shape = case
    m = td.margin(fam, shape, kind, max(td.KS))
    print("%s %s: min decision margin over %d iterations %.2e" % (td.case_id(case), kind, max(td.KS), m))
    assert m >= td.MARGIN
