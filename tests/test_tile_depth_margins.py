"""CPU check of the cases tests/test_gpu_tile_depths.py holds against the numpy twins: every projection decision of every
twin stays at least 1e-9 (relative to alpha^2) away from its threshold, the condition tests/test_color_abi.py sets -- so the
HIP kernels, whose roundings differ from numpy's in the last bits, take the same decisions and the twin's bounds apply.  The
TV-L1 and TV-KL cases also meet what tests/test_l1_abi.py and tests/test_kl_abi.py ask of theirs: the soft threshold's decision
and the sign at a pixel without data stay clear of rounding, the KL iterates stay clear of zero, and both branches of the
threshold, of the prox and of the projection are taken.

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
        assert np.array_equal(wr.step_table(kmax, 0.0)[:K], wr.step_table(K, 0.0))      # l1, kl, a mask or the mosaic
    shape = (1, 33, 32)
    for fam in td.FAMILIES:           # (the sum of regularisers builds its table inside the loop)
        for wkind in td.weights_of(fam):
            _, t7, tab7, _ = td.forward(fam, shape, "patch", 7, wkind)
            _, t50, tab50, _ = td.forward(fam, shape, "patch", 50, wkind)
            assert np.array_equal(t50[:7], t7) and np.array_equal(tab50[:7], tab7), (fam, wkind)
    shape = (1, 2, 17, 70)
    for wkind in td.weights_of("color_weighted"):
        _, t7, tab7, _ = td.forward("color_weighted", shape, "patch", 7, wkind)
        _, t50, tab50, _ = td.forward("color_weighted", shape, "patch", 50, wkind)
        assert np.array_equal(t50[:7], t7) and np.array_equal(tab50[:7], tab7), wkind


def test_the_cases_are_the_ones_the_geometry_asks_for():
    import tiling_ref as tr
    assert td.SHAPES == [(2, 70, 72), (2, 32, 32), (1, 33, 32), (1, 32, 33), (1, 49, 33), (1, 17, 70)]
    assert td.COLOR_SHAPES == [(2, 3, 70, 72), (1, 2, 49, 33), (1, 4, 70, 33), (2, 2, 32, 32), (1, 2, 17, 70)]
    assert sorted(sh[1] for sh in td.COLOR_SHAPES) == [2, 2, 2, 3, 4]
    assert td.FAMILIES == ("tv", "weighted", "sumregs", "l1", "kl") and td.COLOR_FAMILIES == ("color", "color_weighted")
    assert len(td.CASES) == len(set(td.CASES)) == 5 * 6 + 2 * 5
    assert {fam: td.weights_of(fam) for fam in td.FAMILIES + td.COLOR_FAMILIES} == {
        "tv": (None,), "sumregs": (None,), "color": (None,), "weighted": ("real",), "l1": ("real", "mask"), "kl": ("real", "mask"),
        "color_weighted": ("real", "mosaic")}
    for fam, sh in td.CASES:
        N, M = sh[-2:]
        f, gu, df = td.data(fam, sh)
        assert f.shape == gu.shape == df.shape == (int(np.prod(sh[:-2])), N, M)
        assert tr.depth_cap(td.model_of(fam, sh), N, M) == ((7 if fam == "sumregs" else 32) if max(N, M) <= 32 else (7 if fam == "sumregs" else 15))
        for wkind in td.weights_of(fam):
            w = td.weight(fam, sh, wkind)
            assert (w is None) == (wkind is None)
            if w is not None:
                assert w.shape == ((N, M) if wkind == "mask" else f.shape) and (w.min() == 0.0) == (wkind in ("mask", "mosaic")), (fam, sh, wkind)
        if fam == "kl":
            assert f.min() >= 0.1
    # the reverse caps of the new rows, as the headers state them
    assert [tr.REV_CAP[m] for m in ("l1", "kl", "color_weighted2", "color_weighted3", "color_weighted4")] == [8, 8, 5, 2, 1]
    assert {td.model_of("color_weighted", sh) for sh in td.COLOR_SHAPES} == {"color_weighted2", "color_weighted3", "color_weighted4"}
    # colour: 70 rows have a middle tile along j at every depth, the reverse depths 3, 4 and 6 included; 49 rows at the default
    for B, Cc, N, M in td.COLOR_SHAPES:
        if N > 32:
            assert all(tr.interior(N, T) >= 1 for T in (range(1, 16) if N == 70 else (8,))), (N, M)
    # 17 x 70: one tile along j that 15 of its 32 lanes per column lie outside of, and along i a middle tile at every depth
    # (at every halo 2T the sum of regularisers takes)
    for sh in (td.SHAPES[-1], td.COLOR_SHAPES[-1]):
        assert sh[-2:] == (17, 70) and tr.tile_count(17, 15) == 1 and tr.REGION - 17 == 15
    assert all(tr.interior(70, T) >= 1 for T in range(1, 16)) and all(tr.interior(70, 2 * T) >= 1 for T in range(1, 8))


@pytest.mark.parametrize("kind", td.KINDS)
def test_the_flat_patch_holds_pixels_without_data_at_f(kind):
    """tile_depth_ref.l1_flat_twin: the conditions of the l1 cases, and pixels with w == 0 whose x+ is f bit for bit in
    iterations after the first -- inside the patch and at least two pixels from its rim there are 9 x 26 pixels, about 30 % of
    them without data, and iteration 1 alone holds each of those."""
    rows, cols = td.FLAT_PATCH
    w = td.weight("l1", td.FLAT_SHAPE, "mask")
    inner = int((w[rows.start + 2:rows.stop - 2, cols.start + 2:cols.stop - 2] == 0).sum())
    assert td.FLAT_SHAPE in td.SHAPES and inner >= 30
    for K in td.FLAT_KS:
        st = td.l1_flat_twin(kind, K)[5]
        print("flat patch %s K %d: %s" % (kind, K, "  ".join("%s %.3g" % kv for kv in sorted(st.items()))))
        assert st["held"] >= inner
        assert st["decision_margin"] >= td.MARGIN and st["threshold_margin"] >= 1e-9 and st["nodata_margin"] >= 1e-9
        assert 0.1 <= st["active_share"] <= 0.9


@pytest.mark.parametrize("kind", td.KINDS)
@pytest.mark.parametrize("case", td.CASES, ids=td.case_id)
def test_the_twin_s_decisions_stay_clear_of_the_threshold(case, kind):
    """The conditions are on the inputs, not measurements.  Beside the projection's margin: for l1 what tests/test_l1_abi.py
    asks (the threshold's own margin, the sign at a pixel without data, both branches of the threshold taken), for kl what
    tests/test_kl_abi.py asks (x+ clear of zero, both branches of the projection, and with the mask both of the prox: with
    weights in [0.5, 2] nearly every c = v - tau w is negative)."""
    fam, shape = case
    for wkind in td.weights_of(fam):
        stats = {}
        m = td.margin(fam, shape, kind, max(td.KS), wkind, stats)
        print("%s %s %s: min decision margin over %d iterations %.2e  %s" % (td.case_id(case), kind, wkind, max(td.KS), m,
                                                                             "  ".join("%s %.3g" % kv for kv in sorted(stats.items()))))
        assert m >= td.MARGIN
        if fam == "l1":
            assert stats["threshold_margin"] >= 1e-9
            assert 0.1 <= stats["active_share"] <= 0.9
            if wkind == "mask":
                assert stats["nodata_margin"] >= 1e-9
        if fam == "kl":
            assert stats["min_x"] >= 1e-3
            assert 0.02 <= stats["active_share"] <= 0.98
            if wkind == "mask":
                assert 0.05 <= stats["neg_share"] <= 0.95
