"""CPU checks of tests/tiling_ref.py, the plain restatement of the tiling of the 32 x 32 unrolled tile kernels: the cores
partition an axis, every core pixel is a halo away from each region edge that is not an image border, the shapes of
tests/test_gpu_tile_depths.py have the tiles they were chosen for, and the restatement agrees with the one
tests/test_gpu_weighted_shapes.py carries."""
import pytest

import tiling_ref as tr

LENGTHS = range(1, 101)
HALOS = range(1, 16)


def test_the_cores_partition_the_axis():
    for L in LENGTHS:
        for h in HALOS:
            t = tr.tiles(L, h)
            assert t[0][1] == 0 and t[-1][2] == L, (L, h, t)
            assert all(a[2] == b[1] for a, b in zip(t, t[1:])), (L, h, t)          # no gap, no overlap
            assert all(c0 < c1 for _, c0, c1 in t), (L, h, t)                       # no empty core
            assert tr.tile_count(L, h) == len(t) and (len(t) == 1) == (L <= tr.REGION)


def test_every_region_lies_on_the_image_and_holds_its_core_and_halo():
    for L in LENGTHS:
        for h in HALOS:
            for o, c0, c1 in tr.tiles(L, h):
                assert 0 <= o and o + min(L, tr.REGION) <= L, (L, h, o)
                assert o <= c0 and c1 <= o + tr.REGION, (L, h, o, c0, c1)
                # h iterations spoil h pixels from every region edge that is not an image border (Neumann: no halo there)
                if o > 0:
                    assert c0 - o >= h, (L, h, o, c0)
                if o + tr.REGION < L:
                    assert (o + tr.REGION) - c1 >= h, (L, h, o, c1)


def test_a_halo_that_leaves_no_core_is_refused():
    assert tr.tiles(32, 16) == [(0, 0, 32)]              # one region: no halo at all
    with pytest.raises(ValueError):
        tr.tiles(33, 16)


def test_the_last_tile_is_shifted_back_onto_the_image():
    assert tr.tiles(32, 8) == [(0, 0, 32)] and tr.tiles(17, 8) == [(0, 0, 17)]
    for h in HALOS:
        assert tr.tiles(33, h) == [(0, 0, 32 - h), (1, 32 - h, 33)]   # shifted back by 31 pixels
    assert tr.tiles(49, 8) == [(0, 0, 24), (16, 24, 40), (17, 40, 49)]   # a middle tile; the last one overlaps it by 31 rows


# (tiles, interior tiles) at depths 1 ... 15
T70 = [(3, 1)] * 6 + [(4, 2)] * 3 + [(5, 3)] * 2 + [(6, 4), (8, 6), (11, 9), (20, 18)]


def test_the_gpu_shapes_have_the_tiles_they_were_chosen_for():
    got = lambda L: [(tr.tile_count(L, h), tr.interior(L, h)) for h in HALOS]
    assert got(70) == T70
    assert got(72) == T70[:-1] + [(21, 19)]
    assert got(33) == [(2, 0)] * 15
    assert [h for h in HALOS if tr.interior(48, h)] == list(range(9, 16))
    assert got(32) == [(1, 0)] * 15
    assert tr.interior(49, 8) == 1 and tr.interior(40, 8) == 0
    # what the colour cases had before: an axis of 40 has two tiles at the depths their tests use, none of them interior
    assert all(got(40)[h - 1] == (2, 0) for h in (1, 3, 8))
    # the sum of regularisers: halo 2T
    assert [tr.tile_count(70, tr.halo_of("sumregs", T)) for T in range(1, 8)] == [3, 3, 3, 4, 5, 6, 11]
    assert all(tr.interior(70, tr.halo_of("sumregs", T)) >= 1 for T in range(1, 8))


def test_the_depth_caps():
    for model in tr.MODELS:
        sr = model == "sumregs"
        assert tr.depth_cap(model, 70, 72) == (7 if sr else 15)
        assert tr.depth_cap(model, 32, 32) == (7 if sr else 32)
        assert tr.depth_cap(model, 33, 32) == tr.depth_cap(model, 32, 33) == tr.depth_cap(model, 49, 33) == (7 if sr else 15)
        assert tr.depth(model, 70, 72) == (4 if sr else 8) and tr.depth(model, 70, 72, 99) == tr.depth_cap(model, 70, 72)
        assert tr.depth(model, 32, 32, 3) == 3
        assert 1 <= tr.REV_CAP[model] <= tr.depth_cap(model, 70, 72)
    assert tr.tiles_of("tv", 2, 70, 72, 8) == 2 * 4 * 4 and tr.tiles_of("sumregs", 2, 70, 72, 4) == 2 * 4 * 4
    assert tr.tiles_of("color3", 2, 70, 72, 15) == 2 * 20 * 21 and tr.tiles_of("tv", 2, 32, 32, 32) == 2


def test_the_restatement_in_test_gpu_weighted_shapes_agrees():
    import test_gpu_weighted_shapes as ws
    seams = lambda L, h: [c1 for _, _, c1 in tr.tiles(L, h)[:-1]]
    for L, h in ((72, 8), (70, 8), (33, 8), (48, 8), (40, 8), (17, 8), (72, 5), (72, 1)):
        assert ws._seams(L, h) == seams(L, h), (L, h)
    assert ws._depth(70, 72) == tr.depth("weighted", 70, 72) == 8
    assert ws.REGION == tr.REGION
    for L in LENGTHS:
        for h in HALOS:
            assert ws._seams(L, h) == seams(L, h), (L, h)
    for N, M in ((70, 72), (17, 33), (40, 48), (1, 9), (9, 1), (32, 32), (33, 32)):
        for T in (1, 5, 8, 15, 32):
            assert ws._depth(N, M, T) == tr.depth("weighted", N, M, T), (N, M, T)
