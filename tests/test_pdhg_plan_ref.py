"""CPU checks of tests/pdhg_plan_ref.py, the plain restatement of the plain TV solve's geometry: the table has the 36
variants of kVariants, and the shapes tests/test_gpu_pdhg_variants.py runs hold the tiles they promise -- for every
variant, at every depth, every class of tile its min_image admits.  (That the table agrees with the library is what the
GPU file asserts on every solve, from stats().)"""
import pytest

import pdhg_plan_ref as pr

ALL = sorted(pr.VARIANTS)


def test_the_table_has_the_36_variants_and_the_automatic_choices():
    assert ALL == list(range(1, 37))
    region = lambda v: (pr.VARIANTS[v].RI, pr.VARIANTS[v].RJ)
    assert region(pr.AUTO["tile32"]) == (32, 32) and pr.AUTO["tile32"] == 1
    assert region(pr.AUTO["tile48"]) == (48, 48) and pr.AUTO["tile48"] == 13
    assert region(pr.AUTO["rows64"]) == (64, 64) and pr.AUTO["rows64"] == 19
    assert region(pr.AUTO["rows48"]) == (64, 48) and pr.AUTO["rows48"] == 20
    fam = lambda name: [v for v in ALL if pr.VARIANTS[v].family == name]
    assert fam("tile") == list(range(1, 16)) and fam("wave") == [16, 17, 18] and fam("rows") == list(range(19, 30))
    assert fam("rows2") == [30, 31] and fam("stream") == [32, 33] and fam("rowsw") == [34, 35, 36]
    for v in ALL:
        V = pr.VARIANTS[v]
        assert V.lds_rows == (V.family == "tile")                       # the step-row array: pdhg_tile_kernel only
        assert V.min_image == {"tile": 0, "wave": 0, "stream": 2}.get(V.family, 1)
        assert V.tiles_per_block == (4 if V.family == "wave" else 1)
        assert (V.tmax, V.PJ) == ((8, None) if V.family == "stream" else (0, V.PJ))
    # the regions of 96 and 128 pixels the issue names
    assert [v for v in ALL if 96 in region(v) or 128 in region(v)] == [8, 9, 14, 15, 21, 23, 27, 34, 35, 36]


def test_the_depth_caps():
    assert pr.depth_cap(1, 100, 128) == 15 and pr.depth_cap(2, 100, 128) == 31 and pr.depth_cap(3, 100, 128) == 7
    assert pr.depth_cap(13, 300, 60) == 23 and pr.depth_cap(20, 300, 270) == 23 and pr.depth_cap(19, 300, 270) == 31
    assert pr.depth_cap(1, 16, 16) == pr.NO_CAP and pr.deepest(1, 16, 16) == 32 and pr.deepest(16, 32, 32) == pr.NO_CAP
    assert pr.granted(1, 16, 16, 32) == 32 and pr.granted(1, 16, 16, 33) is None        # refused, not clamped
    assert pr.granted(8, 3, 250, 40) is None and pr.granted(8, 3, 250, 32) == 32        # 128 x 16: the halo admits 63
    assert pr.granted(16, 32, 32, 40) == 40 and pr.granted(19, 64, 64, 40) == 40        # no step-row array: no cap
    assert pr.granted(32, 272, 64, 40) == 8 and pr.granted(32, 600, 200, 40) == 8       # the stream kernels' tmax
    assert pr.granted(19, 129, 65, 40) == 31 and pr.granted(20, 300, 270, 24) == 23
    assert pr.depths(19, pr.BIG, pr.BIG) == [1, 2, 8, 9, 30, 31]
    assert pr.depths(13, pr.BIG, pr.BIG) == [1, 2, 4, 8, 22, 23]
    assert pr.depths(3, pr.BIG, pr.BIG) == [1, 2, 6, 7]
    assert pr.depths(16, pr.BIG, pr.BIG) == [1, 2, 8, 14, 15] and pr.depths(16, 32, 32) == [1, 2, 8, 17]
    assert pr.depths(32, pr.BIG, pr.BIG) == [1, 2, 7, 8]
    assert pr.depths(8, 3, pr.BIG) == [1, 2, 8, 31, 32] and pr.depths(8, pr.BIG, 5) == [1, 2, 6, 7]
    assert pr.one_depths(1) == [32] and pr.one_depths(19) == [32, 40] and pr.one_depths(33) == [8]


def test_the_launch_counts():
    for T in range(2, 32):
        assert pr.chain_out_of_phase(8 * T, T)                          # what the two-chain solves of the GPU file run
        assert pr.launches(8 * T, T, 2) == (17, 2) and pr.launches(8 * T, T, 1) == (8, 1)
        assert pr.launches(8 * T, T, 2, graph=False) == (8, 1)
        assert pr.launches(2 * T + 1, T, 1) == (3, 1)
    assert not pr.chain_out_of_phase(8, 1) and pr.launches(8, 1, 2) == (16, 2)
    # tests/test_gpu_pdhg.py: 12 x 128^2, two chains
    assert [pr.launches(n, t, 2)[0] - 2 * -(-n // t) for n, t in ((96, 8), (200, 8), (120, 6), (97, 8))] == [1, 1, 1, 0]


def test_the_automatic_choice_on_long_images():
    assert pr.auto_variant(300, 60, 1) == 13 and pr.auto_variant(60, 300, 1) == 13      # narrower than a rows region
    assert pr.auto_variant(300, 270, 2) == 20 and pr.auto_variant(300, 270, 2, ncu=32) == 19
    assert pr.auto_variant(1024, 1024, 8) == 19                                        # tests/test_gpu_pdhg.py: 8 x 21 x 21 tiles
    assert pr.plan(19, 1024, 1024, 8, 8) == (64, 64, 8 * 21 * 21) and pr.plan(13, 1024, 1024, 8, 8)[2] == 8 * 32 * 32


@pytest.mark.parametrize("v", ALL)
def test_every_variant_reaches_every_tile_class_its_min_image_admits(v):
    V = pr.VARIANTS[v]
    cs = pr.cases(v)
    multi = pr.depths(v, pr.BIG, pr.BIG)                # both axes tiled
    assert multi[-1] == min(x for x in ((V.RI - 1) // 2, (V.RJ - 1) // 2, V.tmax or 99)) and multi[0] == 1
    seen = {}
    for T, cls, (N, M) in cs:
        assert not pr.too_small(v, N, M), (T, cls, N, M)
        assert pr.granted(v, N, M, T) == T, (T, cls, N, M)              # the depth runs as asked: neither clamped nor refused
        ax = {}
        for name, L, R in (("j", N, V.RJ), ("i", M, V.RI)):
            t = pr.tiles(L, T, R)
            assert t[0][1] == 0 and t[-1][2] == L and all(a[2] == b[1] for a, b in zip(t, t[1:]))   # the cores partition the axis
            assert all(c0 < c1 for _, c0, c1 in t)
            for o, c0, c1 in t:                                         # T pixels between the core and a region edge inside the image
                assert 0 <= o and o + min(L, R) <= L and (o == 0 or c0 - o >= T) and (o + R >= L or o + R - c1 >= T)
            ax[name] = pr.tile_classes(L, R, T)
            if len(t) > 1:
                assert t[-1][0] == L - R
        S = {"j": V.RJ - 2 * T, "i": V.RI - 2 * T}
        kinds = sorted((len(pr.tiles(L, T, R)), ax[a][1]) for a, L, R in (("j", N, V.RJ), ("i", M, V.RI)))
        if cls == "shift":      # two tiles and three, each last one pulled back as far as it goes
            assert sorted(kinds) == sorted([(2, S["i" if M == V.RI + 1 else "j"] - 1), (3, S["j" if M == V.RI + 1 else "i"] - 1)]), (T, N, M, kinds)
            assert "interior" in ax["j" if M == V.RI + 1 else "i"][0]
            seen.setdefault(T, set()).add("shift-i" if M == V.RI + 1 else "shift-j")
        elif cls == "fit":      # two tiles on both axes, the last where the stride puts it
            assert kinds == [(2, 0), (2, 0)], (T, N, M, kinds)
            seen.setdefault(T, set()).add("fit")
        elif cls == "one":
            assert (N, M) == (V.RJ, V.RI) and ax["i"][0] == ax["j"][0] == {"single"}
            seen.setdefault(T, set()).add("one")
        else:
            assert cls == "narrow" and (N < V.RJ or M < V.RI)
            assert "single" in ax["i"][0] or "single" in ax["j"][0]
            tag = "narrow-1" if (N < V.RJ and M < V.RI) else ("narrow-j" if M < V.RI else "narrow-i")   # the tiled axis
            if tag != "narrow-1":
                a = tag[-1]
                assert "interior" in ax[a][0] and ax[a][1] == S[a] - 1, (T, N, M)
            seen.setdefault(T, set()).add(tag)
    # every class at every depth of its own geometry: which axes are tiled decides how deep the halo may go
    want = {"shift-i": multi, "shift-j": multi, "fit": multi,
            "one": sorted(set(pr.depths(v, V.RJ, V.RI)) | set(pr.one_depths(v)))}
    if V.min_image == 0:
        want.update({"narrow-i": pr.depths(v, 3, pr.BIG), "narrow-j": pr.depths(v, pr.BIG, 5), "narrow-1": want["one"]})
        assert want["narrow-i"][-1] == min((V.RI - 1) // 2, 32) and want["narrow-j"][-1] == min((V.RJ - 1) // 2, 32)
    elif V.min_image == 2:
        want["narrow-i"] = pr.depths(v, 3, pr.BIG)
    got = {k: sorted(T for T in seen if k in seen[T]) for k in set().union(*seen.values())}
    assert got == want, (got, want)
    # the single tile also at the depth of the step-row array, and beyond it where there is none
    assert pr.one_depths(v) == ([32] if V.lds_rows else [8] if V.family == "stream" else [32, 40])
    assert len(cs) <= 60, len(cs)
