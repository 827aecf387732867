"""oracle/taped_oracle.c pinned on the CPU before it pins the taped tile kernels.

* its tv forward is oracle.pdhg bit for bit, and its weighted forward with w == 1.0 is the same bits again: the fma order;
* on the twins' own tie-free cases its u, tape, du, grad_f, grad_alpha and grad_w agree with the numpy twins within the bounds the
  twins' families are held to (imported, not retyped);
* its reverse reads nothing but the tape it is given, and its tangent and reverse are transposes of each other;
* the data of tests/tie_data.py sit on the decisions they were made for: the oracle's own counters say so, class by class."""
import numpy as np
import pytest

import kl_ref as kr
import l1_kl_jvp_ref as lkj
import l1_ref as lr
import tie_data as ti
import unrolled_jvp_ref as uj
import unrolled_ref as ur
import weighted_unrolled_jvp_ref as wuj
import weighted_unrolled_ref as wur
from oracle import c_oracle as co
from oracle import np_twin as tw
from test_gpu_color import U_CAP                                     # 1e-13: u (and here the tape) against a numpy twin
from test_gpu_kl import _bounds as _kl_bounds
from test_gpu_l1 import _bounds as _l1_bounds
from test_gpu_unrolled import _bounds as _tv_bounds
from test_gpu_weighted_unrolled import _bounds as _weighted_bounds

RTOL = wuj.UNIT_WEIGHT_RTOL                                          # 1e-11: every tangent and transpose bound of the project
TWIN_NAMES = ("2x17x33", "1x1x9", "1x9x1")
TWIN_K = 50


def _same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b))


def _dev(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max())


# ---- 1. the fma order ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ti.SHAPES + [(1, 1, 9), (1, 9, 1)], ids=ti.shape_id)
def test_the_tv_forward_is_the_plain_oracle_s_bits_and_so_is_the_weighted_one_at_unit_weight(oracle, shape):
    O, N, M = shape
    f = ti.blocks8(tuple(shape))
    for kind in ti.kinds_of("tv"):
        alpha = ti.alpha_of("tv", kind, N, M)
        amap = tw.alpha_to_map(alpha, M, N)
        for K in ti.KS:
            u0, y1, y2 = oracle.pdhg(f, alpha, maxiter=K, return_dual=True)
            u, tape, _ = co.taped_forward("tv", f, amap, None, K)
            assert _same(u, u0), (kind, K)
            n2 = tape[K - 1, 0] ** 2 + tape[K - 1, 1] ** 2
            inside = n2 < 0.99 * amap * amap                         # clearly inside the ball: y is the taped z itself
            assert _same(tape[K - 1, 0][inside], y1[inside]) and _same(tape[K - 1, 1][inside], y2[inside])
            for w in (np.ones((N, M)), np.ones(shape)):
                uw, tw_, _ = co.taped_forward("weighted", f, amap, w, K)
                assert _same(uw, u0) and _same(tw_[:, :2], tape), (kind, K, w.ndim)
                assert _same(tw_[K - 1, 2], u0)
    # the three step tables: gamma = 1 is bplo_step_table's, gamma = 0 has omega = 1 and constant steps
    assert _same(co.taped_step_table("tv", None, 50), oracle.step_table(50))
    assert _same(co.taped_step_table("weighted", np.ones((N, M)), 50), oracle.step_table(50))
    flat = co.taped_step_table("l1", None, 50)
    assert _same(flat, co.taped_step_table("kl", None, 50)) and _same(flat, np.tile(flat[:1], (50, 1))) and flat[0, 2] == 1.0


# ---- 2. against the twins, on their own tie-free cases --------------------------------------------------------------------------
def _twin_case(model, name, kind, wkind):
    """(f, gu, alpha, amap, w) of a family's own case."""
    O, N, M = wur.GPU_SHAPES[name]
    if model in ("l1", "kl"):
        return lkj.case(model, name, kind, wkind)
    f, gu = wur.gpu_data(name)
    alpha = wur.alpha_of(kind, N, M)
    return f, gu, alpha, tw.alpha_to_map(alpha, M, N), (wur.weight_of(wkind, O, N, M) if model == "weighted" else None)


def _twin(model, f, amap, w, K, gu, df, dam, dw):
    """(u0, tape0, gf0, ga0, gw0, du0) by the family's numpy twins."""
    if model == "tv":
        u0, tape0, tab = ur.fwd_tape(f, amap, K)
        return (u0, tape0) + ur.reverse(gu, tape0, tab, amap) + (None, uj.forward_tangent(f, amap, K, df, dam)[1])
    if model == "weighted":
        u0, tape0, tab = wur.fwd_tape(f, amap, w, K)
        return (u0, tape0) + wur.reverse(gu, tape0, tab, amap, w, f) + (wuj.forward_tangent(f, amap, w, K, df, dam, dw)[1],)
    ref = lkj.REF[model]
    u0, tape0, tab = ref.fwd_tape(f, amap, w, K)
    return (u0, tape0) + ref.reverse(gu, tape0, tab, amap, w, f) + (lkj.forward_tangent(model, f, amap, w, K, df, dam, dw)[1],)


def _gradient_bounds(model, gf0, ga0, gw0, alpha, w, O, N, M):
    if model == "tv":
        return _tv_bounds(gf0, ga0, alpha, O, N, M) + (None,)
    return {"weighted": _weighted_bounds, "l1": _l1_bounds, "kl": _kl_bounds}[model](gf0, ga0, gw0, alpha, w, O, N, M)


@pytest.mark.parametrize("name", TWIN_NAMES)
@pytest.mark.parametrize("model", ti.MODELS)
def test_the_oracle_agrees_with_the_twins_on_their_own_cases(model, name):
    """u and the tape within U_CAP, the gradients within the family's _bounds, the tangent within RTOL * max|ref|.  The oracle
    fuses what the header comment fuses and the twins fuse nothing: the difference is the rounding of a few fma per iteration."""
    O, N, M = wur.GPU_SHAPES[name]
    worst = {}
    for wkind in (("real", "mask") if model == "weighted" else lr.WEIGHTS if model in ("l1", "kl") else (None,)):
        for kind in lr.KINDS:
            f, gu, alpha, amap, w = _twin_case(model, name, kind, wkind)
            df, _, dam, dw = ti.directions((O, N, M), w, alpha)
            u0, tape0, gf0, ga0, gw0, du0 = _twin(model, f, amap, w, TWIN_K, gu, df, dam, dw)
            u, tape, _ = co.taped_forward(model, f, amap, w, TWIN_K)
            gf, ga, gw = co.taped_reverse(model, tape, f, amap, w, gu)
            du, ut = co.taped_tangent(model, f, amap, w, TWIN_K, df, dam, dw)
            assert _same(ut, u)
            bf, ba, bw = _gradient_bounds(model, gf0, ga0, gw0, alpha, w, O, N, M)
            rows = [("u", _dev(u, u0), U_CAP), ("tape", _dev(tape, tape0), U_CAP), ("grad_f", _dev(gf, gf0), bf),
                    ("grad_alpha", _dev(ur.reduce_alpha(ga, alpha), ur.reduce_alpha(ga0, alpha)), ba),
                    ("du", _dev(du, du0), RTOL * float(np.abs(du0).max()))]
            if w is not None:
                rows.append(("grad_w", _dev(wur.reduce_w(gw, w), wur.reduce_w(gw0, w)), bw))
            for what, d, b in rows:
                assert d <= b, (kind, wkind, what, d, b)
                if b > 0:
                    worst[what] = max(worst.get(what, 0.0), d / b)
    print("%s %s: largest share of the bound: %s" % (model, name, "  ".join("%s %.4f" % kv for kv in sorted(worst.items()))))


# ---- 3. self-consistency ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", ti.MODELS)
def test_the_reverse_reads_the_tape_it_is_given_and_transposes_the_tangent(model):
    name, kind = "2x17x33", "map"
    O, N, M = wur.GPU_SHAPES[name]
    f, gu, alpha, amap, w = _twin_case(model, name, kind, "mask" if model != "tv" else None)
    df, _, dam, dw = ti.directions((O, N, M), w, alpha)
    u, tape, _ = co.taped_forward(model, f, amap, w, TWIN_K)
    g = co.taped_reverse(model, tape, f, amap, w, gu)
    g2 = co.taped_reverse(model, tape.copy(), f.copy(), amap.copy(), None if w is None else w.copy(), gu.copy())
    assert all(_same(a, b) for a, b in zip(g[:2 if w is None else 3], g2))
    other = tape.copy()
    other[TWIN_K // 2] *= 1.5                                         # another tape, other gradients: it is read
    assert not _same(co.taped_reverse(model, other, f, amap, w, gu)[0], g[0])
    du, _ = co.taped_tangent(model, f, amap, w, TWIN_K, df, dam, dw)
    gf, ga, gw = g
    lhs = float((du * gu).sum())
    rhs = float((df * gf).sum()) + float((dam * ga.sum(axis=0)).sum())
    if w is not None:
        rhs += float((dw * wur.reduce_w(gw, w)).sum())
    scale = float(np.abs(du * gu).sum())
    print("%s: <du, gu> %.12g  transposed %.12g  |difference| %.2e (bound %.2e)" % (model, lhs, rhs, abs(lhs - rhs), RTOL * scale))
    assert scale > 0.0 and abs(lhs - rhs) <= RTOL * scale
    # each tangent alone adds up to all of them: the sweep is linear
    parts = [co.taped_tangent(model, f, amap, w, TWIN_K, *t)[0] for t in ((df, None, None), (None, dam, None))]
    if w is not None:
        parts.append(co.taped_tangent(model, f, amap, w, TWIN_K, None, None, dw)[0])
    assert _dev(sum(parts), du) <= RTOL * float(np.abs(du).max())


# ---- 4. the tie data sit on the decisions ---------------------------------------------------------------------------------------
# the classes of co.TAPED_COUNTERS a model's natural and engineered cases must reach.  l1's "let_through_but_x_eq_f" (m > 0 but
# f + m == f) needs 0 < m < ulp(f) / 2, which no natural data here produce: tie_data.l1_rounds_back engineers it
NEEDED = {"tv": ("n2_tie", "n2_zero_beside_projected"), "weighted": ("n2_tie", "n2_zero_beside_projected"),
          "l1": ("m0_w_pos", "m0_w0_first", "m0_w0_later", "n2_tie", "n2_zero_beside_projected", "let_through_but_x_eq_f",
                 "x_eq_f_w0_later"),
          "kl": ("n2_tie", "n2_zero_beside_projected", "x_zero", "D_zero")}
EDGE_WEIGHT = {"tv": None, "weighted": "columns", "l1": "columns/64", "kl": "columns"}


def edge_case(model):
    """(f, amap, w) of the engineered projection tie."""
    w = ti.weight(EDGE_WEIGHT[model], ti.EDGE_SHAPE)
    return ti.step_edge(), ti.edge_alpha(model, w, ti.SCALARS[model][0]), w


@pytest.mark.parametrize("model", ti.MODELS)
def test_every_class_of_tie_is_reached(model):
    K = ti.KS[-1]
    total = dict.fromkeys(co.TAPED_COUNTERS, 0)
    for shape in ti.SHAPES:
        O, N, M = shape
        for dclass, kind, wkind in ti.cases(model, shape):
            f, alpha, amap, w = ti.case(model, shape, dclass, kind, wkind)
            u, tape, c = co.taped_forward(model, f, amap, w, K)
            assert np.isfinite(u).all()
            print("%s %s %s %s %s: %s" % (model, ti.shape_id(shape), dclass, kind, wkind, "  ".join("%s %d" % (k, c[k]) for k in co.TAPED_COUNTERS if c[k])))
            for k in c:
                total[k] += c[k]
            if model == "l1" and wkind == "mask":                    # every pixel without data: d = 0 exactly in iteration 0
                assert c["m0_w0_first"] == O * int((w == 0).sum()) > 0
            if dclass == "flat":                                      # no dual ever leaves the ball: no parameter gradient is passed
                assert not (tape[:, 0] ** 2 + tape[:, 1] ** 2 > 0.5 * amap * amap).any() and _dev(u, f) <= U_CAP
            if model == "kl" and shape == (2, 17, 33) and dclass == "counts" and wkind == "mask":
                assert _same(f, kr.poisson_data("2x17x33")[1])
                assert c["x_zero"] >= 100 and int((u == 0).sum()) > 0
                if kind == ti.SCALARS["kl"][0]:
                    assert c["x_zero"] == 761                        # the oracle's own count; the twin without fma counts the same
    f, amap, w = edge_case(model)
    _, tape, c = co.taped_forward(model, f, amap, w, K)
    print("%s edge: %s" % (model, "  ".join("%s %d" % (k, c[k]) for k in co.TAPED_COUNTERS if c[k])))
    assert c["n2_tie_first"] == ti.EDGE_SHAPE[1] == int(ti.edge_pixels().sum())
    n2 = tape[0, 1] * tape[0, 1] + tape[0, 0] * tape[0, 0]
    assert _same((n2 == amap * amap)[0], ti.edge_pixels())
    if model == "l1":                                                 # sigma_0 * h, sigma_0 read off the step table; and the case is
        assert not _same(co.taped_forward(model, f, amap, w, ti.KS[1])[0], f)   # alive: the threshold lets the edge's neighbours through
        assert _same(amap[ti.edge_pixels()], np.full(ti.EDGE_SHAPE[1], co.taped_step_table("l1", w, 1)[0, 1] * ti.EDGE_H))
        assert _same(np.abs(tape[0, 0, 0])[ti.edge_pixels()], amap[ti.edge_pixels()])
    for k in c:
        total[k] += c[k]
    if model == "l1":                                                 # the engineered step that is let through and rounds back to f
        f, w, pixels = ti.l1_rounds_back()
        amap = np.full(ti.ROUND_SHAPE[1:], ti.ROUND_ALPHA)
        for K in (ti.ROUND_K,) + ti.KS[1:]:
            _, tape, c = co.taped_forward(model, f, amap, w, K)
            assert c["let_through_but_x_eq_f"] == ti.ROUND_PIXELS == len(pixels), (K, c)
        print("%s rounds back: %s at %s, w %s" % (model, "  ".join("%s %d" % (k, c[k]) for k in co.TAPED_COUNTERS if c[k]), pixels,
                                                  [float(w[p]) for p in pixels]))
        _, tape, _ = co.taped_forward(model, f, amap, w, ti.ROUND_K)
        moved = tape[1, 2, 0] != f[0]
        assert not any(moved[p] for p in pixels) and all(0.0 < w[p] < 1.0 for p in pixels) and moved.sum() > 10 * len(pixels)
        one = w.copy()                                                # one ulp less weight on the first of them: it moves
        one[pixels[0]] = np.nextafter(one[pixels[0]], 0.0) - 2.0 ** -50
        assert co.taped_forward(model, f, amap, one, ti.ROUND_K)[1][1, 2, 0][pixels[0]] != f[0][pixels[0]]
        for k in c:
            total[k] += c[k]
    print("%s total: %s" % (model, "  ".join("%s %d" % (k, total[k]) for k in co.TAPED_COUNTERS)))
    for k in NEEDED[model]:
        assert total[k] > 0, k
