"""The cases of tests/test_gpu_tile_depths.py and their numpy twins -- TEST INFRASTRUCTURE ONLY.

Shapes chosen for the geometry of the 32 x 32 tiles (tests/tiling_ref.py), the data, weights, cotangents and tangents of every
case, and one cached call into each family's own twin (unrolled_ref, weighted_unrolled_ref, sumregs_unrolled_ref, color_ref,
l1_ref, kl_ref, color_weighted_ref and the *_jvp_ref modules).  tests/test_tile_depth_margins.py checks on the CPU that no
decision of these cases is close enough to its threshold for rounding to flip it."""
import functools

import numpy as np

import color_jvp_ref as cj
import color_ref as cr
import color_weighted_ref as cw
import kl_ref as kr
import l1_kl_jvp_ref as lkj
import l1_ref as lr
import sumregs_unrolled_ref as sur
import unrolled_jvp_ref as uj
import unrolled_ref as ur
import weighted_unrolled_jvp_ref as wuj
import weighted_unrolled_ref as wur
from oracle import np_twin as tw
from oracle import np_twin_sumregs as sr

# (O, N, M).  2x70x72: middle tiles on both axes at every depth, two images (two launch chains); 2x32x32: exactly one region
# (depths up to 32, no halo); 1x33x32, 1x32x33: one pixel over on one axis, the second tile shifted back by 31; 1x49x33: a
# middle tile along j at the default depth that the last tile overlaps by 31 rows; 1x17x70: 15 out-of-image lanes per column
# in every tile, with a middle tile along i at every depth
SHAPES = [(2, 70, 72), (2, 32, 32), (1, 33, 32), (1, 32, 33), (1, 49, 33), (1, 17, 70)]
# (B, C, N, M)
COLOR_SHAPES = [(2, 3, 70, 72), (1, 2, 49, 33), (1, 4, 70, 33), (2, 2, 32, 32), (1, 2, 17, 70)]
FAMILIES = ("tv", "weighted", "sumregs", "l1", "kl")     # on SHAPES
COLOR_FAMILIES = ("color", "color_weighted")             # on COLOR_SHAPES
CASES = [(fam, sh) for fam in FAMILIES for sh in SHAPES] + [(fam, sh) for fam in COLOR_FAMILIES for sh in COLOR_SHAPES]
# the fidelity weights a family is run with.  weighted: one random plane per image; l1, kl: one plane per image in [0.5, 2]
# (wo = O) and one shared plane in {0, 1} (wo = 1: wstride 0, pixels without data); color_weighted: one plane per channel in
# [0.25, 4] and the mosaic, one channel kept per pixel
WEIGHTS = {"weighted": ("real",), "l1": ("real", "mask"), "kl": ("real", "mask"), "color_weighted": ("real", "mosaic")}
KS = (7, 50, 203)
KINDS = ("scalar", "patch", "map")
MARGIN = 1e-9     # tests/test_color_abi.py's condition on the twin's decisions
SEEDS = {}        # (family, shape, kind) -> data seed, where the default (5) leaves a decision closer than MARGIN


def case_id(case):
    return "%s-%s" % (case[0], "x".join(str(n) for n in case[1]))


def model_of(family, shape):
    """The name tests/tiling_ref.py knows the family's plan by."""
    return "%s%d" % (family, shape[1]) if family in COLOR_FAMILIES else family


def channels_of(family, shape):
    return shape[1] if family in COLOR_FAMILIES else 1


def images_of(family, shape):
    """What stats()["tiles"] counts: images, colour images for the colour models."""
    return shape[0]


def weights_of(family):
    """The weight kinds of a family; (None,) for a family without a weight."""
    return WEIGHTS.get(family, (None,))


def has_tangent(family):
    """Forward mode through the iterations: not for the sum of regularisers, nor for the weighted colour model."""
    return family in ("tv", "weighted", "color", "l1", "kl")


def _frozen(*arrays):
    for a in arrays:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return arrays


def alpha_of(family, kind, N, M):
    """color_ref.alpha_of (color_weighted_ref's too); for the sum of regularisers sumregs_unrolled_ref.alpha_of (the scalar is
    its vector); l1_ref.alpha_of and kl_ref.alpha_of for theirs."""
    if family == "sumregs":
        return sur.alpha_of("vector" if kind == "scalar" else kind, N, M)
    if family == "l1":
        return lr.alpha_of(kind, N, M)
    if family == "kl":
        return kr.alpha_of(kind, N, M)
    return cr.alpha_of(kind, N, M)


@functools.lru_cache(maxsize=None)
def data(family, shape, kind="scalar"):
    """(f, gu, df) of a case, read-only: synth_batch(planes, N, M, seed + M) as color_ref.gpu_data, a standard-normal
    cotangent and a standard-normal tangent of f.  l1: f taken off its grid of 1 / 255 by Gaussian noise of 1e-3, as
    l1_ref.gpu_data does; kl: f clipped at 0 and scaled to a peak of kl_ref.PEAK counts, Poisson samples of it over PEAK, on a
    background of kl_ref.BACKGROUND, as kl_ref.gpu_data does."""
    from conftest import synth_batch
    N, M = shape[-2:]
    planes = int(np.prod(shape[:-2]))
    seed = SEEDS.get((family, tuple(shape), kind), 5)
    _, f = synth_batch(planes, N, M, seed=seed + M)
    if family == "l1":
        f = f + 1e-3 * np.random.default_rng(45).standard_normal(f.shape)
    elif family == "kl":
        clean = np.clip(f, 0.0, None)
        clean = clean * (kr.PEAK / clean.max())
        f = np.random.default_rng(31).poisson(clean).astype(np.float64) / kr.PEAK + kr.BACKGROUND
    gu = np.random.default_rng(seed + 100).standard_normal(f.shape)
    df = np.random.default_rng(seed + 300).standard_normal(f.shape)
    return _frozen(f, gu, df)


@functools.lru_cache(maxsize=None)
def weight(family, shape, wkind="real"):
    """The weight of a case, read-only; None for a family without one.  weighted: weighted_unrolled_ref.weight_of, one random
    plane per image in [0.25, 4]; l1, kl: l1_ref.weight_of; color_weighted: color_weighted_ref.weight_of."""
    if family not in WEIGHTS:
        return None
    assert wkind in WEIGHTS[family], (family, wkind)
    if family == "weighted":
        return _frozen(wur.weight_of("real", *shape))[0]
    if family in ("l1", "kl"):
        return _frozen(lr.weight_of(wkind, *shape))[0]
    return _frozen(cw.weight_of(wkind, *shape))[0]


@functools.lru_cache(maxsize=None)
def tangents(family, shape, kind, wkind="real"):
    """(dalpha shaped like the parameter (a float for a scalar), its map (N, M), dw shaped like the weight): standard normal."""
    N, M = shape[-2:]
    if not has_tangent(family):
        return None, None, None
    rng = np.random.default_rng(311 + M)
    alpha = alpha_of(family, kind, N, M)
    da = float(rng.standard_normal()) if np.ndim(alpha) == 0 else rng.standard_normal(np.shape(alpha))
    damap = np.full((N, M), da) if np.ndim(da) == 0 else tw.alpha_to_map(da, M, N)   # (the patch upsampling is linear)
    w = weight(family, shape, wkind)
    dw = rng.standard_normal(w.shape) if w is not None else None
    return _frozen(da, damap, dw)


def forward(family, shape, kind, K, wkind="real", stats=None):
    """(u, tape, tab, maps) by the family's twin; maps: what its reverse and its margin take for the parameter.  stats: the
    dict l1_ref.fwd_tape / kl_ref.fwd_tape fill."""
    N, M = shape[-2:]
    f, _, _ = data(family, shape, kind)
    alpha = alpha_of(family, kind, N, M)
    if family == "sumregs":
        return sur.fwd_tape(f, alpha, K) + (sr.alpha_maps(alpha, M, N),)
    amap = tw.alpha_to_map(alpha, M, N)
    w = weight(family, shape, wkind)
    if family == "tv":
        return ur.fwd_tape(f, amap, K) + (amap,)
    if family == "weighted":
        return wur.fwd_tape(f, amap, w, K) + (amap,)
    if family == "l1":
        return lr.fwd_tape(f, amap, w, K, stats=stats) + (amap,)
    if family == "kl":
        return kr.fwd_tape(f, amap, w, K, stats=stats) + (amap,)
    if family == "color_weighted":
        return cw.fwd_tape(f, amap, w, K, shape[1]) + (amap,)
    return cr.fwd_tape(f, amap, K, shape[1]) + (amap,)


def margin(family, shape, kind, K, wkind="real", stats=None):
    """min |n2 - alpha^2| / alpha^2 over every pixel and iteration of the case's twin."""
    _, tape, _, maps = forward(family, shape, kind, K, wkind, stats)
    if family == "sumregs":
        return sur.min_decision_margin(tape, maps)
    if family in ("l1", "kl"):
        return lr.min_decision_margin(tape, maps)
    if family == "color_weighted":
        return cw.min_decision_margin(tape, maps, shape[1])
    return cr.min_decision_margin(tape, maps, channels_of(family, shape))   # (channels = 1: z1^2 + z2^2, the TV decision)


@functools.lru_cache(maxsize=None)
def twin(family, shape, kind, K, wkind="real"):
    """(u0, gf0, ga0, gw0) of a case by its twin (gw0: the per-pixel, per-plane terms of a weighted model, else None; ga0: the
    per-pixel terms its reduce_alpha takes), computed once and shared, read-only.  The tape is not kept."""
    f, gu, _ = data(family, shape, kind)
    u0, tape, tab, maps = forward(family, shape, kind, K, wkind)
    w = weight(family, shape, wkind)
    gw0 = None
    if family == "tv":
        gf0, ga0 = ur.reverse(gu, tape, tab, maps)
    elif family == "weighted":
        gf0, ga0, gw0 = wur.reverse(gu, tape, tab, maps, w, f)
    elif family == "sumregs":
        gf0, ga0 = sur.reverse(gu, tape, tab, maps)
    elif family == "l1":
        gf0, ga0, gw0 = lr.reverse(gu, tape, tab, maps, w, f)
    elif family == "kl":
        gf0, ga0, gw0 = kr.reverse(gu, tape, tab, maps, w, f)
    elif family == "color_weighted":
        gf0, ga0, gw0 = cw.reverse(gu, tape, tab, maps, w, f, shape[1])
    else:
        gf0, ga0 = cr.reverse(gu, tape, tab, maps, shape[1])
    return _frozen(u0, gf0, ga0, gw0)


# ---- l1: pixels without data that stay at f ----------------------------------------------------------------------------------
# On the cases above a pixel with w = 0 has x+ == f in iteration 0 only (y = 0, so div = 0 and d = 0), where nothing that the
# reverse tail or the tangent passes on through such a pixel reaches a result.  On a flat patch div stays exactly zero until the
# duals of the patch's rim have spread inwards, one pixel per iteration: the pixels without data inside it are held at f, d = 0,
# for several iterations, and the `w == 0` half of `act = x+ != f || w == 0` is what passes their adjoint and tangent on.
FLAT_SHAPE = (1, 17, 70)
FLAT_PATCH = (slice(2, 15), slice(20, 50))   # rows, columns: 13 x 30 pixels, across the seams along i
FLAT_KS = (7, 50)


@functools.lru_cache(maxsize=None)
def l1_flat_data():
    """(f, gu, df): the l1 case of 1 x 17 x 70 with FLAT_PATCH of f set to 0.5; read-only."""
    f, gu, df = data("l1", FLAT_SHAPE)
    f = f.copy()
    f[0][FLAT_PATCH] = 0.5
    return _frozen(f, gu, df)


@functools.lru_cache(maxsize=None)
def l1_flat_twin(kind, K):
    """(u0, gf0, ga0, gw0, du0, stats) by l1_ref and l1_kl_jvp_ref with the mask; stats: l1_ref.fwd_tape's, the projection's
    decision_margin, and held = the pixel-iterations k >= 1 with w == 0 and x+ == f."""
    N, M = FLAT_SHAPE[-2:]
    f, gu, df = l1_flat_data()
    w = weight("l1", FLAT_SHAPE, "mask")
    amap = tw.alpha_to_map(alpha_of("l1", kind, N, M), M, N)
    _, damap, dw = tangents("l1", FLAT_SHAPE, kind, "mask")
    stats = {}
    u0, tape, tab = lr.fwd_tape(f, amap, w, K, stats=stats)
    stats["decision_margin"] = lr.min_decision_margin(tape, amap)
    stats["held"] = int(((tape[1:, 2] == f) & (w == 0)).sum())
    gf0, ga0, gw0 = lr.reverse(gu, tape, tab, amap, w, f)
    du0 = lkj.forward_tangent("l1", f, amap, w, K, df, damap, dw)[1]
    return _frozen(u0, gf0, ga0, gw0, du0) + (stats,)


@functools.lru_cache(maxsize=None)
def twin_tangent(family, shape, kind, K, wkind="real"):
    """du0 of a case by the family's forward-mode twin, every tangent given (df, dalpha, and dw for a weighted model)."""
    N, M = shape[-2:]
    f, _, df = data(family, shape, kind)
    amap = tw.alpha_to_map(alpha_of(family, kind, N, M), M, N)
    _, damap, dw = tangents(family, shape, kind, wkind)
    w = weight(family, shape, wkind)
    if family == "tv":
        du0 = uj.forward_tangent(f, amap, K, df, damap)[1]
    elif family == "weighted":
        du0 = wuj.forward_tangent(f, amap, w, K, df, damap, dw)[1]
    elif family in ("l1", "kl"):
        du0 = lkj.forward_tangent(family, f, amap, w, K, df, damap, dw)[1]
    else:
        assert family == "color", family
        du0 = cj.forward_tangent(f, amap, K, shape[1], df, damap)[1]
    return _frozen(du0)[0]
