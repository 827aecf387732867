"""The cases of tests/test_gpu_tile_depths.py and their numpy twins -- TEST INFRASTRUCTURE ONLY.

Shapes chosen for the geometry of the 32 x 32 tiles (tests/tiling_ref.py), the data, cotangents and tangents of every case,
and one cached call into each family's own twin (unrolled_ref, weighted_unrolled_ref, sumregs_unrolled_ref, color_ref and
the *_jvp_ref modules).  tests/test_tile_depth_margins.py checks on the CPU that no projection decision of these cases is
close enough to its threshold for rounding to flip it."""
import functools

import numpy as np

import color_jvp_ref as cj
import color_ref as cr
import sumregs_unrolled_ref as sur
import unrolled_jvp_ref as uj
import unrolled_ref as ur
import weighted_unrolled_jvp_ref as wuj
import weighted_unrolled_ref as wur
from oracle import np_twin as tw
from oracle import np_twin_sumregs as sr

# (O, N, M).  2x70x72: middle tiles on both axes at every depth, two images (two launch chains); 2x32x32: exactly one region
# (depths up to 32, no halo); 1x33x32, 1x32x33: one pixel over on one axis, the second tile shifted back by 31; 1x49x33: a
# middle tile along j at the default depth that the last tile overlaps by 31 rows
SHAPES = [(2, 70, 72), (2, 32, 32), (1, 33, 32), (1, 32, 33), (1, 49, 33)]
# (B, C, N, M)
COLOR_SHAPES = [(2, 3, 70, 72), (1, 2, 49, 33), (1, 4, 70, 33), (2, 2, 32, 32)]
FAMILIES = ("tv", "weighted", "sumregs")
CASES = [(fam, sh) for fam in FAMILIES for sh in SHAPES] + [("color", sh) for sh in COLOR_SHAPES]
KS = (7, 50, 203)
KINDS = ("scalar", "patch", "map")
MARGIN = 1e-9     # tests/test_color_abi.py's condition on the twin's decisions
SEEDS = {}        # (family, shape, kind) -> data seed, where the default (5) leaves a decision closer than MARGIN


def case_id(case):
    return "%s-%s" % (case[0], "x".join(str(n) for n in case[1]))


def model_of(family, shape):
    """The name tests/tiling_ref.py knows the family's plan by."""
    return "color%d" % shape[1] if family == "color" else family


def channels_of(family, shape):
    return shape[1] if family == "color" else 1


def images_of(family, shape):
    """What stats()["tiles"] counts: images, colour images for the colour model."""
    return shape[0]


def _frozen(*arrays):
    for a in arrays:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return arrays


def alpha_of(family, kind, N, M):
    """color_ref.alpha_of; for the sum of regularisers sumregs_unrolled_ref.alpha_of (the scalar is its vector)."""
    if family == "sumregs":
        return sur.alpha_of("vector" if kind == "scalar" else kind, N, M)
    return cr.alpha_of(kind, N, M)


@functools.lru_cache(maxsize=None)
def data(family, shape, kind="scalar"):
    """(f, gu, df) of a case, read-only: synth_batch(planes, N, M, seed + M) as color_ref.gpu_data, a standard-normal
    cotangent and a standard-normal tangent of f."""
    from conftest import synth_batch
    N, M = shape[-2:]
    planes = int(np.prod(shape[:-2]))
    seed = SEEDS.get((family, tuple(shape), kind), 5)
    _, f = synth_batch(planes, N, M, seed=seed + M)
    gu = np.random.default_rng(seed + 100).standard_normal(f.shape)
    df = np.random.default_rng(seed + 300).standard_normal(f.shape)
    return _frozen(f, gu, df)


@functools.lru_cache(maxsize=None)
def weight(shape):
    """One random plane per image in [0.25, 4]: weighted_unrolled_ref.weight_of."""
    return _frozen(wur.weight_of("real", *shape))[0]


@functools.lru_cache(maxsize=None)
def tangents(family, shape, kind):
    """(dalpha shaped like the parameter (a float for a scalar), its map (N, M), dw shaped like the weight): standard normal."""
    N, M = shape[-2:]
    if family == "sumregs":          # (no forward mode through its iterations)
        return None, None, None
    rng = np.random.default_rng(311 + M)
    alpha = alpha_of(family, kind, N, M)
    da = float(rng.standard_normal()) if np.ndim(alpha) == 0 else rng.standard_normal(np.shape(alpha))
    damap = np.full((N, M), da) if np.ndim(da) == 0 else tw.alpha_to_map(da, M, N)   # (the patch upsampling is linear)
    dw = rng.standard_normal(shape) if family == "weighted" else None
    return _frozen(da, damap, dw)


def forward(family, shape, kind, K):
    """(u, tape, tab, maps) by the family's twin; maps: what its reverse and its margin take for the parameter."""
    N, M = shape[-2:]
    f, _, _ = data(family, shape, kind)
    alpha = alpha_of(family, kind, N, M)
    if family == "sumregs":
        return sur.fwd_tape(f, alpha, K) + (sr.alpha_maps(alpha, M, N),)
    amap = tw.alpha_to_map(alpha, M, N)
    if family == "tv":
        return ur.fwd_tape(f, amap, K) + (amap,)
    if family == "weighted":
        return wur.fwd_tape(f, amap, weight(shape), K) + (amap,)
    return cr.fwd_tape(f, amap, K, shape[1]) + (amap,)


def margin(family, shape, kind, K):
    """min |n2 - alpha^2| / alpha^2 over every pixel and iteration of the case's twin."""
    _, tape, _, maps = forward(family, shape, kind, K)
    if family == "sumregs":
        return sur.min_decision_margin(tape, maps)
    return cr.min_decision_margin(tape, maps, channels_of(family, shape))   # (channels = 1: z1^2 + z2^2, the TV decision)


@functools.lru_cache(maxsize=None)
def twin(family, shape, kind, K):
    """(u0, gf0, ga0, gw0) of a case by its twin (gw0: the weighted model's, else None; ga0: the per-pixel terms its
    reduce_alpha takes), computed once and shared, read-only.  The tape is not kept."""
    f, gu, _ = data(family, shape, kind)
    u0, tape, tab, maps = forward(family, shape, kind, K)
    gw0 = None
    if family == "tv":
        gf0, ga0 = ur.reverse(gu, tape, tab, maps)
    elif family == "weighted":
        gf0, ga0, gw0 = wur.reverse(gu, tape, tab, maps, weight(shape), f)
    elif family == "sumregs":
        gf0, ga0 = sur.reverse(gu, tape, tab, maps)
    else:
        gf0, ga0 = cr.reverse(gu, tape, tab, maps, shape[1])
    return _frozen(u0, gf0, ga0, gw0)


@functools.lru_cache(maxsize=None)
def twin_tangent(family, shape, kind, K):
    """du0 of a case by the family's forward-mode twin, every tangent given (df, dalpha, and dw for the weighted model)."""
    N, M = shape[-2:]
    f, _, df = data(family, shape, kind)
    amap = tw.alpha_to_map(alpha_of(family, kind, N, M), M, N)
    _, damap, dw = tangents(family, shape, kind)
    if family == "tv":
        du0 = uj.forward_tangent(f, amap, K, df, damap)[1]
    elif family == "weighted":
        du0 = wuj.forward_tangent(f, amap, weight(shape), K, df, damap, dw)[1]
    else:
        du0 = cj.forward_tangent(f, amap, K, shape[1], df, damap)[1]
    return _frozen(du0)[0]
