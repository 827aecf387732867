"""Data that sit ON the decisions of the taped tile kernels -- TEST INFRASTRUCTURE ONLY.

The twins' own cases (l1_ref.gpu_data, kl_ref.gpu_data, tile_depth_ref.data) are built to stay clear of every decision, because a
numpy twin without fma cannot be compared across one.  oracle/taped_oracle.c repeats the kernels' fma sequence, so these makers
do the opposite: 8-bit images with salt-and-pepper noise, {0, 1} masks, dyadic weights, a step edge whose dual lands exactly on
the ball, a constant plane, and photon counts with zeros.  Everything is deterministic (fixed seeds) and read-only.  Arrays follow
np_twin: batches are (O, N, M), a parameter map is (N, M), a weight is (N, M) or (O, N, M)."""
import functools

import numpy as np

import kl_ref as kr
from oracle import c_oracle as co
from oracle import np_twin as tw

# (O, N, M): two images and two launch chains on one region; exactly one region; a second tile pulled back by 31 pixels; 15
# out-of-image lanes per column beside an interior tile (tests/tile_depth_ref.py)
SHAPES = [(2, 17, 33), (2, 32, 32), (1, 33, 32), (1, 17, 70)]
KS = (1, 7, 50)
MODELS = ("tv", "weighted", "l1", "kl")
EDGE_SHAPE = (1, 17, 33)
EDGE_COLUMN, EDGE_LOW, EDGE_H = 16, 0.25, 0.5     # f = 0.25 on columns 0 ... 16 and 0.75 from column 17 on: all dyadic


def shape_id(shape):
    return "x".join(str(n) for n in shape)


def _frozen(*arrays):
    for a in arrays:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


# ---- images ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def blocks8(shape):
    """8-bit block images: blocks of 4 ... 9 pixels a side with grey levels k / 255, then 10 % salt (1.0) and 10 % pepper (0.0).
    Flat block interiors (G f = 0 exactly), values on the grid on which the threshold and the differences cancel exactly."""
    O, N, M = shape
    rng = np.random.default_rng(61 + M)
    f = np.empty(shape)
    for k in range(O):
        bj, bi = int(rng.integers(4, 10)), int(rng.integers(4, 10))
        levels = rng.integers(0, 256, size=(N // bj + 1, M // bi + 1))
        f[k] = np.kron(levels, np.ones((bj, bi)))[:N, :M] / 255.0
    r = rng.random(shape)
    f[r < 0.1] = 1.0
    f[r > 0.9] = 0.0
    return _frozen(f)


@functools.lru_cache(maxsize=None)
def constant(shape):
    """A constant plane, 0.5: no dual ever moves, n2 == 0 everywhere, and no parameter gradient is passed."""
    return _frozen(np.full(shape, 0.5))


@functools.lru_cache(maxsize=None)
def counts(shape):
    """kl_ref.poisson_data's raw counts over PEAK (no background: zeros stay zeros) by the same recipe at any shape."""
    from conftest import synth_batch
    O, N, M = shape
    _, f = synth_batch(O, N, M, seed=5 + M)
    clean = np.clip(f, 0.0, None)
    clean = clean * (kr.PEAK / clean.max())
    return _frozen(np.random.default_rng(31).poisson(clean).astype(np.float64) / kr.PEAK)


@functools.lru_cache(maxsize=None)
def step_edge():
    """1 x 17 x 33: EDGE_LOW up to column EDGE_COLUMN, EDGE_LOW + EDGE_H beyond, constant along the rows."""
    f = np.full(EDGE_SHAPE, EDGE_LOW)
    f[..., EDGE_COLUMN + 1:] = EDGE_LOW + EDGE_H
    return _frozen(f)


def edge_pixels():
    """The N pixels whose forward difference along i crosses the edge: a boolean (N, M) map."""
    m = np.zeros(EDGE_SHAPE[1:], dtype=bool)
    m[:, EDGE_COLUMN] = True
    return m


def edge_alpha(model, w, base):
    """The parameter map that puts the edge pixels' dual of iteration 0 exactly on the ball: `base` everywhere, and on the edge
    column the dual itself.  In iteration 0 y = 0, so z there does not depend on the parameter.  For l1 the first primal step
    returns f exactly (d = 0) and xbar = f, so z1 = sigma_0 * h with sigma_0 read off the step table; the quadratic models and kl
    round in their first primal step, and their z1 is read off a one-iteration run of the oracle."""
    f = step_edge()
    N, M = EDGE_SHAPE[1:]
    amap = np.full((N, M), float(base))
    if model == "l1":
        amap[edge_pixels()] = co.taped_step_table("l1", w, 1)[0, 1] * EDGE_H
    else:
        _, tape, _ = co.taped_forward(model, f, amap, w, 1, counters=False)
        assert not tape[0, 1].any()           # constant along j: n2 = z1^2
        amap[edge_pixels()] = np.abs(tape[0, 0, 0])[edge_pixels()]
    return amap


# ---- l1: a step the threshold lets through that rounds back to f ------------------------------------------------------------------
ROUND_SHAPE, ROUND_ALPHA, ROUND_W, ROUND_K, ROUND_PIXELS = (1, 17, 33), 0.125, 2.0 ** -6, 2, 5


@functools.lru_cache(maxsize=None)
def l1_rounds_back():
    """(f, w, pixels): the 8-bit block image of ROUND_SHAPE and a weight, ROUND_W (small enough for a third of the image to move) except at ROUND_PIXELS pixels, at which iteration 1 has
    m > 0 and yet f + copysign(m, d) == f (0 < m < ulp(f) / 2): the forward lets the step through, and act, which reads x+, calls
    the pixel held.  With w > 0 everywhere iteration 0 holds every pixel at f (d = 0), so d of iteration 1 at a pixel does not
    depend on that pixel's weight, and the pixels are engineered one after the other, each against the oracle itself: bisect w
    between "x+ != f" and "x+ == f" (m changes sign there), then step upward ulp by ulp from the last weight that moved the
    pixel until the oracle counts one more step of this class.  Nothing is typed in.  pixels: [(row, column)]."""
    f = blocks8(ROUND_SHAPE)
    O, N, M = ROUND_SHAPE
    amap = np.full((N, M), ROUND_ALPHA)
    w = np.full((N, M), ROUND_W)

    def run(wt):
        _, tape, c = co.taped_forward("l1", f, amap, wt, ROUND_K)
        return tape[1, 2, 0], c["let_through_but_x_eq_f"]

    probe = np.full((N, M), 2.0 ** -20)              # (next to no threshold: which pixels move in iteration 1 at all)
    moved = run(probe)[0] != f[0]
    pixels = []
    for n, m in zip(*np.nonzero(moved & (f[0] >= 0.5))):      # (f in [0.5, 1]: the widest ulp, dozens of weights per pixel)
        if len(pixels) == ROUND_PIXELS:
            break
        lo, hi, wt = 2.0 ** -20, 1.0, w.copy()          # lo moves the pixel, hi holds it
        while np.nextafter(lo, hi) < hi:
            wt[n, m] = mid = 0.5 * (lo + hi)
            if run(wt)[0][n, m] != f[0, n, m]:
                lo = mid
            else:
                hi = mid
        for _ in range(256):
            lo = np.nextafter(lo, 1.0)
            wt[n, m] = lo
            x, count = run(wt)
            if count == len(pixels) + 1 and x[n, m] == f[0, n, m]:
                w, pixels = wt, pixels + [(int(n), int(m))]
                break
            if count != len(pixels):                 # (held by m <= 0 already: no weight of this class at this pixel)
                break
    assert len(pixels) == ROUND_PIXELS, pixels
    return _frozen(f, w) + (pixels,)


# ---- weights ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def weight(wkind, shape):
    """mask: one plane in {0, 1}, about 30 % zeros (l1_ref.weight_of's); dyadic: one plane per image, multiples of 1 / 8 in
    [0.5, 2]; columns: one such plane that varies along i only (columns/64: that over 64); ones: one plane; None for a model without a weight."""
    O, N, M = shape
    if wkind is None:
        return None
    if wkind == "mask":
        return _frozen((np.random.default_rng(12).random((N, M)) > 0.3).astype(np.float64))
    if wkind == "dyadic":
        return _frozen(np.random.default_rng(13).integers(4, 17, size=shape) / 8.0)
    if wkind == "columns/64":               # (small enough for the l1 threshold to let the edge's neighbours through)
        return _frozen(weight("columns", shape) / 64.0)
    if wkind == "columns":                  # (the step edge's: constant along the rows, as the image is)
        return _frozen(np.ascontiguousarray(np.broadcast_to(np.random.default_rng(13).integers(4, 17, size=M) / 8.0, (N, M))))
    assert wkind == "ones", wkind
    return _frozen(np.ones((N, M)))


# ---- parameters: on dyadic grids ------------------------------------------------------------------------------------------------
SCALARS = {"tv": (0.0625,), "weighted": (0.0625,), "l1": (0.5, 1.0), "kl": (0.15,)}
_UNIT = {"tv": 1.0 / 64, "weighted": 1.0 / 64, "l1": 1.0 / 8, "kl": 1.0 / 32}      # patch and map entries: 3 ... 8 units


def alpha_of(model, kind, N, M):
    """kind: a float (the scalar itself), "patch" (2 x 3, cut down on a single row / column) or "map"; multiples of the model's
    unit, around its scalar."""
    if not isinstance(kind, str):
        return float(kind)
    if kind == "patch":
        return (_UNIT[model] * np.array([[4, 8, 5], [7, 3, 6]], dtype=np.float64))[:min(2, N), :min(3, M)].copy()
    assert kind == "map", kind
    return _UNIT[model] * np.random.default_rng(8).integers(3, 9, size=(N, M)).astype(np.float64)


def kinds_of(model):
    return SCALARS[model] + ("patch", "map")


# ---- cotangents and tangents: the families' existing ones --------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def cotangent(shape):
    """weighted_unrolled_ref.gpu_data's gu."""
    return _frozen(np.random.default_rng(105).standard_normal(shape))


def directions(shape, w, alpha):
    """(df, dalpha, dam, dw) as l1_kl_jvp_ref.tangents_of draws them: standard normal, in the shapes of f, of the parameter (dam:
    its map) and of w (None without one)."""
    O, N, M = shape
    df = np.random.default_rng(305).standard_normal(shape)
    dw = np.random.default_rng(306).standard_normal(np.shape(w)) if w is not None else None
    g = np.random.default_rng(11).standard_normal(np.shape(alpha))
    dalpha = float(g) if np.ndim(alpha) == 0 else g
    dam = np.full((N, M), dalpha) if np.ndim(dalpha) == 0 else tw.alpha_to_map(dalpha, M, N)
    return df, dalpha, dam, dw


# ---- the cases ------------------------------------------------------------------------------------------------------------------
WEIGHTS = {"tv": (None,), "weighted": ("mask", "dyadic"), "l1": ("mask", "dyadic", "ones"), "kl": ("mask", "dyadic", "ones")}


def cases(model, shape):
    """[(data class, parameter kind, weight kind)] of a model on a shape.  blocks: the 8-bit images (kl: the raw counts instead --
    f >= 0 with zeros) with every parameter kind and weight; flat: the constant plane with the first scalar; edge: the engineered
    projection tie, on EDGE_SHAPE's own test."""
    natural = "counts" if model == "kl" else "blocks"
    out = [(natural, kind, wkind) for wkind in WEIGHTS[model] for kind in kinds_of(model)]
    out.append(("flat", SCALARS[model][0], WEIGHTS[model][0]))
    if model == "kl":                       # an 8-bit image under a mask: f = 0 at the pepper, w = 0 at the mask
        out.append(("blocks", SCALARS[model][0], "mask"))
    return out


def image(dclass, shape):
    return {"blocks": blocks8, "flat": constant, "counts": counts}[dclass](tuple(shape))


def case(model, shape, dclass, kind, wkind):
    """(f, alpha, amap, w) of a case."""
    O, N, M = shape
    f = image(dclass, shape)
    alpha = alpha_of(model, kind, N, M)
    return f, alpha, tw.alpha_to_map(alpha, M, N), weight(wkind, tuple(shape))
