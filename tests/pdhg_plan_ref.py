"""The geometry of the plain TV solve, restated in plain Python -- TEST INFRASTRUCTURE ONLY.

kVariants of csrc/bpltv.hip (the 36 instantiations of the six kernel templates of csrc/pdhg_kernels.hpp) and what
plan_pdhg and chain_launches of csrc/tiling.hpp and make_plan of csrc/bpltv.hip make of a request for one of them: the
region, the deepest fusion an image admits, the tiles and the launches.  From these follow the depths and the image
shapes at which tests/test_gpu_pdhg_variants.py runs every variant: the smallest images that hold each class of tile
(interior, shifted last, unshifted last, single) at each depth where a kernel takes another path.

Shapes are (N, M), j over N, as everywhere in the tests; RJ is the region along j (N), RI along i (M)."""
import collections

from tiling_ref import tile_count, tile_span, tiles

NO_CAP = 1 << 20      # plan_pdhg's maxT for an axis of at most one region: no halo, nothing to cap
MAX_T = 32            # PDHG_MAX_T: the step rows pdhg_tile_kernel keeps in LDS
BIG = 1 << 14         # an axis of many regions, for the caps of a geometry class

Variant = collections.namedtuple("Variant", "RI RJ min_image tmax tiles_per_block family lds_rows PJ")


def _tile(PI, PJ, TI, TJ):    # VAR: pdhg_tile_kernel, region (PI * TI) x (PJ * TJ); the func_1d variants
    return Variant(PI * TI, PJ * TJ, 0, 0, 1, "tile", True, PJ)


def _wave(PJ, WPB):           # VARW: pdhg_wave_kernel, one wave per 32 x (2 PJ) region, WPB tiles per workgroup
    return Variant(32, 2 * PJ, 0, 0, WPB, "wave", False, PJ)


def _rows(PJ, TJ, family="rows"):   # VARR / VARR2: 64 lanes along i, PJ pixels per thread, TJ waves
    return Variant(64, PJ * TJ, 1, 0, 1, family, False, PJ)


def _stream(SEG, NL):         # VARS: segments of SEG rows and NL lead-in rows at each end, one wave per fused iteration
    return Variant(64, SEG + 2 * NL, 2, NL, 1, "stream", False, None)


def _rowsw(PJ, TJ):           # VARRW: rows of 128 pixels
    return Variant(128, PJ * TJ, 1, 0, 1, "rowsw", False, PJ)


VARIANTS = {v + 1: V for v, V in enumerate([
    _tile(1, 1, 32, 32), _tile(2, 2, 32, 32), _tile(1, 1, 16, 16), _tile(2, 2, 16, 16), _tile(2, 1, 32, 32),
    _tile(4, 4, 16, 16), _tile(1, 1, 64, 16), _tile(2, 1, 64, 16), _tile(2, 2, 64, 16), _tile(1, 2, 32, 32),
    _tile(1, 2, 40, 20), _tile(2, 2, 20, 20), _tile(1, 3, 48, 16), _tile(3, 2, 32, 32), _tile(2, 3, 48, 16),
    _wave(16, 4), _wave(8, 4), _wave(12, 4),
    _rows(8, 8), _rows(6, 8), _rows(8, 16), _rows(4, 16), _rows(6, 16), _rows(8, 8), _rows(6, 8), _rows(10, 8),
    _rows(12, 8), _rows(12, 4), _rows(16, 4),
    _rows(8, 8, "rows2"), _rows(8, 8, "rows2"),
    _stream(256, 8), _stream(256, 8),
    _rowsw(8, 8), _rowsw(8, 4), _rowsw(6, 8),
])}
AUTO = {"tile32": 1, "tile48": 13, "rows64": 19, "rows48": 20}   # PLAN_V_* + 1: what the automatic choice names
CLASSES = ("shift", "fit", "one", "narrow")


def too_small(v, N, M):
    """plan_too_small: a forced variant on such an image is refused (the automatic plan keeps the 48 x 48 tile kernel)."""
    V = VARIANTS[v]
    return (V.min_image == 1 and (M < V.RI or N < V.RJ)) or (V.min_image >= 2 and M < V.RI)


def depth_cap(v, N, M):
    """Deepest fusion plan_pdhg clamps a request to: per axis no limit where L <= R, else the halo must leave a core;
    then the variant's own tmax.  (The LDS-tile variants: see deepest.)"""
    V = VARIANTS[v]
    ax = lambda L, R: NO_CAP if L <= R else (R - 1) // 2
    cap = min(ax(M, V.RI), ax(N, V.RJ))
    return min(cap, V.tmax) if V.tmax > 0 else cap


def deepest(v, N, M):
    """Deepest fusion that runs: depth_cap, and for the LDS-tile variants the MAX_T step rows of a launch."""
    return min(depth_cap(v, N, M), MAX_T) if VARIANTS[v].lds_rows else depth_cap(v, N, M)


def granted(v, N, M, tile_iters):
    """The depth of a solve that asks for tile_iters >= 1 of a forced variant, or None where make_plan refuses it: the
    LDS-tile variants do not clamp a request beyond MAX_T that the halo admits, they refuse it."""
    T = min(tile_iters, depth_cap(v, N, M))
    return None if (VARIANTS[v].lds_rows and T > MAX_T) else T


def depths(v, N, M):
    """The depths at which variant v is run on an N x M image: the shallowest, the default (8), the first halo wider
    than a thread's strip of PJ pixels (no such strip in the stream kernels), and the deepest two.  An image of one
    region has no deepest (the families without the step-row array): the callers add the depths they want."""
    V = VARIANTS[v]
    cap = deepest(v, N, M)
    want = {1, 2, 8}
    if V.PJ is not None:
        want.add(V.PJ + 1)
    if cap < NO_CAP:
        want |= {cap - 1, cap}
    return sorted(t for t in want if 1 <= t <= cap)


def shapes(v, T):
    """[(class, (N, M))] for variant v at depth T, S = R - 2T the core stride of an interior tile:
    shift   one axis R + 1 (two tiles, the last pulled back by S - 1, as far as it goes), the other R + S + 1 (a border
            tile, an interior tile and a last tile pulled back by S - 1);
    fit     R + S on both axes: two tiles, the last not shifted;
    one     exactly one region: a single tile, no halo;
    narrow  one axis shorter than a region and the other R + S + 1, where min_image admits it (the stream kernels: any
            height, at least a region wide), and one pixel less than a region on both axes.
    Classes whose tiled axes have no core left at T are left out."""
    V = VARIANTS[v]
    Si, Sj = V.RI - 2 * T, V.RJ - 2 * T
    T_i, T_j = T <= (V.RI - 1) // 2, T <= (V.RJ - 1) // 2     # a core is left along i / along j
    out = []
    if T_i and T_j:
        out += [("shift", (V.RJ + Sj + 1, V.RI + 1)), ("shift", (V.RJ + 1, V.RI + Si + 1)), ("fit", (V.RJ + Sj, V.RI + Si))]
    out.append(("one", (V.RJ, V.RI)))
    if V.min_image == 0:
        if T_j:
            out.append(("narrow", (V.RJ + Sj + 1, 5)))
        if T_i:
            out.append(("narrow", (3, V.RI + Si + 1)))
        out.append(("narrow", (V.RJ - 1, V.RI - 1)))
    elif V.min_image == 2 and T_i:
        out.append(("narrow", (3, V.RI + Si + 1)))
    return out


def one_depths(v):
    """Depths of a single tile (an image of at most one region) beyond depths(): the MAX_T rows of the step-row array,
    and 40 for the families without it (the stream kernels: their tmax)."""
    V = VARIANTS[v]
    cap = deepest(v, V.RJ, V.RI)
    return sorted({min(MAX_T, cap), min(40, cap)})


def cases(v):
    """[(T, class, (N, M))]: every shape of variant v at every depth of depths() for that shape's geometry -- which of
    its axes are tiled decides the cap -- and the single tile at one_depths as well."""
    V = VARIANTS[v]
    out = []
    for T in range(1, 65):
        for cls, (N, M) in shapes(v, T):
            single = N <= V.RJ and M <= V.RI
            if T in depths(v, N, M) or (single and T in one_depths(v)):
                out.append((T, cls, (N, M)))
    return out


def plan(v, N, M, images, T):
    """region_i, region_j, tiles of a solve of `images` images at depth T (stats()["tiles"] = Plan::grid)."""
    V = VARIANTS[v]
    return V.RI, V.RJ, tile_count(M, T, V.RI) * tile_count(N, T, V.RJ) * images


def chain_out_of_phase(niter, T, from_state=False):
    nl0, h0 = -(-niter // T), T // 2
    return (not from_state) and T >= 2 and nl0 >= 8 and ((1 + -(-(niter - h0) // T)) - nl0) % 2 == 1


def chain_launches(niter, T, chains, out_of_phase):
    return -(-niter // T) * chains + (chains // 2 if out_of_phase else 0)


def launches(niter, T, chains, graph=True):
    """(stats()["launches"], stats()["launch_chains"]) of a solve from x = f, y = 0 that asks for `chains` launch chains
    (at most one per image: the caller passes min(chains, images)).  Eager launches run as one chain."""
    if not graph:
        return -(-niter // T), 1
    return chain_launches(niter, T, chains, chain_out_of_phase(niter, T)), chains


def auto_variant(N, M, images, ncu=256):
    """The variant plan_pdhg chooses for an image with an axis above 256 pixels (below that its launch-cost model
    decides): the 48 x 48 tile kernel, or -- from 64 x 64 pixels -- 64-lane rows, 64 x 48 while both rows regions fit
    the chip in one round of two workgroups per CU."""
    assert M > 256 or N > 256
    if not (M >= 64 and N >= 64):
        return AUTO["tile48"]
    n = lambda v: tile_count(M, 8, VARIANTS[v].RI) * tile_count(N, 8, VARIANTS[v].RJ) * images
    return AUTO["rows48"] if (n(AUTO["rows64"]) <= 2 * ncu and n(AUTO["rows48"]) <= 2 * ncu) else AUTO["rows64"]


def tile_classes(L, R, T):
    """What the tiles along an axis of L pixels are: {"single"} or a subset of {"first", "interior", "last"}, and the
    shift of the last tile (how far it is pulled back from where the stride would put it)."""
    t = tiles(L, T, R)
    if len(t) == 1:
        return {"single"}, 0
    S = R - 2 * T
    inner = {"interior"} if any(o > 0 and o + R < L for o, _, _ in t) else set()
    natural = (R - T) + (len(t) - 2) * S - T
    return {"first", "last"} | inner, natural - t[-1][0]


__all__ = ["VARIANTS", "AUTO", "CLASSES", "NO_CAP", "MAX_T", "BIG", "too_small", "depth_cap", "deepest", "granted", "depths",
           "shapes", "one_depths", "cases", "plan", "chain_out_of_phase", "chain_launches", "launches", "auto_variant",
           "tile_classes", "tile_span", "tile_count", "tiles"]
