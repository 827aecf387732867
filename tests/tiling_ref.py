"""The tiling of the 32 x 32 unrolled tile kernels, restated in plain Python -- TEST INFRASTRUCTURE ONLY.

tile_span and tile_count of csrc/tiling.hpp, and the depth caps of weighted_plan, unrolled_plan (colour: color_plan) and
sr_unrolled_plan of csrc/bpltv.hip: a region of 32 pixels per axis, a halo of T pixels (2T for the sum of regularisers) on
every region edge that is not an image border, a last tile shifted back onto the image, and no halo at all on an axis of at
most one region."""
REGION = 32       # TV_R, SRUN_R
MAX_T = 32        # PDHG_MAX_T: step rows one launch keeps in LDS
SR_FWD_CAP = 7    # (SRUN_R - 1) / 4: the sum of regularisers' halo 2T must leave a core
REV_CAP = {"tv": 8, "weighted": 8, "sumregs": 4, "color1": 8, "color2": 6, "color3": 4, "color4": 3,   # TV_REV_T, SRUN_REV_T, color_rev_t
           "l1": 8, "kl": 8, "color_weighted2": 5, "color_weighted3": 2, "color_weighted4": 1}          # TV_REV_T, color_weighted_rev_t
MODELS = tuple(sorted(REV_CAP))


def tile_span(a, L, halo, R=REGION):
    """(o, c0, c1) of tile a along an axis of L pixels: the region [o, o + R) and the core [c0, c1) it writes back."""
    if L <= R:
        return 0, 0, L
    S = R - 2 * halo
    cs = 0 if a == 0 else (R - halo) + (a - 1) * S
    o = 0 if a == 0 else cs - halo
    if o + R >= L:
        return L - R, cs, L
    return o, cs, o + R - halo


def tiles(L, halo, R=REGION):
    """[(o, c0, c1)] of every tile along an axis of L pixels (tile_count's loop)."""
    if L > R and R - 2 * halo < 1:
        raise ValueError("a halo of %d leaves no core in a region of %d" % (halo, R))
    out = []
    while True:
        out.append(tile_span(len(out), L, halo, R))
        if out[-1][2] >= L:
            return out


def tile_count(L, halo, R=REGION):
    return len(tiles(L, halo, R))


def interior(L, halo, R=REGION):
    """Tiles with a halo at both ends of the region: neither end is an image border."""
    return sum(1 for o, _, _ in tiles(L, halo, R) if o > 0 and o + R < L)


def halo_of(model, T):
    return 2 * T if model == "sumregs" else T


def depth_cap(model, N, M):
    """Deepest fusion the host grants a taped, tangent or plain solve of `model` on N x M images."""
    if model == "sumregs":
        cap = lambda L: SR_FWD_CAP if L > REGION else 1 << 20
        return min(SR_FWD_CAP, cap(M), cap(N))
    cap = lambda L: MAX_T if L <= REGION else (REGION - 1) // 2
    return min(MAX_T, cap(M), cap(N))


def depth(model, N, M, tile_iters=0):
    """Iterations per launch of a solve that asks for tile_iters (0: the default, 8, or 4 for the sum of regularisers)."""
    T = tile_iters if tile_iters > 0 else (4 if model == "sumregs" else 8)
    return min(T, depth_cap(model, N, M))


def tiles_of(model, images, N, M, T):
    """stats()["tiles"] of a solve at depth T: tiles along both axes times the images (colour images for C > 1)."""
    h = halo_of(model, T)
    return tile_count(M, h) * tile_count(N, h) * images
