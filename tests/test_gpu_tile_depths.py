"""GPU checks of the 32 x 32 unrolled tile kernels at every fusion depth and tile position the host grants (DESIGN.md
section 4.15): tv_tile_kernel<W, TAPE, TANGENT>, tv_reverse_tile_kernel<W>, sr_unrolled_tile_kernel /
sr_unrolled_reverse_tile_kernel, color_tile_kernel<C, TAPE>, color_tangent_tile_kernel<C> and color_reverse_tile_kernel<C>.

A. "Results never depend on the plan": at every legal depth 1 ... depth_cap (15 on an axis longer than one region, 32 on a
   one-region image, 7 for the sum of regularisers) and one request above it, for solves of 1, T + 1 and 50 iterations, a
   scalar and a map parameter, one and two launch chains, every held result has the bits of the default plan -- and the
   statistics say which depth and how many tiles ran (tests/tiling_ref.py).
B. The default and the deepest plan against each family's numpy twin at these shapes, within the caps the family's own tests
   hold it to (imported, not retyped): A alone would pass if every plan were wrong in the same way.

The shapes (tests/tile_depth_ref.py) put tiles in the middle of both axes at every depth, a colour tile in the middle along
j, an image of exactly one region, and a second tile shifted back by 31 pixels."""
import numpy as np
import pytest

import sumregs_unrolled_ref as sur
import tile_depth_ref as td
import tiling_ref as tr
import unrolled_ref as ur
import weighted_unrolled_ref as wur
from test_gpu_color import U_CAP
from test_gpu_color import _bounds as _color_bounds
from test_gpu_sumregs_unrolled import _bounds as _sumregs_bounds
from test_gpu_unrolled import _bounds as _tv_bounds
from test_gpu_weighted_unrolled import _bounds as _weighted_bounds

pytestmark = pytest.mark.gpu

CHAIN_K = 50     # at T <= 6 at least eight launches: what an out-of-phase second chain needs (csrc/tiling.hpp)


def _same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b))


class _Case:
    """A family's calls on one shape with one parameter kind: the handle, the arguments, and what tiling_ref expects."""

    def __init__(self, cls, fam, shape, kind):
        self.fam, self.shape, self.kind = fam, shape, kind
        self.N, self.M = shape[-2:]
        self.C = td.channels_of(fam, shape)
        self.images = td.images_of(fam, shape)
        self.model = td.model_of(fam, shape)
        self.cap = tr.depth_cap(self.model, self.N, self.M)
        self.rev_cap = tr.REV_CAP[self.model]
        self.alpha = td.alpha_of(fam, kind, self.N, self.M)
        self.f, self.gu, self.df = td.data(fam, shape, kind)
        self.da, _, self.dw = td.tangents(fam, shape, kind)
        self.w = td.weight(shape) if fam == "weighted" else None
        self.s = cls(self.M, self.N, self.f.shape[0])
        self.s.set_data(self.f, self.f)

    def close(self):
        self.s.close()

    def check_stats(self, K, kw):
        """After a solve: the depth the host granted and the tiles of tests/tiling_ref.py, times the (colour) images."""
        st = self.s.stats()
        T = tr.depth(self.model, self.N, self.M, kw.get("tile_iters", 0))
        assert st["iterations"] == K and st["tile_iters"] == T, (kw, K, st)
        assert st["tiles"] == tr.tiles_of(self.model, self.images, self.N, self.M, T), (kw, K, st)
        if "chains" in kw:
            assert st["launch_chains"] == min(kw["chains"], self.images), (kw, K, st)

    def solve(self, K, **kw):
        """The taped solve alone: u."""
        s, a = self.s, self.alpha
        if self.fam == "tv":
            return s.unrolled_denoise(a, maxiter=K, **kw)
        if self.fam == "weighted":
            return s.weighted_unrolled_denoise(a, self.w, maxiter=K, **kw)
        if self.fam == "sumregs":
            return s.sumregs_unrolled_denoise(a, maxiter=K, **kw)
        return s.color_unrolled_denoise(a, self.C, maxiter=K, **kw)

    def sweep(self, K, **kw):
        """The reverse sweep over the handle's tape: {grad_f, grad_alpha (, grad_w)}."""
        s, a, gu = self.s, self.alpha, self.gu
        if self.fam == "tv":
            g = s.unrolled_vjp(a, gu, maxiter=K, **kw)
        elif self.fam == "weighted":
            g = s.weighted_unrolled_vjp(a, self.w, gu, maxiter=K, **kw)
        elif self.fam == "sumregs":
            g = s.sumregs_unrolled_vjp(a, gu, maxiter=K, **kw)
        else:
            g = s.color_unrolled_vjp(a, self.C, gu, maxiter=K, **kw)
        return dict(zip(("grad_f", "grad_alpha", "grad_w"), g))

    def held(self, K, **kw):
        """Every result the family is held by, under one plan; the statistics are checked after each solve."""
        s, a = self.s, self.alpha
        out = {}
        if self.fam == "weighted":
            out["weighted_denoise"] = s.weighted_denoise(a, self.w, maxiter=K, **kw)
            self.check_stats(K, kw)
        out["u"] = self.solve(K, **kw)
        self.check_stats(K, kw)
        out.update(self.sweep(K, **kw))
        if self.fam == "tv":
            out["du"] = s.unrolled_jvp(a, df=self.df, dalpha=self.da, maxiter=K, **kw)
            out["denoise"] = s.color_denoise(a, 1, maxiter=K, **kw)
            self.check_stats(K, kw)
        elif self.fam == "weighted":
            out["du"] = s.weighted_unrolled_jvp(a, self.w, df=self.df, dalpha=self.da, dw=self.dw, maxiter=K, **kw)
        elif self.fam == "color":
            out["du"] = s.color_unrolled_jvp(a, self.C, df=self.df, dalpha=self.da, maxiter=K, **kw)
            out["denoise"] = s.color_denoise(a, self.C, maxiter=K, **kw)
            self.check_stats(K, kw)
        return out


def _assert_same(got, ref, what):
    assert sorted(got) == sorted(ref)
    for name in ref:
        assert _same(got[name], ref[name]), (what, name, float(np.abs(np.asarray(got[name]) - np.asarray(ref[name])).max()))


# ---- A. every depth gives the default plan's bits -----------------------------------------------------------------------
@pytest.mark.parametrize("case", td.CASES, ids=td.case_id)
def test_every_depth_gives_the_default_plan_s_bits(gpu_solver_cls, case):
    fam, shape = case
    for kind in ("scalar", "map"):
        c = _Case(gpu_solver_cls, fam, shape, kind)
        ref, plans = {}, 0
        for T in range(1, c.cap + 2):                   # every legal depth, and one request above the cap (clamped)
            for K in sorted({1, T + 1, CHAIN_K}):
                if K not in ref:
                    ref[K] = c.held(K, chains=1)        # the default plan: no tile_iters, one chain
                    assert _same(ref[K]["u"], ref[K].get("denoise", ref[K]["u"]))
                    assert _same(ref[K]["u"], ref[K].get("weighted_denoise", ref[K]["u"]))
                for chains in ((1, 2) if c.images >= 2 else (1,)):
                    _assert_same(c.held(K, tile_iters=T, chains=chains), ref[K], (kind, T, K, chains))
                    plans += 1
        c.close()
        assert plans == (c.cap + 1) * 3 * min(c.images, 2) and len(ref) == c.cap + 3
        assert not _same(ref[1]["u"], ref[2]["u"]) and not _same(ref[CHAIN_K]["grad_f"], ref[2]["grad_f"])   # (no vacuous equality)
        print("%s %s: %d plans of depth 1 ... %d (+1) hold the default plan's bits" % (td.case_id(case), kind, plans, c.cap))


@pytest.mark.parametrize("fam", ["tv", "sumregs"])
def test_the_per_image_forms_at_three_depths(gpu_solver_cls, fam):
    """unrolled_*_each and sumregs_unrolled_*_each run the same kernels with one parameter block per image: depth 1, the
    cap and one in between on 2 x 70 x 72."""
    shape = (2, 70, 72)
    rng = np.random.default_rng(23)
    for kind in ("scalar", "map"):
        c = _Case(gpu_solver_cls, fam, shape, kind)
        s = c.s
        blocks = np.stack([np.asarray(c.alpha, dtype=np.float64), 1.5 * np.asarray(c.alpha, dtype=np.float64)])
        dblocks = rng.standard_normal(blocks.shape)

        def held(K, **kw):
            out = {}
            if fam == "tv":
                out["u"] = s.unrolled_denoise_each(blocks, maxiter=K, **kw)
                c.check_stats(K, kw)
                out["grad_f"], out["grad_alpha"] = s.unrolled_vjp_each(blocks, c.gu, maxiter=K, **kw)
                out["du"] = s.unrolled_jvp_each(blocks, df=c.df, dalphas=dblocks, maxiter=K, **kw)
            else:
                out["u"] = s.sumregs_unrolled_denoise_each(blocks, maxiter=K, **kw)
                c.check_stats(K, kw)
                out["grad_f"], out["grad_alpha"] = s.sumregs_unrolled_vjp_each(blocks, c.gu, maxiter=K, **kw)
            return out

        ref = {}
        for T in (1, (c.cap + c.rev_cap) // 2, c.cap):
            for K in sorted({1, T + 1, CHAIN_K}):
                if K not in ref:
                    ref[K] = held(K, chains=1)
                    assert ref[K]["grad_alpha"].shape == blocks.shape
                for chains in (1, 2):
                    _assert_same(held(K, tile_iters=T, chains=chains), ref[K], (kind, T, K, chains))
        c.close()


@pytest.mark.parametrize("case", [(fam, td.SHAPES[0]) for fam in td.FAMILIES] + [("color", sh) for sh in td.COLOR_SHAPES],
                         ids=td.case_id)
def test_a_tape_does_not_remember_its_plan(gpu_solver_cls, case):
    """A tape written at the deepest plan, swept at depth 1 and at the reverse kernel's cap: the default plan's gradients."""
    fam, shape = case
    for kind in ("scalar", "map"):
        c = _Case(gpu_solver_cls, fam, shape, kind)
        for K in (c.cap + 1, CHAIN_K):
            c.solve(K, chains=1)
            ref = c.sweep(K, chains=1)
            c.solve(K, tile_iters=c.cap)
            c.check_stats(K, dict(tile_iters=c.cap))
            for T in (1, c.rev_cap):
                _assert_same(c.sweep(K, tile_iters=T), ref, (kind, K, T))
        c.close()


# ---- B. the twin at the new shapes --------------------------------------------------------------------------------------
def _deviations(c, K, got):
    """[(name, deviation, cap)] of one plan's results against the twin: u within U_CAP, the gradients within the family's own
    _bounds, the tangent within 1e-11 * max|ref| (tests/test_gpu_unrolled_jvp.py, test_gpu_weighted_unrolled_jvp.py,
    test_gpu_color_jvp.py)."""
    u0, gf0, ga0, gw0 = td.twin(c.fam, c.shape, c.kind, K)
    O, N, M, a = c.f.shape[0], c.N, c.M, c.alpha
    dev = lambda x, y: float(np.abs(np.asarray(x) - np.asarray(y)).max())
    if c.fam == "tv":
        bf, ba = _tv_bounds(gf0, ga0, a, O, N, M)
    elif c.fam == "weighted":
        bf, ba, bw = _weighted_bounds(gf0, ga0, gw0, a, c.w, O, N, M)
    elif c.fam == "sumregs":
        bf, ba = _sumregs_bounds(gf0, ga0, a, O, N, M)
    else:
        bf, ba = _color_bounds(gf0, ga0, a, c.images, N, M)
    reduce_alpha = sur.reduce_alpha if c.fam == "sumregs" else ur.reduce_alpha
    rows = [("u", dev(got["u"], u0), U_CAP), ("grad_f", dev(got["grad_f"], gf0), bf),
            ("grad_alpha", dev(got["grad_alpha"], reduce_alpha(ga0, a)), ba)]
    assert np.shape(got["grad_alpha"]) == np.shape(a)
    if c.fam == "weighted":
        rows.append(("grad_w", dev(got["grad_w"], wur.reduce_w(gw0, c.w)), bw))
    if "du" in got:
        du0 = td.twin_tangent(c.fam, c.shape, c.kind, K)
        rows.append(("du", dev(got["du"], du0), 1e-11 * float(np.abs(du0).max())))
    return rows


@pytest.mark.parametrize("kind", td.KINDS)
@pytest.mark.parametrize("case", td.CASES, ids=td.case_id)
def test_the_default_and_the_deepest_plan_match_the_twin(gpu_solver_cls, case, kind):
    """Measured on MI355X over the 57 cases (DESIGN.md section 4.15 has the table): u at most 1.3e-15; grad_f at most 3.2e-13,
    1.6 % of its bound; grad_alpha at most 1.3e-12, 0.5 %; grad_w 4.5e-15, 0.3 %; the tangent at most 2.4e-13, 0.8 %."""
    fam, shape = case
    c = _Case(gpu_solver_cls, fam, shape, kind)
    failed = []
    for K in td.KS:
        for kw in (dict(), dict(tile_iters=c.cap)):
            rows = _deviations(c, K, c.held(K, **kw))
            print("%s %s K %d depth %d: %s" % (td.case_id(case), kind, K, c.s.stats()["tile_iters"],
                                               "  ".join("%s %.2e (cap %.2e, %.4f)" % (n, d, b, d / b if b else 0.0) for n, d, b in rows)))
            failed += [(K, kw, n, d, b) for n, d, b in rows if not d <= b]
    c.close()
    assert not failed, failed
