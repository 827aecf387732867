"""GPU checks of the 32 x 32 unrolled tile kernels at every fusion depth and tile position the host grants (DESIGN.md
section 4.15): tv_tile_kernel<W, TAPE, TANGENT, L1, KL>, tv_reverse_tile_kernel<W, L1, KL>, sr_unrolled_tile_kernel /
sr_unrolled_reverse_tile_kernel, color_tile_kernel<C, TAPE, WEIGHTED>, color_tangent_tile_kernel<C> and
color_reverse_tile_kernel<C, WEIGHTED>.

A. "Results never depend on the plan": at every legal depth 1 ... depth_cap (15 on an axis longer than one region, 32 on a
   one-region image, 7 for the sum of regularisers) and one request above it, for solves of 1, T + 1 and 50 iterations, a
   scalar and a map parameter, every weight of the family, one and two launch chains, every held result has the bits of the
   default plan -- and the statistics say which depth and how many tiles ran (tests/tiling_ref.py).
A'. A tape written at the deepest plan and swept at depth 1 and at the reverse kernel's own cap (8; 6 / 4 / 3 for colour; 5 / 2 /
   1 for weighted colour; 4 for the sum of regularisers), with the full tape and with checkpoints, gives the same gradients.
B. The default and the deepest plan against each family's numpy twin at these shapes, within the caps the family's own tests
   hold it to (imported, not retyped): A alone would pass if every plan were wrong in the same way.
   And the L1 pixels without data that a flat patch holds at f for several iterations: the one place where the `w == 0` half of the
   L1 kernels' `act` decides anything a result depends on.
C. The first call on a new handle at depth 32 -- a tangent sweep, a reverse sweep on a caller's tape, the four-channel weighted
   colour solve and sweep -- gives the bits of a handle that ran the default plan first.

The shapes (tests/tile_depth_ref.py) put tiles in the middle of both axes at every depth, a colour tile in the middle along
j, an image of exactly one region, a second tile shifted back by 31 pixels, and 15 out-of-image lanes per column next to a
middle tile on the other axis."""
import numpy as np
import pytest

import color_weighted_ref as cw
import l1_ref as lr
import sumregs_unrolled_ref as sur
import tile_depth_ref as td
import tiling_ref as tr
import unrolled_ref as ur
import weighted_unrolled_ref as wur
from test_gpu_color import U_CAP
from test_gpu_color import _bounds as _color_bounds
from test_gpu_color_weighted import _bounds as _color_weighted_bounds
from test_gpu_kl import _bounds as _kl_bounds
from test_gpu_l1 import _bounds as _l1_bounds
from test_gpu_sumregs_unrolled import _bounds as _sumregs_bounds
from test_gpu_unrolled import _bounds as _tv_bounds
from test_gpu_weighted_unrolled import _bounds as _weighted_bounds

pytestmark = pytest.mark.gpu

CHAIN_K = 50     # at T <= 6 at least eight launches: what an out-of-phase second chain needs (csrc/tiling.hpp)
ONE_REGION = td.SHAPES[1]


def _same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b))


class _Case:
    """A family's calls on one shape with one parameter kind and one weight: the handle, the arguments, and what tiling_ref
    expects."""

    def __init__(self, cls, fam, shape, kind, wkind=None, f=None):
        self.fam, self.shape, self.kind, self.wkind = fam, shape, kind, wkind
        self.N, self.M = shape[-2:]
        self.C = td.channels_of(fam, shape)
        self.images = td.images_of(fam, shape)
        self.model = td.model_of(fam, shape)
        self.cap = tr.depth_cap(self.model, self.N, self.M)
        self.rev_cap = tr.REV_CAP[self.model]
        self.alpha = td.alpha_of(fam, kind, self.N, self.M)
        self.f, self.gu, self.df = td.data(fam, shape, kind)
        if f is not None:       # (another image under the case's cotangent and tangents)
            assert f.shape == self.f.shape
            self.f = f
        self.da, _, self.dw = td.tangents(fam, shape, kind, wkind)
        self.w = td.weight(fam, shape, wkind)
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
        if self.fam == "l1":
            return s.l1_unrolled_denoise(a, self.w, maxiter=K, **kw)
        if self.fam == "kl":
            return s.kl_unrolled_denoise(a, self.w, maxiter=K, **kw)
        if self.fam == "color_weighted":
            return s.color_weighted_unrolled_denoise(a, self.C, self.w, maxiter=K, **kw)
        return s.color_unrolled_denoise(a, self.C, maxiter=K, **kw)

    def plain(self, K, **kw):
        """The solve without a tape, where the family is held by one."""
        s, a = self.s, self.alpha
        if self.fam == "tv":
            return s.color_denoise(a, 1, maxiter=K, **kw)
        if self.fam == "weighted":
            return s.weighted_denoise(a, self.w, maxiter=K, **kw)
        if self.fam == "l1":
            return s.l1_denoise(a, self.w, maxiter=K, **kw)
        if self.fam == "kl":
            return s.kl_denoise(a, self.w, maxiter=K, **kw)
        if self.fam == "color_weighted":
            return s.color_weighted_denoise(a, self.C, self.w, maxiter=K, **kw)
        assert self.fam == "color", self.fam
        return s.color_denoise(a, self.C, maxiter=K, **kw)

    def sweep(self, K, **kw):
        """The reverse sweep over the handle's tape: {grad_f, grad_alpha (, grad_w)}."""
        s, a, gu = self.s, self.alpha, self.gu
        if self.fam == "tv":
            g = s.unrolled_vjp(a, gu, maxiter=K, **kw)
        elif self.fam == "weighted":
            g = s.weighted_unrolled_vjp(a, self.w, gu, maxiter=K, **kw)
        elif self.fam == "sumregs":
            g = s.sumregs_unrolled_vjp(a, gu, maxiter=K, **kw)
        elif self.fam == "l1":
            g = s.l1_unrolled_vjp(a, self.w, gu, maxiter=K, **kw)
        elif self.fam == "kl":
            g = s.kl_unrolled_vjp(a, self.w, gu, maxiter=K, **kw)
        elif self.fam == "color_weighted":
            g = s.color_weighted_unrolled_vjp(a, self.C, self.w, gu, maxiter=K, **kw)
        else:
            g = s.color_unrolled_vjp(a, self.C, gu, maxiter=K, **kw)
        return dict(zip(("grad_f", "grad_alpha", "grad_w"), g))

    def tangent(self, K, **kw):
        """The tangent sweep with every tangent given: du."""
        s, a = self.s, self.alpha
        if self.fam == "tv":
            return s.unrolled_jvp(a, df=self.df, dalpha=self.da, maxiter=K, **kw)
        if self.fam == "weighted":
            return s.weighted_unrolled_jvp(a, self.w, df=self.df, dalpha=self.da, dw=self.dw, maxiter=K, **kw)
        if self.fam == "l1":
            return s.l1_unrolled_jvp(a, self.w, df=self.df, dalpha=self.da, dw=self.dw, maxiter=K, **kw)
        if self.fam == "kl":
            return s.kl_unrolled_jvp(a, self.w, df=self.df, dalpha=self.da, dw=self.dw, maxiter=K, **kw)
        assert self.fam == "color", self.fam
        return s.color_unrolled_jvp(a, self.C, df=self.df, dalpha=self.da, maxiter=K, **kw)

    def held(self, K, **kw):
        """Every result the family is held by, under one plan; the statistics are checked after each solve."""
        out = {}
        if self.fam == "weighted":
            out["weighted_denoise"] = self.plain(K, **kw)
            self.check_stats(K, kw)
        out["u"] = self.solve(K, **kw)
        self.check_stats(K, kw)
        out.update(self.sweep(K, **kw))
        if td.has_tangent(self.fam):
            out["du"] = self.tangent(K, **kw)
        if self.fam not in ("weighted", "sumregs"):
            out["denoise"] = self.plain(K, **kw)
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
        for wkind in td.weights_of(fam):
            c = _Case(gpu_solver_cls, fam, shape, kind, wkind)
            ref, plans = {}, 0
            for T in range(1, c.cap + 2):                   # every legal depth, and one request above the cap (clamped)
                for K in sorted({1, T + 1, CHAIN_K}):
                    if K not in ref:
                        ref[K] = c.held(K, chains=1)        # the default plan: no tile_iters, one chain
                        assert _same(ref[K]["u"], ref[K].get("denoise", ref[K]["u"]))
                        assert _same(ref[K]["u"], ref[K].get("weighted_denoise", ref[K]["u"]))
                        assert ("grad_w" in ref[K]) == (c.w is not None) and ("du" in ref[K]) == td.has_tangent(fam)
                        assert "denoise" in ref[K] or "weighted_denoise" in ref[K] or fam == "sumregs"
                    for chains in ((1, 2) if c.images >= 2 else (1,)):
                        _assert_same(c.held(K, tile_iters=T, chains=chains), ref[K], (kind, wkind, T, K, chains))
                        plans += 1
            c.close()
            assert plans == (c.cap + 1) * 3 * min(c.images, 2) and len(ref) == c.cap + 3
            # (no vacuous equality.  l1: two iterations on weights of at least 0.5 leave every pixel at f, as one does)
            assert not _same(ref[1]["u"], ref[CHAIN_K if fam == "l1" else 2]["u"]) and not _same(ref[CHAIN_K]["grad_f"], ref[2]["grad_f"])
            if c.w is not None:
                assert ref[CHAIN_K]["grad_w"].shape == c.w.shape and not _same(ref[CHAIN_K]["grad_w"], ref[2]["grad_w"])
            print("%s %s %s: %d plans of depth 1 ... %d (+1) hold the default plan's bits" % (td.case_id(case), kind, wkind, plans, c.cap))


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


# ---- A'. a tape does not remember its plan ------------------------------------------------------------------------------
TAPE_CASES = ([(fam, td.SHAPES[0]) for fam in td.FAMILIES] + [(fam, sh) for fam in ("l1", "kl") for sh in (ONE_REGION, td.SHAPES[-1])]
              + [(fam, sh) for fam in td.COLOR_FAMILIES for sh in td.COLOR_SHAPES])


@pytest.mark.parametrize("case", TAPE_CASES, ids=td.case_id)
def test_a_tape_does_not_remember_its_plan(gpu_solver_cls, case):
    """A tape written at the deepest plan, swept at depth 1 and at the reverse kernel's cap: the default plan's gradients.  With
    checkpoints instead of the tape (every 5 iterations, and the automatic spacing), written at depth 1 and at the cap, the sweep
    -- which runs the segment again at the depth it is asked for, capped as a solve's, and undoes it at that depth capped as a
    sweep's -- gives them too."""
    fam, shape = case
    for kind in ("scalar", "map"):
        for wkind in td.weights_of(fam):
            c = _Case(gpu_solver_cls, fam, shape, kind, wkind)
            assert 1 <= c.rev_cap <= c.cap
            for K in (c.cap + 1, CHAIN_K):
                u0 = c.solve(K, chains=1)
                ref = c.sweep(K, chains=1)
                assert _same(c.solve(K, tile_iters=c.cap), u0)
                c.check_stats(K, dict(tile_iters=c.cap))
                for T in (1, c.rev_cap):
                    _assert_same(c.sweep(K, tile_iters=T), ref, (kind, wkind, K, T))
            K = CHAIN_K
            for ck in (5, -1):
                for Tw in (1, c.cap):
                    assert _same(c.solve(K, tile_iters=Tw, checkpoint_every=ck), u0), (kind, wkind, ck, Tw)
                    c.check_stats(K, dict(tile_iters=Tw))
                    for T in (1, c.rev_cap, c.cap):
                        _assert_same(c.sweep(K, tile_iters=T, checkpoint_every=ck), ref, (kind, wkind, ck, Tw, T))
            assert _same(c.solve(K), u0)                    # the full tape again
            _assert_same(c.sweep(K), ref, (kind, wkind, "full tape"))
            c.close()


# ---- B. the twin at the new shapes --------------------------------------------------------------------------------------
def _deviations(c, K, got, twin=None, du0=None):
    """[(name, deviation, cap)] of one plan's results against the twin: u within U_CAP (1e-13, which tests/test_gpu_l1.py,
    test_gpu_kl.py and test_gpu_color_weighted.py use too), the gradients within the family's own _bounds, the tangent within
    1e-11 * max|ref| (tests/test_gpu_unrolled_jvp.py, test_gpu_weighted_unrolled_jvp.py, test_gpu_color_jvp.py,
    test_gpu_l1_kl_jvp.py).  twin, du0: the case's own (u0, gf0, ga0, gw0) and tangent, where it is not one of td.CASES."""
    u0, gf0, ga0, gw0 = twin if twin is not None else td.twin(c.fam, c.shape, c.kind, K, c.wkind)
    O, N, M, a = c.f.shape[0], c.N, c.M, c.alpha
    dev = lambda x, y: float(np.abs(np.asarray(x) - np.asarray(y)).max())
    bw = reduce_w = None
    if c.fam == "tv":
        bf, ba = _tv_bounds(gf0, ga0, a, O, N, M)
    elif c.fam == "weighted":
        bf, ba, bw = _weighted_bounds(gf0, ga0, gw0, a, c.w, O, N, M)
        reduce_w = wur.reduce_w
    elif c.fam == "sumregs":
        bf, ba = _sumregs_bounds(gf0, ga0, a, O, N, M)
    elif c.fam == "l1":
        bf, ba, bw = _l1_bounds(gf0, ga0, gw0, a, c.w, O, N, M)
        reduce_w = lr.reduce_w
    elif c.fam == "kl":
        bf, ba, bw = _kl_bounds(gf0, ga0, gw0, a, c.w, O, N, M)
        reduce_w = lr.reduce_w
    elif c.fam == "color_weighted":
        bf, ba, bw = _color_weighted_bounds(gf0, ga0, gw0, a, c.w, c.images, c.C, N, M)
        reduce_w = cw.reduce_w
    else:
        bf, ba = _color_bounds(gf0, ga0, a, c.images, N, M)
    reduce_alpha = sur.reduce_alpha if c.fam == "sumregs" else ur.reduce_alpha
    rows = [("u", dev(got["u"], u0), U_CAP), ("grad_f", dev(got["grad_f"], gf0), bf),
            ("grad_alpha", dev(got["grad_alpha"], reduce_alpha(ga0, a)), ba)]
    assert np.shape(got["grad_alpha"]) == np.shape(a)
    if reduce_w is not None:
        assert got["grad_w"].shape == c.w.shape
        rows.append(("grad_w", dev(got["grad_w"], reduce_w(gw0, c.w)), bw))
    if "du" in got:
        du0 = du0 if du0 is not None else td.twin_tangent(c.fam, c.shape, c.kind, K, c.wkind)
        assert float(np.abs(du0).max()) > 0.0
        rows.append(("du", dev(got["du"], du0), 1e-11 * float(np.abs(du0).max())))
    return rows


@pytest.mark.parametrize("kind", td.KINDS)
@pytest.mark.parametrize("case", td.CASES, ids=td.case_id)
def test_the_default_and_the_deepest_plan_match_the_twin(gpu_solver_cls, case, kind):
    """Measured on MI355X over the 120 cases, 171 with the weights (DESIGN.md section 4.15 has the table by family): u at most
    4.9e-15, 4.9 % of its cap (l1; 1.3e-15 elsewhere); grad_f at most 3.2e-13, 1.6 % of its bound; grad_alpha at most 1.2e-12,
    0.5 %; grad_w at most 2.2e-13, 0.3 %; the tangent at most 5.4e-13, 0.8 %.  The new families: l1 grad_f 0.06 %, grad_alpha
    0.13 %, grad_w 0.27 %, tangent 0.19 %; kl u 0.6 %, gradients and tangent under 0.1 %; weighted colour u 0.8 %, grad_f 0.15 %,
    grad_alpha 0.05 %, grad_w 0.03 %."""
    assert U_CAP == 1e-13
    fam, shape = case
    failed = []
    for wkind in td.weights_of(fam):
        c = _Case(gpu_solver_cls, fam, shape, kind, wkind)
        for K in td.KS:
            for kw in (dict(), dict(tile_iters=c.cap)):
                rows = _deviations(c, K, c.held(K, **kw))
                print("%s %s %s K %d depth %d: %s" % (td.case_id(case), kind, wkind, K, c.s.stats()["tile_iters"],
                                                      "  ".join("%s %.2e (cap %.2e, %.4f)" % (n, d, b, d / b if b else 0.0) for n, d, b in rows)))
                failed += [(wkind, K, kw, n, d, b) for n, d, b in rows if not d <= b]
        c.close()
    assert not failed, failed


@pytest.mark.parametrize("kind", td.KINDS)
def test_l1_pixels_without_data_held_at_f_pass_their_adjoint_and_tangent_on(gpu_solver_cls, kind):
    """tile_depth_ref.l1_flat_twin: on a flat patch the pixels with w == 0 keep x+ == f, d = 0, for several iterations, and only
    the `w == 0` half of the L1 kernels' `act` passes the adjoint and the tangent through them (on the other cases such a pixel
    exists in iteration 0 alone, where what it passes on reaches no result).  Depth 1, the reverse cap and the forward cap give
    the default plan's bits, and the default plan meets the twin within the bounds of test_gpu_l1.py and test_gpu_l1_kl_jvp.py.
    Measured on MI355X: u at most 8.9e-16 (0.9 % of its cap), the gradients and the tangent at most 1.4e-14, under 0.02 % of
    their bounds; with `w == 0` taken out of the reverse kernel's `act` grad_f is off by 2.2, out of the tangent kernel's du by
    3.1."""
    c = _Case(gpu_solver_cls, "l1", td.FLAT_SHAPE, kind, "mask", f=td.l1_flat_data()[0])
    failed = []
    for K in td.FLAT_KS:
        u0, gf0, ga0, gw0, du0, st = td.l1_flat_twin(kind, K)
        assert st["held"] > 0
        ref = c.held(K)
        for T in (1, c.rev_cap, c.cap):
            _assert_same(c.held(K, tile_iters=T), ref, (kind, K, T))
        rows = _deviations(c, K, ref, twin=(u0, gf0, ga0, gw0), du0=du0)
        print("l1 flat patch %s K %d (%d held): %s" % (kind, K, st["held"], "  ".join("%s %.2e (cap %.2e, %.4f)" % (n, d, b, d / b if b else 0.0)
                                                                                        for n, d, b in rows)))
        failed += [(K, n, d, b) for n, d, b in rows if not d <= b]
    c.close()
    assert not failed, failed


# ---- C. first use on a fresh handle -------------------------------------------------------------------------------------
# The tile kernels that take more LDS than the default have the attribute raised per instantiation and per handle, on the
# first call that plans them (tangent_kernel_ready, color_plan in csrc/bpltv.hip).  Each call below is the first one on a new
# handle, at the deepest plan of the one-region image (32 step rows in LDS), and is held to a handle that ran every
# default-plan call of the family before.
FIRST_K = 50     # one launch of 32 iterations and one of 18


@pytest.mark.parametrize("fam", ["l1", "kl"])
def test_a_tangent_sweep_at_depth_32_is_the_first_call_on_a_handle(gpu_solver_cls, fam):
    for kind in ("scalar", "map"):
        for wkind in td.weights_of(fam):
            warm = _Case(gpu_solver_cls, fam, ONE_REGION, kind, wkind)
            assert warm.cap == 32
            warm.held(FIRST_K)
            ref = warm.tangent(FIRST_K, tile_iters=32)
            assert _same(ref, warm.tangent(FIRST_K)) and ref.any()
            warm.close()
            new = _Case(gpu_solver_cls, fam, ONE_REGION, kind, wkind)
            assert _same(new.tangent(FIRST_K, tile_iters=32), ref), (kind, wkind)
            new.close()


def test_an_l1_sweep_on_a_caller_s_tape_is_the_first_call_on_a_handle(gpu_solver_cls):
    """The device form: the tape is the caller's, written by another handle at depth 32; the new handle has its dataset and has
    launched nothing."""
    import torch
    O, N, M = ONE_REGION
    for kind in ("scalar", "map"):
        for wkind in td.weights_of("l1"):
            warm = _Case(gpu_solver_cls, "l1", ONE_REGION, kind, wkind)
            K = FIRST_K
            host = warm.held(K)
            a = np.atleast_1d(np.asarray(warm.alpha, dtype=np.float64))
            an, am = (1, 1) if kind == "scalar" else a.shape
            wo = O if warm.w.ndim == 3 else 1
            at, gt, wt = torch.tensor(a, device="cuda"), torch.tensor(warm.gu, device="cuda"), torch.tensor(warm.w, device="cuda")
            tape = torch.zeros(warm.s.weighted_unrolled_tape_doubles(maxiter=K), dtype=torch.float64, device="cuda")
            assert tape.numel() == 3 * K * M * N * O
            outs = [(torch.zeros(O, N, M, dtype=torch.float64, device="cuda"), torch.zeros(am * an, dtype=torch.float64, device="cuda"),
                     torch.zeros(warm.w.shape, dtype=torch.float64, device="cuda")) for _ in range(2)]
            torch.cuda.synchronize()
            warm.s.l1_unrolled_denoise_device(wt.data_ptr(), wo, at.data_ptr(), am, an, tape_ptr=tape.data_ptr(), maxiter=K, tile_iters=32)
            warm.check_stats(K, dict(tile_iters=32))
            new = _Case(gpu_solver_cls, "l1", ONE_REGION, kind, wkind)
            for c, (gf, ga, gw) in zip((warm, new), outs):
                c.s.l1_unrolled_vjp_device(tape.data_ptr(), wt.data_ptr(), wo, at.data_ptr(), am, an, gt.data_ptr(), gf.data_ptr(),
                                           ga.data_ptr(), gw.data_ptr(), maxiter=K, tile_iters=32)
            for gf, ga, gw in outs:      # the handle's own tape at the default plan, the caller's on both handles: the same bits
                assert _same(gf.cpu().numpy(), host["grad_f"]) and _same(gw.cpu().numpy(), host["grad_w"]), (kind, wkind)
                assert _same(ga.cpu().numpy().reshape(np.shape(host["grad_alpha"])), host["grad_alpha"]), (kind, wkind)
            assert host["grad_f"].any() and host["grad_w"].any()
            warm.close()
            new.close()


def test_the_four_channel_weighted_colour_solve_and_sweep_are_the_first_calls_on_a_handle(gpu_solver_cls):
    """The planes of 2 x 2 x 32 x 32 read as one image of four channels: one region, the reverse sweep at its cap of 1."""
    shape = (1, 4) + ONE_REGION[1:]
    assert np.prod(shape) == np.prod(td.COLOR_SHAPES[3]) and tr.REV_CAP[td.model_of("color_weighted", shape)] == 1
    K = FIRST_K
    for kind in ("scalar", "map"):
        for wkind in td.weights_of("color_weighted"):
            warm = _Case(gpu_solver_cls, "color_weighted", shape, kind, wkind)
            assert warm.cap == 32 and warm.C == 4 and _same(warm.f, td.data("color_weighted", td.COLOR_SHAPES[3], kind)[0])
            ref = warm.held(K)
            warm.close()
            new = _Case(gpu_solver_cls, "color_weighted", shape, kind, wkind)
            got = {"u": new.solve(K, tile_iters=32)}
            new.check_stats(K, dict(tile_iters=32))
            got.update(new.sweep(K, tile_iters=32))
            got["denoise"] = new.plain(K, tile_iters=32)
            _assert_same(got, ref, (kind, wkind))
            assert ref["grad_w"].any() and not _same(ref["u"], new.f)
            new.close()
