"""The one-plane taped family held to oracle/taped_oracle.c on data that sit on its decisions:
tv_tile_kernel<W, TAPE, TANGENT, L1, KL> and tv_reverse_tile_kernel<W, L1, KL> behind bpltv_unrolled_*, bpltv_weighted_unrolled_*,
bpltv_lone_* and bpltv_kl_*.

The numpy twins have no fma and can be compared only where no decision is within rounding of its threshold; the oracle repeats the
header comment of csrc/tv_tile_kernels.hpp operation for operation, so here the data are 8-bit images with salt-and-pepper noise,
{0, 1} masks, dyadic weights, a constant plane, raw photon counts with zeros and a step edge whose dual lands exactly on the ball
(tests/tie_data.py; tests/test_taped_oracle.py counts the ties).

* forward: u of the taped solve, of the plain solve and of the device form, and the whole caller's tape, are the oracle's bits;
* reverse: the oracle's reverse over the GPU's own tape -- the decisions then agree by construction -- within the family's
  _bounds; every output finite; grad_alpha and grad_w exactly 0.0 where the tape says nothing is passed;
* tangent: u of the jvp call is the oracle's bits, du for df, dalpha, dw alone and together within 1e-11 * max|ref|; a clamped KL
  pixel's du is exactly 0 and a held L1 pixel's is df;
* whether the sweeps' bits agree too is printed, not asserted."""
import numpy as np
import pytest

import tie_data as ti
import tiling_ref as tr
import unrolled_ref as ur
import weighted_unrolled_jvp_ref as wuj
import weighted_unrolled_ref as wur
from oracle import c_oracle as co
from oracle import np_twin as tw
from test_gpu_kl import _bounds as _kl_bounds
from test_gpu_l1 import _bounds as _l1_bounds
from test_gpu_unrolled import _bounds as _tv_bounds
from test_gpu_weighted_unrolled import _bounds as _weighted_bounds
from test_taped_oracle import edge_case

pytestmark = pytest.mark.gpu

RTOL = wuj.UNIT_WEIGHT_RTOL       # 1e-11 * max|ref|: the bound every tangent sweep of the project is held to
PREFIX = {"tv": "", "weighted": "weighted_", "l1": "l1_", "kl": "kl_"}
BITS = {}                         # (model, output) -> [cases whose bits are the oracle's, cases]: the report


def _same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b))


def _dev(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max())


def _bits(model, what, got, ref):
    n = BITS.setdefault((model, what), [0, 0])
    n[0] += int(_same(got, ref))
    n[1] += 1


def _report(model):
    print("%s bits of the sweeps: %s" % (model, "  ".join("%s %d/%d" % (k[1], v[0], v[1]) for k, v in sorted(BITS.items()) if k[0] == model)))


class _Handle:
    """One model's calls on one handle, host and device forms."""

    def __init__(self, cls, model, shape):
        import torch
        self.torch, self.model, self.shape = torch, model, shape
        O, N, M = shape
        self.s = cls(M, N, O)
        self.cap = tr.depth_cap(model, N, M)
        self.plans = ([dict(chains=1), dict(tile_iters=self.cap, chains=1), dict(chains=2), dict(tile_iters=self.cap, chains=2)]
                      if O >= 2 else [dict(), dict(tile_iters=self.cap)])

    def close(self):
        self.s.close()

    def _m(self, name):
        return getattr(self.s, PREFIX[self.model] + name)

    def _wargs(self, w):
        return () if self.model == "tv" else (w,)

    def solve(self, alpha, w, K, **kw):
        return self._m("unrolled_denoise")(alpha, *self._wargs(w), maxiter=K, **kw)

    def plain(self, alpha, w, K, **kw):
        if self.model == "tv":
            return self.s.denoise(alpha, maxiter=K)
        return self._m("denoise")(alpha, w, maxiter=K, **kw)

    def device(self, alpha, w, gu, K, **kw):
        """(u, tape, grad_f, grad_alpha, grad_w) of the device forms on a caller's tape: the solve, the tape read back, and the sweep
        over that very tape."""
        torch, s = self.torch, self.s
        O, N, M = self.shape
        a = np.atleast_1d(np.asarray(alpha, dtype=np.float64))
        an, am = (1, 1) if np.ndim(alpha) == 0 else a.shape
        dev = lambda x: torch.tensor(np.ascontiguousarray(x), dtype=torch.float64, device="cuda")
        at, gt = dev(a), dev(gu)
        nc = 2 if self.model == "tv" else 3
        n = (s.unrolled_tape_doubles if self.model == "tv" else s.weighted_unrolled_tape_doubles)(maxiter=K)
        assert n == K * nc * O * N * M
        tape = torch.full((n,), np.nan, dtype=torch.float64, device="cuda")
        out, gf = (torch.full((O, N, M), np.nan, dtype=torch.float64, device="cuda") for _ in range(2))
        ga = torch.full((am * an,), np.nan, dtype=torch.float64, device="cuda")
        wa = ()
        gw = None
        if self.model != "tv":
            wt = dev(w)
            wa = (wt.data_ptr(), O if w.ndim == 3 else 1)
            gw = torch.full(w.shape, np.nan, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        self._m("unrolled_denoise_device")(*wa, at.data_ptr(), am, an, tape_ptr=tape.data_ptr(), maxiter=K, **kw)
        s.copy_u_device(out.data_ptr())
        self._m("unrolled_vjp_device")(tape.data_ptr(), *wa, at.data_ptr(), am, an, gt.data_ptr(), gf.data_ptr(), ga.data_ptr(),
                                       *(() if gw is None else (gw.data_ptr(),)), maxiter=K, **kw)
        torch.cuda.synchronize()
        ga = ga.cpu().numpy()
        ga = float(ga[0]) if np.ndim(alpha) == 0 else ga.reshape(np.shape(alpha))
        return (out.cpu().numpy(), tape.cpu().numpy().reshape(K, nc, O, N, M), gf.cpu().numpy(), ga,
                None if gw is None else gw.cpu().numpy())

    def tangents(self, alpha, w, K, df, dalpha, dw, **kw):
        """(du (4, O, N, M), u): df, dalpha, dw alone and all together, one call of four directions."""
        z = np.zeros_like
        dfs = np.stack([df, z(df), z(df), df])
        da = np.asarray(dalpha, dtype=np.float64)
        das = np.stack([z(da), da, z(da), da])
        if self.model == "tv":            # (the third direction is zero: there is no dw)
            return self.s.unrolled_jvp(alpha, df=dfs, dalpha=das, want_u=True, maxiter=K, **kw)
        dws = np.stack([z(dw), z(dw), dw, dw])
        return self._m("unrolled_jvp")(alpha, w, df=dfs, dalpha=das, dw=dws, want_u=True, maxiter=K, **kw)


def _gradient_bounds(model, gf0, ga0, gw0, alpha, w, O, N, M):
    if model == "tv":
        return _tv_bounds(gf0, ga0, alpha, O, N, M) + (None,)
    return {"weighted": _weighted_bounds, "l1": _l1_bounds, "kl": _kl_bounds}[model](gf0, ga0, gw0, alpha, w, O, N, M)


def _nothing_passed(model, tape, f, amap, w, tab):
    """(per-pixel, per-image masks) of where the header comment passes nothing into ga and into gw, decided on the tape by the
    oracle with the sweeps' own expressions (oracle.taped_decisions): no iteration projects the pixel's dual; l1: x+ == f in
    every iteration (sign 0, or held); kl: D == 0 in every iteration.  The weighted tail always passes into gw."""
    projected, data = co.taped_decisions(model, tape, f, amap, w, tab=tab)
    return ~projected, (~data if model in ("l1", "kl") else None)


def _reduced_zero(mask, like):
    """Entries of a reduced gradient (a float, a patch, a map; one weight plane or one per image) into which only pixels of
    `mask` (O, N, M) are summed."""
    O, N, M = mask.shape
    if np.ndim(like) == 3:
        return mask
    allimg = mask.all(axis=0)
    if np.shape(like) == (N, M):
        return allimg
    if np.ndim(like) == 0:
        return np.asarray(allimg.all())
    return tw.patch_adjoint((~allimg).astype(np.float64), np.shape(like)[1], np.shape(like)[0]) == 0


def _check_case(h, model, shape, tag, f, alpha, amap, w, Ks, failed):
    """One case at every K and plan.  Appends (tag, K, plan, what, deviation, bound) of whatever misses to `failed`."""
    O, N, M = shape
    gu = ti.cotangent(tuple(shape))
    df, dalpha, dam, dw = ti.directions(shape, w, alpha)
    h.s.set_data(f, f)
    for K in Ks:
        tab = co.taped_step_table(model, w, K)
        u0, tape0, _ = co.taped_forward(model, f, amap, w, K, tab=tab)
        for plan in h.plans:
            miss = lambda what, d=1.0, b=0.0: failed.append((tag, K, plan, what, d, b))
            # ---- forward: every form gives the oracle's bits
            u = h.solve(alpha, w, K, **plan)
            ud, tape, gf, ga, gw = h.device(alpha, w, gu, K, **plan)
            for what, got, ref in (("u", u, u0), ("u plain", h.plain(alpha, w, K, **plan), u0), ("u device", ud, u0), ("tape", tape, tape0)):
                if not _same(got, ref):
                    miss(what, _dev(got, ref))
            # ---- reverse: the oracle over the GPU's own tape
            gf0, ga0, gw0 = co.taped_reverse(model, tape, f, amap, w, gu, tab=tab)
            bf, ba, bw = _gradient_bounds(model, gf0, ga0, gw0, alpha, w, O, N, M)
            ra0 = ur.reduce_alpha(ga0, alpha)
            rows = [("grad_f", gf, gf0, bf), ("grad_alpha", ga, ra0, ba)]
            no_ga, no_gw = _nothing_passed(model, tape, f, amap, w, tab)
            zeros = [("grad_alpha", ga, _reduced_zero(no_ga, alpha))]
            if w is not None:
                rows.append(("grad_w", gw, wur.reduce_w(gw0, w), bw))
                if no_gw is not None:
                    zeros.append(("grad_w", gw, _reduced_zero(no_gw, w)))
            for what, got, ref, b in rows:
                _bits(model, what, got, ref)
                if not np.isfinite(got).all():
                    miss(what + " not finite")
                elif not _dev(got, ref) <= b:
                    miss(what, _dev(got, ref), b)
                print("%s K %d %s: %s %.2e (bound %.2e)" % (tag, K, plan, what, _dev(got, ref), b))
            for what, got, where in zeros:
                if np.asarray(got)[where].any():
                    miss(what + " not exactly 0 where nothing is passed", float(np.abs(np.asarray(got)[where]).max()))
            # ---- tangent (the default and the deepest plan)
            if plan.get("chains", 1) != 1:
                continue
            dus, ut = h.tangents(alpha, w, K, df, dalpha, dw, **plan)
            if not _same(ut, u0):
                miss("u of the tangent sweep", _dev(ut, u0))
            for k, (name, t) in enumerate((("df", (df, None, None)), ("dalpha", (None, dam, None)), ("dw", (None, None, dw)),
                                           ("all", (df, dam, dw)))):
                if name == "dw" and w is None:
                    continue
                du0, _ = co.taped_tangent(model, f, amap, w, K, *t, tab=tab)
                b = RTOL * float(np.abs(du0).max())
                _bits(model, "du " + name, dus[k], du0)
                if not np.isfinite(dus[k]).all():
                    miss("du %s not finite" % name)
                elif not _dev(dus[k], du0) <= b:
                    miss("du " + name, _dev(dus[k], du0), b)
                print("%s K %d %s: du %s %.2e (bound %.2e)" % (tag, K, plan, name, _dev(dus[k], du0), b))
                last = tape[K - 1, 2] if model != "tv" else None
                if model == "kl":                     # clamped in the last iteration: D == 0 (the sweeps' own fma), nothing passes
                    clamped = ~co.taped_decisions(model, tape[K - 1:], f, amap, w, tab=tab[K - 1:])[1]
                    if dus[k][clamped].any():
                        miss("du %s of a clamped pixel not exactly 0" % name)
                if model == "l1" and name in ("df", "dalpha", "dw"):   # held at f by the threshold: moves with f alone
                    held = np.broadcast_to((last == f) & (w > 0), f.shape)
                    if not _same(dus[k][held], (df if name == "df" else np.zeros_like(df))[held]):
                        miss("du %s of a held pixel is not df's" % name)


@pytest.mark.parametrize("shape", ti.SHAPES, ids=ti.shape_id)
@pytest.mark.parametrize("model", ti.MODELS)
def test_the_taped_kernels_are_the_oracle_on_data_with_ties(gpu_solver_cls, model, shape):
    """Measured on MI355X: DESIGN.md section 4.21 (largest deviation per family and output, the bit report, the time)."""
    O, N, M = shape
    h = _Handle(gpu_solver_cls, model, shape)
    failed = []
    for dclass, kind, wkind in ti.cases(model, shape):
        f, alpha, amap, w = ti.case(model, shape, dclass, kind, wkind)
        tag = "%s %s %s %s %s" % (model, ti.shape_id(shape), dclass, kind, wkind)
        _check_case(h, model, shape, tag, f, alpha, amap, w, ti.KS, failed)
    h.close()
    _report(model)
    assert not failed, failed


@pytest.mark.parametrize("model", ti.MODELS)
def test_a_dual_exactly_on_the_ball_is_not_projected(gpu_solver_cls, model):
    """The engineered tie (tests/test_taped_oracle.py: all 17 edge pixels have n2 == alpha^2 in iteration 0): forward, tangent and
    reverse leave such a dual alone, as `out = n2 > alpha^2` says."""
    f, amap, w = edge_case(model)
    h = _Handle(gpu_solver_cls, model, ti.EDGE_SHAPE)
    failed = []
    _check_case(h, model, ti.EDGE_SHAPE, "%s edge" % model, f, amap, amap, w, ti.KS, failed)
    h.close()
    _report(model)
    assert not failed, failed


def test_an_l1_step_let_through_that_rounds_back_to_f_counts_as_held(gpu_solver_cls):
    """tie_data.l1_rounds_back: at five pixels iteration 1 has m > 0 and x+ == f.  The header comment reads act off x+, not off m:
    forward bits, the reverse over the GPU's tape, and at K = 2 -- where that iteration is the last -- du of those pixels exactly
    df for the df direction and exactly 0 for dalpha and dw (_check_case's held-pixel check; here the pixels are named)."""
    model, shape = "l1", ti.ROUND_SHAPE
    f, w, pixels = ti.l1_rounds_back()
    O, N, M = shape
    amap = np.full((N, M), ti.ROUND_ALPHA)
    h = _Handle(gpu_solver_cls, model, shape)
    failed = []
    _check_case(h, model, shape, "l1 rounds back", f, ti.ROUND_ALPHA, amap, w, (ti.ROUND_K,) + ti.KS[1:], failed)
    df, dalpha, dam, dw = ti.directions(shape, w, ti.ROUND_ALPHA)
    dus, u = h.tangents(ti.ROUND_ALPHA, w, ti.ROUND_K, df, dalpha, dw)
    h.close()
    _report(model)
    assert not failed, failed
    for n, m in pixels:
        assert u[0, n, m] == f[0, n, m] and w[n, m] > 0
        assert dus[0][0, n, m] == df[0, n, m] and dus[1][0, n, m] == 0.0 and dus[2][0, n, m] == 0.0, (n, m)
    assert (u != f).sum() > 10 * len(pixels)          # (the rest of the image moves)


# ---- the torch layer on the same data ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", ["l1", "kl"])
def test_the_torch_layer_on_masked_8_bit_data_and_on_raw_counts(gpu_solver_cls, model):
    """tv_l1_denoise_unrolled on the masked 8-bit image and tv_kl_denoise_unrolled on the masked raw counts: autograd's gradients
    are the library's bits, and finite."""
    torch = pytest.importorskip("torch")
    from bpldenoising_amd import torch_layer
    shape, K = ti.SHAPES[0], ti.KS[-1]
    O, N, M = shape
    dclass, kind, wkind = ti.cases(model, shape)[0]
    assert dclass == ("counts" if model == "kl" else "blocks") and wkind == "mask"
    f, alpha, amap, w = ti.case(model, shape, dclass, kind, wkind)
    gu = ti.cotangent(tuple(shape))
    ft = torch.tensor(f, device="cuda", requires_grad=True)
    at = torch.tensor(alpha, dtype=torch.float64, device="cuda", requires_grad=True)
    wt = torch.tensor(w, device="cuda", requires_grad=True)
    try:
        fn = torch_layer.tv_l1_denoise_unrolled if model == "l1" else torch_layer.tv_kl_denoise_unrolled
        u = fn(ft, at, wt, maxiter=K)
        (u * torch.tensor(gu, device="cuda")).sum().backward()
        got = [t.detach().cpu().numpy() for t in (u, ft.grad, at.grad, wt.grad)]
    finally:
        torch_layer.clear_solvers()
    s = gpu_solver_cls(M, N, O)
    s.set_data(f, f)
    m = PREFIX[model]
    ref = (getattr(s, m + "unrolled_denoise")(alpha, w, maxiter=K),) + getattr(s, m + "unrolled_vjp")(alpha, w, gu, maxiter=K)
    s.close()
    assert _same(got[0], co.taped_forward(model, f, amap, w, K)[0])
    for g, r in zip(got, ref):
        assert np.isfinite(g).all() and _same(g, r)
