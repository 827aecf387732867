"""GPU checks of bpltv_weighted_vjp on images with a real active set under wide weights.

tests/test_gpu_weighted_shapes.py runs the weighted adjoint on two small planted blocks with w in [0.25, 4] (s = 1/sqrt(w) in
[0.5, 2]) and accepts any adjoint_attempts; tests/test_gpu_tv_active_set.py runs it on strips and a constant image with w = 1 only,
where it is bpltv_vjp bit for bit.  Here the layouts of tests/tv_active_ref.py (strips across tile seams and separators, a constant
image, blocks) meet the weights of tests/weighted_active_ref.py: the old range, six decades (s^2 from 1e-3 to 1e3 next to the
active-set weight), and two noise levels whose jump cuts through the planted regions.  The reference is the literal unreduced system
with diag(w) and kappa = weighted_ref.kappa_default(alpha), ten extended-precision sweeps, solved once per (case, kappa) and pinned
on the CPU by tests/test_weighted_active_ref.py.  The bound everywhere is |a - b| <= 1e-8 max|p| + 1e-6 |b|, elementwise; the
statistics must say that the first attempt, with the default weight, passed the residual gate."""
import numpy as np
import pytest

import tv_active_ref as ta
import weighted_active_ref as wa
import weighted_ref as wr
from test_gpu_tv_active_set import E_UNSUPPORTED, METHOD_IDS, METHODS, _check_stats, _close, _dist, _same
from test_gpu_vjp import _nd_bytes_per_image

pytestmark = pytest.mark.gpu

# (a): the largest |difference| of an output over the largest |entry| of its reference, per factorisation (stats["adjoint_method"]).
# Under log3 and step max|p| reaches 1e2 ... 1e3 while grad_f = w o p is O(1), so 1e-8 max|p| is loose there; this holds each
# output on its own scale, at four times what the MI355X measured, rounded up to one digit (the room is for another elimination
# order, not for a lost digit), and never above 1e-6.
# Measured at six sweeps: 4.0e-9 on the LDS band, block cyclic reduction and nested dissection (grad_f of 2 x 70 x 72 blocks, log3,
# scalar), 2.0e-9 on the band in HBM (grad_f of 1 x 12 x 140 blocks, log3, scalar).  Both are the distance of the system the
# library solves on purpose -- an active element's weight is min(kappa, 4e14 w_min), weighted_adj_setup_kernel -- from the literal
# one: tests/weighted_ref.py's system with that weight per element is 2.0e-9 from the literal grad_f on 1 x 12 x 140 on the CPU.
# (With kappa on every element the figures were 8.1e-10 and 9.3e-12, and 3 x 33 x 17 flat / step / scalar failed outright.)
OWN_SCALE = {"band": 2e-8, "band-hbm": 8e-9, "bcr": 2e-8, "nd": 2e-8}


def _handle(cls, shape, method):
    """A handle and the factorisation it will run: block cyclic reduction is refused with E_UNSUPPORTED above M = 128, after
    which the handle goes on working (with the default factorisation)."""
    from bpldenoising_amd._lib import BpltvError
    O, N, M = shape
    s = cls(M, N, O)
    if method == 2 and M > 128:
        z = np.zeros(shape)
        with pytest.raises(BpltvError) as e:
            s.weighted_vjp(z, z, 0.1, np.ones(shape), z, adjoint_method=2)
        assert e.value.code == E_UNSUPPORTED
        method = 0
    return s, method


def _check(st, method, M, alpha, chunks=1):
    """The first attempt with the default active-set weight passed the gate (a retry with a smaller kappa would pass a comparison
    with a reference rebuilt on stats["kappa_used"])."""
    _check_stats(st, method, M, chunks)
    assert st["kappa_used"] == wr.kappa_default(alpha), st


def distances(cls, case, method, refine):
    """One bpltv_weighted_vjp call on a planted case against the literal system with the default kappa: per output (within the
    bound, max|difference|, max|difference| / max|reference|), the factorisation that ran, max|p|."""
    shape, layout, kind, wname, per_image = case
    O, N, M = shape
    alpha, f, w, u, gu = wa.case(*case)
    s, method = _handle(cls, shape, method)
    kw = {} if refine is None else {"refine": refine}
    got = s.weighted_vjp(u, f, alpha, w, gu, adjoint_method=method, **kw)
    st = s.stats()
    s.close()
    ref = wa.vjp_ref(*case, wr.kappa_default(alpha))
    pmax = ref[3]
    d = [_dist(a, b) for a, b in zip(got, ref[:3])]
    own = [x / float(np.abs(np.asarray(b)).max()) for x, b in zip(d, ref[:3])]
    print("%s %s refine %s: method %s kappa_used %.3e attempts %d residual %.3e max|d| grad_f %.3e grad_alpha %.3e grad_w %.3e "
          "(max|p| %.3e, bound %.1e) own scale %.3e %.3e %.3e"
          % (wa.case_id(*case), METHODS.get(method, "auto"), refine, st["adjoint_method"], st["kappa_used"], st["adjoint_attempts"],
             st["adjoint_residual"], d[0], d[1], d[2], pmax, 1e-8 * pmax, own[0], own[1], own[2]))
    _check(st, method, M, alpha)
    assert got[2].shape == w.shape and np.shape(got[1]) == np.shape(alpha)
    return [(_close(a, b, pmax), x, y) for a, b, x, y in zip(got, ref[:3], d, own)], st["adjoint_method"], pmax


NAMES = ("grad_f", "grad_alpha", "grad_w")


@pytest.mark.parametrize("method", sorted(METHODS), ids=METHOD_IDS)
@pytest.mark.parametrize("case", wa.CASES, ids=wa.IDS)
def test_weighted_vjp_at_converged_refinement_matches_the_literal_system(gpu_solver_cls, case, method):
    """refine = 6: what weighted_adj_setup_kernel, the factorisations and weighted_adj_out_kernel compute on active elements with
    s != 1, apart from the sweep count; each output also on its own scale (OWN_SCALE).

    Measured on the MI355X, largest |difference| of grad_f / grad_alpha / grad_w, largest fraction of the bound and largest own-scale
    distance over the cases (max|p| 1.7 ... 1.6e3; kappa_used the default, adjoint_attempts 1 and adjoint_residual <= 1.3e-13
    everywhere), the LDS band, block cyclic reduction and nested dissection alike:
        scalar      rand  1.5e-10 / 1.0e-10 / 3.8e-12  0.00075  5.2e-11     patch, map  rand  2.8e-9 / 2.2e-9 / 5.4e-11   0.029   8.1e-10
        scalar      log3  4.4e-8 / 1.2e-8 / 4.9e-10    0.013    4.0e-9      patch, map  log3  1.5e-10 / 1.0e-8 / 1.2e-9   6.8e-5  3.2e-11
        scalar      step  3.8e-10 / 7.3e-8 / 1.5e-8    0.0023   2.3e-10     patch, map  step  5.0e-10 / 2.0e-7 / 1.2e-8   0.0021  2.0e-10
        band in HBM (1 x 12 x 140)  log3 1.0e-8 / 4.3e-9 / 1.2e-9  0.013  2.0e-9     step 1.6e-11 / 1.7e-9 / 1.7e-10  4.1e-5  1.8e-11
    Until the weight of an active element was made relative to the fidelity weight (min(kappa, 4e14 w_min))
    3 x 33 x 17 "flat" with `step` and a scalar failed here on every factorisation: its border block lies wholly in w = 0.01, where
    kappa s^2 = 1e16 passes 2^53, and at six sweeps grad_f was 7.4e-6 from the literal system on the LDS band (11 times the bound),
    1.2e-4 on nested dissection and 8.2e7 on block cyclic reduction, whose refinement diverged, all with adjoint_attempts 1 and the
    residual under the gate.  Now 8.5e-12 / 1.4e-9 / 4.8e-11 on all three, 6.2e-6 of the bound.  The price is the scalar / log3 row:
    1.6e-10 (own scale 9.5e-12) before, now the distance between the two systems."""
    out, ran, _ = distances(gpu_solver_cls, case, method, 6)
    for name, (ok, d, own) in zip(NAMES, out):
        assert ok, name
        assert own <= OWN_SCALE[ran], (name, own)


@pytest.mark.parametrize("method", sorted(METHODS), ids=METHOD_IDS)
@pytest.mark.parametrize("case", wa.CASES, ids=wa.IDS)
def test_weighted_vjp_at_the_default_refinement_matches_the_literal_system(gpu_solver_cls, case, method):
    """The same calls with the sweep count left to the library (AdjPlan::nref of run_gradient: 3 on the LDS band and block
    cyclic reduction, 4 on nested dissection and the band in HBM with a scalar; 2 and 1 with a patch or a map).

    Measured on the MI355X: the figures of the test above, except with a scalar under `step` on block cyclic reduction:
    9.4e-8 / 7.1e-7 / 1.1e-6, 0.14 of the bound (3 x 33 x 17 flat, its three sweeps; four leave 0.003, five 6.4e-5).  Per sweep
    count with a scalar, worst fraction of the bound: two sweeps LDS band 0.055, block cyclic reduction 6.8 (that case), nested
    dissection 0.19, band in HBM 0.013; three 0.0061 / 0.14 / 0.013 / 0.013; from four on 0.0061 / 0.0061 / 0.013 / 0.013, which
    is the distance between the two systems and does not move.  The patch and the map are at their converged figures from two
    sweeps on.  The defaults stay as they are."""
    out, _, _ = distances(gpu_solver_cls, case, method, None)
    for name, (ok, d, own) in zip(NAMES, out):
        assert ok, name


# ---- (d) a constant image on a handle of its own ------------------------------------------------------------------------------
FLAT = ((3, 40, 48), "flat", "map", "log3", True)


@pytest.mark.parametrize("method", sorted(METHODS), ids=METHOD_IDS)
def test_a_flat_image_alone_has_no_map_gradient(gpu_solver_cls, method):
    """Image 0 of 3 x 40 x 48 "flat" under log3 on a one-image handle: every row of its matrix carries the active-set weight times
    s^2 (the residual gate's skip rule leaves all of them out), h = 0 on every element, so its own grad_alpha is exactly zero
    for a map, while grad_f = w o p and grad_w = -(u - f) o p are the literal system's (bound with the image's own max|p|)."""
    shape = FLAT[0]
    O, N, M = shape
    alpha, f, w, u, gu = wa.case(*FLAT)
    assert ta.active_counts(u)[0] == N * M - 1
    s = gpu_solver_cls(M, N, 1)
    gf, ga, gw = s.weighted_vjp(u[:1], f[:1], alpha, w[:1], gu[:1], adjoint_method=method)
    st = s.stats()
    s.close()
    rf, _, rw, p = wa.vjp_full(*FLAT, wr.kappa_default(alpha))
    pmax = float(np.abs(p[0]).max())
    print("flat image, %s: kappa_used %.3e attempts %d residual %.3e max|d| grad_f %.3e grad_w %.3e max|grad_alpha| %.3e (max|p| %.3e)"
          % (METHODS[method], st["kappa_used"], st["adjoint_attempts"], st["adjoint_residual"], _dist(gf[0], rf[0]), _dist(gw[0], rw[0]),
             float(np.abs(ga).max()), pmax))
    _check(st, method, M, alpha)
    assert ga.shape == (N, M) and not np.any(ga)
    assert gw.shape == (1, N, M)
    assert _close(gf[0], rf[0], pmax), "grad_f"
    assert _close(gw[0], rw[0], pmax), "grad_w"


# ---- (e) one weight plane for the batch -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", wa.ONE_PLANE, ids=[wa.case_id(*c) for c in wa.ONE_PLANE])
def test_one_plane_grad_w_is_the_image_order_sum(gpu_solver_cls, case):
    """grad_w of an (N, M) weight is the reference's sum over the images within the bound (the constant image's term included), and
    on nested dissection bitwise the sum, in image order, of the one-image calls' grad_w."""
    shape, layout, kind, wname, per_image = case
    O, N, M = shape
    alpha, f, w, u, gu = wa.case(*case)
    assert w.shape == (N, M)
    s = gpu_solver_cls(M, N, O)
    gf, ga, gw = s.weighted_vjp(u, f, alpha, w, gu, adjoint_method=3)
    st = s.stats()
    s.close()
    rf, ra, rw, pmax = wa.vjp_ref(*case, wr.kappa_default(alpha))
    print("%s: max|d| grad_f %.3e grad_alpha %.3e grad_w %.3e (max|p| %.3e)" % (wa.case_id(*case), _dist(gf, rf), _dist(ga, ra),
                                                                            _dist(gw, rw), pmax))
    _check(st, 3, M, alpha)
    assert gw.shape == (N, M) and _close(gw, rw, pmax)
    s1 = gpu_solver_cls(M, N, 1)
    total = np.zeros((N, M))
    for k in range(O):
        gf1, _, gw1 = s1.weighted_vjp(u[k:k + 1], f[k:k + 1], alpha, w, gu[k:k + 1], adjoint_method=3)
        _check(s1.stats(), 3, M, alpha)
        assert gw1.shape == (N, M) and _same(gf1[0], gf[k]), k
        total = total + gw1
    s1.close()
    assert _same(total, gw)


# ---- (f) image groups -------------------------------------------------------------------------------------------------------------
GROUP_CASES = [((3, 40, 48), "flat", kind, "log3", True) for kind in wa.KINDS] + \
              [((3, 33, 17), "flat", kind, "step", True) for kind in wa.KINDS] + [wa.ONE_PLANE[0]]


@pytest.mark.parametrize("case", GROUP_CASES, ids=[wa.case_id(*c) for c in GROUP_CASES])
def test_one_image_per_group_is_the_ungrouped_vjp_bitwise(gpu_solver_cls, case):
    """A budget of 1.5 images' nested-dissection workspace: the constant image, the one with blocks and the untouched one each in
    a group of its own, w read at each group's own plane (one plane: grad_w summed behind the group loop)."""
    shape, layout, kind, wname, per_image = case
    O, N, M = shape
    alpha, f, w, u, gu = wa.case(*case)
    s = gpu_solver_cls(M, N, O)
    gf, ga, gw = s.weighted_vjp(u, f, alpha, w, gu)
    st = s.stats()
    s.close()
    _check(st, 0, M, alpha)
    rf, ra, rw, pmax = wa.vjp_ref(*case, wr.kappa_default(alpha))
    assert _close(gf, rf, pmax) and _close(ga, ra, pmax) and _close(gw, rw, pmax)
    sg = gpu_solver_cls(M, N, O)
    sg.set_option("adjoint_budget_mb", 1.5 * _nd_bytes_per_image(M, N) / 1e6)
    gfg, gag, gwg = sg.weighted_vjp(u, f, alpha, w, gu)
    stg = sg.stats()
    sg.close()
    _check(stg, 0, M, alpha, chunks=3)
    assert gwg.shape == w.shape
    assert _same(gfg, gf) and _same(gag, ga) and _same(gwg, gw)


# ---- (g) device form ----------------------------------------------------------------------------------------------------------------
def test_device_form_on_strips_is_the_host_form_bitwise(gpu_solver_cls):
    import torch
    case = ((2, 40, 48), "strips", "map", "log3", True)
    O, N, M = case[0]
    alpha, f, w, u, gu = wa.case(*case)
    s = gpu_solver_cls(M, N, O)
    gf, ga, gw = s.weighted_vjp(u, f, alpha, w, gu)
    _check(s.stats(), 0, M, alpha)
    t = lambda a: torch.tensor(np.ascontiguousarray(a), device="cuda")
    an, am = alpha.shape
    ut, ft, wt, at, gt = t(u), t(f), t(w), t(alpha), t(gu)
    of, oa, ow = torch.empty_like(ut), torch.empty(am * an, dtype=torch.float64, device="cuda"), torch.empty_like(wt)
    torch.cuda.synchronize()
    s.weighted_vjp_device(ut.data_ptr(), ft.data_ptr(), wt.data_ptr(), O, at.data_ptr(), am, an, gt.data_ptr(),
                          of.data_ptr(), oa.data_ptr(), ow.data_ptr())
    _check(s.stats(), 0, M, alpha)
    s.close()
    assert _same(of.cpu().numpy(), gf) and _same(oa.cpu().numpy().reshape(an, am), ga) and _same(ow.cpu().numpy(), gw)
