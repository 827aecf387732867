"""GPU checks of the weighted TV model with a weight that is NOT one, at the shapes, plans and adjoint solvers that
tests/test_gpu_weighted.py reaches with w = 1 only.  With w = 1 a weight read from the wrong pixel, tile, halo row, image
or plane is still 1, and the plane stride and first-image offset of a launch chain or an image group are invisible; here
every plane is random and differs from every other.

A. bpltv_weighted_denoise against the numpy twin tests/weighted_ref.py (bound 1e-13: the twin itself is 9e-16 from an
   80-bit restatement at these shapes and 203 iterations), the same bits on every plan, another minimum -- another step
   table, another graph -- on a live handle, the duality gap on one row and one column, the device form.
B. bpltv_weighted_vjp against the literal scipy system of tests/weighted_ref.py (pinned on the CPU at these shapes by
   tests/test_weighted_abi.py) on every factorisation -- the band in LDS and in HBM, block cyclic reduction, nested
   dissection -- and in image groups."""
import functools

import numpy as np
import pytest
from conftest import synth_batch

import weighted_ref as wr
from test_gpu_vjp import _nd_bytes_per_image
from test_gpu_weighted import E_UNSUPPORTED, _alpha, _same

pytestmark = pytest.mark.gpu


def _id(shape):
    return "x".join(str(n) for n in shape)


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


# ---- the tiling of a weighted solve, restated (csrc/tiling.hpp tile_span, bpltv.hip weighted_plan) -----------------------
REGION = 32


def _depth(N, M, tile_iters=8):
    """Iterations per launch: a halo must leave a core on an axis longer than one region."""
    cap = lambda L: 32 if L <= REGION else (REGION - 1) // 2
    return min(tile_iters, cap(M), cap(N))


def _seams(L, T):
    """Where the core of one tile ends and the next one's begins along an axis of L pixels, halo T."""
    if L <= REGION:
        return []
    out, a = [], 0
    while True:
        cs = 0 if a == 0 else (REGION - T) + (a - 1) * (REGION - 2 * T)
        o = 0 if a == 0 else cs - T
        if o + REGION >= L:
            return out
        out.append(o + REGION - T)
        a += 1


def test_the_restated_tiling_has_the_seams_the_mask_is_built_on():
    assert _depth(70, 72) == 8 and _seams(72, 8) == [24, 40, 56] and _seams(70, 8) == [24, 40, 56]
    assert _seams(33, 8) == [24] and _seams(48, 8) == [24] and _seams(40, 8) == [24] and _seams(17, 8) == []
    assert _seams(72, 5) == [27, 49] and len(_seams(72, 1)) == 2


# ---- A. denoise --------------------------------------------------------------------------------------------------------
# (2, 70, 72): four tiles per axis, the middle ones with a halo on both sides; (2, 17, 33): odd sizes, two tiles along i;
# (3, 40, 48): two tiles per axis, three images (two launch chains of two and one); one row; one column
SHAPES = [(2, 70, 72), (2, 17, 33), (3, 40, 48), (1, 1, 9), (1, 9, 1)]
KINDS = ["scalar", "patch", "map"]
WEIGHTS = ["rand1", "randO", "log", "mask"]


@functools.lru_cache(maxsize=None)
def _data(shape):
    O, N, M = shape
    return _frozen(synth_batch(O, N, M, seed=40 + M)[1])[0]


@functools.lru_cache(maxsize=None)
def _weight(shape, name):
    """rand1 / randO: 0.25 + 3.75 U(0, 1) as one plane / one plane per image, the planes all different, the global minimum in
    the LAST image and every other image's own minimum larger (gamma is the minimum over the call);
    log: 10^U(-3, 3) per image, 1e-3 and 1e3 both present;
    mask: randO with zeros on the first and last image row and column and in a 6 x 6 block across a tile seam in both axes
    (across the image centre on an axis of one tile); on one row / one column a run of zeros that includes an end pixel."""
    O, N, M = shape
    rng = np.random.default_rng(1000 + 7 * N + M + {"rand1": 0, "randO": 1, "log": 2, "mask": 1}[name])
    if name == "rand1":
        return _frozen(0.25 + 3.75 * rng.random((N, M)))[0]
    if name == "log":
        w = 10.0 ** rng.uniform(-3.0, 3.0, (O, N, M))
        w[-1, N // 2, M // 2] = 1e-3
        w[0, 0, 0] = 1e3
        return _frozen(w)[0]
    w = 0.25 + 3.75 * rng.random((O, N, M))
    w[:-1] = np.maximum(w[:-1], 0.5)
    w[-1, N // 2, M // 3] = 0.25
    if name == "mask":
        if N == 1 or M == 1:
            w.reshape(O, -1)[:, -3:] = 0.0
        else:
            T = _depth(N, M)
            si, sj = _seams(M, T), _seams(N, T)
            ci = si[len(si) // 2] if si else M // 2
            cj = sj[0] if sj else N // 2
            w[:, cj - 3:cj + 3, ci - 3:ci + 3] = 0.0
            w[:, 0, :] = w[:, -1, :] = 0.0
            w[:, :, 0] = w[:, :, -1] = 0.0
    return _frozen(w)[0]


@functools.lru_cache(maxsize=None)
def _twin(shape, kind, wname, maxiter, scale=1.0):
    """(u, y1, y2) of the numpy twin; computed once per case and shared, read-only."""
    O, N, M = shape
    return _frozen(*wr.pdhg(_data(shape), _alpha(kind, N, M), scale * _weight(shape, wname), maxiter, return_dual=True))


def _solver(cls, shape):
    O, N, M = shape
    s = cls(M, N, O)
    s.set_data(_data(shape), _data(shape))
    return s


def test_the_weights_are_what_the_checks_need():
    for shape in SHAPES:
        O, N, M = shape
        w1, wO, wl, wm = (_weight(shape, n) for n in WEIGHTS)
        assert w1.shape == (N, M) and wO.shape == wl.shape == wm.shape == shape
        assert wO.min() == wO[-1].min() == 0.25 and all(wO[k].min() >= 0.5 for k in range(O - 1))
        assert all(not _same(wO[a], wO[b]) for a in range(O) for b in range(a)) and not _same(wO[0], w1)
        assert wl.min() == 1e-3 and wl.max() == 1e3
        assert wm.min() == 0.0 and wm[0].flat[-1] == 0.0 and np.count_nonzero(wm) > wm.size // 3
    # the mask's block lies across the seams between the cores of two tiles, in both axes, at the default depth
    wm = _weight((2, 70, 72), "mask")
    assert _depth(70, 72) == 8 and 40 in _seams(72, 8) and 24 in _seams(70, 8)
    assert not wm[:, 21:27, 37:43].any() and wm[:, 20, 37:43].all() and wm[:, 21:27, 43].all()


@pytest.mark.parametrize("wname", WEIGHTS)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_denoise_with_a_real_weight_matches_the_twin(gpu_solver_cls, shape, kind, wname):
    """max|u - twin| <= 1e-13 after 7 and 203 iterations.  Measured on the MI355X over the 60 cases: at most 4.4e-16 (one
    plane), 5.6e-16 (per image), 5.6e-16 (six decades), 4.4e-16 (mask)."""
    O, N, M = shape
    w = _weight(shape, wname)
    s = _solver(gpu_solver_cls, shape)
    for maxiter in (7, 203):
        u = s.weighted_denoise(_alpha(kind, N, M), w, maxiter=maxiter)
        d = float(np.abs(u - _twin(shape, kind, wname, maxiter)[0]).max())
        print("%s %s %s maxiter %d: max|du| = %.3e" % (_id(shape), kind, wname, maxiter, d))
        assert d <= 1e-13
        st = s.stats()
        assert st["iterations"] == maxiter and st["tile_iters"] == _depth(N, M), st
        assert st["tiles"] == O * (len(_seams(M, st["tile_iters"])) + 1) * (len(_seams(N, st["tile_iters"])) + 1), st
    s.close()


@pytest.mark.parametrize("kind", KINDS)
def test_each_image_reads_its_own_weight_plane(gpu_solver_cls, kind):
    """Teeth of the twin check: the twin with the two images' planes swapped is more than 1e-6 away."""
    shape = (2, 70, 72)
    O, N, M = shape
    wO = _weight(shape, "randO")
    s = _solver(gpu_solver_cls, shape)
    u = s.weighted_denoise(_alpha(kind, N, M), wO, maxiter=203)
    s.close()
    swapped = wr.pdhg(_data(shape), _alpha(kind, N, M), wO[::-1].copy(), 203)
    d = np.abs(u - swapped).max(axis=(1, 2))
    print("%s: max|u - twin(swapped planes)| per image = %s" % (kind, d))
    assert np.all(d > 1e-6)
    assert float(np.abs(u - _twin(shape, kind, "randO", 203)[0]).max()) <= 1e-13


@pytest.mark.parametrize("wname", ["randO", "mask"])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", [(2, 70, 72), (3, 40, 48)], ids=_id)
def test_every_plan_gives_the_same_bits_with_a_real_weight(gpu_solver_cls, shape, kind, wname):
    """Other fusion depths (other tiles, other halos), no graph, and two launch chains -- the second chain starts at image
    1 (3 x 40 x 48: at image 2), so its w is read at img0 * wstride -- in and out of phase (203 / 200 iterations)."""
    O, N, M = shape
    alpha, w = _alpha(kind, N, M), _weight(shape, wname)
    s = _solver(gpu_solver_cls, shape)
    u0 = s.weighted_denoise(alpha, w, maxiter=203)
    assert s.stats()["tile_iters"] == 8
    assert float(np.abs(u0 - _twin(shape, kind, wname, 203)[0]).max()) <= 1e-13
    for kw in (dict(tile_iters=5), dict(tile_iters=1), dict(use_graph=0)):
        u1 = s.weighted_denoise(alpha, w, maxiter=203, **kw)
        assert _same(u1, u0), (kw, float(np.abs(u1 - u0).max()))
        assert s.stats()["tile_iters"] == kw.get("tile_iters", 8)
    for maxiter in (203, 200):
        u0 = s.weighted_denoise(alpha, w, maxiter=maxiter)
        assert s.stats()["launch_chains"] == 1      # (the default plan of so small a batch)
        u2 = s.weighted_denoise(alpha, w, maxiter=maxiter, chains=2)
        assert s.stats()["launch_chains"] == min(2, O)
        assert _same(u2, u0), (maxiter, float(np.abs(u2 - u0).max()))
    s.close()


@pytest.mark.parametrize("wname", ["rand1", "randO"])
def test_another_minimum_on_a_live_handle(gpu_solver_cls, wname):
    """A weight of the same shape with another minimum after a graph replay: another gamma, another step table, another
    graph.  0.5 w against the twin; w again: the first solve's bits."""
    shape, kind = (2, 70, 72), "map"
    O, N, M = shape
    alpha, w = _alpha(kind, N, M), _weight(shape, wname)
    s = _solver(gpu_solver_cls, shape)
    u1 = s.weighted_denoise(alpha, w, maxiter=203)
    assert _same(s.weighted_denoise(alpha, w, maxiter=203), u1)
    assert s.stats()["graph_used"] == 1
    uh = s.weighted_denoise(alpha, 0.5 * w, maxiter=203)
    d = float(np.abs(uh - _twin(shape, kind, wname, 203, 0.5)[0]).max())
    print("%s, 0.5 w: max|du| = %.3e" % (wname, d))
    assert d <= 1e-13
    assert float(np.abs(uh - u1).max()) > 1e-6        # (another problem, not the first one replayed)
    assert _same(s.weighted_denoise(alpha, w, maxiter=203), u1)
    assert float(np.abs(u1 - _twin(shape, kind, wname, 203)[0]).max()) <= 1e-13
    s.close()


@pytest.mark.parametrize("wname", ["rand1", "randO"])
@pytest.mark.parametrize("shape", [(1, 1, 9), (1, 9, 1), (2, 70, 72)], ids=_id)
def test_gap_at_the_edges_is_the_twin_s(gpu_solver_cls, shape, wname):
    O, N, M = shape
    alpha, w, f = _alpha("map", N, M), _weight(shape, wname), _data(shape)
    s = _solver(gpu_solver_cls, shape)
    s.weighted_denoise(alpha, w, maxiter=50, fetch=False)
    g = s.duality_gap()
    s.close()
    u, y1, y2 = _twin(shape, "map", wname, 50)
    ref = wr.gap(u, y1, y2, f, alpha, w)
    energy = wr.primal_energy(u, f, alpha, w)
    print("%s %s: gap %s twin %s energy %s" % (_id(shape), wname, g, ref, energy))
    assert g.shape == ref.shape == (O,) and np.all(np.abs(g - ref) <= 1e-11 * energy)


@pytest.mark.parametrize("kind", ["scalar", "map"])
def test_device_form_under_two_chains_is_the_host_form_bitwise(gpu_solver_cls, kind):
    import torch
    shape = (2, 70, 72)
    O, N, M = shape
    alpha, w = _alpha(kind, N, M), _weight(shape, "randO")
    a = np.atleast_1d(np.asarray(alpha, dtype=np.float64))
    an, am = (1, 1) if kind == "scalar" else a.shape
    s = _solver(gpu_solver_cls, shape)
    u0 = s.weighted_denoise(alpha, w, maxiter=203, chains=2)
    assert float(np.abs(u0 - _twin(shape, kind, "randO", 203)[0]).max()) <= 1e-13
    wt, at = torch.tensor(w, device="cuda"), torch.tensor(a, device="cuda")
    out = torch.empty(O, N, M, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    s.weighted_denoise_device(wt.data_ptr(), O, at.data_ptr(), am, an, maxiter=203, chains=2)
    assert s.stats()["launch_chains"] == 2
    s.copy_u_device(out.data_ptr())
    assert _same(out.cpu().numpy(), u0)
    s.close()


# ---- B. the vector-Jacobian product ------------------------------------------------------------------------------------
# params.reserved[4] -> what stats()["adjoint_method"] must say (bpltv_stats_t::adjoint_method 5 / 1 / 3 / 2)
METHODS = {0: "auto", 1: "band", 2: "bcr", 3: "nd"}


def _expected_method(m, M):
    return {0: "nd", 1: "band" if M <= 138 else "band-hbm", 2: "bcr", 3: "nd"}[m]


def _bcr_applies(M, N):
    return M <= 128 and N >= 2


@functools.lru_cache(maxsize=None)
def _vjp_case(shape, kind, per_image=True):
    """(alpha, f, w, u, gu) of weighted_ref.vjp_case at this shape: the twin's iterate with two flat blocks planted."""
    O, N, M = shape
    alpha = _alpha(kind, N, M)
    return (alpha,) + _frozen(*wr.vjp_case(alpha, seed=21, O=O, N=N, M=M, per_image=per_image))


@functools.lru_cache(maxsize=None)
def _vjp_ref(shape, kind, per_image, kappa):
    """The literal system with the weight the library used, solved once per (case, kappa) and shared."""
    alpha, f, w, u, gu = _vjp_case(shape, kind, per_image)
    gf, ga, gw, p = wr.vjp(u, f, alpha, w, gu, kappa, refine=10)
    return gf, ga, gw, float(np.abs(p).max())


def _close(a, b, pmax, factor=1.0):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and bool(np.all(np.abs(a - b) <= factor * (1e-8 * pmax + 1e-6 * np.abs(b))))


# per-image weights with every parameter kind, and one case per shape with one plane for the batch
VJP_CASES = [(shape, kind, True) for shape in wr.VJP_SHAPES for kind in KINDS] + [(shape, "map", False) for shape in wr.VJP_SHAPES]
VJP_IDS = ["%s-%s-%s" % (_id(sh), k, "wO" if per else "w1") for sh, k, per in VJP_CASES]


@pytest.mark.parametrize("method", sorted(METHODS), ids=[METHODS[m] for m in sorted(METHODS)])
@pytest.mark.parametrize("case", VJP_CASES, ids=VJP_IDS)
def test_vjp_on_every_factorisation_matches_the_literal_system(gpu_solver_cls, case, method):
    """grad_f, grad_alpha and grad_w against the literal (diag(w) + K) p = gu with the kappa the library reports, rtol 1e-6
    / atol 1e-8 max|p|, on the band (LDS; HBM at M = 140), block cyclic reduction (refused at M = 140) and nested
    dissection: systems with s = 1/sqrt(w) != 1 next to the 1e14 active-set weight.

    Measured on the MI355X (largest |difference| of grad_f / grad_alpha / grad_w over the shapes; kappa_used 1e14 for a scalar,
    6.7e7 for a patch or a map; adjoint_attempts 1 and adjoint_residual <= 9.7e-11 everywhere):
        patch, map   every method                     9.2e-9 / 1.6e-9 / 1.3e-10
        scalar       band (LDS, 3 sweeps)             3.6e-9 / 9.4e-9 / 1.2e-10
        scalar       block cyclic reduction (3)       3.6e-9 / 2.1e-9 / 1.2e-10
        scalar       band in HBM (4 sweeps), M = 140  4.7e-11 / 1.6e-10 / 7.0e-12
        scalar       nested dissection (4 sweeps)     3.6e-9 / 2.0e-9 / 1.2e-10
    With the two sweeps bpltv_vjp runs on the direct factorisations nested dissection left 5.3e-7 / 5.0e-7 / 1.9e-8 on
    1 x 12 x 140 (max|p| 1.7, a 2 x 125 flat block) and failed here, the band in HBM 2.1e-8; the scalar system gets four
    (DESIGN.md sections 4.3 and 4.5)."""
    from bpldenoising_amd._lib import BpltvError
    shape, kind, per_image = case
    O, N, M = shape
    alpha, f, w, u, gu = _vjp_case(shape, kind, per_image)
    s = gpu_solver_cls(M, N, O)
    if method == 2 and not _bcr_applies(M, N):
        with pytest.raises(BpltvError) as e:
            s.weighted_vjp(u, f, alpha, w, gu, adjoint_method=2)
        assert e.value.code == E_UNSUPPORTED
        method = 0                                   # ... and the handle goes on working
    gf, ga, gw = s.weighted_vjp(u, f, alpha, w, gu, adjoint_method=method)
    st = s.stats()
    s.close()
    rf, ra, rw, pmax = _vjp_ref(shape, kind, per_image, st["kappa_used"])
    d = [float(np.abs(np.asarray(a) - np.asarray(b)).max()) for a, b in ((gf, rf), (ga, ra), (gw, rw))]
    print("%s %s %s %s: method %s kappa_used %.3e attempts %d residual %.3e max|d| grad_f %.3e grad_alpha %.3e grad_w %.3e "
          "(max|p| %.3e)" % (_id(shape), kind, "wO" if per_image else "w1", METHODS[method], st["adjoint_method"],
                             st["kappa_used"], st["adjoint_attempts"], st["adjoint_residual"], d[0], d[1], d[2], pmax))
    assert st["adjoint_method"] == _expected_method(method, M), st
    assert st["adjoint_residual"] <= 1e-6 and st["adjoint_attempts"] == 1 and st["adjoint_chunks"] == 1, st
    assert gw.shape == w.shape
    for name, a, b in (("grad_f", gf, rf), ("grad_alpha", ga, ra), ("grad_w", gw, rw)):
        assert _close(a, b, pmax), name


@pytest.mark.parametrize("shape,kind", list(zip(wr.VJP_SHAPES, ["map", "scalar", "patch", "map"])),
                         ids=[_id(sh) for sh in wr.VJP_SHAPES])
def test_the_factorisations_agree_with_each_other(gpu_solver_cls, shape, kind):
    """grad_f of the band, block cyclic reduction and nested dissection pairwise within twice the tolerance each is held to
    against the literal system (a sanity line beside the test above, not in its place)."""
    O, N, M = shape
    alpha, f, w, u, gu = _vjp_case(shape, kind, True)
    s = gpu_solver_cls(M, N, O)
    out, kap = {}, {}
    for m in (1, 2, 3):
        if m == 2 and not _bcr_applies(M, N):
            continue
        out[m] = s.weighted_vjp(u, f, alpha, w, gu, adjoint_method=m, want_alpha=False, want_w=False)[0]
        kap[m] = s.stats()["kappa_used"]
    s.close()
    assert len(set(kap.values())) == 1, kap          # (one system: no factorisation retried with a smaller weight)
    pmax = _vjp_ref(shape, kind, True, kap[1])[3]
    for a in out:
        for b in out:
            if a < b:
                print("%s %s: methods %d / %d max|d grad_f| = %.3e" % (_id(shape), kind, a, b, float(np.abs(out[a] - out[b]).max())))
                assert _close(out[a], out[b], pmax, 2.0), (a, b)


@pytest.mark.parametrize("method", [1, 2, 3], ids=["band", "bcr", "nd"])
@pytest.mark.parametrize("kind", KINDS)
def test_unit_weight_vjp_is_the_unweighted_vjp_on_every_factorisation(gpu_solver_cls, kind, method):
    O, N, M = 3, 20, 16
    _, f = synth_batch(O, N, M, seed=15)
    alpha = _alpha(kind, N, M)
    s = gpu_solver_cls(M, N, O)
    s.set_data(f, f)
    u = s.denoise(alpha, maxiter=300)
    gu = np.random.default_rng(16).standard_normal(u.shape)
    gf0, ga0 = s.vjp(u, alpha, gu, adjoint_method=method)
    st0 = s.stats()
    assert st0["adjoint_method"] == _expected_method(method, M)
    for w in (np.ones((N, M)), np.ones((O, N, M))):
        gf, ga, gw = s.weighted_vjp(u, f, alpha, w, gu, adjoint_method=method)
        st = s.stats()
        assert _same(gf, gf0) and _same(ga, ga0)
        assert st["adjoint_method"] == st0["adjoint_method"] and st["kappa_used"] == st0["kappa_used"], (st, st0)
        assert st["adjoint_attempts"] == st0["adjoint_attempts"] and st["adjoint_residual"] <= 1e-6, st
        want = -(u - f) * gf0
        assert np.linalg.norm(gw - (want.sum(axis=0) if w.ndim == 2 else want)) <= 1e-15 * np.linalg.norm(want)
    s.close()


@pytest.mark.parametrize("per_image", [True, False], ids=["wO", "w1"])
@pytest.mark.parametrize("shape", [(3, 33, 17), (2, 70, 72)], ids=_id)
def test_vjp_in_image_groups_is_the_ungrouped_vjp_bitwise(gpu_solver_cls, shape, per_image):
    """A budget of 2.5 images' nested-dissection workspace: groups of two images (2 x 70 x 72: of one), the second group's w
    read at its first image's plane; with one plane for the batch grad_w is summed over the images behind the group loop."""
    O, N, M = shape
    kind = "map"
    alpha, f, w, u, gu = _vjp_case(shape, kind, per_image)
    s = gpu_solver_cls(M, N, O)
    gf, ga, gw = s.weighted_vjp(u, f, alpha, w, gu)
    st = s.stats()
    assert st["adjoint_chunks"] == 1 and st["adjoint_method"] == "nd"
    rf, ra, rw, pmax = _vjp_ref(shape, kind, per_image, st["kappa_used"])
    assert _close(gf, rf, pmax) and _close(ga, ra, pmax) and _close(gw, rw, pmax)
    s.close()
    sg = gpu_solver_cls(M, N, O)
    sg.set_option("adjoint_budget_mb", (2.5 if O > 2 else 1.5) * _nd_bytes_per_image(M, N) / 1e6)
    gfg, gag, gwg = sg.weighted_vjp(u, f, alpha, w, gu)
    stg = sg.stats()
    sg.close()
    assert stg["adjoint_chunks"] > 1 and stg["kappa_used"] == st["kappa_used"], stg
    assert gwg.shape == w.shape
    assert _same(gfg, gf) and _same(gag, ga) and _same(gwg, gw)


def test_vjp_device_form_on_the_hbm_band_is_the_host_form_bitwise(gpu_solver_cls):
    import torch
    shape, kind = (1, 12, 140), "patch"
    O, N, M = shape
    alpha, f, w, u, gu = _vjp_case(shape, kind, True)
    s = gpu_solver_cls(M, N, O)
    gf, ga, gw = s.weighted_vjp(u, f, alpha, w, gu, adjoint_method=1)
    assert s.stats()["adjoint_method"] == "band-hbm"
    t = lambda a: torch.tensor(np.ascontiguousarray(a), device="cuda")
    an, am = alpha.shape
    ut, ft, wt, at, gt = t(u), t(f), t(w), t(alpha), t(gu)
    of, oa, ow = torch.empty_like(ut), torch.empty(am * an, dtype=torch.float64, device="cuda"), torch.empty_like(wt)
    torch.cuda.synchronize()
    s.weighted_vjp_device(ut.data_ptr(), ft.data_ptr(), wt.data_ptr(), O, at.data_ptr(), am, an, gt.data_ptr(),
                          of.data_ptr(), oa.data_ptr(), ow.data_ptr(), adjoint_method=1)
    assert s.stats()["adjoint_method"] == "band-hbm"
    s.close()
    assert _same(of.cpu().numpy(), gf) and _same(oa.cpu().numpy().reshape(an, am), ga) and _same(ow.cpu().numpy(), gw)
