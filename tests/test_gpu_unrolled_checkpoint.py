"""GPU checks of the checkpointed tapes (option "tape_checkpoint" / checkpoint_every=) of the three
unrolled models, shared and per image.

Checkpointing is a memory / time switch, not another method: the sweep re-runs each segment with the taping kernel from a
saved state and reverses it with the same reverse kernel, so u and every gradient are held BITWISE to the full-tape run --
for every spacing (not a multiple of a fusion depth, the reverse depth itself, one segment, one iteration per segment,
automatic), every plan, the host and device forms, the handle's buffer and a caller's.  The buffer has the documented size
and nothing is written outside it or, by the sweep, inside it; the handle's last solve, its tape record and the rejections
behave as the full tape's do."""
import ctypes as C
import functools

import numpy as np
import pytest
from conftest import synth_batch

import weighted_unrolled_ref as wur

pytestmark = pytest.mark.gpu

E_ARG, E_NODATA = 1, 3
_dp = C.POINTER(C.c_double)
SHAPES = {"2x70x72": (2, 70, 72), "2x17x33": (2, 17, 33), "1x1x9": (1, 1, 9), "1x9x1": (1, 9, 1)}
K_MAIN, SPACINGS = 203, (7, 8, 64, 203, 500, -1)   # 7: no multiple of a fusion depth; 8: the reverse depth; 203, 500: one segment
PLANES = {"tv": (3, 2), "weighted": (3, 3), "sumregs": (7, 6)}   # (state planes, tape planes per iteration)


def _same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b))


def _all_same(got, ref):
    return all((g is None and r is None) or _same(g, r) for g, r in zip(got, ref))


def _ptr(a):
    return a.ctypes.data_as(_dp) if a is not None else None


@functools.lru_cache(maxsize=None)
def _data(name, seed=5):
    O, N, M = SHAPES[name]
    _, f = synth_batch(O, N, M, seed=seed + M)
    gu = np.random.default_rng(seed + 100).standard_normal(f.shape)
    for a in (f, gu):
        a.setflags(write=False)
    return f, gu


def _alpha(kind, N, M):
    if kind == "scalar":
        return 0.08
    if kind == "patch":
        return np.array([[0.05, 0.1, 0.07], [0.12, 0.06, 0.09]])[:min(2, N), :min(3, M)].copy()
    return 0.05 + 0.1 * np.random.default_rng(8).random((N, M))


def _alpha_each(kind, O, N, M):
    scale = [1.0, 0.6, 1.4][:O]
    if kind == "scalar":
        return np.array([0.08 * c for c in scale])
    return np.stack([c * _alpha(kind, N, M) for c in scale])


def _alpha3(kind, N, M):
    if kind == "vector":
        return np.array([0.03, 0.02, 0.04])
    return 0.02 + 0.04 * np.random.default_rng(8).random((3, N, M))


def _segments(K, c):
    return -(-K // min(c, K))


def _expected_doubles(model, K, c, tot, auto):
    nplanes, _ = PLANES[model]
    ceff = auto(K, model) if c == -1 else min(c, K)
    return nplanes * _segments(K, ceff) * tot


# the three models behind one face: (solve, sweep, tape_doubles) of a solver for fixed arguments
def _model_calls(s, model, each, alpha, w=None):
    if model == "tv":
        solve = s.unrolled_denoise_each if each else s.unrolled_denoise
        sweep = s.unrolled_vjp_each if each else s.unrolled_vjp
        return (lambda **kw: solve(alpha, **kw)), (lambda gu, **kw: sweep(alpha, gu, **kw)), s.unrolled_tape_doubles
    if model == "weighted":
        return ((lambda **kw: s.weighted_unrolled_denoise(alpha, w, **kw)),
                (lambda gu, **kw: s.weighted_unrolled_vjp(alpha, w, gu, **kw)), s.weighted_unrolled_tape_doubles)
    solve = s.sumregs_unrolled_denoise_each if each else s.sumregs_unrolled_denoise
    sweep = s.sumregs_unrolled_vjp_each if each else s.sumregs_unrolled_vjp
    return (lambda **kw: solve(alpha, **kw)), (lambda gu, **kw: sweep(alpha, gu, **kw)), s.sumregs_unrolled_tape_doubles


def _check_bitwise(gpu_solver_cls, name, model, each, alpha, w=None, accels=(1, 0), plain_bytes=None):
    """Every spacing of SPACINGS at K_MAIN, and one iteration per segment at K = 50, against the full tape."""
    O, N, M = SHAPES[name]
    f, gu = _data(name)
    s = gpu_solver_cls(M, N, O)
    s.set_data(f, f)
    solve, sweep, doubles = _model_calls(s, model, each, alpha, w)
    nplanes, tape_planes = PLANES[model]
    for accel in accels:
        for K, spacings in ((K_MAIN, SPACINGS), (50, (1,))):
            u0 = solve(maxiter=K, accel=accel)
            g0 = sweep(gu, maxiter=K, accel=accel)
            full = doubles(maxiter=K)
            assert full == tape_planes * K * M * N * O
            for c in spacings:
                n = doubles(maxiter=K, checkpoint_every=c)
                assert n == _expected_doubles(model, K, c, M * N * O, s.auto_checkpoint_every), (K, c, n)
                u = solve(maxiter=K, accel=accel, checkpoint_every=c)
                st = s.stats()
                assert st["iterations"] == K and st["launches"] >= _segments(K, K if c == -1 else c), st
                if plain_bytes is not None:
                    assert st["bytes_per_px_iter"] == plain_bytes, st
                g = sweep(gu, maxiter=K, accel=accel, checkpoint_every=c)
                assert _same(u, u0), (accel, K, c, float(np.abs(u - u0).max()))
                assert _all_same(g, g0), (accel, K, c, [float(np.abs(np.asarray(a) - np.asarray(b)).max()) for a, b in zip(g, g0)])
                assert s.stats()["adjoint_ms"] > 0.0
    s.close()


# ---- 1. bitwise equality with the full tape ----------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["scalar", "patch", "map"])
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_tv_is_the_full_tape_bitwise(gpu_solver_cls, name, kind):
    O, N, M = SHAPES[name]
    _check_bitwise(gpu_solver_cls, name, "tv", False, _alpha(kind, N, M), plain_bytes=64.0 if kind == "map" and N * M > 1 else 56.0)


@pytest.mark.parametrize("kind", ["scalar", "patch", "map"])
def test_tv_each_is_the_full_tape_bitwise(gpu_solver_cls, kind):
    O, N, M = SHAPES["2x70x72"]
    _check_bitwise(gpu_solver_cls, "2x70x72", "tv", True, _alpha_each(kind, O, N, M))


@pytest.mark.parametrize("wkind", ["mask", "real"])      # mask: one plane with real zeros (gamma = 0); real: O positive planes
@pytest.mark.parametrize("kind", ["scalar", "map"])
def test_weighted_is_the_full_tape_bitwise(gpu_solver_cls, kind, wkind):
    O, N, M = SHAPES["2x70x72"]
    w = wur.weight_of(wkind, O, N, M)
    assert (wkind == "mask") == bool((w == 0).any()) and w.ndim == (2 if wkind == "mask" else 3)
    _check_bitwise(gpu_solver_cls, "2x70x72", "weighted", False, _alpha(kind, N, M), w=w, accels=(1,),
                   plain_bytes=72.0 if kind == "map" else 64.0)


@pytest.mark.parametrize("each", [False, True])
@pytest.mark.parametrize("kind", ["vector", "map"])
@pytest.mark.parametrize("name", ["2x70x72", "2x17x33"])
def test_sumregs_is_the_full_tape_bitwise(gpu_solver_cls, name, kind, each):
    O, N, M = SHAPES[name]
    a = _alpha3(kind, N, M)
    if each:
        a = np.stack([c * a for c in [1.0, 0.7][:O]])
    _check_bitwise(gpu_solver_cls, name, "sumregs", each, a, accels=(1,), plain_bytes=144.0 if kind == "map" else 120.0)


# ---- 2. every plan gives the same bits ---------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["scalar", "map"])
def test_results_do_not_depend_on_the_plan(gpu_solver_cls, kind):
    import torch
    name, K, c = "2x70x72", 200, 24
    O, N, M = SHAPES[name]
    f, gu = _data(name)
    alpha = _alpha(kind, N, M)
    a = np.atleast_1d(np.asarray(alpha, dtype=np.float64))
    an, am = (1, 1) if kind == "scalar" else a.shape
    s = gpu_solver_cls(M, N, O)
    s.set_data(f, f)
    u0 = s.unrolled_denoise(alpha, maxiter=K)
    gf0, ga0 = s.unrolled_vjp(alpha, gu, maxiter=K)
    plans = [dict(), dict(tile_iters=4), dict(tile_iters=8), dict(chains=1), dict(chains=2), dict(use_graph=0),
             dict(chains=2, use_graph=0), dict(tile_iters=4, chains=2)]
    for kw in plans:
        u = s.unrolled_denoise(alpha, maxiter=K, checkpoint_every=c, **kw)
        if "chains" in kw:
            assert s.stats()["launch_chains"] == (kw["chains"] if kw.get("use_graph", 1) else 1)
        gf, ga = s.unrolled_vjp(alpha, gu, maxiter=K, checkpoint_every=c, **kw)
        assert _same(u, u0) and _same(gf, gf0) and _same(ga, ga0), kw
    # the device forms, on the handle's buffer and on a caller's
    at, gt = torch.tensor(a, device="cuda"), torch.tensor(gu, device="cuda")
    out, gfd = torch.empty(O, N, M, dtype=torch.float64, device="cuda"), torch.empty(O, N, M, dtype=torch.float64, device="cuda")
    gad = torch.empty(am * an, dtype=torch.float64, device="cuda")
    ck = torch.empty(s.unrolled_tape_doubles(maxiter=K, checkpoint_every=c), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    for tp in (None, ck.data_ptr(), ck.data_ptr()):   # (a repeated call replays the cached graphs)
        gfd.zero_(); gad.zero_(); torch.cuda.synchronize()
        s.unrolled_denoise_device(at.data_ptr(), am, an, tape_ptr=tp, maxiter=K, checkpoint_every=c)
        s.copy_u_device(out.data_ptr())
        s.unrolled_vjp_device(tp, at.data_ptr(), am, an, gt.data_ptr(), gfd.data_ptr(), gad.data_ptr(), maxiter=K, checkpoint_every=c)
        assert _same(out.cpu().numpy(), u0) and _same(gfd.cpu().numpy(), gf0)
        assert _same(gad.cpu().numpy().reshape(np.shape(ga0)), ga0)
    # a full-tape call between two checkpointed ones of the same shape replays its own graphs, and the reverse
    assert _same(s.unrolled_denoise(alpha, maxiter=K), u0) and _all_same(s.unrolled_vjp(alpha, gu, maxiter=K), (gf0, ga0))
    assert _same(s.unrolled_denoise(alpha, maxiter=K, checkpoint_every=c), u0)
    assert _all_same(s.unrolled_vjp(alpha, gu, maxiter=K, checkpoint_every=c), (gf0, ga0))
    s.close()


# ---- 3. sizes and bounds -----------------------------------------------------------------------------------------------
def test_sizes_match_the_formula_and_the_helper(gpu_solver_cls):
    O, N, M = 2, 17, 33
    s = gpu_solver_cls(M, N, O)
    tot = M * N * O
    for model, doubles in (("tv", s.unrolled_tape_doubles), ("weighted", s.weighted_unrolled_tape_doubles),
                           ("sumregs", s.sumregs_unrolled_tape_doubles)):
        nplanes, tape_planes = PLANES[model]
        for K in (1, 2, 50, 203, 5000):
            full = doubles(maxiter=K)
            assert full == tape_planes * K * tot
            for c in (1, 7, 8, 64, K, K + 300):
                n = doubles(maxiter=K, checkpoint_every=c)
                assert n == nplanes * _segments(K, c) * tot
                if c >= 2 * nplanes and K >= c:    # a segment's state set is then smaller than its tape
                    assert n < full, (model, K, c)
            auto = s.auto_checkpoint_every(K, model)
            assert 1 <= auto <= K
            assert doubles(maxiter=K, checkpoint_every=-1) == nplanes * _segments(K, auto) * tot
            if K >= 50:
                assert doubles(maxiter=K, checkpoint_every=-1) < full
            assert doubles(maxiter=K) == full      # an absent keyword is the full tape again
    s.close()


@pytest.mark.parametrize("model", ["tv", "weighted", "sumregs"])
def test_a_caller_s_buffer_is_written_inside_only_and_read_only_by_the_sweep(gpu_solver_cls, model):
    import torch
    name, K, c, guard = "2x70x72", 203, 7, 4096
    O, N, M = SHAPES[name]
    f, gu = _data(name)
    s = gpu_solver_cls(M, N, O)
    s.set_data(f, f)
    gt = torch.tensor(gu, device="cuda")
    gfd = torch.empty(O, N, M, dtype=torch.float64, device="cuda")
    if model == "sumregs":
        at = torch.tensor(_alpha3("vector", N, M), device="cuda")
        n = s.sumregs_unrolled_tape_doubles(maxiter=K, checkpoint_every=c)
    else:
        at = torch.tensor([0.08], dtype=torch.float64, device="cuda")
        n = (s.unrolled_tape_doubles if model == "tv" else s.weighted_unrolled_tape_doubles)(maxiter=K, checkpoint_every=c)
    gad = torch.empty(at.numel(), dtype=torch.float64, device="cuda")
    wt = torch.tensor(wur.weight_of("mask", O, N, M), device="cuda")
    buf = torch.full((n + guard,), float("nan"), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    if model == "tv":
        s.unrolled_denoise_device(at.data_ptr(), 1, 1, tape_ptr=buf.data_ptr(), maxiter=K, checkpoint_every=c)
    elif model == "weighted":
        s.weighted_unrolled_denoise_device(wt.data_ptr(), 1, at.data_ptr(), 1, 1, tape_ptr=buf.data_ptr(), maxiter=K, checkpoint_every=c)
    else:
        s.sumregs_unrolled_denoise_device(at.data_ptr(), 1, 1, tape_ptr=buf.data_ptr(), maxiter=K, checkpoint_every=c)
    assert bool(torch.isnan(buf[n:]).all()) and not bool(torch.isnan(buf[:n]).any())
    before = buf[:n].clone()
    if model == "tv":
        s.unrolled_vjp_device(buf.data_ptr(), at.data_ptr(), 1, 1, gt.data_ptr(), gfd.data_ptr(), gad.data_ptr(), maxiter=K, checkpoint_every=c)
    elif model == "weighted":
        s.weighted_unrolled_vjp_device(buf.data_ptr(), wt.data_ptr(), 1, at.data_ptr(), 1, 1, gt.data_ptr(), gfd.data_ptr(), gad.data_ptr(),
                                       None, maxiter=K, checkpoint_every=c)
    else:
        s.sumregs_unrolled_vjp_device(buf.data_ptr(), at.data_ptr(), 1, 1, gt.data_ptr(), gfd.data_ptr(), gad.data_ptr(), maxiter=K,
                                      checkpoint_every=c)
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf[n:]).all())
    assert torch.equal(buf[:n].view(torch.int64), before.view(torch.int64))
    assert bool(torch.isfinite(gfd).all()) and bool(gfd.any())
    s.close()


# ---- 4. the handle's state ---------------------------------------------------------------------------------------------
def _code(fn, *a, **kw):
    from bpldenoising_amd._lib import BpltvError
    with pytest.raises(BpltvError) as e:
        fn(*a, **kw)
    return e.value.code


def test_the_last_solve_is_the_plain_solve_s_and_a_sweep_leaves_it(gpu_solver_cls):
    import torch
    name, K, c = "2x70x72", 60, 7
    O, N, M = SHAPES[name]
    f, gu = _data(name)
    s = gpu_solver_cls(M, N, O)
    s.set_data(f, f)
    out = torch.zeros(O, N, M, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    u0 = s.denoise(0.08, maxiter=K)
    g0 = s.duality_gap()
    u = s.unrolled_denoise(0.08, maxiter=K, checkpoint_every=c)
    assert _same(u, u0) and _same(s.duality_gap(), g0)
    s.copy_u_device(out.data_ptr())
    assert _same(out.cpu().numpy(), u0)
    s.unrolled_vjp(0.08, gu, maxiter=K, checkpoint_every=c)
    assert _same(s.duality_gap(), g0)
    out.zero_()
    torch.cuda.synchronize()       # (the library copies on a stream of its own)
    s.copy_u_device(out.data_ptr())
    assert _same(out.cpu().numpy(), u0)
    s.close()


def test_the_tape_record_remembers_the_spacing(gpu_solver_cls):
    import torch
    name, K = "2x17x33", 60
    O, N, M = SHAPES[name]
    f, gu = _data(name)
    f2 = np.ascontiguousarray(f[:, ::-1, :])
    s = gpu_solver_cls(M, N, O)
    s.set_data(f, f)
    u0 = s.unrolled_denoise(0.08, maxiter=K)
    g0 = s.unrolled_vjp(0.08, gu, maxiter=K)
    # a full tape, a checkpointed sweep -- and the other way round, and another spacing
    assert _code(s.unrolled_vjp, 0.08, gu, maxiter=K, checkpoint_every=8) == E_ARG
    assert _all_same(s.unrolled_vjp(0.08, gu, maxiter=K), g0)
    assert _same(s.unrolled_denoise(0.08, maxiter=K, checkpoint_every=8), u0)
    assert _code(s.unrolled_vjp, 0.08, gu, maxiter=K) == E_ARG
    assert _code(s.unrolled_vjp, 0.08, gu, maxiter=K, checkpoint_every=9) == E_ARG
    assert _all_same(s.unrolled_vjp(0.08, gu, maxiter=K, checkpoint_every=8), g0)
    assert s.auto_checkpoint_every(K) == 10         # ceil(sqrt(3 * 60 / 2)): the automatic spacing is another one too
    assert _code(s.unrolled_vjp, 0.08, gu, maxiter=K, checkpoint_every=-1) == E_ARG
    assert _all_same(s.unrolled_vjp(0.08, gu, maxiter=K, checkpoint_every=8), g0)
    # new data: the checkpoints no longer belong to the resident f; a full tape is unaffected
    s.set_data(f2, f2)
    assert _code(s.unrolled_vjp, 0.08, gu, maxiter=K, checkpoint_every=8) == E_NODATA
    s.set_data(f, f)
    assert _code(s.unrolled_vjp, 0.08, gu, maxiter=K, checkpoint_every=8) == E_NODATA
    assert _same(s.unrolled_denoise(0.08, maxiter=K, checkpoint_every=8), u0)
    assert _all_same(s.unrolled_vjp(0.08, gu, maxiter=K, checkpoint_every=8), g0)
    s.unrolled_denoise(0.08, maxiter=K)
    s.set_data(f, f)
    assert _all_same(s.unrolled_vjp(0.08, gu, maxiter=K), g0)
    # a handle without data, a caller's checkpoints: the recompute has no f to read
    ck = torch.empty(s.unrolled_tape_doubles(maxiter=K, checkpoint_every=8), dtype=torch.float64, device="cuda")
    at, gt = torch.tensor([0.08], dtype=torch.float64, device="cuda"), torch.tensor(gu, device="cuda")
    gfd = torch.empty(O, N, M, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    s.unrolled_denoise_device(at.data_ptr(), 1, 1, tape_ptr=ck.data_ptr(), maxiter=K, checkpoint_every=8)
    n = gpu_solver_cls(M, N, O)
    assert _code(n.unrolled_vjp_device, ck.data_ptr(), at.data_ptr(), 1, 1, gt.data_ptr(), gfd.data_ptr(), None, maxiter=K,
                 checkpoint_every=8) == E_NODATA
    n.set_data(f, f)
    n.unrolled_vjp_device(ck.data_ptr(), at.data_ptr(), 1, 1, gt.data_ptr(), gfd.data_ptr(), None, maxiter=K, checkpoint_every=8)
    assert _same(gfd.cpu().numpy(), g0[0])
    n.close()
    s.close()


def test_option_values_and_the_untouched_handle(gpu_solver_cls):
    """The raw ABI: the option is set by hand and stays until it is set again."""
    name, K = "2x17x33", 60
    O, N, M = SHAPES[name]
    f, gu = _data(name)
    s = gpu_solver_cls(M, N, O)
    s.set_data(f, f)
    lib, p, a = s._lib, s.params(maxiter=K), np.array([0.08])
    tot = M * N * O

    def raw():
        u, gf, ga = np.empty((O, N, M)), np.empty((O, N, M)), np.empty(1)
        assert lib.bpltv_unrolled_denoise(s._h, _ptr(a), 1, 1, C.byref(p), _ptr(u)) == 0
        assert lib.bpltv_unrolled_vjp(s._h, _ptr(a), 1, 1, C.byref(p), _ptr(gu), _ptr(gf), _ptr(ga)) == 0
        return u, gf, ga

    def doubles():
        n = C.c_ulonglong(0)
        assert lib.bpltv_unrolled_tape_doubles(s._h, C.byref(p), C.byref(n)) == 0
        return int(n.value)

    first = raw()                                  # before the option was ever touched
    assert doubles() == 2 * K * tot
    s.set_option("tape_checkpoint", 8)
    assert doubles() == 3 * _segments(K, 8) * tot
    assert _all_same(raw(), first)
    for bad in (2.5, -2, -1.5, float("nan"), float("inf"), -float("inf")):
        assert _code(s.set_option, "tape_checkpoint", bad) == E_ARG
        assert doubles() == 3 * _segments(K, 8) * tot       # the old spacing still holds
        assert _all_same(raw(), first)
    s.set_option("tape_checkpoint", -1)
    assert doubles() == 3 * _segments(K, s.auto_checkpoint_every(K)) * tot
    assert _all_same(raw(), first)
    s.set_option("tape_checkpoint", 0)
    assert doubles() == 2 * K * tot
    assert _all_same(raw(), first)
    # a TVSolver method's checkpoint_every= lasts for that call: the handle keeps no spacing for the raw ABI, rejected or not
    assert _same(s.unrolled_denoise(0.08, maxiter=K, checkpoint_every=8), first[0])
    assert doubles() == 2 * K * tot
    assert _code(s.unrolled_vjp, 0.08, gu, maxiter=K + 1, checkpoint_every=8) == E_ARG
    assert doubles() == 2 * K * tot
    assert s.unrolled_tape_doubles(maxiter=K, checkpoint_every=8) == 3 * _segments(K, 8) * tot and doubles() == 2 * K * tot
    s.close()
