"""GPU checks of forward mode through the TV-L1 and the TV-KL iterations (bpltv_lone_unrolled_jvp, bpltv_kl_unrolled_jvp, their
device forms and the two _gauss_newton calls), both models parametrised.

The sweep's primal is tied to bpltv_lone_denoise / bpltv_kl_denoise bit for bit; its tangent is held against the numpy twin
tests/l1_kl_jvp_ref.py (pinned on the CPU by tests/test_l1_kl_jvp_abi.py), against the model's reverse sweep by the transpose
identity and against central differences of the solve itself; every plan (fusion depth, launch chains, graphs, host or device
form, one direction or several) gives the same bits; the weighted, the L1 and the KL sweep on one handle, in every order, each
give what a fresh handle gives; and a sweep, accepted or rejected, leaves the handle's last solve, tapes and statistics as they
were."""
import ctypes as C
import functools
import itertools

import numpy as np
import pytest

import kl_ref as kr
import l1_kl_jvp_ref as j
import unrolled_ref as ur
import weighted_unrolled_jvp_ref as wuj
from oracle import np_twin as tw

pytestmark = pytest.mark.gpu

E_ARG, E_NODATA, E_UNSUPPORTED = 1, 3, 6
_dp = C.POINTER(C.c_double)
SHAPES = j.GPU_SHAPES
METHOD = {"l1": "l1-unrolled-jvp", "kl": "kl-unrolled-jvp"}
CNAME = {"l1": "lone", "kl": "kl"}


def _same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b))


def _ptr(a):
    return a.ctypes.data_as(_dp) if a is not None else None


def _m(s, model, what):
    """TVSolver's entry of a model: l1_denoise, kl_unrolled_jvp, ..."""
    return getattr(s, "%s_%s" % (model, what))


@functools.lru_cache(maxsize=None)
def _data(model, name):
    """(f, cotangent gu) of a model's shape: the committed helpers'; read-only."""
    f, gu = j.REF[model].gpu_data(name)
    f.setflags(write=False)
    gu.setflags(write=False)
    return f, gu


def _alpha(model, kind, N, M):
    return j.REF[model].alpha_of(kind, N, M)


@functools.lru_cache(maxsize=None)
def _weight(name, wkind):
    w = j.REF["l1"].weight_of(wkind, *SHAPES[name])
    w.setflags(write=False)
    return w


# ---- 1. the primal is the model's denoise, bit for bit -----------------------------------------------------------------
@pytest.mark.parametrize("kind", j.KINDS)
@pytest.mark.parametrize("name", sorted(SHAPES))
@pytest.mark.parametrize("model", j.MODELS)
def test_primal_is_the_model_s_denoise_bitwise(gpu_solver_cls, model, name, kind):
    O, N, M = SHAPES[name]
    f, _ = _data(model, name)
    alpha = _alpha(model, kind, N, M)
    s = gpu_solver_cls(M, N, O)
    s.set_data(f, f)
    for wkind in j.WEIGHTS:
        w = _weight(name, wkind)
        df, dalpha, _, dw = j.tangents_of(name, wkind, kind)
        for maxiter in (1, 7, 203):
            u0 = _m(s, model, "denoise")(alpha, w, maxiter=maxiter)
            du, u1 = _m(s, model, "unrolled_jvp")(alpha, w, df=df, dalpha=dalpha, dw=dw, want_u=True, maxiter=maxiter)
            assert _same(u1, u0), (wkind, maxiter, float(np.abs(u1 - u0).max()))
            assert np.isfinite(du).all() and du.any()
            assert s.stats()["adjoint_method"] == METHOD[model] and s.stats()["adjoint_ms"] > 0.0
    s.close()


# ---- 2. the tangent against the twin -----------------------------------------------------------------------------------
@pytest.mark.parametrize("wkind", j.WEIGHTS)
@pytest.mark.parametrize("kind", j.KINDS)
@pytest.mark.parametrize("name", j.GRADIENT_SHAPES)
@pytest.mark.parametrize("model", j.MODELS)
def test_tangent_matches_the_twin(gpu_solver_cls, model, name, kind, wkind):
    """1e-11 * max|du0|, the bound every tangent sweep of the project meets (DESIGN.md section 4.20 holds the measured maximum):
    each tangent alone and all three together.  The listed dalpha-alone cases of L1 whose tangent is identically zero
    (l1_kl_jvp_ref.L1_ZERO_DALPHA) must be exactly zero here too and are no tangent check."""
    O, N, M = SHAPES[name]
    f, _ = _data(model, name)
    w = _weight(name, wkind)
    alpha = _alpha(model, kind, N, M)
    tangents = j.tangents_of(name, wkind, kind)
    s = gpu_solver_cls(M, N, O)
    s.set_data(f, f)
    checked = 0
    for K in j.GRADIENT_K:
        for direction in j.DIRECTIONS:
            tf, ta, _, tw_ = j.select(direction, *tangents)
            _, du0 = j.twin_tangent(model, name, kind, wkind, K, direction)
            du = _m(s, model, "unrolled_jvp")(alpha, w, df=tf, dalpha=ta, dw=tw_, maxiter=K)
            if j.is_zero_case(model, name, kind, wkind, K, direction):
                assert not du0.any() and not du.any()
                continue
            d, m = float(np.abs(du - du0).max()), float(np.abs(du0).max())
            print("%s %s %s %s K %d d%s: du %.2e (bound %.2e, max|ref| %.2e, rel %.1e)" % (model, name, kind, wkind, K, direction, d, 1e-11 * m, m, d / m))
            assert m > 0.0 and d <= 1e-11 * m
            checked += 1
    assert checked >= 7
    s.close()


# ---- 3. the transpose identity against the model's reverse sweep -----------------------------------------------------------
@pytest.mark.parametrize("wkind", ["real", "mask"])       # real: wo = O, mask: wo = 1
@pytest.mark.parametrize("kind", j.KINDS)
@pytest.mark.parametrize("name", j.GRADIENT_SHAPES)
@pytest.mark.parametrize("model", j.MODELS)
def test_tangent_is_the_transpose_of_the_reverse_sweep(gpu_solver_cls, model, name, kind, wkind):
    """<du, gu> = <df, grad_f(gu)> + <dalpha, grad_alpha(gu)> + <dw, grad_w(gu)> to 1e-11 * sum|du * gu|: the taped solve, the
    tangent sweep and the reverse sweep on one handle."""
    O, N, M = SHAPES[name]
    f, gu = _data(model, name)
    w = _weight(name, wkind)
    assert w.ndim == (3 if wkind == "real" else 2)
    alpha = _alpha(model, kind, N, M)
    df, da, _, dw = j.tangents_of(name, wkind, kind)
    s = gpu_solver_cls(M, N, O)
    s.set_data(f, f)
    for K in j.GRADIENT_K:
        _m(s, model, "unrolled_denoise")(alpha, w, maxiter=K)
        du = _m(s, model, "unrolled_jvp")(alpha, w, df=df, dalpha=da, dw=dw, maxiter=K)
        gf, ga, gw = _m(s, model, "unrolled_vjp")(alpha, w, gu, maxiter=K)
        lhs = float((du * gu).sum())
        rhs = float((df * gf).sum()) + float((np.asarray(da) * np.asarray(ga)).sum()) + float((dw * gw).sum())
        scale = float(np.abs(du * gu).sum())
        print("%s %s %s %s K %d: |lhs - rhs| %.2e  bound %.2e" % (model, name, kind, wkind, K, abs(lhs - rhs), 1e-11 * scale))
        assert scale > 0.0 and abs(lhs - rhs) <= 1e-11 * scale
    s.close()


# ---- 4. central differences of the model's denoise itself ---------------------------------------------------------------
@pytest.mark.parametrize("model", j.MODELS)
def test_tangents_against_central_differences_on_the_device(gpu_solver_cls, model):
    """The case, step and bound (1e-5 relative in the maximum norm) of tests/test_l1_kl_jvp_abi.py, where the twin alone meets it:
    one direction each in alpha, f and w."""
    ref = j.REF[model]
    _, f, w, df, dw = ref.central_difference_case()
    alpha, K, h = ref.CD_ALPHA, ref.CD_K, ref.CD_H
    s = gpu_solver_cls(28, 24, 1)
    for what, tf, ta, tw_ in (("alpha", None, 1.0, None), ("f", df, None, None), ("w", None, None, dw)):
        s.set_data(f, f)
        du = _m(s, model, "unrolled_jvp")(alpha, w, df=tf, dalpha=ta, dw=tw_, maxiter=K)
        ap, am = (alpha + h * ta, alpha - h * ta) if ta is not None else (alpha, alpha)
        wp, wm = (w + h * tw_, w - h * tw_) if tw_ is not None else (w, w)
        if tf is not None:
            s.set_data(f + h * tf, f + h * tf)
        up = _m(s, model, "denoise")(ap, wp, maxiter=K)
        if tf is not None:
            s.set_data(f - h * tf, f - h * tf)
        fd = (up - _m(s, model, "denoise")(am, wm, maxiter=K)) / (2 * h)
        d, m = float(np.abs(du - fd).max()), float(np.abs(fd).max())
        print("%s d/d%s: max|du - fd| %.3e  max|fd| %.3e  rel %.2e" % (model, what, d, m, d / m))
        assert d <= 1e-5 * m, what
    s.close()


# ---- 5. every plan gives the same bits --------------------------------------------------------------------------------
@pytest.mark.parametrize("wkind", ["real", "mask"])       # real: wo = O, mask: wo = 1
@pytest.mark.parametrize("kind", ["scalar", "map"])
@pytest.mark.parametrize("model", j.MODELS)
def test_results_do_not_depend_on_the_plan(gpu_solver_cls, model, kind, wkind):
    import torch
    name = "2x70x72"
    O, N, M = SHAPES[name]
    f, _ = _data(model, name)
    w = _weight(name, wkind)
    wo = O if w.ndim == 3 else 1
    alpha = _alpha(model, kind, N, M)
    a = np.atleast_1d(np.asarray(alpha, dtype=np.float64))
    an, am = (1, 1) if kind == "scalar" else a.shape
    rng = np.random.default_rng(21)
    df3 = rng.standard_normal((3,) + f.shape)
    da3 = rng.standard_normal((3,) + np.shape(alpha))
    dw3 = rng.standard_normal((3,) + w.shape)
    s = gpu_solver_cls(M, N, O)
    s.set_data(f, f)
    jvp, dev = _m(s, model, "unrolled_jvp"), _m(s, model, "unrolled_jvp_device")
    for K in (203, 200):   # 200 iterations at depth 8: the second chain runs half a launch out of phase
        du0, u0 = jvp(alpha, w, df=df3, dalpha=da3, dw=dw3, want_u=True, maxiter=K)
        assert _same(u0, _m(s, model, "denoise")(alpha, w, maxiter=K))
        for d in range(3):   # direction d of a call is the single call
            assert _same(jvp(alpha, w, df=df3[d], dalpha=da3[d], dw=dw3[d], maxiter=K), du0[d])
        plans = [dict(), dict(tile_iters=1), dict(tile_iters=3), dict(tile_iters=8), dict(chains=1), dict(chains=2),
                 dict(use_graph=0), dict(chains=2, use_graph=0), dict(tile_iters=3, chains=2)]
        for kw in plans:
            for rep in range(2):   # (the second call replays the cached graphs)
                du, u = jvp(alpha, w, df=df3, dalpha=da3, dw=dw3, want_u=True, maxiter=K, **kw)
                assert _same(du, du0) and _same(u, u0), (kw, rep)
        # one tangent at a time: a NULL tangent is an explicit zero
        zf, za, zw = np.zeros_like(f), np.zeros_like(da3[0]), np.zeros_like(w)
        only_f = jvp(alpha, w, df=df3[0], maxiter=K)
        only_a = jvp(alpha, w, dalpha=da3[0], maxiter=K)
        only_w = jvp(alpha, w, dw=dw3[0], maxiter=K)
        assert _same(only_f, jvp(alpha, w, df=df3[0], dalpha=za, dw=zw, maxiter=K))
        assert _same(only_a, jvp(alpha, w, df=zf, dalpha=da3[0], dw=zw, maxiter=K))
        assert _same(only_w, jvp(alpha, w, df=zf, dalpha=za, dw=dw3[0], maxiter=K))
        assert only_f.any() and only_a.any() and only_w.any()
        # the device form
        at, wt = torch.tensor(a, device="cuda"), torch.tensor(w, device="cuda")
        dft, dat, dwt = torch.tensor(df3, device="cuda"), torch.tensor(da3, device="cuda"), torch.tensor(dw3, device="cuda")
        dud = torch.empty(3, O, N, M, dtype=torch.float64, device="cuda")
        ud = torch.empty(O, N, M, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        for kw in (dict(), dict(), dict(chains=1, use_graph=0), dict(tile_iters=3, chains=2)):
            dud.zero_(); ud.zero_(); torch.cuda.synchronize()
            dev(wt.data_ptr(), wo, at.data_ptr(), am, an, dft.data_ptr(), dat.data_ptr(), dwt.data_ptr(), dud.data_ptr(), ud.data_ptr(),
                ndir=3, maxiter=K, **kw)
            assert _same(dud.cpu().numpy(), du0) and _same(ud.cpu().numpy(), u0), kw
        for ptrs, ref in (((dft.data_ptr(), None, None), only_f), ((None, dat.data_ptr(), None), only_a),
                          ((None, None, dwt.data_ptr()), only_w)):
            dud.zero_(); torch.cuda.synchronize()
            dev(wt.data_ptr(), wo, at.data_ptr(), am, an, *ptrs, dud.data_ptr(), None, ndir=1, maxiter=K)
            assert _same(dud[0].cpu().numpy(), ref)
    s.close()


# ---- 6. across the models: no shared graph, no missing LDS attribute ------------------------------------------------------
def test_the_three_models_sweeps_on_one_handle_in_every_order(gpu_solver_cls):
    """The weighted, the L1 and the KL sweep with the same w (min w = 0: the same step table), alpha and K on one handle, in each
    of the six orders, twice (the second round replays what the first cached): each gives the bits of a fresh handle.  The three
    tangents differ pairwise by more than 1e-3 * max|du|, on the twin and here, so a replayed graph of another model would show."""
    f, alpha, w, K, df, dam, dw = j.cross_model_case()
    O, N, M = f.shape
    amap = tw.alpha_to_map(alpha, M, N)
    twin = {"weighted": wuj.forward_tangent(f, amap, w, K, df, dam, dw)[1],
            "l1": j.forward_tangent("l1", f, amap, w, K, df, dam, dw)[1],
            "kl": j.forward_tangent("kl", f, amap, w, K, df, dam, dw)[1]}

    def differ(du):
        for a, b in itertools.combinations(sorted(du), 2):
            d = float(np.abs(du[a] - du[b]).max())
            assert d > 1e-3 * max(float(np.abs(du[a]).max()), float(np.abs(du[b]).max())), (a, b, d)
    differ(twin)

    def sweep(h, model):
        return _m(h, model, "unrolled_jvp")(alpha, w, df=df, dalpha=1.0, dw=dw, want_u=True, maxiter=K)
    fresh = {}
    for model in sorted(twin):
        h = gpu_solver_cls(M, N, O)
        h.set_data(f, f)
        fresh[model] = sweep(h, model)
        h.close()
    # (no comparison with the twin here: the counts sit on a grid of 1 / 30, where the L1 threshold meets ties that the device's
    # fma and the twin's rounding decide differently -- test_tangent_matches_the_twin runs on data whose margins are pinned)
    differ({k: v[0] for k, v in fresh.items()})
    for order in itertools.permutations(sorted(twin)):
        h = gpu_solver_cls(M, N, O)
        h.set_data(f, f)
        for rnd in range(2):
            for model in order:
                du, u = sweep(h, model)
                assert _same(du, fresh[model][0]) and _same(u, fresh[model][1]), (order, rnd, model)
        h.close()


# ---- 7. the handle stays as it was --------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", j.MODELS)
def test_a_sweep_leaves_the_last_solve_the_tapes_and_the_statistics(gpu_solver_cls, model):
    import torch
    name = "2x17x33"
    O, N, M = SHAPES[name]
    f, gu = _data("kl", name)                                # (f > 0: every model takes it)
    w = _weight(name, "mask")
    df, _, _, dw = j.tangents_of(name, "mask", "scalar")
    s = gpu_solver_cls(M, N, O)
    s.set_data(f, f)
    amap = _alpha("kl", "map", N, M)
    s.l1_unrolled_denoise(0.7, w, maxiter=20)                # an L1 tape ...
    l10 = s.l1_unrolled_vjp(0.7, w, gu, maxiter=20)
    s.kl_unrolled_denoise(0.15, w, maxiter=20)               # ... a KL one ...
    kl0 = s.kl_unrolled_vjp(0.15, w, gu, maxiter=20)
    s.weighted_unrolled_denoise(0.08, w, maxiter=20)         # ... and a weighted one
    wt0 = s.weighted_unrolled_vjp(0.08, w, gu, maxiter=20)
    u0 = s.denoise(amap, maxiter=57)                         # the last solve: another model, parameter and shape
    gap0 = s.duality_gap()
    st0 = s.stats()
    out = torch.empty(O, N, M, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    s.copy_u_device(out.data_ptr())
    ptr0 = s.u_device_ptr()
    du = _m(s, model, "unrolled_jvp")(0.3, w, df=df, dalpha=1.0, dw=dw, maxiter=33)
    assert du.any()
    st1 = s.stats()
    assert st1["adjoint_method"] == METHOD[model] and st1["adjoint_ms"] > 0.0
    for k in st0:
        if k not in ("adjoint_ms", "adjoint_method"):
            assert st1[k] == st0[k], (k, st0[k], st1[k])
    assert s.u_device_ptr() == ptr0
    out2 = torch.empty_like(out)
    torch.cuda.synchronize()
    s.copy_u_device(out2.data_ptr())
    assert _same(out2.cpu().numpy(), u0) and _same(out.cpu().numpy(), u0)
    assert _same(s.duality_gap(), gap0)
    for a, b in zip(s.weighted_unrolled_vjp(0.08, w, gu, maxiter=20), wt0):   # the earlier tapes
        assert _same(a, b)
    for a, b in zip(s.kl_unrolled_vjp(0.15, w, gu, maxiter=20), kl0):
        assert _same(a, b)
    for a, b in zip(s.l1_unrolled_vjp(0.7, w, gu, maxiter=20), l10):
        assert _same(a, b)
    s.close()


# ---- 8. rejections -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", j.MODELS)
def test_rejections_leave_the_handle_as_it_was(gpu_solver_cls, model):
    import torch
    from bpldenoising_amd._lib import BpltvError
    name = "2x17x33"
    O, N, M = SHAPES[name]
    f, gu = _data("kl", name)
    w = _weight(name, "mask")
    df, _, _, dw = j.tangents_of(name, "mask", "scalar")
    s = gpu_solver_cls(M, N, O)
    s.set_data(f, f)
    amap = _alpha("kl", "map", N, M)
    _m(s, model, "unrolled_denoise")(0.3, w, maxiter=20)
    t0 = _m(s, model, "unrolled_vjp")(0.3, w, gu, maxiter=20)
    s.weighted_unrolled_denoise(0.08, w, maxiter=20)
    wt0 = s.weighted_unrolled_vjp(0.08, w, gu, maxiter=20)
    u0 = s.denoise(amap, maxiter=57)
    gap0 = s.duality_gap()
    ptr0 = s.u_device_ptr()
    out = torch.empty(O, N, M, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()

    def unchanged(st0):
        st1 = s.stats()
        assert st1 == st0, {k: (st0[k], st1[k]) for k in st0 if st0[k] != st1[k]}
        assert s.u_device_ptr() == ptr0
        s.copy_u_device(out.data_ptr())
        assert _same(out.cpu().numpy(), u0)
        assert _same(s.duality_gap(), gap0)
        assert _same(s.denoise(amap, maxiter=57), u0) and _same(s.duality_gap(), gap0)

    def rejected(code, call, *a, **k):
        st0 = s.stats()
        with pytest.raises(BpltvError) as e:
            call(*a, **k)
        assert e.value.code == code, (e.value.code, str(e.value))
        unchanged(st0)
        return str(e.value)

    jvp, gn = _m(s, model, "unrolled_jvp"), _m(s, model, "unrolled_gauss_newton")
    bad_df = df.copy(); bad_df[1, 3, 4] = np.inf
    bad_dw = dw.copy(); bad_dw[3, 4] = np.nan
    nan_map = amap.copy(); nan_map[2, 5] = np.nan
    neg_w = w.copy(); neg_w[3, 4] = -0.5
    nan_w = w.copy(); nan_w[3, 4] = np.nan
    for bad in (float("nan"), -0.1, nan_map):
        rejected(E_ARG, jvp, bad, w, df=df, maxiter=20)
        if np.ndim(bad) == 0:
            rejected(E_ARG, gn, bad, w, maxiter=20)
    for bad in (neg_w, nan_w):
        rejected(E_ARG, jvp, 0.3, bad, df=df, maxiter=20)
        rejected(E_ARG, gn, 0.3, bad, maxiter=20)
    rejected(E_ARG, jvp, 0.3, w, df=bad_df, maxiter=20)          # a non-finite tangent, each of the three
    rejected(E_ARG, jvp, 0.3, w, dalpha=float("nan"), maxiter=20)
    rejected(E_ARG, jvp, 0.3, w, dw=bad_dw, maxiter=20)
    rejected(E_ARG, jvp, 0.3, w, df=df, maxiter=0)
    rejected(E_ARG, gn, 0.3, w, maxiter=0)
    for kw in (dict(rho=0.01), dict(init=1), dict(order=1)):
        rejected(E_UNSUPPORTED, jvp, 0.3, w, df=df, maxiter=20, **kw)
        rejected(E_UNSUPPORTED, gn, 0.3, w, maxiter=20, **kw)
    p = s.params(maxiter=20)
    a1 = np.array([0.3])
    du = np.empty_like(df)
    lib, h = s._lib, s._h
    st0 = s.stats()
    fn = getattr(lib, "bpltv_%s_unrolled_jvp" % CNAME[model])
    assert fn(h, _ptr(w), 1, _ptr(a1), 1, 1, C.byref(p), 1, None, None, None, _ptr(du), None) == E_ARG         # all tangents NULL
    assert fn(h, _ptr(w), 1, _ptr(a1), 1, 1, C.byref(p), 0, _ptr(df), None, None, _ptr(du), None) == E_ARG     # ndir < 1
    assert fn(h, _ptr(w), 1, _ptr(a1), 1, 1, C.byref(p), 1, _ptr(df), None, None, None, None) == E_ARG         # no du_out
    assert fn(h, None, 1, _ptr(a1), 1, 1, C.byref(p), 1, _ptr(df), None, None, _ptr(du), None) == E_ARG        # no w
    assert fn(h, _ptr(w), 3, _ptr(a1), 1, 1, C.byref(p), 1, _ptr(df), None, None, _ptr(du), None) == E_ARG     # wo not in {1, O}
    assert fn(h, _ptr(w), 1, _ptr(a1), M + 1, 1, C.byref(p), 1, _ptr(df), None, None, _ptr(du), None) == E_ARG   # shape
    assert fn(h, _ptr(w), 1, _ptr(a1), 0, 1, C.byref(p), 1, _ptr(df), None, None, _ptr(du), None) == E_ARG
    cost, g1, h1 = C.c_double(0.0), np.empty(1), np.empty(1)
    gfn = getattr(lib, "bpltv_%s_unrolled_gauss_newton" % CNAME[model])
    assert gfn(h, None, 1, _ptr(a1), 1, 1, C.byref(p), C.byref(cost), _ptr(g1), _ptr(h1)) == E_ARG
    assert gfn(h, _ptr(w), 3, _ptr(a1), 1, 1, C.byref(p), C.byref(cost), _ptr(g1), _ptr(h1)) == E_ARG
    unchanged(st0)
    # the device form
    good = torch.tensor([0.3], dtype=torch.float64, device="cuda")
    wt = torch.tensor(w, device="cuda")
    dft, dud = torch.tensor(df, device="cuda"), torch.empty(O, N, M, dtype=torch.float64, device="cuda")
    dwt = torch.tensor(dw, device="cuda")
    bdt, bdw = torch.tensor(bad_df, device="cuda"), torch.tensor(bad_dw, device="cuda")
    bda = torch.tensor([float("inf")], dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    dev = _m(s, model, "unrolled_jvp_device")
    for bad in (float("nan"), -0.1):
        bt = torch.tensor([bad], dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        rejected(E_ARG, dev, wt.data_ptr(), 1, bt.data_ptr(), 1, 1, dft.data_ptr(), None, None, dud.data_ptr(), maxiter=20)
    for bad in (neg_w, nan_w):
        bw = torch.tensor(bad, device="cuda")
        torch.cuda.synchronize()
        rejected(E_ARG, dev, bw.data_ptr(), 1, good.data_ptr(), 1, 1, dft.data_ptr(), None, None, dud.data_ptr(), maxiter=20)
    rejected(E_ARG, dev, wt.data_ptr(), 1, good.data_ptr(), 1, 1, bdt.data_ptr(), None, None, dud.data_ptr(), maxiter=20)
    rejected(E_ARG, dev, wt.data_ptr(), 1, good.data_ptr(), 1, 1, dft.data_ptr(), bda.data_ptr(), None, dud.data_ptr(), maxiter=20)
    rejected(E_ARG, dev, wt.data_ptr(), 1, good.data_ptr(), 1, 1, dft.data_ptr(), None, bdw.data_ptr(), dud.data_ptr(), maxiter=20)
    rejected(E_ARG, dev, wt.data_ptr(), 1, good.data_ptr(), 1, 1, None, None, None, dud.data_ptr(), maxiter=20)
    rejected(E_ARG, dev, wt.data_ptr(), 1, good.data_ptr(), 1, 1, dft.data_ptr(), None, dwt.data_ptr(), dud.data_ptr(), ndir=0, maxiter=20)
    rejected(E_ARG, dev, wt.data_ptr(), 3, good.data_ptr(), 1, 1, dft.data_ptr(), None, None, dud.data_ptr(), maxiter=20)
    # the tapes recorded before all this
    for a, b in zip(s.weighted_unrolled_vjp(0.08, w, gu, maxiter=20), wt0):
        assert _same(a, b)
    for a, b in zip(_m(s, model, "unrolled_vjp")(0.3, w, gu, maxiter=20), t0):
        assert _same(a, b)
    n = gpu_solver_cls(M, N, O)                # no dataset
    with pytest.raises(BpltvError) as e:
        _m(n, model, "unrolled_jvp")(0.3, w, df=df, maxiter=5)
    assert e.value.code == E_NODATA
    with pytest.raises(BpltvError) as e:
        _m(n, model, "unrolled_gauss_newton")(0.3, w, maxiter=5)
    assert e.value.code == E_NODATA
    n.close()
    s.close()


@pytest.mark.parametrize("bad", [-1e-300, np.nan])
def test_kl_a_dataset_with_a_negative_entry_is_rejected(gpu_solver_cls, bad):
    """BPLTV_E_ARG with a message that names f, host and device form and the Gauss-Newton call, before anything of the handle
    changes; the L1 sweep takes the same dataset when it is finite; a good dataset installed afterwards is accepted again."""
    import torch
    from bpldenoising_amd._lib import BpltvError
    name = "2x17x33"
    O, N, M = SHAPES[name]
    f, gu = _data("kl", name)
    w = _weight(name, "real")
    df, _, _, dw = j.tangents_of(name, "real", "scalar")
    fb = f.copy()
    fb[1, 9, 20] = bad
    s = gpu_solver_cls(M, N, O)
    s.set_data(f, f)
    s.kl_unrolled_denoise(0.15, w, maxiter=20)
    g0 = s.kl_unrolled_vjp(0.15, w, gu, maxiter=20)
    du0 = s.kl_unrolled_jvp(0.15, w, df=df, dw=dw, maxiter=20)
    s.set_data(f, fb)
    if np.isfinite(bad):
        ref = gpu_solver_cls(M, N, O)
        ref.set_data(f, fb)
        assert _same(s.l1_unrolled_jvp(0.7, w, df=df, dw=dw, maxiter=20), ref.l1_unrolled_jvp(0.7, w, df=df, dw=dw, maxiter=20))
        ref.close()
    st0 = s.stats()
    wt = torch.tensor(w, device="cuda")
    good = torch.tensor([0.15], dtype=torch.float64, device="cuda")
    dft, dud = torch.tensor(df, device="cuda"), torch.empty(O, N, M, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    for call, args, kw in ((s.kl_unrolled_jvp, (0.15, w), dict(df=df)), (s.kl_unrolled_gauss_newton, (0.15, w), dict()),
                           (s.kl_unrolled_jvp_device, (wt.data_ptr(), O, good.data_ptr(), 1, 1, dft.data_ptr(), None, None, dud.data_ptr()), dict())):
        for rnd in range(2):                                # (the second call answers from what the first remembered)
            with pytest.raises(BpltvError) as e:
                call(*args, maxiter=20, **kw)
            assert e.value.code == E_ARG and " f " in str(e.value) and "dataset" in str(e.value), str(e.value)
            assert s.stats() == st0
    s.set_data(f, f)
    assert all(_same(x, y) for x, y in zip(s.kl_unrolled_vjp(0.15, w, gu, maxiter=20), g0))   # the KL tape is still valid
    assert _same(s.kl_unrolled_jvp(0.15, w, df=df, dw=dw, maxiter=20), du0)                      # a good dataset again: looked at anew
    s.close()


@pytest.mark.parametrize("model", j.MODELS)
def test_two_shards_are_unsupported_and_one_is_forwarded(gpu_solver_cls, model):
    from bpldenoising_amd._lib import BpltvError
    name = "2x17x33"
    O, N, M = SHAPES[name]
    f, _ = _data("kl", name)
    w = _weight(name, "mask")
    df, _, _, dw = j.tangents_of(name, "mask", "scalar")
    m = gpu_solver_cls(M, N, O, devices=[0, 0])
    m.set_data(f, f)
    u0 = m.denoise(0.07, maxiter=30)
    gap0 = m.duality_gap()
    for call, args, kw in ((_m(m, model, "unrolled_jvp"), (0.3, w), dict(df=df)), (_m(m, model, "unrolled_gauss_newton"), (0.3, w), dict()),
                           (_m(m, model, "unrolled_jvp_device"), (1, 1, 1, 1, 1, 1, 1, 1, 1), dict())):
        with pytest.raises(BpltvError) as e:     # (the device form is refused before any pointer is read)
            call(*args, maxiter=30, **kw)
        assert e.value.code == E_UNSUPPORTED
        assert _same(m.duality_gap(), gap0) and _same(m.denoise(0.07, maxiter=30), u0)
    m.close()
    one = gpu_solver_cls(M, N, O, ngpus=1)       # one shard holds everything: forwarded
    one.set_data(f, f)
    s = gpu_solver_cls(M, N, O)
    s.set_data(f, f)
    kw = dict(df=df, dalpha=1.0, dw=dw, maxiter=30)
    assert _same(_m(one, model, "unrolled_jvp")(0.3, w, **kw), _m(s, model, "unrolled_jvp")(0.3, w, **kw))
    for a, b in zip(_m(one, model, "unrolled_gauss_newton")(0.3, w, maxiter=30), _m(s, model, "unrolled_gauss_newton")(0.3, w, maxiter=30)):
        assert _same(a, b)
    one.close()
    s.close()


# ---- 9. the Gauss-Newton model of the K-step loss -----------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["scalar", "patch"])
@pytest.mark.parametrize("model", j.MODELS)
def test_gauss_newton_of_the_k_step_loss(gpu_solver_cls, model, kind):
    """cost = 0.5 ||u_K - ubar||^2, grad = the model's unrolled VJP at gu = u_K - ubar, H = the Gram matrix of the columns from the
    model's _jvp, with the bounds of tests/test_gpu_weighted_unrolled_jvp.py; a map and a 17-entry patch are unsupported."""
    from conftest import synth_batch
    from bpldenoising_amd._lib import BpltvError
    ref = j.REF[model]
    name, K = "3x40x48", 50
    O, N, M = SHAPES[name]
    f, _ = _data(model, name)
    ub = synth_batch(O, N, M, seed=5 + M)[0] if model == "l1" else kr.poisson_data(name)[0] + kr.BACKGROUND
    w = _weight(name, "mask")
    alpha = _alpha(model, kind, N, M)
    P = int(np.size(alpha))
    s = gpu_solver_cls(M, N, O)
    s.set_data(ub, f)
    cost, grad, H = _m(s, model, "unrolled_gauss_newton")(alpha, w, maxiter=K)
    assert s.stats()["adjoint_method"] == METHOD[model]
    assert H.shape == (P, P) and _same(H, H.T)
    eye = np.eye(P).reshape((P,) + np.shape(alpha))
    J, u = _m(s, model, "unrolled_jvp")(alpha, w, dalpha=eye if P > 1 else 1.0, want_u=True, maxiter=K)
    J = J.reshape(P, -1)
    assert J.any(axis=1).all()
    H0 = J @ J.T
    dH = float(np.abs(H - H0).max())
    print("%s %s: max|H - J J^T| %.2e (bound %.2e)" % (model, kind, dH, 1e-11 * float(np.abs(H0).max())))
    assert dH <= 1e-11 * float(np.abs(H0).max())
    # the gradient against the model's reverse sweep, within the dL/dalpha bound of the reverse sweeps' own tests
    assert _same(_m(s, model, "unrolled_denoise")(alpha, w, maxiter=K), u)
    _, ga, _ = _m(s, model, "unrolled_vjp")(alpha, w, u - ub, want_f=False, want_w=False, maxiter=K)
    amap = tw.alpha_to_map(alpha, M, N)
    u_t, tape, tab = ref.fwd_tape(f, amap, w, K)
    _, ga0, _ = ref.reverse(u_t - ub, tape, tab, amap, w, f)
    ba = 1e-11 * float(np.abs(ga0).max()) * O * ur.pixels_per_entry(alpha, M, N)
    dg = float(np.abs(np.asarray(grad) - np.asarray(ga)).max())
    print("%s %s: max|grad - reverse sweep| %.2e (bound %.2e)" % (model, kind, dg, ba))
    assert dg <= ba
    c0 = 0.5 * float(((u - ub) ** 2).sum())
    print("%s %s: cost %.15g numpy %.15g rel %.1e" % (model, kind, cost, c0, abs(cost - c0) / c0))
    assert cost == pytest.approx(c0, rel=1e-12, abs=0.0)
    for bad in (_alpha(model, "map", N, M), np.full((1, 17), float(np.mean(alpha)))):
        with pytest.raises(BpltvError) as e:
            _m(s, model, "unrolled_gauss_newton")(bad, w, maxiter=K)
        assert e.value.code == E_UNSUPPORTED and "bpltv_%s_unrolled_jvp" % CNAME[model] in str(e.value), str(e.value)
    s.close()
