"""Forward mode through the iterations of the weighted model on a machine without a GPU: the library exports
bpltv_weighted_unrolled_jvp, its device form and bpltv_weighted_unrolled_gauss_newton with the header's argument lists, the
binding covers them, TVSolver and the torch layer have the entries, and the numpy twin the GPU tests compare against
(tests/weighted_unrolled_jvp_ref.py) is pinned: its primal to weighted_unrolled_ref.fwd_tape bit for bit, its tangent to the
transpose identity against weighted_unrolled_ref.reverse, to torch forward-mode AD, to the TV twin at w == 1 and to central
differences of weighted_ref.pdhg."""
import ctypes as C
import functools
import os
import re
import types

import numpy as np
import pytest
from conftest import ROOT, synth_batch

import unrolled_jvp_ref as uj
import weighted_ref as wr
import weighted_unrolled_jvp_ref as wuj
import weighted_unrolled_ref as wur
from oracle import np_twin as tw

NAMES = {"bpltv_weighted_unrolled_jvp": 13, "bpltv_weighted_unrolled_jvp_device": 13, "bpltv_weighted_unrolled_gauss_newton": 10}
UNIT_WEIGHT_RTOL, CD_H, CD_RTOL = wuj.UNIT_WEIGHT_RTOL, wuj.CD_H, wuj.CD_RTOL
central_difference_case = wuj.central_difference_case


def _header_text():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bpltv.h")).read(), flags=re.S)


def _header_args(name):
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name, _header_text())
    assert m, name
    return [" ".join(a.split()) for a in m.group(1).split(",")]


@pytest.mark.parametrize("name", sorted(NAMES))
def test_library_exports_and_binds_the_weighted_unrolled_jvp_functions(name):
    from bpldenoising_amd import _lib
    lib = _lib.load()
    assert hasattr(lib, name)
    res, args = _lib.SYMBOLS[name]
    assert res is C.c_int
    hdr = _header_args(name)
    assert len(args) == len(hdr) == NAMES[name]
    assert getattr(lib, name).argtypes == args
    for a, decl in zip(args, hdr):
        if decl.startswith("bpltv_t *"):
            assert a is C.c_void_p
        elif decl.startswith("const bpltv_params *"):
            assert a is _lib._PP
        elif decl.startswith("int "):
            assert a is C.c_int
        else:   # arrays: host forms take POINTER(c_double), device forms raw addresses
            assert "double *" in decl, decl
            assert a is (C.c_void_p if name.endswith("_device") else C.POINTER(C.c_double)), (decl, a)


def test_header_argument_order_is_the_issue_s():
    names = lambda fn: [d.split()[-1].lstrip("*") for d in _header_args(fn)]
    assert names("bpltv_weighted_unrolled_jvp") == ["h", "w", "wo", "alpha", "am", "an", "p", "ndir", "df", "dalpha", "dw",
                                                    "du_out", "u_out"]
    assert names("bpltv_weighted_unrolled_jvp_device") == ["h", "d_w", "wo", "d_alpha", "am", "an", "p", "ndir", "d_df",
                                                           "d_dalpha", "d_dw", "d_du", "d_u"]
    assert names("bpltv_weighted_unrolled_gauss_newton") == ["h", "w", "wo", "alpha", "am", "an", "p", "cost_out", "grad_out",
                                                             "hess_out"]
    txt = open(os.path.join(ROOT, "include", "bpltv.h")).read()
    assert "11 tangent sweep through the weighted iterations" in txt
    from bpldenoising_amd import _lib
    st = _lib.BpltvStats()
    st.adjoint_method = 11
    assert st.as_dict()["adjoint_method"] == "weighted-unrolled-jvp"
    st.adjoint_method = 9
    assert st.as_dict()["adjoint_method"] == "weighted-unrolled"
    st.adjoint_method = 8
    assert st.as_dict()["adjoint_method"] == "unrolled-jvp"


def test_solver_and_layer_have_the_forward_mode_entries():
    from bpldenoising_amd import TVSolver
    for m in ("weighted_unrolled_jvp", "weighted_unrolled_jvp_device", "weighted_unrolled_gauss_newton"):
        assert callable(getattr(TVSolver, m))
    torch = pytest.importorskip("torch")
    from bpldenoising_amd import torch_layer as tl
    assert issubclass(tl.TVDenoiseWeightedUnrolledForwardFunction, tl.TVDenoiseWeightedUnrolledFunction)
    assert tl.TVDenoiseWeightedUnrolledForwardFunction.jvp is not torch.autograd.Function.jvp
    assert tl.TVDenoiseWeightedUnrolledFunction.jvp is torch.autograd.Function.jvp      # the default stays without one


def test_forward_mode_selects_the_function_and_never_reaches_the_solver_parameters(monkeypatch):
    torch = pytest.importorskip("torch")
    from bpldenoising_amd import torch_layer as tl
    seen = []
    for cls in (tl.TVDenoiseWeightedUnrolledFunction, tl.TVDenoiseWeightedUnrolledForwardFunction):
        monkeypatch.setattr(cls, "apply", staticmethod(lambda f, a, w, kw, cls=cls: seen.append((cls, kw))))
    f, a = torch.zeros(1, 4, 4, dtype=torch.float64), torch.tensor(0.1, dtype=torch.float64)
    w = torch.ones(4, 4, dtype=torch.float64)
    tl.tv_denoise_weighted_unrolled(f, a, w, maxiter=5)
    tl.tv_denoise_weighted_unrolled(f, a, w, maxiter=5, forward_mode=True)
    tl.tv_denoise_weighted_unrolled(f, a, w, 7, forward_mode=True, checkpoint_every=3, accel=0)
    assert [c for c, _ in seen] == [tl.TVDenoiseWeightedUnrolledFunction, tl.TVDenoiseWeightedUnrolledForwardFunction,
                                    tl.TVDenoiseWeightedUnrolledForwardFunction]
    assert [kw for _, kw in seen] == [{"maxiter": 5}, {"maxiter": 5}, {"maxiter": 7, "accel": 0, "checkpoint_every": 3}]


@pytest.fixture
def layer(monkeypatch):
    """torch_layer with every library entry refused: a rejection must come before any library call."""
    pytest.importorskip("torch")
    from bpldenoising_amd import torch_layer

    def no_library(*a, **k):
        raise AssertionError("the library was called")
    monkeypatch.setattr(torch_layer, "_solver", no_library)
    monkeypatch.setattr(torch_layer, "_sync", no_library)
    return torch_layer


def test_forward_mode_layer_rejects_before_any_library_call(layer):
    import torch
    fn = functools.partial(layer.tv_denoise_weighted_unrolled, forward_mode=True)
    f = torch.zeros(2, 8, 6, dtype=torch.float64)
    a = torch.tensor(0.1, dtype=torch.float64)
    w = torch.ones(8, 6, dtype=torch.float64)
    with pytest.raises(TypeError, match="float64"):
        fn(f.float(), a, w, maxiter=5)
    with pytest.raises(TypeError, match="tv_denoise_weighted_unrolled: w must be float64"):
        fn(f, a, w.float(), maxiter=5)
    with pytest.raises(ValueError, match="w must have shape"):
        fn(f, a, torch.ones(6, 8, dtype=torch.float64), maxiter=5)
    wb = w.clone()
    wb[3, 2] = -0.5
    with pytest.raises(ValueError, match="finite and >= 0"):
        fn(f, a, wb, maxiter=5)
    mask = w.clone()
    mask[::2] = 0.0
    with pytest.raises(ValueError, match="ROCm device"):           # CPU tensors, everything else valid
        fn(f, a, mask, maxiter=5)
    # the jvp checks its tangents before the library sees them; an input without a tangent is None
    ctx = types.SimpleNamespace(saved_tensors=(f, a, w), solver=None, am=1, an=1, wo=1, solver_kw={"maxiter": 5})
    jvp = layer.TVDenoiseWeightedUnrolledForwardFunction.jvp
    with pytest.raises(TypeError, match="tangent of w must be float64"):
        jvp(ctx, None, None, w.float(), None)
    with pytest.raises(ValueError, match="tangent of w has shape"):
        jvp(ctx, None, None, torch.ones(2, 8, 6, dtype=torch.float64), None)
    with pytest.raises(TypeError, match="tangent of f must be float64"):
        jvp(ctx, f.float(), None, None, None)
    du = jvp(ctx, None, None, None, None)                          # no tangent at all: zero, without a library call
    assert du.shape == f.shape and not du.any()


# ---- the twin -------------------------------------------------------------------------------------------------------
WKINDS = ["real", "mask", "ones"]


@functools.lru_cache(maxsize=None)
def case(name, kind, wkind, seed=5):
    """(f, amap, w, df, damap, dw, gu) of a GPU case: standard-normal tangents (dw in the shape of w) and a cotangent."""
    O, N, M = wur.GPU_SHAPES[name]
    f, gu = wur.gpu_data(name)
    alpha = wur.alpha_of(kind, N, M)
    w = wur.weight_of(wkind, O, N, M)
    rng = np.random.default_rng(seed + 200)
    df = rng.standard_normal(f.shape)
    dalpha = rng.standard_normal(np.shape(alpha))
    damap = tw.alpha_to_map(dalpha, M, N) if kind != "scalar" else np.full((N, M), float(dalpha))
    dw = rng.standard_normal(w.shape)
    for a in (f, df, damap, dw, gu, w):
        a.setflags(write=False)
    return f, tw.alpha_to_map(alpha, M, N), w, df, damap, dw, gu


@pytest.mark.parametrize("accel", [True, False])
@pytest.mark.parametrize("wkind", WKINDS)
@pytest.mark.parametrize("name", ["2x17x33", "3x40x48"])
def test_twin_primal_is_fwd_tape_bit_for_bit(name, wkind, accel):
    for kind in ("scalar", "patch", "map"):
        f, amap, w, df, damap, dw, _ = case(name, kind, wkind)
        for K in (50, 203):
            u, du = wuj.forward_tangent(f, amap, w, K, df, damap, dw, accel=accel)
            u0, _, _ = wur.fwd_tape(f, amap, w, K, accel=accel)
            assert np.array_equal(u, u0)
            assert du.shape == f.shape and np.isfinite(du).all() and du.any()
            u1, du1 = wuj.forward_tangent(f, amap, w, K, accel=accel)      # no tangent: zero
            assert np.array_equal(u1, u) and not du1.any()


@pytest.mark.parametrize("wkind", WKINDS)
@pytest.mark.parametrize("kind", ["scalar", "patch", "map"])
@pytest.mark.parametrize("name", wur.GRADIENT_SHAPES)
def test_twin_tangent_is_the_transpose_of_the_reverse_sweep(name, kind, wkind):
    """<du, gu> = <df, grad_f> + <damap, sum over the images of ga> + <dw, grad_w> to 1e-12 * sum|du * gu|, all three
    tangents at once (measured: at most 8.8e-15)."""
    f, amap, w, df, damap, dw, gu = case(name, kind, wkind)
    for K in wur.GRADIENT_K:
        _, du = wuj.forward_tangent(f, amap, w, K, df, damap, dw)
        _, tape, tab = wur.fwd_tape(f, amap, w, K)
        gf, ga, gw = wur.reverse(gu, tape, tab, amap, w, f)
        lhs = float((du * gu).sum())
        rhs = float((df * gf).sum()) + float((damap * ga.sum(axis=0)).sum()) + float((dw * wur.reduce_w(gw, w)).sum())
        scale = float(np.abs(du * gu).sum())
        print("%s %s %s K %d: |lhs - rhs| %.2e  sum|du gu| %.2e  rel %.1e" % (name, kind, wkind, K, abs(lhs - rhs), scale, abs(lhs - rhs) / scale))
        assert abs(lhs - rhs) <= 1e-12 * scale


@pytest.mark.parametrize("accel", [True, False])
@pytest.mark.parametrize("wkind", WKINDS)
@pytest.mark.parametrize("kind", ["scalar", "map"])
@pytest.mark.parametrize("name", ["2x17x33", "1x1x9", "1x9x1"])
def test_twin_tangent_agrees_with_torch_forward_mode(name, kind, wkind, accel):
    """1e-11 * max|ref|, the bound tests/test_unrolled_jvp_abi.py holds the TV twin to (measured: at most 4.7e-14 * max|ref|);
    all three tangents at once and, with the acceleration at K = 50, each alone."""
    pytest.importorskip("torch")
    f, amap, w, df, damap, dw, _ = case(name, kind, wkind)
    singles = ((df, None, None), (None, damap, None), (None, None, dw)) if accel else ()
    for K in (50, 203):
        for tf, ta, tw_ in (singles if K == 50 else ()) + ((df, damap, dw),):
            u, du = wuj.forward_tangent(f, amap, w, K, tf, ta, tw_, accel=accel)
            u0, du0 = wuj.torch_forward_reference(f, amap, w, K, tf, ta, tw_, accel=accel)
            d, m = float(np.abs(du - du0).max()), float(np.abs(du0).max())
            print("%s %s %s accel %d K %d (%d%d%d): du %.2e (max %.2e)  u %.2e"
                  % (name, kind, wkind, accel, K, tf is not None, ta is not None, tw_ is not None, d, m, float(np.abs(u - u0).max())))
            assert d <= 1e-11 * m


@pytest.mark.parametrize("kind", ["scalar", "patch", "map"])
@pytest.mark.parametrize("name", wur.GRADIENT_SHAPES)
def test_unit_weight_twin_agrees_with_the_tv_twin(name, kind):
    """w == 1, dw = 0: unrolled_jvp_ref.forward_tangent's du to rounding, u bit for bit or to rounding ((div - 1*f) * r against
    (div - f) / (1 + tau)).  Measured maximum over all cases: 7.8e-14 * max|ref|, so UNIT_WEIGHT_RTOL = 1e-11 is
    more than two decades inside."""
    f, amap, w, df, damap, _, _ = case(name, kind, "ones")
    for K in wur.GRADIENT_K:
        u, du = wuj.forward_tangent(f, amap, w, K, df, damap, None)
        u0, du0 = uj.forward_tangent(f, amap, K, df, damap)
        d, m = float(np.abs(du - du0).max()), float(np.abs(du0).max())
        print("%s %s K %d: du %.2e (max|ref| %.2e, rel %.1e)  u %.2e" % (name, kind, K, d, m, d / m, float(np.abs(u - u0).max())))
        assert d <= UNIT_WEIGHT_RTOL * m
        assert d <= 0.1 * UNIT_WEIGHT_RTOL * m, "the bound no longer sits a decade above the twins' own difference"


@pytest.mark.parametrize("wkind", ["mask", "real"])
@pytest.mark.parametrize("K", [30, 300])
def test_twin_tangent_against_central_differences(K, wkind):
    """h = 1e-7, 1e-5 relative in the maximum norm (measured: at most 2.5e-8; at h = 1e-6 the masked K = 300 case flips a
    projection decision)."""
    f, alpha, w, directions = central_difference_case(wkind)
    amap = tw.alpha_to_map(alpha, 28, 24)
    h = CD_H
    for what, df, da, dw in directions:
        _, du = wuj.forward_tangent(f, amap, w, K, df, None if da is None else np.full_like(amap, da), dw)
        fp, fm = (f + h * df, f - h * df) if df is not None else (f, f)
        ap, am = (alpha + h * da, alpha - h * da) if da is not None else (alpha, alpha)
        wp, wm = (w + h * dw, w - h * dw) if dw is not None else (w, w)
        fd = (wr.pdhg(fp, ap, wp, K) - wr.pdhg(fm, am, wm, K)) / (2 * h)
        d, m = float(np.abs(du - fd).max()), float(np.abs(fd).max())
        print("%s K %d d/d%s: max|du - fd| %.3e  max|fd| %.3e  rel %.2e" % (wkind, K, what, d, m, d / m))
        assert d <= CD_RTOL * m, what
