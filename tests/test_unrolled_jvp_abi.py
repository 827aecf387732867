"""Forward mode through the PDHG iterations on a machine without a GPU: the library exports bpltv_unrolled_jvp,
bpltv_unrolled_jvp_device and bpltv_unrolled_gauss_newton with the header's argument lists, the binding covers them, TVSolver
has the methods, and the numpy twin the GPU tests compare against (tests/unrolled_jvp_ref.py) is pinned: its primal to
oracle.np_twin.pdhg_denoise bit for bit, its tangent to torch forward-mode AD, to the transpose identity against
unrolled_ref.reverse and to central differences of np_twin.pdhg_denoise."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest
from conftest import ROOT, synth_batch

import unrolled_jvp_ref as uj
import unrolled_ref as ur
from oracle import np_twin as tw

NAMES = {"bpltv_unrolled_jvp": 10, "bpltv_unrolled_jvp_device": 10, "bpltv_unrolled_gauss_newton": 8}


def _header_args(name):
    txt = open(os.path.join(ROOT, "include", "bpltv.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name, txt)
    assert m, name
    return [" ".join(a.split()) for a in m.group(1).split(",")]


@pytest.mark.parametrize("name", sorted(NAMES))
def test_library_exports_and_binds_the_unrolled_jvp_functions(name):
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
    assert names("bpltv_unrolled_jvp") == ["h", "alpha", "am", "an", "p", "ndir", "df", "dalpha", "du_out", "u_out"]
    assert names("bpltv_unrolled_jvp_device") == ["h", "d_alpha", "am", "an", "p", "ndir", "d_df", "d_dalpha", "d_du", "d_u"]
    assert names("bpltv_unrolled_gauss_newton") == ["h", "alpha", "am", "an", "p", "cost_out", "grad_out", "hess_out"]
    txt = open(os.path.join(ROOT, "include", "bpltv.h")).read()
    assert "8 tangent sweep through the iterations" in txt
    from bpldenoising_amd import _lib
    st = _lib.BpltvStats()
    st.adjoint_method = 8
    assert st.as_dict()["adjoint_method"] == "unrolled-jvp"
    st.adjoint_method = 7
    assert st.as_dict()["adjoint_method"] == "unrolled"


def test_solver_and_layer_have_the_forward_mode_entries():
    from bpldenoising_amd import TVSolver
    for m in ("unrolled_jvp", "unrolled_jvp_device", "unrolled_gauss_newton"):
        assert callable(getattr(TVSolver, m))
    torch = pytest.importorskip("torch")
    from bpldenoising_amd import torch_layer as tl
    assert issubclass(tl.TVDenoiseUnrolledForwardFunction, tl.TVDenoiseUnrolledFunction)
    assert tl.TVDenoiseUnrolledForwardFunction.jvp is not torch.autograd.Function.jvp
    assert tl.TVDenoiseUnrolledFunction.jvp is torch.autograd.Function.jvp          # the default stays without one
    m = tl.TVDenoiseUnrolled(0.1, forward_mode=True, maxiter=5)
    assert m.forward_mode is True and m.solver_kw == {"maxiter": 5}                 # forward_mode does not reach solver_kw
    assert tl.TVDenoiseUnrolled(0.1, maxiter=5).forward_mode is False


def test_forward_mode_never_reaches_the_solver_parameters(monkeypatch):
    torch = pytest.importorskip("torch")
    from bpldenoising_amd import torch_layer as tl
    seen = []
    for cls in (tl.TVDenoiseUnrolledFunction, tl.TVDenoiseUnrolledForwardFunction):
        monkeypatch.setattr(cls, "apply", staticmethod(lambda f, a, kw, cls=cls: seen.append((cls, kw))))
    f, a = torch.zeros(1, 4, 4, dtype=torch.float64), torch.tensor(0.1, dtype=torch.float64)
    tl.tv_denoise_unrolled(f, a, maxiter=5)
    tl.tv_denoise_unrolled(f, a, forward_mode=True, maxiter=5)
    tl.TVDenoiseUnrolled(0.1, forward_mode=True, maxiter=7)(f)
    assert [c for c, _ in seen] == [tl.TVDenoiseUnrolledFunction, tl.TVDenoiseUnrolledForwardFunction, tl.TVDenoiseUnrolledForwardFunction]
    assert [kw for _, kw in seen] == [{"maxiter": 5}, {"maxiter": 5}, {"maxiter": 7}]


# ---- the twin -------------------------------------------------------------------------------------------------------
SHAPES = [(2, 17, 33), (3, 40, 48)]          # (O, N, M)
DEGENERATE = [(1, 9, 1), (1, 1, 9)]


def alpha_of(kind, N, M):
    if kind == "scalar":
        return 0.08
    if kind == "patch":
        return np.array([[0.05, 0.1, 0.07], [0.12, 0.06, 0.09]])[:min(2, N), :min(3, M)]   # (an, am) = (2, 3)
    return 0.05 + 0.1 * np.random.default_rng(8).random((N, M))


@functools.lru_cache(maxsize=None)
def case(shape, kind, seed=5):
    """(f, alpha, amap, df, dalpha, damap, w): standard-normal tangents, dalpha in the type / shape of alpha, and a cotangent."""
    O, N, M = shape
    _, f = synth_batch(O, N, M, seed=seed)
    alpha = alpha_of(kind, N, M)
    rng = np.random.default_rng(seed + 200)
    df = rng.standard_normal(f.shape)
    dalpha = rng.standard_normal(np.shape(alpha))
    damap = tw.alpha_to_map(dalpha, M, N) if kind != "scalar" else np.full((N, M), float(dalpha))
    w = rng.standard_normal(f.shape)
    for a in (f, df, damap, w):
        a.setflags(write=False)
    return f, alpha, tw.alpha_to_map(alpha, M, N), df, dalpha, damap, w


@pytest.mark.parametrize("accel", [True, False])
@pytest.mark.parametrize("kind", ["scalar", "patch", "map"])
@pytest.mark.parametrize("shape", SHAPES)
def test_twin_primal_is_np_twin_bit_for_bit(shape, kind, accel):
    f, alpha, amap, df, _, damap, _ = case(shape, kind)
    for K in (50, 203):
        u, du = uj.forward_tangent(f, amap, K, df, damap, accel=accel)
        assert np.array_equal(u, tw.pdhg_denoise(f, alpha, maxiter=K, accel=accel))
        assert du.shape == f.shape and np.isfinite(du).all()
        u0, du0 = uj.forward_tangent(f, amap, K, None, None, accel=accel)      # no tangent: zero
        assert np.array_equal(u0, u) and not du0.any()


@pytest.mark.parametrize("accel", [True, False])
@pytest.mark.parametrize("kind", ["scalar", "patch", "map"])
@pytest.mark.parametrize("shape", SHAPES + DEGENERATE)
def test_twin_tangent_agrees_with_torch_forward_mode(shape, kind, accel):
    """1e-11 * max|ref|: the bound of DESIGN.md section 4.6 (the x200 margin of section 4.5)."""
    pytest.importorskip("torch")
    f, _, amap, df, _, damap, _ = case(shape, kind)
    for K in (50, 203):
        u, du = uj.forward_tangent(f, amap, K, df, damap, accel=accel)
        u0, du0 = uj.torch_forward_reference(f, amap, K, df, damap, accel=accel)
        d, m = float(np.abs(du - du0).max()), float(np.abs(du0).max())
        print("%s %s accel %d K %d: du %.2e (max %.2e)  u %.2e" % (shape, kind, accel, K, d, m, float(np.abs(u - u0).max())))
        assert d <= 1e-11 * m


@pytest.mark.parametrize("accel", [True, False])
@pytest.mark.parametrize("kind", ["scalar", "patch", "map"])
@pytest.mark.parametrize("shape", SHAPES + DEGENERATE)
def test_twin_tangent_is_the_transpose_of_the_reverse_sweep(shape, kind, accel):
    """<du, w> = <df, grad_f(w)> + <damap, sum over the images of ga(w)> to 1e-11 * sum|du * w|."""
    f, _, amap, df, _, damap, w = case(shape, kind)
    for K in (50, 203):
        _, du = uj.forward_tangent(f, amap, K, df, damap, accel=accel)
        _, tape, tab = ur.fwd_tape(f, amap, K, accel=accel)
        gf, ga = ur.reverse(w, tape, tab, amap)
        lhs = float((du * w).sum())
        rhs = float((df * gf).sum()) + float((damap * ga.sum(axis=0)).sum())
        scale = float(np.abs(du * w).sum())
        print("%s %s accel %d K %d: |lhs - rhs| %.2e  sum|du w| %.2e" % (shape, kind, accel, K, abs(lhs - rhs), scale))
        assert abs(lhs - rhs) <= 1e-11 * scale


@pytest.mark.parametrize("K", [30, 300])
def test_twin_tangent_against_central_differences(K):
    """du/dalpha (direction dalpha = 1, df = 0) on 1 x 24 x 28, alpha = 0.08, against the central difference (h = 1e-6) of
    np_twin.pdhg_denoise: 1e-5 relative in the maximum norm.  (Random unit-size tangents do not meet this at h = 1e-6: the
    perturbation moves pixels across the projection's kink.)"""
    _, f = synth_batch(1, 24, 28, seed=9)
    alpha, h = 0.08, 1e-6
    amap = tw.alpha_to_map(alpha, 28, 24)
    _, du = uj.forward_tangent(f, amap, K, None, np.ones_like(amap))
    fd = (tw.pdhg_denoise(f, alpha + h, maxiter=K) - tw.pdhg_denoise(f, alpha - h, maxiter=K)) / (2 * h)
    d, m = float(np.abs(du - fd).max()), float(np.abs(fd).max())
    print("K %d: max|du - fd| %.3e  max|fd| %.3e  rel %.2e" % (K, d, m, d / m))
    assert d <= 1e-5 * m
