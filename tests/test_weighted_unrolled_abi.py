"""Reverse mode through the iterations of the weighted model on a machine without a GPU: the library exports the five
bpltv_weighted_unrolled_* functions with the header's argument lists, the binding covers them, TVSolver and the torch layer
have the entries, tv_denoise_weighted_unrolled rejects wrong inputs before it touches the library, and the numpy twin the GPU
tests compare against (tests/weighted_unrolled_ref.py) is pinned: its forward to weighted_ref.pdhg bit for bit, its reverse
sweep to torch autograd and to central differences of weighted_ref.pdhg, and every GPU case keeps its projection decisions
away from the threshold."""
import ctypes as C
import os
import re

import numpy as np
import pytest
from conftest import ROOT, synth_batch

import weighted_ref as wr
import weighted_unrolled_ref as wur
from oracle import np_twin as tw

NAMES = {"bpltv_weighted_unrolled_tape_doubles": 3, "bpltv_weighted_unrolled_denoise": 8,
         "bpltv_weighted_unrolled_denoise_device": 8, "bpltv_weighted_unrolled_vjp": 11,
         "bpltv_weighted_unrolled_vjp_device": 12}


def _header_text():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bpltv.h")).read(), flags=re.S)


def _header_args(name):
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name, _header_text())
    assert m, name
    return [" ".join(a.split()) for a in m.group(1).split(",")]


@pytest.mark.parametrize("name", sorted(NAMES))
def test_library_exports_and_binds_the_weighted_unrolled_functions(name):
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
        elif decl.startswith("unsigned long long *"):
            assert a._type_ is C.c_ulonglong
        else:   # arrays: host forms take POINTER(c_double), device forms raw addresses
            assert "double *" in decl, decl
            assert a is (C.c_void_p if name.endswith("_device") else C.POINTER(C.c_double)), (decl, a)


def test_header_argument_order_is_the_issue_s():
    names = lambda fn: [d.split()[-1].lstrip("*") for d in _header_args(fn)]
    assert names("bpltv_weighted_unrolled_tape_doubles") == ["h", "p", "n_out"]
    assert names("bpltv_weighted_unrolled_denoise") == ["h", "w", "wo", "alpha", "am", "an", "p", "u_out"]
    assert names("bpltv_weighted_unrolled_denoise_device") == ["h", "d_w", "wo", "d_alpha", "am", "an", "p", "d_tape"]
    assert names("bpltv_weighted_unrolled_vjp") == ["h", "w", "wo", "alpha", "am", "an", "p", "gu", "grad_f_out",
                                                    "grad_alpha_out", "grad_w_out"]
    assert names("bpltv_weighted_unrolled_vjp_device") == ["h", "d_tape", "d_w", "wo", "d_alpha", "am", "an", "p", "d_gu",
                                                           "d_grad_f", "d_grad_alpha", "d_grad_w"]


def test_binding_still_covers_the_header_and_the_version_is_4():
    from bpldenoising_amd import _lib
    declared = set(re.findall(r"\b(bpltv_\w+)\s*\(", _header_text()))
    assert set(NAMES) <= declared
    assert declared == set(_lib.SYMBOLS), declared ^ set(_lib.SYMBOLS)
    assert re.search(r"#define BPLTV_VERSION 4\b", open(os.path.join(ROOT, "include", "bpltv.h")).read())
    assert _lib.load().bpltv_version() == 4
    assert "9 reverse sweep over the taped weighted iterations" in open(os.path.join(ROOT, "include", "bpltv.h")).read()


def test_solver_and_layer_have_the_entries():
    pytest.importorskip("torch")
    from bpldenoising_amd import TVSolver, torch_layer
    for m in ("weighted_unrolled_tape_doubles", "weighted_unrolled_denoise", "weighted_unrolled_denoise_device",
              "weighted_unrolled_vjp", "weighted_unrolled_vjp_device"):
        assert callable(getattr(TVSolver, m))
    assert callable(torch_layer.tv_denoise_weighted_unrolled)
    import torch
    assert torch_layer.TVDenoiseWeightedUnrolledFunction.jvp is torch.autograd.Function.jvp   # no forward mode


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


def test_tv_denoise_weighted_unrolled_rejects_before_any_library_call(layer):
    import torch
    fn = layer.tv_denoise_weighted_unrolled
    f = torch.zeros(2, 8, 6, dtype=torch.float64)
    a = torch.tensor(0.1, dtype=torch.float64)
    w = torch.ones(8, 6, dtype=torch.float64)
    # dtypes
    with pytest.raises(TypeError, match="torch tensors"):
        fn(np.zeros((2, 8, 6)), a, w, maxiter=5)
    with pytest.raises(TypeError, match="float64"):
        fn(f.float(), a, w, maxiter=5)
    with pytest.raises(TypeError, match="float64"):
        fn(f, a.float(), w, maxiter=5)
    with pytest.raises(TypeError, match="tv_denoise_weighted_unrolled: w must be a torch tensor"):
        fn(f, a, np.ones((8, 6)), maxiter=5)
    with pytest.raises(TypeError, match="tv_denoise_weighted_unrolled: w must be float64"):
        fn(f, a, w.float(), maxiter=5)
    # shapes
    with pytest.raises(ValueError, match="f must have shape"):
        fn(torch.zeros(6, dtype=torch.float64), a, w, maxiter=5)
    for bad in (torch.zeros(3, dtype=torch.float64), torch.zeros(9, 6, dtype=torch.float64)):
        with pytest.raises(ValueError, match="alpha must be"):
            fn(f, bad, w, maxiter=5)
    for bad in (torch.ones(6, 8, dtype=torch.float64), torch.ones(3, 8, 6, dtype=torch.float64), torch.ones(6, dtype=torch.float64)):
        with pytest.raises(ValueError, match="w must have shape"):
            fn(f, a, bad, maxiter=5)
    # devices
    with pytest.raises(ValueError, match="w is on"):
        fn(f, a, torch.ones(8, 6, dtype=torch.float64, device="meta"), maxiter=5)
    with pytest.raises(ValueError, match="alpha is on"):
        fn(f, torch.tensor(0.1, dtype=torch.float64, device="meta"), w, maxiter=5)
    # a negative or NaN weight; zeros pass this check
    for bad in (-0.5, float("nan")):
        wb = w.clone()
        wb[3, 2] = bad
        with pytest.raises(ValueError, match="finite and >= 0"):
            fn(f, a, wb, maxiter=5)
        with pytest.raises(ValueError, match="finite and >= 0"):
            fn(f, a, wb.expand(2, 8, 6).clone(), maxiter=5)
    mask = w.clone()
    mask[::2] = 0.0
    with pytest.raises(ValueError, match="ROCm device"):           # CPU tensors, everything else valid
        fn(f, a, mask, maxiter=5)
    with pytest.raises(ValueError, match="ROCm device"):
        fn(f, a, w.expand(2, 8, 6).clone())


# ---- the twin -------------------------------------------------------------------------------------------------------
SHAPES = [(2, 17, 33), (3, 40, 48)]          # (O, N, M)
WKINDS = ["real", "mask", "ones"]


def case(shape, kind, wkind, seed=5):
    O, N, M = shape
    _, f = synth_batch(O, N, M, seed=seed)
    alpha = wur.alpha_of(kind, N, M)
    gu = np.random.default_rng(seed + 100).standard_normal(f.shape)
    return f, alpha, tw.alpha_to_map(alpha, M, N), wur.weight_of(wkind, O, N, M), gu


@pytest.mark.parametrize("accel", [True, False])
@pytest.mark.parametrize("wkind", WKINDS)
@pytest.mark.parametrize("shape", SHAPES)
def test_twin_forward_is_weighted_ref_bit_for_bit(shape, wkind, accel):
    for kind in ("scalar", "patch", "map"):
        f, alpha, amap, w, _ = case(shape, kind, wkind)
        for K in (50, 203):
            u, tape, _ = wur.fwd_tape(f, amap, w, K, accel=accel)
            assert np.array_equal(u, wr.pdhg(f, alpha, w, K, accel=accel))
            assert tape.shape == (K, 3) + f.shape and np.isfinite(tape).all()
            assert np.array_equal(tape[-1, 2], u)


@pytest.mark.parametrize("wkind", WKINDS)
@pytest.mark.parametrize("kind", ["scalar", "map"])
@pytest.mark.parametrize("shape", SHAPES)
def test_twin_reverse_agrees_with_torch_autograd(shape, kind, wkind):
    """1e-11 * max|ref| on grad_f, the per-pixel grad_alpha and grad_w (measured: at most 1e-13 absolute at max|ref|
    0.3 ... 14)."""
    pytest.importorskip("torch")
    f, alpha, amap, w, gu = case(shape, kind, wkind)
    for K in (50, 203):
        _, tape, tab = wur.fwd_tape(f, amap, w, K)
        gf, ga, gw = wur.reverse(gu, tape, tab, amap, w, f)
        gf0, ga0, gw0 = wur.torch_reference(f, amap, w, K, gu)
        ga, gw = ga.sum(axis=0), (gw if w.ndim == 3 else gw.sum(axis=0))
        for what, g, g0 in (("grad_f", gf, gf0), ("grad_alpha", ga, ga0), ("grad_w", gw, gw0)):
            d, m = float(np.abs(g - g0).max()), float(np.abs(g0).max())
            print("%s %s %s K %d: %s %.2e (max %.2e)" % (shape, kind, wkind, K, what, d, m))
            assert d <= 1e-11 * m, what


@pytest.mark.parametrize("K", [30, 300])
def test_twin_gradient_against_central_differences_on_a_mask(K):
    """0.5 |u_K - ubar|^2 on a masked 1 x 24 x 28, alpha = 0.08: the reverse sweep against central differences (h = 1e-6)
    of weighted_ref.pdhg in f, alpha and w -- the w direction supported on the kept pixels, so that gamma stays 0 -- relative
    1e-5 (measured: at most 1.7e-6)."""
    ub, f = synth_batch(1, 24, 28, seed=9)
    alpha, h = 0.08, 1e-6
    amap = tw.alpha_to_map(alpha, 28, 24)
    w = wur.weight_of("mask", 1, 24, 28)
    assert 0.1 < 1.0 - w.mean() < 0.5 and w.min() == 0.0
    rng = np.random.default_rng(21)
    df, dw = rng.standard_normal(f.shape), rng.standard_normal(w.shape) * w
    u, tape, tab = wur.fwd_tape(f, amap, w, K)
    gf, ga, gw = wur.reverse(u - ub, tape, tab, amap, w, f)
    loss = lambda ff, aa, ww: tw.l2_cost(wr.pdhg(ff, aa, ww, K), ub)
    for what, g, fd in (("f", float((gf * df).sum()), (loss(f + h * df, alpha, w) - loss(f - h * df, alpha, w)) / (2 * h)),
                        ("alpha", float(ga.sum()), (loss(f, alpha + h, w) - loss(f, alpha - h, w)) / (2 * h)),
                        ("w", float((gw[0] * dw).sum()), (loss(f, alpha, w + h * dw) - loss(f, alpha, w - h * dw)) / (2 * h))):
        print("K %d, d/d%s: reverse %.10g central difference %.10g rel %.2e" % (K, what, g, fd, abs(g - fd) / abs(fd)))
        assert abs(g - fd) <= 1e-5 * abs(fd), what


@pytest.mark.parametrize("wkind", ["real", "mask"])
@pytest.mark.parametrize("name", wur.GRADIENT_SHAPES)
def test_gpu_cases_keep_their_projection_decisions_clear_of_the_threshold(name, wkind):
    """min |n2 - alpha^2| / alpha^2 >= 1e-9 over all pixels and iterations of every case test_gpu_weighted_unrolled.py holds
    against the twin (measured: at least 7.8e-8): a projection decision that differs between the kernel's fma and the twin's
    plain arithmetic would need an error six orders of magnitude above rounding."""
    O, N, M = wur.GPU_SHAPES[name]
    f, _ = wur.gpu_data(name)
    w = wur.weight_of(wkind, O, N, M)
    for kind in ("scalar", "patch", "map"):
        amap = tw.alpha_to_map(wur.alpha_of(kind, N, M), M, N)
        _, tape, _ = wur.fwd_tape(f, amap, w, max(wur.GRADIENT_K))   # (the shorter runs are its prefixes: one table per gamma)
        m = wur.min_decision_margin(tape, amap)
        print("%s %s %s: margin %.2e" % (name, wkind, kind, m))
        assert m >= 1e-9
