"""Reverse mode through the iterations of the sum-of-regularisers model on a machine without a GPU: the library exports the
nine bpltv_sumregs_unrolled_* functions with the header's argument lists, the binding covers them, TVSolver and the torch
layer have the entries, the layer rejects wrong inputs before it touches the library, and the numpy twin the GPU tests compare
against (tests/sumregs_unrolled_ref.py) is pinned: its forward to np_twin_sumregs.pdhg bit for bit, its reverse sweep to
torch autograd and to central differences of np_twin_sumregs.pdhg, and every GPU case keeps its projection decisions away
from the threshold."""
import ctypes as C
import os
import re

import numpy as np
import pytest
from conftest import ROOT, synth_batch

import sumregs_unrolled_ref as sur
from oracle import np_twin as tw
from oracle import np_twin_sumregs as sr

NAMES = {"bpltv_sumregs_unrolled_tape_doubles": 3, "bpltv_sumregs_unrolled_denoise": 6,
         "bpltv_sumregs_unrolled_denoise_device": 6, "bpltv_sumregs_unrolled_vjp": 8, "bpltv_sumregs_unrolled_vjp_device": 9,
         "bpltv_sumregs_unrolled_denoise_each": 6, "bpltv_sumregs_unrolled_denoise_each_device": 6,
         "bpltv_sumregs_unrolled_vjp_each": 8, "bpltv_sumregs_unrolled_vjp_each_device": 9}


def _header_text():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bpltv.h")).read(), flags=re.S)


def _header_args(name):
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name, _header_text())
    assert m, name
    return [" ".join(a.split()) for a in m.group(1).split(",")]


@pytest.mark.parametrize("name", sorted(NAMES))
def test_library_exports_and_binds_the_sumregs_unrolled_functions(name):
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
    assert names("bpltv_sumregs_unrolled_tape_doubles") == ["h", "p", "n_out"]
    assert names("bpltv_sumregs_unrolled_denoise") == ["h", "alpha", "am", "an", "p", "u_out"]
    assert names("bpltv_sumregs_unrolled_denoise_device") == ["h", "d_alpha", "am", "an", "p", "d_tape"]
    assert names("bpltv_sumregs_unrolled_vjp") == ["h", "alpha", "am", "an", "p", "gu", "grad_f_out", "grad_alpha_out"]
    assert names("bpltv_sumregs_unrolled_vjp_device") == ["h", "d_tape", "d_alpha", "am", "an", "p", "d_gu", "d_grad_f",
                                                          "d_grad_alpha"]
    assert names("bpltv_sumregs_unrolled_denoise_each") == ["h", "alphas", "am", "an", "p", "u_out"]
    assert names("bpltv_sumregs_unrolled_denoise_each_device") == ["h", "d_alphas", "am", "an", "p", "d_tape"]
    assert names("bpltv_sumregs_unrolled_vjp_each") == ["h", "alphas", "am", "an", "p", "gu", "grad_f_out", "grad_alphas_out"]
    assert names("bpltv_sumregs_unrolled_vjp_each_device") == ["h", "d_tape", "d_alphas", "am", "an", "p", "d_gu", "d_grad_f",
                                                               "d_grad_alphas"]


def test_binding_still_covers_the_header_and_the_version_is_4():
    from bpldenoising_amd import _lib
    declared = set(re.findall(r"\b(bpltv_\w+)\s*\(", _header_text()))
    assert set(NAMES) <= declared
    assert declared == set(_lib.SYMBOLS), declared ^ set(_lib.SYMBOLS)
    hdr = open(os.path.join(ROOT, "include", "bpltv.h")).read()
    assert re.search(r"#define BPLTV_VERSION 4\b", hdr)
    assert _lib.load().bpltv_version() == 4
    assert "10 reverse sweep over the taped sum-of-regularisers iterations" in hdr
    assert "reserved[0], the forward variant, is ignored" in hdr
    st = _lib.BpltvStats()
    st.adjoint_method = 10
    assert st.as_dict()["adjoint_method"] == "sumregs-unrolled"


def test_solver_and_layer_have_the_entries():
    pytest.importorskip("torch")
    from bpldenoising_amd import TVSolver, torch_layer
    for m in ("sumregs_unrolled_tape_doubles", "sumregs_unrolled_denoise", "sumregs_unrolled_denoise_device",
              "sumregs_unrolled_vjp", "sumregs_unrolled_vjp_device", "sumregs_unrolled_denoise_each",
              "sumregs_unrolled_denoise_each_device", "sumregs_unrolled_vjp_each", "sumregs_unrolled_vjp_each_device"):
        assert callable(getattr(TVSolver, m))
    assert callable(torch_layer.sumregs_denoise_unrolled) and callable(torch_layer.sumregs_denoise_unrolled_each)
    import torch
    assert issubclass(torch_layer.SumRegsDenoiseUnrolled, torch.nn.Module)
    assert torch_layer.SumRegsDenoiseUnrolledFunction.jvp is torch.autograd.Function.jvp   # no forward mode


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


def test_the_layer_rejects_before_any_library_call(layer):
    import torch
    f = torch.zeros(2, 8, 6, dtype=torch.float64)
    a = torch.tensor([0.03, 0.02, 0.04], dtype=torch.float64)
    fn, each = layer.sumregs_denoise_unrolled, layer.sumregs_denoise_unrolled_each
    with pytest.raises(TypeError, match="torch tensors"):
        fn(np.zeros((2, 8, 6)), a, maxiter=5)
    with pytest.raises(TypeError, match="float64"):
        fn(f.float(), a, maxiter=5)
    with pytest.raises(TypeError, match="float64"):
        fn(f, a.float(), maxiter=5)
    with pytest.raises(ValueError, match="f must have shape"):
        fn(torch.zeros(6, dtype=torch.float64), a, maxiter=5)
    for bad in (torch.zeros(2, dtype=torch.float64), torch.zeros((), dtype=torch.float64), torch.zeros(3, 9, 6, dtype=torch.float64),
                torch.zeros(2, 3, dtype=torch.float64)):
        with pytest.raises(ValueError, match="alpha must be"):
            fn(f, bad, maxiter=5)
    with pytest.raises(ValueError, match="alpha is on"):
        fn(f, a.to("meta"), maxiter=5)
    with pytest.raises(ValueError, match="ROCm device"):     # CPU tensors, everything else valid
        fn(f, a, maxiter=5)
    with pytest.raises(ValueError, match="ROCm device"):
        fn(f, torch.zeros(3, 8, 6, dtype=torch.float64))
    # one block per image
    ae = a.expand(2, 3).clone()
    with pytest.raises(TypeError, match="float64"):
        each(f, ae.float(), maxiter=5)
    with pytest.raises(ValueError, match="sumregs_denoise_unrolled_each: f must have shape"):
        each(f[0], ae, maxiter=5)
    for bad in (a, torch.zeros(3, 3, dtype=torch.float64), torch.zeros(2, 3, 9, 6, dtype=torch.float64)):
        with pytest.raises(ValueError, match="sumregs_denoise_unrolled_each: alpha must be"):
            each(f, bad, maxiter=5)
    with pytest.raises(ValueError, match="ROCm device"):
        each(f, ae)
    # no forward mode through these iterations: a ValueError that names the implicit alternative
    for call in (lambda: fn(f, a, forward_mode=True), lambda: each(f, ae, forward_mode=True),
                 lambda: layer.SumRegsDenoiseUnrolled([0.03, 0.02, 0.04], forward_mode=True)):
        with pytest.raises(ValueError, match=r"sumregs_denoise\(\.\.\., forward_mode=True\)") as e:
            call()
        assert not isinstance(e.value, NotImplementedError)
    m = layer.SumRegsDenoiseUnrolled([0.03, 0.02, 0.04], maxiter=7)
    assert m.alpha.requires_grad and m.alpha.dtype == torch.float64 and tuple(m.alpha.shape) == (3,)
    with pytest.raises(ValueError, match="ROCm device"):
        m(f)


# ---- the twin -------------------------------------------------------------------------------------------------------
SHAPES = [(2, 17, 33), (1, 9, 1), (1, 1, 9), (1, 2, 2)]          # (O, N, M)


def case(shape, kind, seed=5):
    """The data of sumregs_unrolled_ref.gpu_data (seed + M).  A 2 x 2 image of little contrast (synth_batch seed 5: 0.33) is
    flat after 203 iterations with the patch and map weights, u no longer depends on them, and the reference gradient is what
    is left of O(1) terms cancelling to 1e-11: max|ref| would not measure the terms summed.  Seed 7 has contrast 0.6."""
    O, N, M = shape
    _, f = synth_batch(O, N, M, seed=seed + M)
    gu = np.random.default_rng(seed + 100).standard_normal(f.shape)
    return f, sur.alpha_of(kind, N, M), gu


@pytest.mark.parametrize("accel", [True, False])
@pytest.mark.parametrize("shape", SHAPES)
def test_twin_forward_is_np_twin_sumregs_bit_for_bit(shape, accel):
    for kind in sur.ALPHA_KINDS:
        f, alpha, _ = case(shape, kind)
        for K in (7, 50):
            u, tape, tab = sur.fwd_tape(f, alpha, K, accel=accel)
            assert np.array_equal(u, sr.pdhg(f, alpha, maxiter=K, accel=accel))
            assert tape.shape == (K, 6) + f.shape and np.isfinite(tape).all() and tab.shape == (K, 3)
    # one block per image is the shared solve image by image
    f, alpha, _ = case((2, 17, 33), "patch")
    blocks = np.stack([alpha, 1.5 * alpha])
    u, tape, _ = sur.fwd_tape(f, blocks, 20)
    for k in range(2):
        uk, tk, _ = sur.fwd_tape(f[k:k + 1], blocks[k], 20)
        assert np.array_equal(u[k], uk[0]) and np.array_equal(tape[:, :, k], tk[:, :, 0])


@pytest.mark.parametrize("kind", sur.ALPHA_KINDS)
@pytest.mark.parametrize("shape", SHAPES)
def test_twin_reverse_agrees_with_torch_autograd(shape, kind):
    """1e-11 * max|ref| on grad_f and on each per-pixel, per-image ga slice -- the margin the two other twins are held to.
    One slice is left out: a_r = 0 on an image with both axes.  There y^(r) = 0, z = sigma G_r xbar, and ga_r sums e . gy with
    e = z / |z|; where the image is nearly flat |z| falls to 1e-12 and the DIRECTION of z carries the forward pass's rounding
    at 1e-16 / 1e-12, which the twin's and torch's forward passes (other summation orders) do not share -- measured 1.3e-10
    at max|ref| 4.3 on 2 x 17 x 33, with grad_f and the two other slices at 1e-15.  On one row or one column e = +-1 and the
    slice is held like the others."""
    pytest.importorskip("torch")
    f, alpha, gu = case(shape, kind)
    O, N, M = shape
    amaps = sr.alpha_maps(alpha, M, N)
    for K in (50, 203):
        _, tape, tab = sur.fwd_tape(f, alpha, K)
        gf, ga = sur.reverse(gu, tape, tab, amaps)
        gf0, ga0 = sur.torch_reference(f, amaps, K, gu)
        for what, g, g0 in [("grad_f", gf, gf0)] + [("ga[%d]" % r, ga[r], ga0[r]) for r in range(3)]:
            d, m = float(np.abs(g - g0).max()), float(np.abs(g0).max())
            print("%s %s K %d: %s %.2e (max %.2e)" % (shape, kind, K, what, d, m))
            if not (kind == "zero" and what == "ga[1]" and min(N, M) > 1):
                assert d <= 1e-11 * m, what
        if kind == "zero":
            assert np.abs(ga[1]).max() > 0     # the slice of zeros has a gradient: every pixel with a difference projects


def test_reduce_alpha_shapes_and_order():
    ga = np.random.default_rng(3).standard_normal((3, 2, 17, 33))
    v = sur.reduce_alpha(ga, np.zeros(3))
    assert v.shape == (3,) and np.allclose(v, ga.sum(axis=(1, 2, 3)), rtol=1e-13)
    p = sur.reduce_alpha(ga, np.zeros((3, 2, 3)))
    assert p.shape == (3, 2, 3) and np.allclose(p.sum(axis=(1, 2)), v, rtol=1e-12)
    assert np.array_equal(sur.reduce_alpha(ga, np.zeros((3, 17, 33))), ga[:, 0] + ga[:, 1])
    e = sur.reduce_alpha(ga, np.zeros((2, 3)))
    assert e.shape == (2, 3) and np.allclose(e[0] + e[1], v, rtol=1e-12)


@pytest.mark.parametrize("K", [30, 300])
def test_twin_gradient_against_central_differences(K):
    """0.5 |u_K - ubar|^2 on synth_batch(1, 24, 28, seed=9), alpha = (0.03, 0.02, 0.04): the reverse sweep against central
    differences (h = 1e-7) of np_twin_sumregs.pdhg in each of the three weights, relative 1e-7 (the issue measured 2.5e-9 at
    most; h = 1e-6 crosses projection kinks and reaches 3.2e-5)."""
    ub, f, alpha, h = sur.fd_case()
    u, tape, tab = sur.fwd_tape(f, alpha, K)
    _, ga = sur.reverse(u - ub, tape, tab, sr.alpha_maps(alpha, 28, 24))
    g = sur.reduce_alpha(ga, alpha)
    loss = lambda a: tw.l2_cost(sr.pdhg(f, a, maxiter=K), ub)
    for r in range(3):
        e = np.zeros(3)
        e[r] = h
        fd = (loss(alpha + e) - loss(alpha - e)) / (2 * h)
        rel = abs(g[r] - fd) / abs(fd)
        print("K %d, d/da%d: reverse %.12g central difference %.12g rel %.2e" % (K, r + 1, g[r], fd, rel))
        assert rel <= 1e-7, r


@pytest.mark.parametrize("kind", sur.ALPHA_KINDS)
@pytest.mark.parametrize("name", sur.GRADIENT_SHAPES)
def test_gpu_cases_keep_their_projection_decisions_clear_of_the_threshold(name, kind):
    """min | |z|^2 - a^2 | / a^2 >= 1e-9 over all pixels, iterations and regularisers (slices of zeros skipped) of every case
    test_gpu_sumregs_unrolled.py holds against the twin: a projection decision that differs between the kernel's fma and the
    twin's plain arithmetic would need an error six orders of magnitude above rounding."""
    O, N, M = sur.GPU_SHAPES[name]
    f, _ = sur.gpu_data(name, kind)
    alpha = sur.alpha_of(kind, N, M)
    _, tape, _ = sur.fwd_tape(f, alpha, max(sur.GRADIENT_K))   # (the shorter runs are its prefixes)
    m = sur.min_decision_margin(tape, sr.alpha_maps(alpha, M, N))
    print("%s %s: margin %.2e" % (name, kind, m))
    assert m >= 1e-9
