"""Channel-coupled TV for colour images on a machine without a GPU: the library exports the six bpltv_color_* functions with
the header's argument lists, the binding covers them, TVSolver and the torch layer have the entries, the layer rejects wrong
inputs before it touches the library, and the numpy twin the GPU tests compare against (tests/color_ref.py) is pinned: with
one channel it is unrolled_ref bit for bit, its reverse sweep agrees with torch autograd and with central differences of its
forward, identical channels reproduce TV with alpha / sqrt(C), and every GPU case keeps its projection decisions away from
the threshold."""
import ctypes as C
import os
import re

import numpy as np
import pytest
from conftest import ROOT, synth_batch

import color_ref as cr
import unrolled_ref as ur
from oracle import np_twin as tw

NAMES = {"bpltv_color_denoise": 7, "bpltv_color_denoise_device": 6, "bpltv_color_unrolled_denoise": 7,
         "bpltv_color_unrolled_denoise_device": 7, "bpltv_color_unrolled_vjp": 9, "bpltv_color_unrolled_vjp_device": 10}


def _header_text():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bpltv.h")).read(), flags=re.S)


def _header_args(name):
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name, _header_text())
    assert m, name
    return [" ".join(a.split()) for a in m.group(1).split(",")]


@pytest.mark.parametrize("name", sorted(NAMES))
def test_library_exports_and_binds_the_color_functions(name):
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
    assert names("bpltv_color_denoise") == ["h", "channels", "alpha", "am", "an", "p", "u_out"]
    assert names("bpltv_color_denoise_device") == ["h", "channels", "d_alpha", "am", "an", "p"]
    assert names("bpltv_color_unrolled_denoise") == ["h", "channels", "alpha", "am", "an", "p", "u_out"]
    assert names("bpltv_color_unrolled_denoise_device") == ["h", "channels", "d_alpha", "am", "an", "p", "d_tape"]
    assert names("bpltv_color_unrolled_vjp") == ["h", "channels", "alpha", "am", "an", "p", "gu", "grad_f_out", "grad_alpha_out"]
    assert names("bpltv_color_unrolled_vjp_device") == ["h", "channels", "d_tape", "d_alpha", "am", "an", "p", "d_gu", "d_grad_f",
                                                        "d_grad_alpha"]


def test_binding_still_covers_the_header_and_the_version_is_4():
    from bpldenoising_amd import _lib
    declared = set(re.findall(r"\b(bpltv_\w+)\s*\(", _header_text()))
    assert set(NAMES) <= declared
    assert declared == set(_lib.SYMBOLS), declared ^ set(_lib.SYMBOLS)
    assert all(re.fullmatch(r"bpltv_[a-z_]+", n) for n in NAMES)
    hdr = open(os.path.join(ROOT, "include", "bpltv.h")).read()
    assert re.search(r"#define BPLTV_VERSION 4\b", hdr)
    assert _lib.load().bpltv_version() == 4
    assert "12 reverse sweep over the taped channel-coupled iterations" in hdr
    assert "bpltv_unrolled_tape_doubles gives the doubles of a caller-owned d_tape" in hdr
    st = _lib.BpltvStats()
    st.adjoint_method = 12
    assert st.as_dict()["adjoint_method"] == "color-unrolled"


def test_solver_and_layer_have_the_entries():
    pytest.importorskip("torch")
    from bpldenoising_amd import TVSolver, torch_layer
    for m in ("color_denoise", "color_unrolled_denoise", "color_unrolled_denoise_device", "color_unrolled_vjp",
              "color_unrolled_vjp_device"):
        assert callable(getattr(TVSolver, m))
    assert callable(torch_layer.tv_denoise_color_unrolled)
    import torch
    assert issubclass(torch_layer.TVDenoiseColorUnrolled, torch.nn.Module)
    assert issubclass(torch_layer.TVDenoiseColorUnrolledFunction, torch.autograd.Function)


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
    f = torch.zeros(2, 3, 8, 6, dtype=torch.float64)
    a = torch.tensor(0.08, dtype=torch.float64)
    fn = layer.tv_denoise_color_unrolled
    with pytest.raises(TypeError, match="torch tensors"):
        fn(np.zeros((2, 3, 8, 6)), a, maxiter=5)
    with pytest.raises(TypeError, match="float64"):
        fn(f.float(), a, maxiter=5)
    with pytest.raises(TypeError, match="float64"):
        fn(f, a.float(), maxiter=5)
    with pytest.raises(ValueError, match="channels"):          # 3-D f: (C, H, W) with C > 4
        fn(torch.zeros(5, 8, 6, dtype=torch.float64), a, maxiter=5)
    with pytest.raises(ValueError, match="channels"):
        fn(torch.zeros(2, 5, 8, 6, dtype=torch.float64), a, maxiter=5)
    with pytest.raises(ValueError, match="f must have shape"):  # 2-D f
        fn(torch.zeros(8, 6, dtype=torch.float64), a, maxiter=5)
    for bad in (torch.zeros(2, dtype=torch.float64), torch.zeros(9, 6, dtype=torch.float64), torch.zeros(8, 7, dtype=torch.float64),
                torch.zeros(3, 8, 6, dtype=torch.float64), torch.zeros(2, 3, 8, 6, dtype=torch.float64)):
        with pytest.raises(ValueError, match="alpha must be"):
            fn(f, bad, maxiter=5)
    with pytest.raises(ValueError, match="alpha is on"):
        fn(f, a.to("meta"), maxiter=5)
    with pytest.raises(ValueError, match="ROCm device"):        # CPU tensors, everything else valid
        fn(f, a, maxiter=5)
    with pytest.raises(ValueError, match="ROCm device"):
        fn(f[0], torch.zeros(8, 6, dtype=torch.float64), checkpoint_every=5)
    m = layer.TVDenoiseColorUnrolled(0.08, maxiter=7)
    assert m.alpha.requires_grad and m.alpha.dtype == torch.float64 and tuple(m.alpha.shape) == () and m.maxiter == 7
    with pytest.raises(ValueError, match="ROCm device"):
        m(f)
    # the existing functions keep refusing 4-D input
    for old in (layer.tv_denoise, layer.tv_denoise_unrolled):
        with pytest.raises(ValueError, match=r"f must have shape \(B, H, W\) or \(H, W\)"):
            old(f, a)


# ---- the twin -------------------------------------------------------------------------------------------------------
def _case(name, kind):
    B, Cc, N, M = cr.SHAPES[name]
    f, gu = cr.gpu_data(name)
    alpha = cr.alpha_of(kind, N, M)
    return f, gu, alpha, tw.alpha_to_map(alpha, M, N)


@pytest.mark.parametrize("accel", [True, False])
@pytest.mark.parametrize("name", ["2x3x17x33", "1x2x9x1", "1x4x1x9", "1x3x2x2"])
def test_twin_with_one_channel_is_the_tv_twin_bit_for_bit(name, accel):
    for kind in cr.KINDS:
        f, _, _, amap = _case(name, kind)
        for K in (7, 50):
            u, tape, tab = cr.fwd_tape(f, amap, K, 1, accel=accel)
            u0, tape0, tab0 = ur.fwd_tape(f, amap, K, accel=accel)
            assert np.array_equal(u, u0) and np.array_equal(tape, tape0) and np.array_equal(tab, tab0)


@pytest.mark.parametrize("kind", cr.KINDS)
@pytest.mark.parametrize("name", sorted(cr.SHAPES))
def test_twin_reverse_agrees_with_torch_autograd(name, kind):
    """1e-11 * max|ref| on grad_f and on the per-pixel parameter terms summed over the colour images (measured: at most
    6.1e-14 on ga and 3.2e-14 on grad_f at max|ref| 2 ... 5)."""
    pytest.importorskip("torch")
    B, Cc, N, M = cr.SHAPES[name]
    f, gu, _, amap = _case(name, kind)
    K = 50
    _, tape, tab, gf, ga = cr.twin_case(name, kind, K)
    gf0, ga0 = cr.torch_reference(f, amap, K, gu, Cc)
    gas = np.zeros((N, M))
    for b in range(B):
        gas = gas + ga[b]
    df, da = float(np.abs(gf - gf0).max()), float(np.abs(gas - ga0).max())
    print("%s %s: grad_f %.2e (max|ref| %.2e)  ga %.2e (max|ref| %.2e)" % (name, kind, df, np.abs(gf0).max(), da, np.abs(ga0).max()))
    assert df <= 1e-11 * float(np.abs(gf0).max())
    assert da <= 1e-11 * float(np.abs(ga0).max())


@pytest.mark.parametrize("K", [30, 300])
def test_twin_gradient_against_central_differences(K):
    """d/dalpha of 0.5 |u_K - ubar|^2 on synth_batch(3, 24, 28, seed=9) as one colour image, alpha = 0.08: the reverse sweep
    against central differences of the twin forward, h = 1e-6, relative 1e-5 (the margin of the TV twin's test)."""
    ub, f = synth_batch(3, 24, 28, seed=9)
    alpha, h = 0.08, 1e-6
    amap = tw.alpha_to_map(alpha, 28, 24)
    u, tape, tab = cr.fwd_tape(f, amap, K, 3)
    _, ga = cr.reverse(u - ub, tape, tab, amap, 3)
    g = float(ga.sum())
    cost = lambda a: tw.l2_cost(cr.fwd_tape(f, tw.alpha_to_map(a, 28, 24), K, 3)[0], ub)
    fd = (cost(alpha + h) - cost(alpha - h)) / (2 * h)
    print("K %d: reverse sweep %.10g central difference %.10g rel %.2e" % (K, g, fd, abs(g - fd) / abs(fd)))
    assert abs(g - fd) <= 1e-5 * abs(fd)


@pytest.mark.parametrize("Cc", [2, 3, 4])
def test_identical_channels_are_tv_with_alpha_over_sqrt_c(Cc):
    """C copies of one image: every channel of the coupled solve is the TV solve with alpha / sqrt(C), to 1e-14 (measured
    4.4e-16)."""
    _, f1 = synth_batch(2, 17, 33, seed=38)
    f = np.repeat(f1, Cc, axis=0)   # (b, c) -> plane b*C + c
    for alpha in (0.08, cr.alpha_of("map", 17, 33)):
        amap = tw.alpha_to_map(alpha, 33, 17)
        for K in (7, 50, 203):
            u = cr.fwd_tape(f, amap, K, Cc)[0]
            u1 = ur.fwd_tape(f1, amap / np.sqrt(Cc), K)[0]
            d = float(np.abs(u - np.repeat(u1, Cc, axis=0)).max())
            assert d <= 1e-14, (Cc, K, d)


@pytest.mark.parametrize("kind", cr.KINDS)
@pytest.mark.parametrize("name", sorted(cr.SHAPES))
def test_gpu_cases_keep_their_projection_decisions_clear_of_the_threshold(name, kind):
    """min | n2 - alpha^2 | / alpha^2 >= 1e-9 over all pixels and iterations of every case test_gpu_color.py holds against the
    twin (measured: at least 9.7e-6 for the scalar and the map): a decision that differs between the kernel's fma and the
    twin's plain arithmetic would need an error orders of magnitude above rounding."""
    B, Cc, N, M = cr.SHAPES[name]
    _, _, _, amap = _case(name, kind)
    for K in cr.KS:
        m = cr.min_decision_margin(cr.twin_case(name, kind, K)[1], amap, Cc)
        print("%s %s K %d: margin %.2e" % (name, kind, K, m))
        assert m >= 1e-9
