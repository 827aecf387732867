"""Forward mode through the channel-coupled iterations on a machine without a GPU: the library exports the three
bpltv_color_unrolled_jvp / _gauss_newton functions with the header's argument lists, the binding covers them, TVSolver and the
torch layer have the entries, the layer with forward_mode=True rejects wrong inputs before it touches the library, and the numpy
twin the GPU tests compare against (tests/color_jvp_ref.py) is pinned: its primal is color_ref's bit for bit, it is the transpose
of color_ref.reverse, it agrees with torch.func.jvp and with central differences of the twin forward, identical channels
reproduce the TV tangent with alpha / sqrt(C), and with one channel it is unrolled_jvp_ref bit for bit.

The GPU cases reuse color_ref.SHAPES, KINDS, KS and alpha_of unchanged: test_color_abi.py's margin test already holds their
projection decisions clear of the threshold."""
import ctypes as C
import os
import re

import numpy as np
import pytest
from conftest import ROOT, synth_batch

import color_jvp_ref as cj
import color_ref as cr
import unrolled_jvp_ref as uj
from oracle import np_twin as tw

NAMES = {"bpltv_color_unrolled_jvp": 11, "bpltv_color_unrolled_jvp_device": 11, "bpltv_color_unrolled_gauss_newton": 9}


def _header_text():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bpltv.h")).read(), flags=re.S)


def _header_args(name):
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name, _header_text())
    assert m, name
    return [" ".join(a.split()) for a in m.group(1).split(",")]


@pytest.mark.parametrize("name", sorted(NAMES))
def test_library_exports_and_binds_the_color_jvp_functions(name):
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
    assert names("bpltv_color_unrolled_jvp") == ["h", "channels", "alpha", "am", "an", "p", "ndir", "df", "dalpha", "du_out", "u_out"]
    assert names("bpltv_color_unrolled_jvp_device") == ["h", "channels", "d_alpha", "am", "an", "p", "ndir", "d_df", "d_dalpha", "d_du",
                                                        "d_u"]
    assert names("bpltv_color_unrolled_gauss_newton") == ["h", "channels", "alpha", "am", "an", "p", "cost_out", "grad_out", "hess_out"]


def test_binding_still_covers_the_header_and_the_version_is_4():
    from bpldenoising_amd import _lib
    declared = set(re.findall(r"\b(bpltv_\w+)\s*\(", _header_text()))
    assert set(NAMES) <= declared
    assert declared == set(_lib.SYMBOLS), declared ^ set(_lib.SYMBOLS)
    hdr = open(os.path.join(ROOT, "include", "bpltv.h")).read()
    assert re.search(r"#define BPLTV_VERSION 4\b", hdr)
    assert _lib.load().bpltv_version() == 4
    assert "13 tangent sweep through the channel-coupled iterations" in hdr
    st = _lib.BpltvStats()
    st.adjoint_method = 13
    assert st.as_dict()["adjoint_method"] == "color-unrolled-jvp"


def test_solver_and_layer_have_the_entries():
    pytest.importorskip("torch")
    import inspect
    import torch
    from bpldenoising_amd import TVSolver, torch_layer
    for m in ("color_unrolled_jvp", "color_unrolled_jvp_device", "color_unrolled_gauss_newton"):
        assert callable(getattr(TVSolver, m))
    fwd = torch_layer.TVDenoiseColorUnrolledForwardFunction
    assert issubclass(fwd, torch_layer.TVDenoiseColorUnrolledFunction) and issubclass(fwd, torch.autograd.Function)
    assert "jvp" in vars(fwd) and "jvp" not in vars(torch_layer.TVDenoiseColorUnrolledFunction)
    assert inspect.signature(torch_layer.tv_denoise_color_unrolled).parameters["forward_mode"].default is False
    assert inspect.signature(torch_layer.TVDenoiseColorUnrolled.__init__).parameters["forward_mode"].default is False


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


def test_the_forward_mode_layer_rejects_before_any_library_call(layer):
    """test_color_abi.py's rejections, with forward_mode=True."""
    import torch
    f = torch.zeros(2, 3, 8, 6, dtype=torch.float64)
    a = torch.tensor(0.08, dtype=torch.float64)
    fn = lambda *args, **kw: layer.tv_denoise_color_unrolled(*args, forward_mode=True, **kw)
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
    m = layer.TVDenoiseColorUnrolled(0.08, maxiter=7, forward_mode=True)
    assert m.forward_mode is True and m.alpha.requires_grad and m.alpha.dtype == torch.float64 and m.maxiter == 7
    assert layer.TVDenoiseColorUnrolled(0.08).forward_mode is False
    with pytest.raises(ValueError, match="ROCm device"):
        m(f)


# ---- the twin -------------------------------------------------------------------------------------------------------
def _case(name, kind):
    B, Cc, N, M = cr.SHAPES[name]
    f, gu = cr.gpu_data(name)
    return f, gu, tw.alpha_to_map(cr.alpha_of(kind, N, M), M, N)


@pytest.mark.parametrize("kind", cr.KINDS)
@pytest.mark.parametrize("name", sorted(cr.SHAPES))
def test_twin_primal_is_color_ref_bit_for_bit_and_the_tangent_its_reverse_s_transpose(name, kind):
    """u bitwise color_ref.fwd_tape's; <du, gu> = <df, gf> + <dalpha, sum_b ga_b> to 1e-11 * sum|du * gu| (measured: at most
    3.8e-16 of that sum over all shapes, kinds and K in {50, 203})."""
    B, Cc, N, M = cr.SHAPES[name]
    f, gu, amap = _case(name, kind)
    df, _, damap = cj.tangents(name, kind)
    for K in (50, 203):
        u0, _, _, gf0, ga0 = cr.twin_case(name, kind, K)
        u, du = cj.twin_tangent(name, kind, K, "both")
        assert np.array_equal(u, u0)
        lhs = float((du * gu).sum())
        rhs = float((df * gf0).sum()) + float((damap * ga0.sum(axis=0)).sum())
        scale = float(np.abs(du * gu).sum())
        print("%s %s K %d: |lhs - rhs| %.2e = %.2e of sum|du * gu|" % (name, kind, K, abs(lhs - rhs), abs(lhs - rhs) / scale))
        assert abs(lhs - rhs) <= 1e-11 * scale


@pytest.mark.parametrize("kind", cr.KINDS)
@pytest.mark.parametrize("name", sorted(cr.SHAPES))
def test_twin_agrees_with_torch_func_jvp(name, kind):
    """1e-11 * max|ref| at K = 50 (measured: at most 6.3e-15 relative)."""
    pytest.importorskip("torch")
    B, Cc, N, M = cr.SHAPES[name]
    f, _, amap = _case(name, kind)
    df, _, damap = cj.tangents(name, kind)
    u, du = cj.twin_tangent(name, kind, 50, "both")
    u0, du0 = cj.torch_forward_reference(f, amap, 50, Cc, df, damap)
    d, m = float(np.abs(du - du0).max()), float(np.abs(du0).max())
    print("%s %s: du %.2e (max|ref| %.2e)" % (name, kind, d, m))
    assert d <= 1e-11 * m


@pytest.mark.parametrize("K", [30, 300])
def test_twin_tangent_against_central_differences(K):
    """du/dalpha on synth_batch(3, 24, 28, seed=9) as one colour image, alpha = 0.08, h = 1e-6: 1e-5 relative in the maximum
    norm (measured 5.9e-10 at K = 30, 3.4e-10 at K = 300)."""
    _, f = synth_batch(3, 24, 28, seed=9)
    alpha, h = 0.08, 1e-6
    _, du = cj.forward_tangent(f, tw.alpha_to_map(alpha, 28, 24), K, 3, damap=np.ones((24, 28)))
    fwd = lambda a: cr.fwd_tape(f, tw.alpha_to_map(a, 28, 24), K, 3)[0]
    fd = (fwd(alpha + h) - fwd(alpha - h)) / (2 * h)
    d, m = float(np.abs(du - fd).max()), float(np.abs(fd).max())
    print("K %d: max|du - fd| %.3e  max|fd| %.3e  rel %.2e" % (K, d, m, d / m))
    assert d <= 1e-5 * m


@pytest.mark.parametrize("Cc", [2, 3, 4])
def test_identical_channels_are_the_tv_tangent_with_alpha_over_sqrt_c(Cc):
    """C copies of one image and of one tangent: every channel of the coupled tangent is the TV tangent with alpha / sqrt(C) and
    dalpha / sqrt(C), to 1e-11 * max|ref| (measured at most 4.8e-14, 1.6e-14 of max|ref|)."""
    _, f1 = synth_batch(2, 17, 33, seed=38)
    rng = np.random.default_rng(39)
    df1 = rng.standard_normal(f1.shape)
    f, df = np.repeat(f1, Cc, axis=0), np.repeat(df1, Cc, axis=0)   # (b, c) -> plane b*C + c
    for alpha, damap in ((0.08, np.full((17, 33), 0.7)), (cr.alpha_of("map", 17, 33), rng.standard_normal((17, 33)))):
        amap = tw.alpha_to_map(alpha, 33, 17)
        for K in (7, 50, 203):
            _, du = cj.forward_tangent(f, amap, K, Cc, df, damap)
            _, du1 = uj.forward_tangent(f1, amap / np.sqrt(Cc), K, df1, damap / np.sqrt(Cc))
            d, m = float(np.abs(du - np.repeat(du1, Cc, axis=0)).max()), float(np.abs(du1).max())
            print("C %d K %d: %.2e (max|ref| %.2e)" % (Cc, K, d, m))
            assert d <= 1e-11 * m, (Cc, K, d)


@pytest.mark.parametrize("accel", [True, False])
@pytest.mark.parametrize("name", ["2x3x17x33", "1x2x9x1", "1x4x1x9", "1x3x2x2"])
def test_twin_with_one_channel_is_the_tv_twin_bit_for_bit(name, accel):
    for kind in cr.KINDS:
        f, _, amap = _case(name, kind)
        df, _, damap = cj.tangents(name, kind)
        for K in (7, 50):
            u, du = cj.forward_tangent(f, amap, K, 1, df, damap, accel=accel)
            u0, du0 = uj.forward_tangent(f, amap, K, df, damap, accel=accel)
            assert np.array_equal(u, u0) and np.array_equal(du, du0)
