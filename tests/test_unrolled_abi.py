"""Reverse mode through the PDHG iterations on a machine without a GPU: the library exports the five bpltv_unrolled_*
functions with the header's argument lists, the binding covers them, TVSolver has the methods, tv_denoise_unrolled rejects
wrong inputs before it touches the library, and the numpy twin the GPU tests compare against (tests/unrolled_ref.py) is
pinned: its forward to oracle.np_twin.pdhg_denoise bit for bit, its reverse sweep to torch autograd and to central
differences of np_twin.pdhg_denoise."""
import ctypes as C
import os
import re

import numpy as np
import pytest
from conftest import ROOT, synth_batch

import unrolled_ref as ur
from oracle import np_twin as tw

NAMES = {"bpltv_unrolled_tape_doubles": 3, "bpltv_unrolled_denoise": 6, "bpltv_unrolled_denoise_device": 6,
         "bpltv_unrolled_vjp": 8, "bpltv_unrolled_vjp_device": 9}


def _header_args(name):
    txt = open(os.path.join(ROOT, "include", "bpltv.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name, txt)
    assert m, name
    return [" ".join(a.split()) for a in m.group(1).split(",")]


@pytest.mark.parametrize("name", sorted(NAMES))
def test_library_exports_and_binds_the_unrolled_functions(name):
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
    assert names("bpltv_unrolled_tape_doubles") == ["h", "p", "n_out"]
    assert names("bpltv_unrolled_denoise") == ["h", "alpha", "am", "an", "p", "u_out"]
    assert names("bpltv_unrolled_denoise_device") == ["h", "d_alpha", "am", "an", "p", "d_tape"]
    assert names("bpltv_unrolled_vjp") == ["h", "alpha", "am", "an", "p", "gu", "grad_f_out", "grad_alpha_out"]
    assert names("bpltv_unrolled_vjp_device") == ["h", "d_tape", "d_alpha", "am", "an", "p", "d_gu", "d_grad_f", "d_grad_alpha"]
    txt = open(os.path.join(ROOT, "include", "bpltv.h")).read()
    assert re.search(r"#define BPLTV_VERSION 4\b", txt)
    assert "7 reverse sweep over the taped iterations" in txt


def test_solver_has_the_unrolled_methods():
    from bpldenoising_amd import TVSolver
    for m in ("unrolled_denoise", "unrolled_denoise_device", "unrolled_vjp", "unrolled_vjp_device", "unrolled_tape_doubles"):
        assert callable(getattr(TVSolver, m))


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


def test_tv_denoise_unrolled_rejects_before_any_library_call(layer):
    import torch
    f = torch.zeros(2, 8, 6, dtype=torch.float64)
    a = torch.tensor(0.1, dtype=torch.float64)
    with pytest.raises(TypeError, match="torch tensors"):
        layer.tv_denoise_unrolled(np.zeros((2, 8, 6)), a, maxiter=5)
    with pytest.raises(TypeError, match="float64"):
        layer.tv_denoise_unrolled(f.float(), a, maxiter=5)
    with pytest.raises(TypeError, match="float64"):
        layer.tv_denoise_unrolled(f, a.float(), maxiter=5)
    with pytest.raises(ValueError, match="f must have shape"):
        layer.tv_denoise_unrolled(torch.zeros(6, dtype=torch.float64), a, maxiter=5)
    for bad in (torch.zeros(3, dtype=torch.float64), torch.zeros(9, 6, dtype=torch.float64),
                torch.zeros(2, 8, 6, dtype=torch.float64)):
        with pytest.raises(ValueError, match="alpha must be"):
            layer.tv_denoise_unrolled(f, bad, maxiter=5)
    with pytest.raises(ValueError, match="alpha is on"):
        layer.tv_denoise_unrolled(f, torch.tensor(0.1, dtype=torch.float64, device="meta"), maxiter=5)
    with pytest.raises(ValueError, match="ROCm device"):           # CPU tensors, everything else valid
        layer.tv_denoise_unrolled(f, a, maxiter=5)
    with pytest.raises(ValueError, match="ROCm device"):
        layer.TVDenoiseUnrolled(0.1, maxiter=5)(f)
    assert layer.TVDenoiseUnrolledFunction.jvp is torch.autograd.Function.jvp   # no forward mode
    assert isinstance(layer.TVDenoiseUnrolled(0.1).alpha, torch.nn.Parameter)


def test_importing_the_package_does_not_import_torch():
    import subprocess
    import sys
    code = "import sys; import bpldenoising_amd; assert 'torch' not in sys.modules; assert not hasattr(bpldenoising_amd, 'tv_denoise_unrolled')"
    subprocess.check_call([sys.executable, "-c", code], cwd=ROOT)


# ---- the twin -------------------------------------------------------------------------------------------------------
SHAPES = [(2, 17, 33), (3, 40, 48)]          # (O, N, M)
DEGENERATE = [(1, 9, 1), (1, 1, 9)]


def alpha_of(kind, N, M):
    if kind == "scalar":
        return 0.08
    if kind == "patch":
        return np.array([[0.05, 0.1, 0.07], [0.12, 0.06, 0.09]])[:min(2, N), :min(3, M)]   # (an, am) = (2, 3)
    return 0.05 + 0.1 * np.random.default_rng(8).random((N, M))


def case(shape, kind, seed=5):
    O, N, M = shape
    _, f = synth_batch(O, N, M, seed=seed)
    alpha = alpha_of(kind, N, M)
    gu = np.random.default_rng(seed + 100).standard_normal(f.shape)
    return f, alpha, tw.alpha_to_map(alpha, M, N), gu


@pytest.mark.parametrize("accel", [True, False])
@pytest.mark.parametrize("kind", ["scalar", "patch", "map"])
@pytest.mark.parametrize("shape", SHAPES)
def test_twin_forward_is_np_twin_bit_for_bit(shape, kind, accel):
    f, alpha, amap, _ = case(shape, kind)
    for K in (50, 203):
        u, tape, _ = ur.fwd_tape(f, amap, K, accel=accel)
        assert np.array_equal(u, tw.pdhg_denoise(f, alpha, maxiter=K, accel=accel))
        assert tape.shape == (K, 2) + f.shape and np.isfinite(tape).all()


@pytest.mark.parametrize("accel", [True, False])
@pytest.mark.parametrize("kind", ["scalar", "patch", "map"])
@pytest.mark.parametrize("shape", SHAPES + DEGENERATE)
def test_twin_reverse_agrees_with_torch_autograd(shape, kind, accel):
    """1e-11 * max|ref| on both gradients: the x200 margin the project gives u against its numpy twin (DESIGN.md
    section 4.5), over the 9e-16 ... 5.1e-14 absolute measured at max|ref| 1.2 ... 4.6."""
    pytest.importorskip("torch")
    f, alpha, amap, gu = case(shape, kind)
    for K in (50, 203):
        _, tape, tab = ur.fwd_tape(f, amap, K, accel=accel)
        gf, ga = ur.reverse(gu, tape, tab, amap)
        gf0, ga0 = ur.torch_reference(f, amap, K, gu, accel=accel)
        ga = ga.sum(axis=0)
        df, da = float(np.abs(gf - gf0).max()), float(np.abs(ga - ga0).max())
        mf, ma = float(np.abs(gf0).max()), float(np.abs(ga0).max())
        print("%s %s accel %d K %d: grad_f %.2e (max %.2e)  grad_alpha %.2e (max %.2e)" % (shape, kind, accel, K, df, mf, da, ma))
        assert df <= 1e-11 * mf
        assert da <= 1e-11 * ma


@pytest.mark.parametrize("K", [30, 300])
def test_twin_gradient_against_central_differences(K):
    """d/dalpha of 0.5 |u_K - ubar|^2 on 1 x 24 x 28, alpha = 0.08: the reverse sweep against the central difference
    (h = 1e-6) of np_twin.pdhg_denoise, relative 1e-5 (measured 3.3e-9 at K = 30, 1.1e-7 at K = 300)."""
    ub, f = synth_batch(1, 24, 28, seed=9)
    alpha, h = 0.08, 1e-6
    amap = tw.alpha_to_map(alpha, 28, 24)
    u, tape, tab = ur.fwd_tape(f, amap, K)
    _, ga = ur.reverse(u - ub, tape, tab, amap)
    g = ur.reduce_alpha(ga, alpha)
    fd = (tw.l2_cost(tw.pdhg_denoise(f, alpha + h, maxiter=K), ub) - tw.l2_cost(tw.pdhg_denoise(f, alpha - h, maxiter=K), ub)) / (2 * h)
    print("K %d: reverse %.10g central difference %.10g rel %.2e" % (K, g, fd, abs(g - fd) / abs(fd)))
    assert abs(g - fd) <= 1e-5 * abs(fd)
