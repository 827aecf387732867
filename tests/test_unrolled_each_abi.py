"""Per-image parameters through the PDHG iterations on a machine without a GPU: the library exports the six
bpltv_unrolled_*_each functions with the header's argument lists, the binding covers them, TVSolver has the methods and
rejects wrong block counts before any library call, tv_denoise_unrolled_each rejects wrong inputs before it touches the
library, and the per-image helper twin the GPU tests compare against (tests/unrolled_each_ref.py) is pinned: image-wise
bitwise to the one-image twins, and per image to torch's reverse and forward mode."""
import ctypes as C
import os
import re

import numpy as np
import pytest
from conftest import ROOT, synth_batch

import unrolled_each_ref as ue
import unrolled_jvp_ref as uj
import unrolled_ref as ur

NAMES = {"bpltv_unrolled_denoise_each": 6, "bpltv_unrolled_denoise_each_device": 6, "bpltv_unrolled_vjp_each": 8,
         "bpltv_unrolled_vjp_each_device": 9, "bpltv_unrolled_jvp_each": 10, "bpltv_unrolled_jvp_each_device": 10}
METHODS = ("unrolled_denoise_each", "unrolled_denoise_each_device", "unrolled_vjp_each", "unrolled_vjp_each_device",
           "unrolled_jvp_each", "unrolled_jvp_each_device")


def _header_args(name):
    txt = open(os.path.join(ROOT, "include", "bpltv.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name, txt)
    assert m, name
    return [" ".join(a.split()) for a in m.group(1).split(",")]


@pytest.mark.parametrize("name", sorted(NAMES))
def test_library_exports_and_binds_the_each_functions(name):
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
    assert names("bpltv_unrolled_denoise_each") == ["h", "alphas", "am", "an", "p", "u_out"]
    assert names("bpltv_unrolled_denoise_each_device") == ["h", "d_alphas", "am", "an", "p", "d_tape"]
    assert names("bpltv_unrolled_vjp_each") == ["h", "alphas", "am", "an", "p", "gu", "grad_f_out", "grad_alphas_out"]
    assert names("bpltv_unrolled_vjp_each_device") == ["h", "d_tape", "d_alphas", "am", "an", "p", "d_gu", "d_grad_f",
                                                        "d_grad_alphas"]
    assert names("bpltv_unrolled_jvp_each") == ["h", "alphas", "am", "an", "p", "ndir", "df", "dalphas", "du_out", "u_out"]
    assert names("bpltv_unrolled_jvp_each_device") == ["h", "d_alphas", "am", "an", "p", "ndir", "d_df", "d_dalphas", "d_du",
                                                        "d_u"]
    txt = open(os.path.join(ROOT, "include", "bpltv.h")).read()
    assert re.search(r"#define BPLTV_VERSION 4\b", txt)


class _NoLibrary:
    def __getattr__(self, name):
        raise AssertionError("the library was called (%s)" % name)


def test_solver_methods_reject_wrong_blocks_before_any_library_call():
    from bpldenoising_amd import TVSolver
    for m in METHODS:
        assert callable(getattr(TVSolver, m))
    s = TVSolver.__new__(TVSolver)      # no handle: every library entry is refused
    s.M, s.N, s.O, s._h, s._lib = 6, 8, 3, None, _NoLibrary()
    gu = np.zeros((3, 8, 6))
    for bad in (np.full(2, 0.1), np.full(4, 0.1), np.full((2, 2, 2), 0.1), np.full((4, 8, 6), 0.1)):   # wrong block counts
        with pytest.raises(ValueError, match="blocks"):
            s.unrolled_denoise_each(bad, maxiter=5)
        with pytest.raises(ValueError, match="blocks"):
            s.unrolled_vjp_each(bad, gu, maxiter=5)
        with pytest.raises(ValueError, match="blocks"):
            s.unrolled_jvp_each(bad, df=gu, maxiter=5)
    for bad in (np.full((3, 2), 0.1), np.full((3, 1, 2, 2), 0.1)):                                      # wrong shapes
        with pytest.raises(ValueError, match="alphas must have shape"):
            s.unrolled_denoise_each(bad, maxiter=5)
        with pytest.raises(ValueError, match="alphas must have shape"):
            s.unrolled_vjp_each(bad, gu, maxiter=5)
        with pytest.raises(ValueError, match="alphas must have shape"):
            s.unrolled_jvp_each(bad, df=gu, maxiter=5)
    ok = np.full(3, 0.1)
    with pytest.raises(ValueError, match="both False"):
        s.unrolled_vjp_each(ok, gu, want_f=False, want_alpha=False)
    with pytest.raises(ValueError, match="both None"):
        s.unrolled_jvp_each(ok)
    with pytest.raises(ValueError, match="dalpha has shape"):        # a tangent shaped like ONE block
        s.unrolled_jvp_each(np.full((3, 2, 2), 0.1), dalphas=np.zeros((2, 2)))
    with pytest.raises(ValueError, match="df has shape"):
        s.unrolled_jvp_each(ok, df=np.zeros((2, 8, 6)))
    s._h = None   # (nothing to destroy)


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


def test_tv_denoise_unrolled_each_rejects_before_any_library_call(layer):
    import torch
    f = torch.zeros(2, 8, 6, dtype=torch.float64)
    a = torch.full((2,), 0.1, dtype=torch.float64)
    with pytest.raises(TypeError, match="torch tensors"):
        layer.tv_denoise_unrolled_each(np.zeros((2, 8, 6)), a, maxiter=5)
    with pytest.raises(TypeError, match="float64"):
        layer.tv_denoise_unrolled_each(f.float(), a, maxiter=5)
    with pytest.raises(TypeError, match="float64"):
        layer.tv_denoise_unrolled_each(f, a.float(), maxiter=5)
    with pytest.raises(ValueError, match=r"tv_denoise_unrolled_each: f must have shape \(B, H, W\)"):
        layer.tv_denoise_unrolled_each(f[0], a, maxiter=5)
    for bad in (torch.tensor(0.1, dtype=torch.float64), torch.zeros(3, dtype=torch.float64), torch.zeros(8, 6, dtype=torch.float64),
                torch.zeros(2, 9, 6, dtype=torch.float64), torch.zeros(3, 2, 2, dtype=torch.float64),
                torch.zeros(2, 1, 2, 2, dtype=torch.float64)):
        with pytest.raises(ValueError, match="tv_denoise_unrolled_each: alpha must be"):
            layer.tv_denoise_unrolled_each(f, bad, maxiter=5)
    with pytest.raises(ValueError, match="alpha is on"):
        layer.tv_denoise_unrolled_each(f, torch.full((2,), 0.1, dtype=torch.float64, device="meta"), maxiter=5)
    for ok in (a, torch.full((2, 2, 3), 0.1, dtype=torch.float64), torch.full((2, 8, 6), 0.1, dtype=torch.float64)):
        for fm in (False, True):   # CPU tensors, everything else valid
            with pytest.raises(ValueError, match="ROCm device"):
                layer.tv_denoise_unrolled_each(f, ok, forward_mode=fm, maxiter=5)
    assert layer.TVDenoiseUnrolledEachFunction.jvp is torch.autograd.Function.jvp   # no forward mode by default
    assert layer.TVDenoiseUnrolledEachForwardFunction.jvp is not torch.autograd.Function.jvp
    assert not hasattr(layer, "TVDenoiseUnrolledEach")                               # no module class


def test_tv_denoise_unrolled_still_rejects_a_batch_of_parameters(layer):
    import torch
    f = torch.zeros(2, 8, 6, dtype=torch.float64)
    for fm in (False, True):
        with pytest.raises(ValueError, match="tv_denoise: alpha must be"):
            layer.tv_denoise_unrolled(f, torch.full((2,), 0.1, dtype=torch.float64), forward_mode=fm, maxiter=5)
        with pytest.raises(ValueError, match="tv_denoise: alpha must be"):
            layer.tv_denoise_unrolled(f, torch.full((2, 8, 6), 0.1, dtype=torch.float64), forward_mode=fm, maxiter=5)


def test_importing_the_package_does_not_import_torch():
    import subprocess
    import sys
    code = ("import sys; import bpldenoising_amd; assert 'torch' not in sys.modules; "
            "assert not hasattr(bpldenoising_amd, 'tv_denoise_unrolled_each'); "
            "assert hasattr(bpldenoising_amd.TVSolver, 'unrolled_vjp_each')")
    subprocess.check_call([sys.executable, "-c", code], cwd=ROOT)


# ---- the helper twin ------------------------------------------------------------------------------------------------
SHAPES = [(2, 17, 33), (1, 1, 9)]          # (O, N, M)


def case(shape, kind, seed=5):
    O, N, M = shape
    _, f = synth_batch(O, N, M, seed=seed)
    alphas = ue.alphas_of(kind, O, N, M)
    rng = np.random.default_rng(seed + 100)
    gu, df = rng.standard_normal(f.shape), rng.standard_normal(f.shape)
    da = rng.standard_normal(alphas.shape)
    return f, alphas, gu, df, da


@pytest.mark.parametrize("accel", [True, False])
@pytest.mark.parametrize("kind", ["scalar", "patch", "map"])
@pytest.mark.parametrize("shape", SHAPES)
def test_helper_twin_is_the_one_image_twin_per_image_bitwise(shape, kind, accel):
    O, N, M = shape
    f, alphas, gu, df, da = case(shape, kind)
    amaps, damaps = ue.stack_maps(alphas, M, N), ue.stack_maps(da, M, N)
    assert amaps.shape == f.shape
    for K in (1, 7, 50):
        u, tape, tab = ur.fwd_tape(f, amaps, K, accel=accel)
        gf, ga = ur.reverse(gu, tape, tab, amaps)
        gae = ue.reduce_alpha_each(ga, alphas)
        assert gae.shape == alphas.shape
        u2, du = uj.forward_tangent(f, amaps, K, df=df, damap=damaps, accel=accel)
        assert np.array_equal(u2, u)
        for k in range(O):
            u1, tape1, tab1 = ur.fwd_tape(f[k:k + 1], amaps[k], K, accel=accel)
            gf1, ga1 = ur.reverse(gu[k:k + 1], tape1, tab1, amaps[k])
            _, du1 = uj.forward_tangent(f[k:k + 1], amaps[k], K, df=df[k:k + 1], damap=damaps[k], accel=accel)
            assert np.array_equal(u[k], u1[0]) and np.array_equal(gf[k], gf1[0]) and np.array_equal(ga[k], ga1[0])
            assert np.array_equal(du[k], du1[0])
            assert np.array_equal(gae[k], np.asarray(ur.reduce_alpha(ga1, alphas[k])))
        if shape == (2, 17, 33) and K == 50:   # both branches of the projection, neither everywhere nor nowhere
            z = tape[-1]
            frac = float((z[0] * z[0] + z[1] * z[1] > amaps * amaps).mean())
            assert 0.05 < frac < 0.95, frac


@pytest.mark.parametrize("accel", [True, False])
@pytest.mark.parametrize("kind", ["scalar", "patch", "map"])
@pytest.mark.parametrize("shape", SHAPES)
def test_helper_twin_agrees_per_image_with_torch(shape, kind, accel):
    """1e-11 * max|ref| on grad_f, on the per-image per-pixel parameter terms and on du: the tolerances of
    tests/test_unrolled_abi.py and tests/test_unrolled_jvp_abi.py for the shared twins (a reference of 0 -- the 1 x 1 x 9
    image at K = 1 -- demands 0)."""
    pytest.importorskip("torch")
    O, N, M = shape
    f, alphas, gu, df, da = case(shape, kind)
    amaps, damaps = ue.stack_maps(alphas, M, N), ue.stack_maps(da, M, N)
    for K in (1, 7, 50):
        _, tape, tab = ur.fwd_tape(f, amaps, K, accel=accel)
        gf, ga = ur.reverse(gu, tape, tab, amaps)
        gf0, ga0 = ur.torch_reference(f, amaps, K, gu, accel=accel)      # a stacked map: at.grad is per image
        ga0 = np.broadcast_to(ga0, ga.shape)
        for k in range(O):
            assert float(np.abs(gf[k] - gf0[k]).max()) <= 1e-11 * float(np.abs(gf0[k]).max())
            assert float(np.abs(ga[k] - ga0[k]).max()) <= 1e-11 * float(np.abs(ga0[k]).max())
        for tdf, tda in ((df, None), (None, damaps), (df, damaps)):
            _, du = uj.forward_tangent(f, amaps, K, df=tdf, damap=tda, accel=accel)
            _, du0 = uj.torch_forward_reference(f, amaps, K, df=tdf, damap=tda, accel=accel)
            for k in range(O):
                assert float(np.abs(du[k] - du0[k]).max()) <= 1e-11 * float(np.abs(du0[k]).max())
