"""Forward mode on a machine without a GPU: the library exports bpltv_jvp, its _device / _each / _each_device forms and
bpltv_gauss_newton with the header's argument lists, the binding covers the header, the torch layer's forward mode
rejects wrong inputs before it touches the library, and the numpy reference the GPU tests compare against
(tests/jvp_ref.py) is pinned to the oracle's own vector-Jacobian product by the transpose identity."""
import ctypes as C
import os
import re

import numpy as np
import pytest
from conftest import ROOT, synth_batch

import jvp_ref

JVP = ["bpltv_jvp", "bpltv_jvp_device", "bpltv_jvp_each", "bpltv_jvp_each_device"]


def _header_args(name):
    txt = open(os.path.join(ROOT, "include", "bpltv.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name, txt)
    assert m, name
    return [a.strip() for a in m.group(1).split(",")]


def _ctype_of(decl):
    from bpldenoising_amd import _lib
    d = " ".join(decl.split())
    if d.startswith("bpltv_t *"):
        return C.c_void_p
    if d.startswith("const bpltv_params *"):
        return _lib._PP
    if d.startswith("int "):
        return C.c_int
    assert "double *" in d, decl
    return "double*"


@pytest.mark.parametrize("name", JVP + ["bpltv_gauss_newton"])
def test_library_exports_and_binds_forward_mode(name):
    from bpldenoising_amd import _lib
    lib = _lib.load()
    assert hasattr(lib, name)
    res, args = _lib.SYMBOLS[name]
    assert res is C.c_int
    hdr = _header_args(name)
    assert len(args) == len(hdr) == (10 if name == "bpltv_gauss_newton" else 11)
    assert getattr(lib, name).argtypes == args
    for a, decl in zip(args, hdr):
        want = _ctype_of(decl)
        if want == "double*":   # host arrays: POINTER(c_double); device arrays: raw addresses
            assert a is (C.c_void_p if name.endswith("_device") else C.POINTER(C.c_double)), (decl, a)
        else:
            assert a is want, (decl, a)


def test_jvp_signatures_follow_the_vjp():
    """(handle, u, alpha, am, an, reg, params) as bpltv_vjp, then ndir and the three arrays."""
    from bpldenoising_amd import _lib
    for name in JVP:
        args = _lib.SYMBOLS[name][1]
        assert args[:7] == _lib.SYMBOLS["bpltv_vjp_device" if name.endswith("_device") else "bpltv_vjp"][1][:7]
        assert args[7] is C.c_int
    dev = _lib.SYMBOLS["bpltv_jvp_device"][1]
    assert [i for i, a in enumerate(dev) if a is C.c_void_p] == [0, 1, 2, 8, 9, 10]


def test_binding_covers_the_header_and_the_version_stays():
    from bpldenoising_amd import _lib
    txt = open(os.path.join(ROOT, "include", "bpltv.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    assert sorted(_lib.SYMBOLS) == sorted(set(re.findall(r"\b(bpltv_[a-z_]+)\s*\(", txt)))
    assert _lib.load().bpltv_version() == 4
    assert re.search(r"#define BPLTV_VERSION 4\b", txt)


def test_solver_has_the_forward_mode_methods():
    from bpldenoising_amd import TVSolver
    for m in ("jvp", "jvp_device", "jvp_each", "jvp_each_device", "gauss_newton"):
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


def test_torch_layer_has_a_jvp_for_the_tv_functions_only(layer):
    import torch
    base = torch.autograd.Function.jvp
    assert layer.TVDenoiseFunction.jvp is not base and layer.TVDenoiseEachFunction.jvp is not base
    assert layer.SumRegsDenoiseFunction.jvp is base and layer.SumRegsDenoiseEachFunction.jvp is base
    assert "no forward mode" in layer.__doc__


def test_torch_layer_forward_mode_rejects_wrong_inputs(layer):
    """Dual inputs go through the same checks as plain ones, before any library call."""
    import torch
    import torch.autograd.forward_ad as fwAD
    f = torch.zeros(2, 8, 6, dtype=torch.float64)
    a = torch.tensor(0.1, dtype=torch.float64)
    with fwAD.dual_level():
        with pytest.raises(ValueError, match="ROCm device"):
            layer.tv_denoise(fwAD.make_dual(f, torch.ones_like(f)), a)
        with pytest.raises(ValueError, match="ROCm device"):
            layer.tv_denoise(f, fwAD.make_dual(a, torch.ones_like(a)))
        with pytest.raises(TypeError, match="float64"):
            layer.tv_denoise(fwAD.make_dual(f.float(), torch.ones_like(f).float()), a)
        with pytest.raises(ValueError, match="alpha must be"):
            a3 = torch.zeros(3, dtype=torch.float64)
            layer.tv_denoise(f, fwAD.make_dual(a3, torch.ones_like(a3)))
        with pytest.raises(ValueError, match="alpha must be"):
            layer.tv_denoise_each(fwAD.make_dual(f, torch.ones_like(f)), a)
        ae = torch.full((2,), 0.1, dtype=torch.float64)
        with pytest.raises(ValueError, match="ROCm device"):
            layer.tv_denoise_each(f, fwAD.make_dual(ae, torch.ones_like(ae)))


def test_torch_layer_tangent_checks(layer):
    """The tangents jvp hands to the library: float64, the primal's size and device; None stays None."""
    import torch
    u = torch.zeros(2, 8, 6, dtype=torch.float64)
    assert layer._tangent(None, u, "f") is None
    t = layer._tangent(torch.ones(2, 8, 6, dtype=torch.float64).transpose(1, 2).transpose(1, 2), u, "f")
    assert t.is_contiguous() and t.shape == u.shape
    with pytest.raises(TypeError, match="float64"):
        layer._tangent(torch.ones(2, 8, 6), u, "f")
    with pytest.raises(ValueError, match="tangent of alpha"):
        layer._tangent(torch.ones(3, dtype=torch.float64), torch.zeros((), dtype=torch.float64), "alpha")
    with pytest.raises(ValueError, match="tangent of f"):
        layer._tangent(torch.ones(2, 8, 6, dtype=torch.float64, device="meta"), u, "f")


KINDS = ["scalar", "patch22", "map"]


def _alpha(kind, N, M):
    if kind == "scalar":
        return 0.08
    if kind == "patch22":
        return np.array([[0.08, 0.12], [0.1, 0.05]])
    return 0.05 + 0.1 * np.random.default_rng(8).random((N, M))


@pytest.mark.parametrize("reg", [0, 1])
@pytest.mark.parametrize("kind", KINDS)
def test_reference_jvp_is_the_transpose_of_the_oracle_vjp(oracle, kind, reg):
    """<gu, jvp(df, dalpha)> == <vjp_f(gu), df> + <vjp_alpha(gu), dalpha> on the oracle alone, 20 x 16 image.

    Both sides apply the SAME Cholesky factor of the oracle to two right-hand sides, so they differ by the rounding
    of the substitutions and of the 5-point operators around them, not by the conditioning of the system: of the
    order n * eps = 320 * 2.2e-16 = 7e-14 of the terms' magnitude at worst.  Bound: 1e-12 of |<gf,df>| + |<ga,dalpha>|."""
    N, M = 16, 20
    ub, f = synth_batch(1, N, M, seed=61)
    alpha = _alpha(kind, N, M)
    u = oracle.pdhg(f, alpha, maxiter=400)[0]
    g1, g2 = oracle.grad_fwd(u)
    ng = np.sqrt(g1 * g1 + g2 * g2)
    assert 0 < np.count_nonzero(ng < (1e-8 if reg else 1e-12)) < N * M    # both branches of the h plane are exercised
    rng = np.random.default_rng(62)
    gu, df = rng.standard_normal((N, M)), rng.standard_normal((N, M))
    dalpha = float(rng.standard_normal()) if kind == "scalar" else rng.standard_normal(np.shape(alpha))
    du = jvp_ref.jvp_image(oracle, u, alpha, df, dalpha, reg)
    gf, ga = jvp_ref.vjp_image(oracle, u, alpha, gu, reg)
    lhs = float(np.sum(gu * du))
    t1, t2 = float(np.sum(gf * df)), float(np.sum(np.asarray(ga) * np.asarray(dalpha)))
    print("kind %s reg %d: lhs %.17g rhs %.17g rel %.3e" % (kind, reg, lhs, t1 + t2, abs(lhs - (t1 + t2)) / (abs(t1) + abs(t2))))
    assert abs(lhs - (t1 + t2)) <= 1e-12 * (abs(t1) + abs(t2))
    # each tangent alone, and linearity of the reference in its two arguments
    du_f = jvp_ref.jvp_image(oracle, u, alpha, df, None, reg)
    du_a = jvp_ref.jvp_image(oracle, u, alpha, None, dalpha, reg)
    assert np.linalg.norm(du - (du_f + du_a)) <= 1e-10 * np.linalg.norm(du)
