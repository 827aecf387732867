"""The per-pixel fidelity weight on a machine without a GPU: the library exports the four bpltv_weighted_* functions with
the header's argument lists, the binding covers them, TVSolver has the methods, tv_denoise_weighted rejects wrong inputs
before it touches the library, and the numpy reference the GPU tests compare against (tests/weighted_ref.py) is pinned:
its PDHG loop to oracle.np_twin's with w = 1, its scaled adjoint system to the literal one."""
import ctypes as C
import os
import re

import numpy as np
import pytest
from conftest import ROOT, synth_batch

import weighted_ref as wr
from oracle import np_twin as tw

NAMES = {"bpltv_weighted_denoise": 8, "bpltv_weighted_denoise_device": 7, "bpltv_weighted_vjp": 13,
         "bpltv_weighted_vjp_device": 13}


def _header_args(name):
    txt = open(os.path.join(ROOT, "include", "bpltv.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name, txt)
    assert m, name
    return [" ".join(a.split()) for a in m.group(1).split(",")]


@pytest.mark.parametrize("name", sorted(NAMES))
def test_library_exports_and_binds_the_weighted_functions(name):
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
    assert [d.split()[-1].lstrip("*") for d in _header_args("bpltv_weighted_denoise")] == \
        ["h", "w", "wo", "alpha", "am", "an", "p", "u_out"]
    assert [d.split()[-1].lstrip("*") for d in _header_args("bpltv_weighted_vjp")] == \
        ["h", "u", "f", "w", "wo", "alpha", "am", "an", "p", "gu", "grad_f_out", "grad_alpha_out", "grad_w_out"]
    txt = open(os.path.join(ROOT, "include", "bpltv.h")).read()
    assert re.search(r"#define BPLTV_VERSION 4\b", txt)


def test_solver_has_the_weighted_methods():
    from bpldenoising_amd import TVSolver
    for m in ("weighted_denoise", "weighted_denoise_device", "weighted_vjp", "weighted_vjp_device"):
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


def test_tv_denoise_weighted_rejects_before_any_library_call(layer):
    import torch
    f = torch.zeros(2, 8, 6, dtype=torch.float64)
    a = torch.tensor(0.1, dtype=torch.float64)
    w = torch.ones(8, 6, dtype=torch.float64)
    with pytest.raises(TypeError, match="w must be float64"):
        layer.tv_denoise_weighted(f, a, w.float())
    with pytest.raises(TypeError, match="torch tensor"):
        layer.tv_denoise_weighted(f, a, np.ones((8, 6)))
    for bad in (torch.ones(6, 8, dtype=torch.float64), torch.ones(3, 8, 6, dtype=torch.float64),
                torch.ones(48, dtype=torch.float64), torch.ones((), dtype=torch.float64)):
        with pytest.raises(ValueError, match="w must have shape"):
            layer.tv_denoise_weighted(f, a, bad)
    with pytest.raises(ValueError, match="w must have shape"):    # a batched weight needs a batched f
        layer.tv_denoise_weighted(f[0], a, torch.ones(2, 8, 6, dtype=torch.float64))
    with pytest.raises(ValueError, match="w is on"):
        layer.tv_denoise_weighted(f, a, torch.ones(8, 6, dtype=torch.float64, device="meta"))
    with pytest.raises(ValueError, match="ROCm device"):           # CPU tensors, everything else valid
        layer.tv_denoise_weighted(f, a, w)
    with pytest.raises(ValueError, match="ROCm device"):
        layer.tv_denoise_weighted(f, a, torch.ones(2, 8, 6, dtype=torch.float64))
    with pytest.raises(TypeError, match="float64"):                # f and alpha keep tv_denoise's checks
        layer.tv_denoise_weighted(f.float(), a, w)
    with pytest.raises(ValueError, match="alpha must be"):
        layer.tv_denoise_weighted(f, torch.zeros(3, dtype=torch.float64), w)
    assert layer.TVDenoiseWeightedFunction.jvp is torch.autograd.Function.jvp   # no forward mode


def test_twin_with_unit_weight_is_the_unweighted_twin():
    """w = 1: the weighted numpy loop against oracle.np_twin.pdhg_denoise, 16 x 20, 203 iterations, to 1e-13 -- the
    level tests/test_unpinned.py holds numpy restatements to."""
    _, f = synth_batch(2, 16, 20, seed=3)
    for alpha in (0.1, np.array([[0.05, 0.1], [0.2, 0.08]])):
        u0 = tw.pdhg_denoise(f, alpha, maxiter=203)
        for w in (np.ones((16, 20)), np.ones((2, 16, 20))):
            u1 = wr.pdhg(f, alpha, w, 203)
            d = float(np.abs(u1 - u0).max())
            print("alpha %s w %s: max|du| = %.3e" % (np.shape(alpha), w.shape, d))
            assert d <= 1e-13


@pytest.mark.parametrize("shape", [(2, 70, 72), (2, 17, 33), (3, 40, 48), (1, 1, 9), (1, 9, 1)], ids=lambda s: "x".join(map(str, s)))
def test_twin_with_a_real_weight_is_its_extended_precision_restatement(shape):
    """The GPU tests hold the library to 1e-13 of this twin (tests/test_gpu_weighted_shapes.py); the twin's own rounding has
    to sit well inside that: float64 against numpy's 80-bit longdouble, 203 iterations, at those tests' shapes, with a random
    weight, six decades of weight and a mask, scalar and map parameter.  Measured: 9e-16 at most; the bound keeps a decade
    between the twin's error and what the library is allowed."""
    if np.finfo(np.longdouble).nmant < 63:
        pytest.skip("numpy's longdouble is no wider than float64 on this platform")
    O, N, M = shape
    _, f = synth_batch(O, N, M, seed=40 + M)
    rng = np.random.default_rng(77)
    rand = 0.25 + 3.75 * rng.random((O, N, M))
    mask = rand.copy()
    mask.reshape(O, -1)[:, -3:] = 0.0
    mask[:, N // 3:N // 3 + 6, M // 3:M // 3 + 6] = 0.0
    for alpha in (0.1, 0.05 + 0.1 * np.random.default_rng(8).random((N, M))):
        for name, w in (("rand", rand), ("log", 10.0 ** rng.uniform(-3.0, 3.0, (O, N, M))), ("mask", mask)):
            d = float(np.abs(wr.pdhg(f, alpha, w, 203) - wr.pdhg(f, alpha, w, 203, dtype=np.longdouble)).max())
            print("%s alpha %s %s: max|du| = %.3e" % (shape, np.shape(alpha), name, d))
            assert d <= 1e-14


def test_twin_gap_with_unit_weight_is_the_rof_gap():
    _, f = synth_batch(2, 16, 20, seed=4)
    u, y1, y2 = wr.pdhg(f, 0.1, np.ones((16, 20)), 150, return_dual=True)
    g0 = tw.rof_gap(u, y1, y2, f, 0.1)
    g1 = wr.gap(u, y1, y2, f, 0.1, np.ones((16, 20)))
    assert np.all(g1 >= 0) and np.allclose(g0, g1, rtol=0, atol=1e-12 * float(wr.primal_energy(u, f, 0.1, 1.0).max()))


KINDS = {"scalar": 0.08, "patch22": np.array([[0.08, 0.12], [0.1, 0.05]]),
         "map": 0.05 + 0.1 * np.random.default_rng(8).random((16, 20))}


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_scaled_system_is_the_literal_system(kind):
    """p = S q from (I + S K S) q = S gu equals the direct solve of (diag(w) + K) p = gu to 1e-12 relative, with the
    kappa the library starts from and an active set for it to act on.  (Measured: 2e-15 ... 1e-14.  The image is
    weighted_ref.vjp_case's: on a converged u both systems carry entries alpha / |G u| up to 1e11 and two LU solves of
    either one already differ by 1e-7; that would measure the LU, not the identity.)"""
    alpha = KINDS[kind]
    f, w, u, gu = wr.vjp_case(alpha, seed=11, O=1, iters=30)
    g1, g2 = tw.grad_fwd(u[0])
    assert 0 < np.count_nonzero(np.sqrt(g1 * g1 + g2 * g2) < 1e-12) < u[0].size
    kap = wr.kappa_default(alpha)
    for refine in (0, 10):
        p0 = wr.vjp_image(u[0], f[0], alpha, w[0], gu[0], kap, refine=refine)[3]
        p1 = wr.vjp_image_scaled(u[0], alpha, w[0], gu[0], kap, refine=refine)
        rel = float(np.linalg.norm(p1 - p0) / np.linalg.norm(p0))
        print("%s refine %d: |S q - p| / |p| = %.3e" % (kind, refine, rel))
        assert rel <= 1e-12


def _vjp_pin_cases():
    """(2, 16, 20) with KINDS, as tests/test_gpu_weighted.py uses it, and tests/test_gpu_weighted_shapes.py's four shapes
    with that file's own parameters (scalar 0.1, the 2 x 2 patch, a map of the image's size).  The first three keep the
    ids they had before the shapes were added."""
    from test_gpu_weighted import _alpha
    cases = [pytest.param((2, 16, 20), KINDS[k], id=k) for k in sorted(KINDS)]
    for O, N, M in wr.VJP_SHAPES:
        cases += [pytest.param((O, N, M), _alpha(k, N, M), id="%dx%dx%d-%s" % (O, N, M, k)) for k in ("map", "patch", "scalar")]
    return cases


@pytest.mark.parametrize("shape,alpha", _vjp_pin_cases())
def test_reference_vjp_is_stable_under_refinement(shape, alpha):
    """The tolerances the GPU tests hold the library to (rtol 1e-6, atol 1e-8 max|p|, tests/test_gpu_vjp.py) must be wider
    than the reference's own error: its plain sparse LU (refine 0) against ten extended-precision sweeps on the GPU
    tests' own cases, seed 21, one weight plane per image.  Measured: 4e-12 absolute at most on (2, 16, 20); 4.2e-11 on
    (2, 40, 48), (3, 33, 17), (2, 70, 72) and (1, 12, 140), where max|p| is 1.7 ... 5.8."""
    O, N, M = shape
    f, w, u, gu = wr.vjp_case(alpha, seed=21, O=O, N=N, M=M)
    kap = wr.kappa_default(alpha)
    r0 = wr.vjp(u, f, alpha, w, gu, kap, refine=0)
    r1 = wr.vjp(u, f, alpha, w, gu, kap, refine=10)
    pmax = float(np.abs(r1[3]).max())
    for name, a, b in zip(("grad_f", "grad_alpha", "grad_w"), r0, r1):
        a, b = np.asarray(a), np.asarray(b)
        print("%s %s: max|d| = %.3e (max|ref| %.3e, max|p| %.3e)" % (shape, name, float(np.abs(a - b).max()),
                                                                   float(np.abs(b).max()), pmax))
        assert np.allclose(a, b, rtol=1e-6, atol=1e-8 * pmax)
        assert np.allclose(a, b, rtol=1e-9, atol=1e-10 * pmax)    # ... with two digits to spare


def test_reference_vjp_with_unit_weight_is_the_oracle_adjoint(oracle):
    """w = 1: the weighted reference against the C oracle's adjoint state and gradient (its own reduced system)."""
    alpha = KINDS["patch22"]
    f, _, u, gu = wr.vjp_case(alpha, seed=31)
    ones = np.ones(u.shape)
    gf, ga, gw, p = wr.vjp(u, f, alpha, ones, gu, wr.kappa_default(alpha), refine=10)
    amap = oracle.patch_upsample(alpha, 20, 16)
    for k in range(2):
        _, p0, _ = oracle.gradient_image(u[k], u[k] - gu[k], amap, patch=True, reg=False)
        assert np.allclose(gf[k], p0, rtol=1e-6, atol=1e-8 * np.abs(p0).max())
    g0 = oracle.gradient(alpha, u, u - gu, reg=False)
    assert np.allclose(ga, g0, rtol=1e-6, atol=1e-8 * np.abs(g0).max())
    assert np.array_equal(gw, -(u - f) * p)
