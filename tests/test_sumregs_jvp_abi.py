"""Forward mode of the sum-of-regularisers model on a machine without a GPU: the library exports bpltv_sumregs_jvp, its
_device / _each / _each_device forms and bpltv_sumregs_gauss_newton with the header's argument lists, the Python and
Julia bindings carry them, the torch layer's forward mode rejects wrong inputs before it touches the library, and the
numpy / scipy reference the GPU tests compare against (tests/sumregs_jvp_ref.py) is pinned to the oracle's own
gradients by the transpose identity."""
import ctypes as C
import os
import re

import numpy as np
import pytest
from conftest import ROOT, synth_batch

import sumregs_jvp_ref as ref

JVP = ["bpltv_sumregs_jvp", "bpltv_sumregs_jvp_device", "bpltv_sumregs_jvp_each", "bpltv_sumregs_jvp_each_device"]
GN = "bpltv_sumregs_gauss_newton"


def _header_args(name):
    txt = open(os.path.join(ROOT, "include", "bpltv.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name, txt)
    assert m, name
    return [" ".join(a.split()) for a in m.group(1).split(",")]


@pytest.mark.parametrize("name", JVP + [GN])
def test_library_exports_and_binds_the_sumregs_forward_mode(name):
    """Declared in bpltv.h, exported by the library, bound in _lib.py with the argument list of the TV twin."""
    from bpldenoising_amd import _lib
    lib = _lib.load()
    assert hasattr(lib, name)
    res, args = _lib.SYMBOLS[name]
    twin = name.replace("sumregs_", "")
    assert res is C.c_int and args == _lib.SYMBOLS[twin][1]
    assert getattr(lib, name).argtypes == args
    hdr = _header_args(name)
    assert len(hdr) == len(args) == (10 if name == GN else 11)
    strip = lambda decls: [re.sub(r"\w+$", "", d) for d in decls]   # the types, without the argument names
    assert strip(hdr) == strip(_header_args(twin))


def test_solver_and_julia_glue_carry_the_five_entry_points():
    from bpldenoising_amd import TVSolver
    for m in ("sumregs_jvp", "sumregs_jvp_device", "sumregs_jvp_each", "sumregs_jvp_each_device", "sumregs_gauss_newton"):
        assert callable(getattr(TVSolver, m))
    jl = open(os.path.join(ROOT, "integration", "TVLearningFunctionHIP.jl")).read()
    exports = re.search(r"^export ([^#]*?)\n\n", jl, flags=re.S | re.M).group(1)
    names = [n.strip() for n in exports.replace("\n", " ").split(",")]
    assert "sumregs_jvp" in names and "sumregs_gauss_newton" in names
    for fn, sym in (("sumregs_jvp", "bpltv_sumregs_jvp"), ("sumregs_gauss_newton", GN)):
        assert re.search(r"^function %s\(" % fn, jl, flags=re.M) and (":%s, libbpltv" % sym) in jl


def test_solver_tangents_take_three_slices():
    """TVSolver._tangents on the (3,) / (3, n, m) / (O, 3, ...) parameter shapes: stacks of K directions, no library."""
    from bpldenoising_amd import TVSolver
    s = TVSolver.__new__(TVSolver)
    s.O, s.N, s.M = 2, 6, 5
    df = np.zeros((2, 6, 5))
    for shape in ((3,), (3, 2, 2), (3, 6, 5), (2, 3), (2, 3, 2, 2)):
        f1, a1, K, batched = s._tangents("t", df, np.ones(shape), shape)
        assert f1.shape == (1, 2, 6, 5) and a1.shape == (1,) + shape and K == 1 and not batched
        f4, a4, K, batched = s._tangents("t", None, np.ones((4,) + shape), shape)
        assert f4 is None and a4.shape == (4,) + shape and K == 4 and batched
    with pytest.raises(ValueError):
        s._tangents("t", df, np.ones((3, 2)), (3, 2, 2))
    with pytest.raises(ValueError):
        s._tangents("t", None, None, (3,))


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


def test_torch_layer_has_forward_mode_functions_for_the_sumregs_layers(layer):
    """The plain functions stay without a jvp (tests/test_jvp_abi.py); forward_mode=True selects subclasses that carry
    one and share forward and backward with them."""
    import torch
    base = torch.autograd.Function.jvp
    for fn, parent in ((layer.SumRegsDenoiseForwardFunction, layer.SumRegsDenoiseFunction),
                       (layer.SumRegsDenoiseEachForwardFunction, layer.SumRegsDenoiseEachFunction)):
        assert issubclass(fn, parent) and fn.jvp is not base and parent.jvp is base
    assert "forward_mode=True" in layer.__doc__ and "bpltv_sumregs_jvp_device" in layer.__doc__
    assert layer.SumRegsDenoise([0.1, 0.1, 0.1]).forward_mode is False
    assert layer.SumRegsDenoise([0.1, 0.1, 0.1], forward_mode=True).forward_mode is True


def test_torch_layer_sumregs_forward_mode_rejects_wrong_inputs(layer):
    """Dual inputs go through the same checks as plain ones, before any library call."""
    import torch
    import torch.autograd.forward_ad as fwAD
    f = torch.zeros(2, 8, 6, dtype=torch.float64)
    a = torch.full((3,), 0.1, dtype=torch.float64)
    with fwAD.dual_level():
        with pytest.raises(ValueError, match="ROCm device"):
            layer.sumregs_denoise(fwAD.make_dual(f, torch.ones_like(f)), a, forward_mode=True)
        with pytest.raises(ValueError, match="ROCm device"):
            layer.sumregs_denoise(f, fwAD.make_dual(a, torch.ones_like(a)), forward_mode=True)
        with pytest.raises(TypeError, match="float64"):
            layer.sumregs_denoise(fwAD.make_dual(f.float(), torch.ones_like(f).float()), a, forward_mode=True)
        with pytest.raises(ValueError, match="alpha must be"):
            a2 = torch.zeros(2, dtype=torch.float64)
            layer.sumregs_denoise(f, fwAD.make_dual(a2, torch.ones_like(a2)), forward_mode=True)
        ae = torch.full((2, 3), 0.1, dtype=torch.float64)
        with pytest.raises(ValueError, match="ROCm device"):
            layer.sumregs_denoise_each(f, fwAD.make_dual(ae, torch.ones_like(ae)), forward_mode=True)


def test_torch_layer_sumregs_jvp_checks_tangents_before_the_library(layer):
    """jvp itself, on a stand-in context: a float32 tangent is a TypeError and two missing tangents give zeros, both
    without a library call (the solver of the context refuses every call)."""
    import torch

    class Ctx:
        saved_tensors = (torch.zeros(2, 8, 6, dtype=torch.float64), torch.full((3,), 0.1, dtype=torch.float64))
        am = an = 1
        reg = False
        solver_kw = {}

        class solver:
            def __getattr__(self, name):
                raise AssertionError("the library was called")
        solver = solver()
    for fn in (layer.SumRegsDenoiseForwardFunction, layer.SumRegsDenoiseEachForwardFunction):
        with pytest.raises(TypeError, match="float64"):
            fn.jvp(Ctx, torch.ones(2, 8, 6), None, None, None)
        with pytest.raises(TypeError, match="float64"):
            fn.jvp(Ctx, None, torch.ones(3), None, None)
        z = fn.jvp(Ctx, None, None, None, None)
        assert z.shape == (2, 8, 6) and z.dtype == torch.float64 and not z.any()


# ---- the reference of the GPU tests, pinned on the CPU -----------------------------------------------------------------
SHAPE = (3, 48, 40)
A3 = np.array([0.03, 0.02, 0.05])
P22 = np.stack([np.array([[0.03, 0.05], [0.02, 0.04]]), np.array([[0.02, 0.03], [0.05, 0.02]]),
                np.array([[0.04, 0.02], [0.03, 0.06]])])
KINDS = ["vector", "patch22", "patch35", "map"]
# Measured on the CPU with the oracle alone (this very test, seeds as below), relative to the magnitude of the pairing:
#   <g, dx> against <u - ubar, jvp(dx)>:   vector 2.6e-10 / 9.6e-15 (reg 0 / 1), patch22 2.5e-10 / 1.1e-10,
#                                         patch35 2.9e-10 / 1.8e-10, map 6.2e-9 / 7.8e-9
#   <p, df> against <gu, jvp(df)>:         vector 3.1e-9 / 4.3e-15, patch22 7.2e-9 / 3.5e-10, patch35 2.1e-9 / 4.7e-9,
#                                         map 9.1e-9 / 1.5e-9
# The two sides solve the same system by different routes (the C oracle's banded factor with three refinement sweeps, the
# literal saddle system with kappa = 1/eps, scipy's LU of the reduced one), so they differ by the conditioning of the
# kappa = 1e14 rows, not by rounding alone.  Bound: about ten times the worst case.
IDENTITY_TOL = 1e-7


def _alpha(kind, N, M):
    if kind == "vector":
        return A3
    if kind == "patch22":
        return P22
    if kind == "patch35":
        return 0.02 + 0.04 * np.random.default_rng(31).random((3, 5, 3))
    return 0.02 + 0.04 * np.random.default_rng(32).random((3, N, M))


@pytest.mark.parametrize("reg", [0, 1])
@pytest.mark.parametrize("kind", KINDS)
def test_reference_jvp_is_the_transpose_of_the_oracle_gradients(oracle, kind, reg):
    """(3, 48, 40): <g(ubar), dx> == <u - ubar, jvp_ref(dx)> summed over the images with g = oracle.sumregs_gradient,
    and <p, df> == <gu, jvp_ref(df)> image by image with p the adjoint state of the literal systems
    (np_twin_sumregs.gradient_image; -p of gradient_reg_image).  Worst cases and the bound: IDENTITY_TOL above.  The
    reg = 1 array cases hold only with the TRANSPOSED row-scaled system: with A in place of A^T they miss by 1e-2."""
    from oracle import np_twin_sumregs as TS
    O, N, M = SHAPE
    ub, f = synth_batch(O, N, M, seed=60 + M + O)
    x = _alpha(kind, N, M)
    u = oracle.sumregs_pdhg(f, x, maxiter=300, nthreads=4)
    rng = np.random.default_rng(5)
    dx, df, gu = rng.standard_normal(x.shape), rng.standard_normal(u.shape), rng.standard_normal(u.shape)
    g = oracle.sumregs_gradient(x, u, ub, reg=bool(reg))
    lhs = float(np.sum(g * dx))
    rhs = sum(float(np.sum((u[k] - ub[k]) * ref.jvp_image(u[k], x, None, dx, reg))) for k in range(O))
    e1 = abs(lhs - rhs) / abs(lhs)
    print("%s reg %d: <g, dx> %.15g, <u - ubar, jvp> %.15g, rel %.3e" % (kind, reg, lhs, rhs, e1))
    assert e1 <= IDENTITY_TOL
    for k in range(O):
        p = -TS.gradient_reg_image(x, u[k], u[k] - gu[k])[1] if reg else TS.gradient_image(x, u[k], u[k] - gu[k])[1]
        l2 = float(np.sum(p.reshape(N, M) * df[k]))
        r2 = float(np.sum(gu[k] * ref.jvp_image(u[k], x, df[k], None, reg)))
        print("   image %d: <p, df> %.15g, <gu, jvp> %.15g, rel %.3e" % (k, l2, r2, abs(l2 - r2) / abs(l2)))
        assert abs(l2 - r2) <= IDENTITY_TOL * abs(l2)
    if reg and kind != "vector":   # the untransposed solve is a different map: the identity tells them apart
        wrong = sum(float(np.sum((u[k] - ub[k]) * ref.jvp_image(u[k], x, None, dx, reg, transposed=False)))
                    for k in range(O))
        assert abs(lhs - wrong) > 1e4 * IDENTITY_TOL * abs(lhs)


def test_reference_is_linear_and_plain_on_one_pixel(oracle):
    O, N, M = SHAPE
    _, f = synth_batch(1, N, M, seed=7)
    u = oracle.sumregs_pdhg(f, P22, maxiter=100)[0]
    rng = np.random.default_rng(8)
    df, dx = rng.standard_normal((N, M)), rng.standard_normal(P22.shape)
    for reg in (0, 1):
        both = ref.jvp_image(u, P22, df, dx, reg)
        parts = ref.jvp_image(u, P22, df, None, reg) + ref.jvp_image(u, P22, None, dx, reg)
        assert np.linalg.norm(both - parts) <= 1e-10 * np.linalg.norm(both)
        one = ref.jvp_image(np.array([[0.4]]), A3, np.array([[1.5]]), np.ones(3), reg)
        assert one.shape == (1, 1) and one[0, 0] == 1.5   # no differences on one pixel: du == df


def test_rational_reference_agrees_with_scipy_where_double_precision_suffices(oracle):
    """jvp_image_exact against jvp_image on 3 x 5 images (cond(A) <= 3e7, so scipy is good to cond eps = 7e-9; measured
    1.1e-10 / 6.7e-11), both values of reg and the row-scaled system; on the 1 x 9 image of the edge cases, where
    cond(A) = 6e14, scipy's LU is 8e-3 away from the exact solution, and jvp_image_small picks the rational solve."""
    from test_oracle_sumregs import EDGE_MAXITER, edge_case
    for shape, kind, reg in (((2, 3, 5), "vector", 0), ((2, 3, 5), "patch", 1), ((2, 3, 5), "vector", 1)):
        _, f, x = edge_case(shape, kind)
        u = oracle.sumregs_pdhg(f, x, maxiter=EDGE_MAXITER)[0]
        rng = np.random.default_rng(3)
        df, dx = rng.standard_normal(u.shape), rng.standard_normal(np.shape(x))
        assert np.linalg.cond(ref.matrix(u, x, reg).toarray()) < 1e8
        ex, sp = ref.jvp_image_exact(u, x, df, dx, reg), ref.jvp_image(u, x, df, dx, reg)
        assert np.abs(ex - sp).max() <= 1e-8 * np.abs(ex).max()
        assert np.array_equal(ref.jvp_image_small(u, x, df, dx, reg), sp)
    _, f, x = edge_case((2, 1, 9), "map")
    u = oracle.sumregs_pdhg(f, x, maxiter=EDGE_MAXITER)[0]
    rng = np.random.default_rng(4)
    df, dx = rng.standard_normal(u.shape), rng.standard_normal(np.shape(x))
    assert np.linalg.cond(ref.matrix(u, x, 0).toarray()) > 1e13
    ex = ref.jvp_image_exact(u, x, df, dx, 0)
    assert np.array_equal(ref.jvp_image_small(u, x, df, dx, 0), ex)
    # the exact solution satisfies the transpose identity with the exact solve of the untransposed system
    gu = rng.standard_normal(u.shape)
    p = ref.jvp_image_exact(u, x, gu, None, 0, transposed=False)
    assert abs(np.sum(gu * ex) - np.sum(p * ref.rhs(u, x, df, dx, 0))) <= 1e-12 * abs(np.sum(gu * ex))
