"""GPU checks of forward-mode AD through the sum-of-regularisers PyTorch layer: with forward_mode=True the tangent of
sumregs_denoise, sumregs_denoise_each and SumRegsDenoise under torch.autograd.forward_ad is bitwise TVSolver.sumregs_jvp
(without the option forward-mode AD raises, as tests/test_gpu_torch_layer_jvp.py pins it; the host form
of the same entry) on the u of the forward pass, it is the transpose of what loss.backward() computes -- also for
reg = 1 with an array parameter, whose row-scaled system is solved transposed --, and reverse mode is what it was."""
import numpy as np
import pytest
from conftest import synth_batch

from test_gpu_sumregs_torch_layer import A3, P22, torch_cuda  # noqa: F401

pytestmark = pytest.mark.gpu

O, N, M = 2, 24, 20
KINDS = ["vector", "patch22", "map"]
MAXITER = 200


def _alpha(kind):
    if kind == "vector":
        return A3
    if kind == "patch22":
        return P22
    return 0.02 + 0.04 * np.random.default_rng(9).random((3, N, M))


def _inputs(torch, kind, each, seed=90):
    _, f = synth_batch(O, N, M, seed=seed)
    a = np.asarray(_alpha(kind), dtype=np.float64)
    if each:
        a = np.stack([a * (1.0 + 0.3 * k) for k in range(O)])
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(seed + 1)
    tf, ta = torch.from_numpy(f).to(dev), torch.from_numpy(a).to(dev)
    tdf = torch.from_numpy(rng.standard_normal(f.shape)).to(dev)
    tda = torch.from_numpy(rng.standard_normal(a.shape)).to(dev)
    return tf, ta, tdf, tda


def _library_jvp(gpu_solver_cls, each, u, ta, tdf, tda, reg):
    s = gpu_solver_cls(M, N, O)
    fn = s.sumregs_jvp_each if each else s.sumregs_jvp
    kw = {"dalphas" if each else "dalpha": tda.cpu().numpy() if tda is not None else None}
    du = fn(u.cpu().numpy(), ta.cpu().numpy(), df=tdf.cpu().numpy() if tdf is not None else None, reg=reg, **kw)
    s.close()
    return du


@pytest.mark.parametrize("reg", [0, 1])
@pytest.mark.parametrize("which", ["both", "f", "alpha"])
@pytest.mark.parametrize("each", [False, True], ids=["shared", "each"])
@pytest.mark.parametrize("kind", KINDS)
def test_forward_ad_tangent_is_the_library_sumregs_jvp_bitwise(torch_cuda, gpu_solver_cls, kind, each, which, reg):
    torch = torch_cuda
    import torch.autograd.forward_ad as fwAD
    from bpldenoising_amd.torch_layer import sumregs_denoise, sumregs_denoise_each
    fn = sumregs_denoise_each if each else sumregs_denoise
    tf, ta, tdf, tda = _inputs(torch, kind, each)
    if which == "f":
        tda = None
    if which == "alpha":
        tdf = None
    with fwAD.dual_level():
        fd = fwAD.make_dual(tf, tdf) if tdf is not None else tf
        ad = fwAD.make_dual(ta, tda) if tda is not None else ta
        out = fwAD.unpack_dual(fn(fd, ad, reg=bool(reg), forward_mode=True, maxiter=MAXITER))
        u, du = out.primal.clone(), out.tangent.clone()
    assert du.shape == u.shape and bool(torch.isfinite(du).all()) and float(du.abs().max()) > 0
    want = _library_jvp(gpu_solver_cls, each, u, ta, tdf, tda, reg)
    assert np.array_equal(du.cpu().numpy(), want)
    assert torch.equal(u, fn(tf, ta, reg=bool(reg), maxiter=MAXITER))   # the plain function: the same values


def test_forward_ad_without_a_tangent_gives_zeros(torch_cuda):
    """No dual input: the output carries no tangent; a dual input whose tangent does not reach the function (jvp called
    with both tangents None) returns zeros without a library call -- checked on the function itself."""
    torch = torch_cuda
    import torch.autograd.forward_ad as fwAD
    from bpldenoising_amd.torch_layer import SumRegsDenoiseForwardFunction, sumregs_denoise
    tf, ta, _, _ = _inputs(torch, "vector", False)
    with fwAD.dual_level():
        out = fwAD.unpack_dual(sumregs_denoise(tf, ta, forward_mode=True, maxiter=MAXITER))
        assert out.tangent is None

    class Ctx:
        saved_tensors = (tf, ta)
    z = SumRegsDenoiseForwardFunction.jvp(Ctx, None, None, None, None)
    assert z.shape == tf.shape and not bool(z.any())


@pytest.mark.parametrize("reg", [0, 1])
@pytest.mark.parametrize("kind", KINDS)
def test_forward_ad_through_the_module(torch_cuda, gpu_solver_cls, kind, reg):
    """SumRegsDenoise under forward_ad: a tangent on its parameter (torch.func.functional_call) and on f."""
    torch = torch_cuda
    import torch.autograd.forward_ad as fwAD
    from bpldenoising_amd.torch_layer import SumRegsDenoise
    tf, ta, tdf, tda = _inputs(torch, kind, False, seed=96)
    layer = SumRegsDenoise(_alpha(kind), reg=bool(reg), forward_mode=True, maxiter=MAXITER).to(tf.device)
    with fwAD.dual_level():
        dual_a = fwAD.make_dual(layer.alpha.detach(), tda)
        out = fwAD.unpack_dual(torch.func.functional_call(layer, {"alpha": dual_a}, (fwAD.make_dual(tf, tdf),)))
        u, du = out.primal.clone(), out.tangent.clone()
    want = _library_jvp(gpu_solver_cls, False, u, ta, tdf, tda, reg)
    assert np.array_equal(du.cpu().numpy(), want)


@pytest.mark.parametrize("reg", [0, 1])
@pytest.mark.parametrize("each", [False, True], ids=["shared", "each"])
@pytest.mark.parametrize("kind", KINDS)
def test_forward_and_reverse_mode_are_transposes_and_reverse_is_unchanged(torch_cuda, kind, each, reg):
    """<gu, du> = <f.grad, df> + <alpha.grad, dalpha> with gu the cotangent of a random linear loss (bound: the 1e-6 of
    tests/test_gpu_jvp.py); loss.backward() after a forward-mode call gives the bits it gave before."""
    torch = torch_cuda
    import torch.autograd.forward_ad as fwAD
    from bpldenoising_amd.torch_layer import sumregs_denoise, sumregs_denoise_each
    fn = sumregs_denoise_each if each else sumregs_denoise
    tf, ta, tdf, tda = _inputs(torch, kind, each, seed=92)
    gu = torch.from_numpy(np.random.default_rng(94).standard_normal(tuple(tf.shape))).to(tf.device)

    def reverse():
        f, a = tf.clone().requires_grad_(True), ta.clone().requires_grad_(True)
        (fn(f, a, reg=bool(reg), maxiter=MAXITER, **kw) * gu).sum().backward()
        return f.grad.clone(), a.grad.clone()
    kw = {}
    gf0, ga0 = reverse()   # the plain function
    with fwAD.dual_level():
        out = fn(fwAD.make_dual(tf, tdf), fwAD.make_dual(ta, tda), reg=bool(reg), forward_mode=True, maxiter=MAXITER)
        du = fwAD.unpack_dual(out).tangent.clone()
    gf1, ga1 = reverse()
    assert torch.equal(gf1, gf0) and torch.equal(ga1, ga0)
    kw = {"forward_mode": True}   # backward of the forward-mode function: the same bits
    gf2, ga2 = reverse()
    assert torch.equal(gf2, gf0) and torch.equal(ga2, ga0)
    lhs = float((gu * du).sum())
    t1, t2 = float((gf0 * tdf).sum()), float((ga0 * tda).sum())
    print("%s each %d reg %d: lhs %.15g rhs %.15g" % (kind, each, reg, lhs, t1 + t2))
    assert abs(lhs - (t1 + t2)) <= 1e-6 * (abs(t1) + abs(t2))


def test_a_float32_tangent_is_a_type_error(torch_cuda):
    """torch itself refuses a dual whose tangent has another dtype than its primal, so the layer's own check is reached
    through the function's jvp: TypeError, before any library call."""
    torch = torch_cuda
    from bpldenoising_amd.torch_layer import SumRegsDenoiseEachForwardFunction, SumRegsDenoiseForwardFunction
    tf, ta, tdf, tda = _inputs(torch, "vector", False)

    class Ctx:
        saved_tensors = (tf, ta)
    for fn in (SumRegsDenoiseForwardFunction, SumRegsDenoiseEachForwardFunction):
        with pytest.raises(TypeError, match="float64"):
            fn.jvp(Ctx, tdf.float(), tda, None, None)
        with pytest.raises(TypeError, match="float64"):
            fn.jvp(Ctx, None, tda.float(), None, None)
