"""GPU checks of forward-mode AD through the PyTorch layer: the tangent of tv_denoise / tv_denoise_each under
torch.autograd.forward_ad is bitwise TVSolver.jvp_device / jvp_each_device on the u of the forward pass, it is the
transpose of what loss.backward() computes, and reverse mode is what it was."""
import numpy as np
import pytest
from conftest import synth_batch

from test_gpu_torch_layer import KINDS, M, MAXITER, N, O, _alpha, torch_cuda  # noqa: F401

pytestmark = pytest.mark.gpu


def _inputs(torch, kind, each, seed=90):
    _, f = synth_batch(O, N, M, seed=seed)
    a = np.asarray(_alpha(kind), dtype=np.float64)
    if each:
        a = np.stack([a * (1.0 + 0.2 * k) for k in range(O)])
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(seed + 1)
    tf, ta = torch.from_numpy(f).to(dev), torch.from_numpy(a).to(dev)
    tdf = torch.from_numpy(rng.standard_normal(f.shape)).to(dev)
    tda = torch.from_numpy(rng.standard_normal(a.shape)).to(dev)
    return tf, ta, tdf, tda


def _library_jvp(torch, gpu_solver_cls, each, u, ta, tdf, tda, reg):
    s = gpu_solver_cls(M, N, O)
    shape = tuple(ta.shape[1:] if each else ta.shape)
    am, an = (1, 1) if shape == () else (shape[1], shape[0])
    du = torch.zeros_like(u)
    torch.cuda.synchronize()
    (s.jvp_each_device if each else s.jvp_device)(u.data_ptr(), ta.data_ptr(), am, an, tdf.data_ptr() if tdf is not None else None,
                                                   tda.data_ptr() if tda is not None else None, du.data_ptr(), reg=reg)
    s.close()
    return du


@pytest.mark.parametrize("reg", [0, 1])
@pytest.mark.parametrize("which", ["both", "f", "alpha"])
@pytest.mark.parametrize("each", [False, True], ids=["shared", "each"])
@pytest.mark.parametrize("kind", KINDS)
def test_forward_ad_tangent_is_the_library_jvp_bitwise(torch_cuda, gpu_solver_cls, kind, each, which, reg):
    torch = torch_cuda
    import torch.autograd.forward_ad as fwAD
    from bpldenoising_amd.torch_layer import tv_denoise, tv_denoise_each
    fn = tv_denoise_each if each else tv_denoise
    tf, ta, tdf, tda = _inputs(torch, kind, each)
    if which == "f":
        tda = None
    if which == "alpha":
        tdf = None
    with fwAD.dual_level():
        fd = fwAD.make_dual(tf, tdf) if tdf is not None else tf
        ad = fwAD.make_dual(ta, tda) if tda is not None else ta
        out = fwAD.unpack_dual(fn(fd, ad, reg=bool(reg), maxiter=MAXITER))
        u, du = out.primal.clone(), out.tangent.clone()
    assert du.shape == u.shape and bool(torch.isfinite(du).all()) and float(du.abs().max()) > 0
    want = _library_jvp(torch, gpu_solver_cls, each, u.contiguous(), ta, tdf, tda, reg)
    assert torch.equal(du, want)
    assert torch.equal(u, fn(tf, ta, reg=bool(reg), maxiter=MAXITER))


@pytest.mark.parametrize("reg", [0, 1])
@pytest.mark.parametrize("each", [False, True], ids=["shared", "each"])
@pytest.mark.parametrize("kind", KINDS)
def test_forward_and_reverse_mode_are_transposes_and_reverse_is_unchanged(torch_cuda, kind, each, reg):
    """<gu, du> = <f.grad, df> + <alpha.grad, dalpha> with gu the cotangent of a random linear loss (bound: the 1e-6 of
    tests/test_gpu_jvp.py); loss.backward() after a forward-mode call gives the bits it gave before."""
    torch = torch_cuda
    import torch.autograd.forward_ad as fwAD
    from bpldenoising_amd.torch_layer import tv_denoise, tv_denoise_each
    fn = tv_denoise_each if each else tv_denoise
    tf, ta, tdf, tda = _inputs(torch, kind, each, seed=92)
    gu = torch.from_numpy(np.random.default_rng(94).standard_normal(tuple(tf.shape))).to(tf.device)

    def reverse():
        f, a = tf.clone().requires_grad_(True), ta.clone().requires_grad_(True)
        (fn(f, a, reg=bool(reg), maxiter=MAXITER) * gu).sum().backward()
        return f.grad.clone(), a.grad.clone()
    gf0, ga0 = reverse()
    with fwAD.dual_level():
        f, a = tf.clone().requires_grad_(True), ta.clone().requires_grad_(True)
        out = fn(fwAD.make_dual(f, tdf), fwAD.make_dual(a, tda), reg=bool(reg), maxiter=MAXITER)
        du = fwAD.unpack_dual(out).tangent.clone()
        # reverse mode through the very output that carries a tangent
        (fwAD.unpack_dual(out).primal * gu).sum().backward()
        assert torch.equal(f.grad, gf0) and torch.equal(a.grad, ga0)
    gf1, ga1 = reverse()
    assert torch.equal(gf1, gf0) and torch.equal(ga1, ga0)
    lhs = float((gu * du).sum())
    t1, t2 = float((gf0 * tdf).sum()), float((ga0 * tda).sum())
    print("%s each %d reg %d: lhs %.15g rhs %.15g" % (kind, each, reg, lhs, t1 + t2))
    assert abs(lhs - (t1 + t2)) <= 1e-6 * (abs(t1) + abs(t2))


def test_sumregs_layers_have_no_forward_mode(torch_cuda):
    torch = torch_cuda
    import torch.autograd.forward_ad as fwAD
    from bpldenoising_amd.torch_layer import sumregs_denoise
    tf, _, tdf, _ = _inputs(torch, "scalar", False, seed=95)
    a3 = torch.full((3,), 0.03, dtype=torch.float64, device=tf.device)
    with fwAD.dual_level():
        with pytest.raises((NotImplementedError, RuntimeError)):
            sumregs_denoise(fwAD.make_dual(tf, tdf), a3, maxiter=50)
