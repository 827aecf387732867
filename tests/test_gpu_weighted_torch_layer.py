"""GPU checks of tv_denoise_weighted (bpldenoising_amd/torch_layer.py): with w = 1 it is tv_denoise bit for bit, in value
and in f.grad / alpha.grad; w.grad has w's shape and is TVSolver.weighted_vjp's; forward-mode AD raises."""
import numpy as np
import pytest
from conftest import synth_batch

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

B, H, W = 3, 20, 16


def _alpha(kind):
    if kind == "scalar":
        return np.asarray(0.1)
    if kind == "patch":
        return np.array([[0.08, 0.12], [0.1, 0.05]])
    return 0.05 + 0.1 * np.random.default_rng(8).random((H, W))


@pytest.fixture(scope="module")
def data(gpu_solver_cls):
    _, f = synth_batch(B, H, W, seed=25)
    g = np.random.default_rng(26).standard_normal(f.shape)
    return f, g


def _leaf(a):
    return torch.tensor(np.asarray(a, dtype=np.float64), device="cuda", requires_grad=True)


@pytest.mark.parametrize("kind", ["scalar", "patch", "map"])
def test_unit_weight_is_tv_denoise_bitwise(data, kind):
    from bpldenoising_amd.torch_layer import tv_denoise, tv_denoise_weighted
    f, g = data
    gt = torch.tensor(g, device="cuda")
    f0, a0 = _leaf(f), _leaf(_alpha(kind))
    u0 = tv_denoise(f0, a0, maxiter=300)
    (u0 * gt).sum().backward()
    for wshape in ((H, W), (B, H, W)):
        f1, a1 = _leaf(f), _leaf(_alpha(kind))
        w1 = torch.ones(wshape, dtype=torch.float64, device="cuda", requires_grad=True)
        u1 = tv_denoise_weighted(f1, a1, w1, maxiter=300)
        (u1 * gt).sum().backward()
        assert torch.equal(u1, u0) and torch.equal(f1.grad, f0.grad) and torch.equal(a1.grad, a0.grad)
        assert a1.grad.shape == a0.shape and w1.grad.shape == w1.shape
        want = -(u0.detach() - f0.detach()) * f0.grad
        if len(wshape) == 2:
            want = want.sum(dim=0)
        assert torch.allclose(w1.grad, want, rtol=1e-14, atol=0)


@pytest.mark.parametrize("wshape", [(H, W), (B, H, W)], ids=["HW", "BHW"])
def test_weight_gradient_is_the_solver_s(gpu_solver_cls, data, wshape):
    from bpldenoising_amd.torch_layer import tv_denoise_weighted
    f, g = data
    w = 0.25 + 3.75 * np.random.default_rng(27).random(wshape)
    alpha = _alpha("patch")
    ft, at, wt = _leaf(f), _leaf(alpha), _leaf(w)
    u = tv_denoise_weighted(ft, at, wt, maxiter=300)
    (u * torch.tensor(g, device="cuda")).sum().backward()
    s = gpu_solver_cls(W, H, B)
    s.set_data(f, f)
    u0 = s.weighted_denoise(alpha, w, maxiter=300)
    gf, ga, gw = s.weighted_vjp(u0, f, alpha, w, g)
    s.close()
    assert np.array_equal(u.detach().cpu().numpy(), u0)
    assert wt.grad.shape == wt.shape and np.array_equal(wt.grad.cpu().numpy(), gw)
    assert np.array_equal(ft.grad.cpu().numpy(), gf) and np.array_equal(at.grad.cpu().numpy(), ga)
    # only w asks for a gradient: the same w.grad
    w2 = _leaf(w)
    u2 = tv_denoise_weighted(torch.tensor(f, device="cuda"), torch.tensor(alpha, device="cuda"), w2, maxiter=300)
    (u2 * torch.tensor(g, device="cuda")).sum().backward()
    assert np.array_equal(w2.grad.cpu().numpy(), gw)


def test_single_image_and_forward_mode(data):
    import torch.autograd.forward_ad as fwAD
    from bpldenoising_amd.torch_layer import tv_denoise_weighted
    f, _ = data
    f2 = _leaf(f[0])                                   # (H, W): one image
    w = torch.full((H, W), 2.0, dtype=torch.float64, device="cuda", requires_grad=True)
    a = _leaf(0.1)
    u = tv_denoise_weighted(f2, a, w, maxiter=100)
    assert u.shape == (H, W)
    u.sum().backward()
    assert w.grad.shape == (H, W) and f2.grad.shape == (H, W) and a.grad.shape == ()
    with fwAD.dual_level():
        fd = fwAD.make_dual(f2.detach(), torch.ones_like(f2))
        with pytest.raises((NotImplementedError, RuntimeError)):
            tv_denoise_weighted(fd, a.detach(), w.detach(), maxiter=10)
