"""GPU checks of torch_layer.tv_denoise_each: u[k] = denoise(f[k], alpha[k]) with one parameter per sample, whose
backward pass is one bpltv_vjp_each_device.  For the L2 loss alpha.grad is bitwise TVSolver.vjp_each on u - ubar; for
another loss every sample's gradients agree with a one-image tv_denoise of that sample; a small network that predicts
per-pixel maps trains through it."""
import numpy as np
import pytest
from conftest import synth_batch

pytestmark = pytest.mark.gpu

O, N, M = 3, 48, 40
KINDS = ["scalar", "patch23", "map"]
MAXITER = 300


def _alpha(kind, seed=8):
    rng = np.random.default_rng(seed)
    shape = {"scalar": (O,), "patch23": (O, 2, 3), "map": (O, N, M)}[kind]
    return 0.04 + 0.12 * rng.random(shape)


@pytest.fixture(scope="module")
def torch_cuda(gpu_solver_cls):
    import torch
    if not torch.cuda.is_available():
        pytest.fail("torch sees no ROCm device although the library does")
    return torch


def _tensors(torch, kind, seed=60):
    ub, f = synth_batch(O, N, M, seed=seed)
    dev = torch.device("cuda", 0)
    tf = torch.from_numpy(f).to(dev).requires_grad_(True)
    tub = torch.from_numpy(ub).to(dev)
    ta = torch.tensor(_alpha(kind), dtype=torch.float64, device=dev, requires_grad=True)
    return ub, f, tub, tf, ta


@pytest.mark.parametrize("reg", [0, 1])
@pytest.mark.parametrize("kind", KINDS)
def test_l2_loss_backward_is_vjp_each_bitwise(torch_cuda, gpu_solver_cls, kind, reg):
    torch = torch_cuda
    from bpldenoising_amd.torch_layer import tv_denoise_each
    ub, f, tub, tf, ta = _tensors(torch, kind)
    u = tv_denoise_each(tf, ta, reg=bool(reg), maxiter=MAXITER)
    loss = 0.5 * ((u - tub) ** 2).sum()
    loss.backward()
    s = gpu_solver_cls(M, N, O)
    s.set_data(ub, f)
    a = _alpha(kind)
    ue = s.denoise_each(a, maxiter=MAXITER)
    gf, ga = s.vjp_each(ue, a, ue - ub, reg=reg)
    s.close()
    assert np.array_equal(u.detach().cpu().numpy(), ue)
    assert ta.grad.shape == ta.shape and tf.grad.shape == tf.shape
    assert np.array_equal(ta.grad.cpu().numpy(), ga)
    assert np.array_equal(tf.grad.cpu().numpy(), gf)


@pytest.mark.parametrize("kind", KINDS)
def test_charbonnier_loss_matches_one_image_layers(torch_cuda, kind):
    """alpha.grad[k] and f.grad[k] of the batched layer against tv_denoise on sample k alone (1e-9: the adjoint's
    nested-dissection kernels are chosen by batch size)."""
    torch = torch_cuda
    from bpldenoising_amd.torch_layer import tv_denoise, tv_denoise_each

    def charbonnier(u, ub):
        return torch.sqrt((u - ub) ** 2 + 1e-4).sum()

    ub, f, tub, tf, ta = _tensors(torch, kind, seed=61)
    u = tv_denoise_each(tf, ta, maxiter=MAXITER)
    charbonnier(u, tub).backward()
    for k in range(O):
        fk = tf.detach()[k:k + 1].clone().requires_grad_(True)
        ak = ta.detach()[k].clone().requires_grad_(True)
        uk = tv_denoise(fk, ak, maxiter=MAXITER)
        assert torch.equal(uk[0], u.detach()[k]), k
        charbonnier(uk, tub[k:k + 1]).backward()
        for got, want in ((ta.grad[k], ak.grad), (tf.grad[k], fk.grad[0])):
            g, w = got.cpu().numpy(), want.cpu().numpy()
            assert np.allclose(g, w, rtol=1e-9, atol=1e-9 * np.abs(w).max()), k


def test_a_small_network_predicting_maps_trains(torch_cuda):
    """A two-layer conv net outputs a positive (B, H, W) map per noisy image; one optimiser step through the layer
    gives finite, non-zero gradients to every weight and changes them."""
    torch = torch_cuda
    from bpldenoising_amd.torch_layer import tv_denoise_each
    torch.manual_seed(0)
    dev = torch.device("cuda", 0)
    ub, f = synth_batch(O, N, M, seed=62)
    tf, tub = torch.from_numpy(f).to(dev), torch.from_numpy(ub).to(dev)
    net = torch.nn.Sequential(torch.nn.Conv2d(1, 4, 3, padding=1), torch.nn.Tanh(),
                              torch.nn.Conv2d(4, 1, 3, padding=1)).to(dev, torch.float64)
    opt = torch.optim.SGD(net.parameters(), lr=1e-3)
    before = [p.detach().clone() for p in net.parameters()]
    alpha = 0.02 + torch.nn.functional.softplus(net(tf[:, None]))[:, 0]   # (B, H, W), every entry > 0
    assert alpha.shape == (O, N, M)
    u = tv_denoise_each(tf, alpha, maxiter=MAXITER)
    loss = 0.5 * ((u - tub) ** 2).sum()
    opt.zero_grad()
    loss.backward()
    for p in net.parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all() and p.grad.abs().max() > 0
    opt.step()
    assert any(not torch.equal(b, p.detach()) for b, p in zip(before, net.parameters()))
