"""GPU checks of the PyTorch layer of channel-coupled TV (torch_layer.tv_denoise_color_unrolled, TVDenoiseColorUnrolled):
autograd's gradients are the C ABI's VJP, every node keeps its own tape, a (C, H, W) input is the batch of one, a few Adam
steps on the learnable parameter reduce a loss, and checkpoints give the same bits."""
import numpy as np
import pytest

import color_ref as cr

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

NAME = "2x3x17x33"


def _same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b))


@pytest.fixture
def layer(gpu_solver_cls):
    from bpldenoising_amd import torch_layer
    yield torch_layer
    torch_layer.clear_solvers()


def _tensors(kind="scalar"):
    B, Cc, N, M = cr.SHAPES[NAME]
    f, gu = cr.gpu_data(NAME)
    alpha = cr.alpha_of(kind, N, M)
    ft = torch.tensor(f.reshape(B, Cc, N, M), device="cuda", requires_grad=True)
    at = torch.tensor(alpha, dtype=torch.float64, device="cuda", requires_grad=True)
    return f, gu, alpha, ft, at, torch.tensor(gu.reshape(B, Cc, N, M), device="cuda")


@pytest.mark.parametrize("kind", cr.KINDS)
def test_backward_is_the_abi_s_vjp(gpu_solver_cls, layer, kind):
    B, Cc, N, M = cr.SHAPES[NAME]
    f, gu, alpha, ft, at, gt = _tensors(kind)
    K = 50
    u = layer.tv_denoise_color_unrolled(ft, at, maxiter=K)
    assert tuple(u.shape) == (B, Cc, N, M)
    (u * gt).sum().backward()
    s = gpu_solver_cls(M, N, B * Cc)
    s.set_data(f, f)
    u0 = s.color_unrolled_denoise(alpha, Cc, maxiter=K)
    gf0, ga0 = s.color_unrolled_vjp(alpha, Cc, gu, maxiter=K)
    s.close()
    assert _same(u.detach().cpu().numpy().reshape(u0.shape), u0)
    assert _same(ft.grad.cpu().numpy().reshape(gf0.shape), gf0)
    assert tuple(at.grad.shape) == tuple(at.shape) and _same(at.grad.cpu().numpy(), ga0)


def test_two_nodes_keep_their_own_tapes(gpu_solver_cls, layer):
    B, Cc, N, M = cr.SHAPES[NAME]
    f, gu, alpha, ft, at, gt = _tensors()
    bt = torch.tensor(0.05, dtype=torch.float64, device="cuda", requires_grad=True)
    u1 = layer.tv_denoise_color_unrolled(ft, at, maxiter=30)
    u2 = layer.tv_denoise_color_unrolled(ft, bt, maxiter=30)     # the same handle: a second solve before any backward
    ((u1 + 2.0 * u2) * gt).sum().backward()
    s = gpu_solver_cls(M, N, B * Cc)
    s.set_data(f, f)
    s.color_unrolled_denoise(0.08, Cc, maxiter=30)
    gf1, ga1 = s.color_unrolled_vjp(0.08, Cc, gu, maxiter=30)
    s.color_unrolled_denoise(0.05, Cc, maxiter=30)
    gf2, ga2 = s.color_unrolled_vjp(0.05, Cc, 2.0 * gu, maxiter=30)
    s.close()
    assert _same(at.grad.item(), ga1) and _same(bt.grad.item(), ga2)
    assert _same(ft.grad.cpu().numpy().reshape(gf1.shape), gf1 + gf2)   # (an addition of two terms: either order)


def test_a_single_image_is_the_batch_of_one(layer):
    B, Cc, N, M = cr.SHAPES[NAME]
    f, gu, alpha, ft, at, gt = _tensors("patch")
    f1 = ft.detach()[0].clone().requires_grad_(True)
    f4 = ft.detach()[:1].clone().requires_grad_(True)
    a1, a4 = at.detach().clone().requires_grad_(True), at.detach().clone().requires_grad_(True)
    u1 = layer.tv_denoise_color_unrolled(f1, a1, maxiter=30)
    u4 = layer.tv_denoise_color_unrolled(f4, a4, maxiter=30)
    assert tuple(u1.shape) == (Cc, N, M) and torch.equal(u1, u4[0])
    (u1 * gt[0]).sum().backward()
    (u4 * gt[:1]).sum().backward()
    assert torch.equal(f1.grad, f4.grad[0]) and torch.equal(a1.grad, a4.grad)


def test_checkpoints_give_the_same_gradients_bitwise(layer):
    f, gu, alpha, ft, at, gt = _tensors("map")
    (layer.tv_denoise_color_unrolled(ft, at, maxiter=50) * gt).sum().backward()
    gf0, ga0 = ft.grad.clone(), at.grad.clone()
    ft.grad = None
    at.grad = None
    (layer.tv_denoise_color_unrolled(ft, at, maxiter=50, checkpoint_every=5) * gt).sum().backward()
    assert torch.equal(ft.grad, gf0) and torch.equal(at.grad, ga0)


def test_adam_steps_reduce_the_loss(layer):
    from conftest import synth_batch
    ub, f = synth_batch(6, 24, 28, seed=9)
    ubt = torch.tensor(ub.reshape(2, 3, 24, 28), device="cuda")
    ft = torch.tensor(f.reshape(2, 3, 24, 28), device="cuda")
    m = layer.TVDenoiseColorUnrolled(0.4, maxiter=50).to("cuda")
    opt = torch.optim.Adam(m.parameters(), lr=0.05)
    losses = []
    for _ in range(5):
        opt.zero_grad()
        loss = 0.5 * ((m(ft) - ubt) ** 2).sum()
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    print(losses, float(m.alpha.detach()))
    assert losses[-1] < losses[0] and all(np.isfinite(losses))
