"""GPU checks of the PyTorch layer (bpldenoising_amd.torch_layer): u = tv_denoise(f, alpha) as an autograd operation
whose backward pass is one bpltv_vjp_device.  For the L2 loss torch's cotangent is exactly u - ubar, so alpha.grad is
bitwise the gradient of TVSolver.evaluate; for any other loss it is bitwise TVSolver.vjp on torch's own cotangent."""
import numpy as np
import pytest
from conftest import synth_batch

pytestmark = pytest.mark.gpu

O, N, M = 3, 48, 40
P22 = np.array([[0.08, 0.12], [0.1, 0.05]])
KINDS = ["scalar", "patch22", "map"]
MAXITER = 300


def _alpha(kind):
    if kind == "scalar":
        return 0.1
    if kind == "patch22":
        return P22
    return 0.05 + 0.1 * np.random.default_rng(8).random((N, M))


@pytest.fixture(scope="module")
def torch_cuda(gpu_solver_cls):
    import torch
    if not torch.cuda.is_available():
        pytest.fail("torch sees no ROCm device although the library does")
    return torch


def _tensors(torch, kind, seed=60, f_grad=False):
    ub, f = synth_batch(O, N, M, seed=seed)
    dev = torch.device("cuda", 0)
    tf = torch.from_numpy(f).to(dev).requires_grad_(f_grad)
    tub = torch.from_numpy(ub).to(dev)
    ta = torch.tensor(_alpha(kind), dtype=torch.float64, device=dev, requires_grad=True)
    return ub, f, tub, tf, ta


@pytest.mark.parametrize("reg", [0, 1])
@pytest.mark.parametrize("kind", KINDS)
def test_l2_loss_backward_is_the_evaluate_gradient_bitwise(torch_cuda, gpu_solver_cls, kind, reg):
    torch = torch_cuda
    from bpldenoising_amd.torch_layer import tv_denoise
    ub, f, tub, tf, ta = _tensors(torch, kind)
    u = tv_denoise(tf, ta, reg=bool(reg), maxiter=MAXITER)
    loss = 0.5 * ((u - tub) ** 2).sum()
    loss.backward()
    s = gpu_solver_cls(M, N, O)
    s.set_data(ub, f)
    ue, cost, g = s.evaluate(_alpha(kind), 0.0 if reg else 0.1, maxiter=MAXITER)
    s.close()
    assert np.array_equal(u.detach().cpu().numpy(), ue)
    assert abs(loss.item() - cost) <= 1e-13 * cost
    assert ta.grad.shape == ta.shape
    assert np.array_equal(ta.grad.cpu().numpy(), np.asarray(g))


def _losses(torch):
    import torch.nn.functional as F
    k = torch.tensor([[0.0, 1.0, 0.0], [1.0, -4.0, 1.0], [0.0, 1.0, 0.0]], dtype=torch.float64, device="cuda")[None, None]
    return {
        "l1": lambda u, ub: (u - ub).abs().sum(),
        "charbonnier": lambda u, ub: torch.sqrt((u - ub) ** 2 + 1e-6).sum(),
        "after_conv2d": lambda u, ub: 0.5 * ((F.conv2d(u[:, None], k) - F.conv2d(ub[:, None], k)) ** 2).sum(),
    }


@pytest.mark.parametrize("reg", [0, 1])
@pytest.mark.parametrize("loss_name", ["l1", "charbonnier", "after_conv2d"])
@pytest.mark.parametrize("kind", KINDS)
def test_other_losses_match_the_vjp_of_torchs_cotangent(torch_cuda, gpu_solver_cls, kind, loss_name, reg):
    torch = torch_cuda
    from bpldenoising_amd.torch_layer import tv_denoise
    ub, f, tub, tf, ta = _tensors(torch, kind, seed=61, f_grad=True)
    u = tv_denoise(tf, ta, reg=bool(reg), maxiter=MAXITER)
    loss = _losses(torch)[loss_name](u, tub)
    (gu,) = torch.autograd.grad(loss, u, retain_graph=True)
    loss.backward()
    s = gpu_solver_cls(M, N, O)
    gf, ga = s.vjp(u.detach().cpu().numpy(), _alpha(kind), gu.cpu().numpy(), reg=reg)
    s.close()
    assert tf.grad.shape == tf.shape and np.array_equal(tf.grad.cpu().numpy(), gf)
    assert np.array_equal(ta.grad.cpu().numpy(), np.asarray(ga))


def test_single_image_and_needs_input_grad(torch_cuda, gpu_solver_cls):
    """An (H, W) image is a batch of one; only the requested gradients are computed."""
    torch = torch_cuda
    from bpldenoising_amd.torch_layer import tv_denoise
    ub, f, tub, tf, ta = _tensors(torch, "patch22", seed=62, f_grad=True)
    u = tv_denoise(tf[1], ta, maxiter=MAXITER)
    assert u.shape == (N, M)
    ((u - tub[1]) ** 2).sum().backward()
    s = gpu_solver_cls(M, N, 1)
    gu = 2.0 * (u.detach().cpu().numpy() - ub[1])
    gf, ga = s.vjp(u.detach().cpu().numpy()[None], P22, gu[None])
    s.close()
    assert np.array_equal(tf.grad[1].cpu().numpy(), gf[0]) and not tf.grad[0].any() and not tf.grad[2].any()
    assert np.array_equal(ta.grad.cpu().numpy(), ga)
    tf2 = tf.detach().clone().requires_grad_(True)
    ta2 = ta.detach().clone()
    tv_denoise(tf2, ta2, maxiter=MAXITER).sum().backward()
    assert ta2.grad is None and tf2.grad is not None and torch.isfinite(tf2.grad).all()


@pytest.mark.parametrize("kind", ["scalar", "patch22"])
def test_adam_on_tvdenoise_lowers_the_l2_loss(torch_cuda, kind):
    torch = torch_cuda
    from bpldenoising_amd.torch_layer import TVDenoise
    ub, f = synth_batch(4, 64, 64, seed=3)
    tf, tub = torch.from_numpy(f).cuda(), torch.from_numpy(ub).cuda()
    init = 0.02 if kind == "scalar" else np.full((2, 2), 0.02)
    model = TVDenoise(init, maxiter=MAXITER).cuda()
    opt = torch.optim.Adam(model.parameters(), lr=0.01)
    losses = []
    for _ in range(6):
        opt.zero_grad()
        loss = 0.5 * ((model(tf) - tub) ** 2).sum()
        loss.backward()
        losses.append(loss.item())
        opt.step()
    assert losses[-1] < losses[0], losses


def test_backward_is_reproducible(torch_cuda):
    torch = torch_cuda
    from bpldenoising_amd.torch_layer import tv_denoise
    grads = []
    for _ in range(2):
        ub, f, tub, tf, ta = _tensors(torch, "map", seed=63, f_grad=True)
        u = tv_denoise(tf, ta, maxiter=MAXITER)
        (u - tub).abs().sum().backward()
        grads.append((tf.grad.cpu().numpy(), ta.grad.cpu().numpy()))
    assert np.array_equal(grads[0][0], grads[1][0]) and np.array_equal(grads[0][1], grads[1][1])
