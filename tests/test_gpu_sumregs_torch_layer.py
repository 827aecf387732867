"""GPU checks of the sum-of-regularisers PyTorch layer (torch_layer.sumregs_denoise / SumRegsDenoise): the forward pass
is bpltv_sumregs_denoise_device, the backward pass one bpltv_sumregs_vjp_device.  For the L2 loss torch's cotangent is
exactly u - ubar, so alpha.grad is bitwise the gradient of TVSolver.sumregs_evaluate; for any other loss it is bitwise
TVSolver.sumregs_vjp on torch's own cotangent."""
import numpy as np
import pytest
from conftest import synth_batch

pytestmark = pytest.mark.gpu

O, N, M = 3, 48, 40
A3 = np.array([0.03, 0.02, 0.05])
P22 = np.stack([np.array([[0.03, 0.05], [0.02, 0.04]]), np.array([[0.02, 0.03], [0.05, 0.02]]),
                np.array([[0.04, 0.02], [0.03, 0.06]])])
KINDS = ["vector", "patch22", "map"]
MAXITER = 300
DELTA = {0: 0.1, 1: 1e-4}   # sumregs_evaluate's branch: delta > delta_t = 1e-3 -> sumregs_gradient


def _alpha(kind):
    if kind == "vector":
        return A3
    if kind == "patch22":
        return P22
    return 0.02 + 0.04 * np.random.default_rng(9).random((3, N, M))


@pytest.fixture(scope="module")
def torch_cuda(gpu_solver_cls):
    import torch
    if not torch.cuda.is_available():
        pytest.fail("torch sees no ROCm device although the library does")
    return torch


def _tensors(torch, kind, seed=90, f_grad=False):
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
    from bpldenoising_amd.torch_layer import sumregs_denoise
    ub, f, tub, tf, ta = _tensors(torch, kind)
    u = sumregs_denoise(tf, ta, reg=bool(reg), maxiter=MAXITER)
    loss = 0.5 * ((u - tub) ** 2).sum()
    loss.backward()
    s = gpu_solver_cls(M, N, O)
    s.set_data(ub, f)
    ue, cost, g = s.sumregs_evaluate(_alpha(kind), DELTA[reg], maxiter=MAXITER)
    s.close()
    assert np.array_equal(u.detach().cpu().numpy(), ue)
    assert abs(loss.item() - cost) <= 1e-13 * cost
    assert ta.grad.shape == ta.shape
    assert np.array_equal(ta.grad.cpu().numpy(), np.asarray(g))


def _losses(torch):
    w = torch.linspace(0.5, 2.0, M, dtype=torch.float64, device="cuda")
    return {
        "charbonnier": lambda u, ub: torch.sqrt((u - ub) ** 2 + 1e-6).sum(),
        "weighted_l2": lambda u, ub: 0.5 * (w * (u - ub) ** 2).sum(),
    }


@pytest.mark.parametrize("reg", [0, 1])
@pytest.mark.parametrize("loss_name", ["charbonnier", "weighted_l2"])
@pytest.mark.parametrize("kind", KINDS)
def test_other_losses_match_the_vjp_of_torchs_cotangent(torch_cuda, gpu_solver_cls, kind, loss_name, reg):
    torch = torch_cuda
    from bpldenoising_amd.torch_layer import sumregs_denoise
    ub, f, tub, tf, ta = _tensors(torch, kind, seed=91, f_grad=True)
    u = sumregs_denoise(tf, ta, reg=bool(reg), maxiter=MAXITER)
    loss = _losses(torch)[loss_name](u, tub)
    (gu,) = torch.autograd.grad(loss, u, retain_graph=True)
    loss.backward()
    s = gpu_solver_cls(M, N, O)
    gf, ga = s.sumregs_vjp(u.detach().cpu().numpy(), _alpha(kind), gu.cpu().numpy(), reg=reg)
    s.close()
    assert tf.grad.shape == tf.shape and np.array_equal(tf.grad.cpu().numpy(), gf)
    assert np.array_equal(ta.grad.cpu().numpy(), np.asarray(ga))


def test_single_image_and_needs_input_grad(torch_cuda, gpu_solver_cls):
    """An (H, W) image is a batch of one; only the requested gradients are computed."""
    torch = torch_cuda
    from bpldenoising_amd.torch_layer import sumregs_denoise
    ub, f, tub, tf, ta = _tensors(torch, "patch22", seed=92, f_grad=True)
    u = sumregs_denoise(tf[1], ta, maxiter=MAXITER)
    assert u.shape == (N, M)
    ((u - tub[1]) ** 2).sum().backward()
    s = gpu_solver_cls(M, N, 1)
    gu = 2.0 * (u.detach().cpu().numpy() - ub[1])
    gf, ga = s.sumregs_vjp(u.detach().cpu().numpy()[None], P22, gu[None])
    s.close()
    assert np.array_equal(tf.grad[1].cpu().numpy(), gf[0]) and not tf.grad[0].any() and not tf.grad[2].any()
    assert np.array_equal(ta.grad.cpu().numpy(), ga)
    tf2 = tf.detach().clone().requires_grad_(True)
    ta2 = ta.detach().clone()
    sumregs_denoise(tf2, ta2, maxiter=MAXITER).sum().backward()
    assert ta2.grad is None and tf2.grad is not None and torch.isfinite(tf2.grad).all()
    tf3 = tf.detach().clone()
    ta3 = ta.detach().clone().requires_grad_(True)
    sumregs_denoise(tf3, ta3, maxiter=MAXITER).sum().backward()
    assert tf3.grad is None and ta3.grad is not None and torch.isfinite(ta3.grad).all()


@pytest.mark.parametrize("kind", ["vector", "patch22"])
def test_adam_on_sumregsdenoise_lowers_the_l2_loss(torch_cuda, kind):
    torch = torch_cuda
    from bpldenoising_amd.torch_layer import SumRegsDenoise
    ub, f = synth_batch(4, 64, 64, seed=3)
    tf, tub = torch.from_numpy(f).cuda(), torch.from_numpy(ub).cuda()
    init = np.full(3, 0.01) if kind == "vector" else np.full((3, 2, 2), 0.01)
    model = SumRegsDenoise(init, maxiter=MAXITER).cuda()
    opt = torch.optim.Adam(model.parameters(), lr=0.005)
    losses = []
    for _ in range(6):
        opt.zero_grad()
        loss = 0.5 * ((model(tf) - tub) ** 2).sum()
        loss.backward()
        losses.append(loss.item())
        opt.step()
    assert losses[-1] < losses[0], losses


def test_tv_and_sumregs_layers_in_one_graph(torch_cuda):
    """Both layers on the same shape share one cached handle; in one graph each gives the gradients it gives alone."""
    torch = torch_cuda
    from bpldenoising_amd.torch_layer import sumregs_denoise, tv_denoise

    def run(which):
        ub, f, tub, tf, ta = _tensors(torch, "patch22", seed=93, f_grad=True)
        tt = torch.tensor(0.1, dtype=torch.float64, device="cuda", requires_grad=True)
        loss = 0.0
        if "tv" in which:
            loss = loss + 0.5 * ((tv_denoise(tf, tt, maxiter=MAXITER) - tub) ** 2).sum()
        if "sr" in which:
            loss = loss + (sumregs_denoise(tf, ta, maxiter=MAXITER) - tub).abs().sum()
        loss.backward()
        return (tf.grad.cpu().numpy(), None if tt.grad is None else tt.grad.cpu().numpy(),
                None if ta.grad is None else ta.grad.cpu().numpy())

    tv, sr, both = run(("tv",)), run(("sr",)), run(("tv", "sr"))
    assert np.array_equal(both[1], tv[1]) and np.array_equal(both[2], sr[2])
    assert np.array_equal(both[0], tv[0] + sr[0])


def test_backward_is_reproducible(torch_cuda):
    torch = torch_cuda
    from bpldenoising_amd.torch_layer import sumregs_denoise
    grads = []
    for _ in range(2):
        ub, f, tub, tf, ta = _tensors(torch, "map", seed=94, f_grad=True)
        u = sumregs_denoise(tf, ta, maxiter=MAXITER)
        (u - tub).abs().sum().backward()
        grads.append((tf.grad.cpu().numpy(), ta.grad.cpu().numpy()))
    assert np.array_equal(grads[0][0], grads[1][0]) and np.array_equal(grads[0][1], grads[1][1])
