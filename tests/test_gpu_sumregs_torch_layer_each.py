"""GPU checks of torch_layer.sumregs_denoise_each: u[k] = sumregs_denoise(f[k], alpha[k]) with three weights per sample,
whose backward pass is one bpltv_sumregs_vjp_each_device.  The forward is bitwise TVSolver.sumregs_denoise_each and, for
a loss that is not the L2 loss, f.grad and alpha.grad are bitwise TVSolver.sumregs_vjp_each on torch's cotangent; every
needs_input_grad combination skips the unused output; a small network that predicts the weights trains through it."""
import numpy as np
import pytest
from conftest import synth_batch

pytestmark = pytest.mark.gpu

O, N, M = 3, 48, 40
KINDS = ["vector", "patch23", "map"]
MAXITER = 300


def _alpha(kind, seed=8):
    rng = np.random.default_rng(seed)
    shape = {"vector": (O, 3), "patch23": (O, 3, 2, 3), "map": (O, 3, N, M)}[kind]
    return 0.02 + 0.05 * rng.random(shape)


@pytest.fixture(scope="module")
def torch_cuda(gpu_solver_cls):
    import torch
    if not torch.cuda.is_available():
        pytest.fail("torch sees no ROCm device although the library does")
    return torch


def _tensors(torch, kind, seed=60, f_grad=True, a_grad=True):
    ub, f = synth_batch(O, N, M, seed=seed)
    dev = torch.device("cuda", 0)
    tf = torch.from_numpy(f).to(dev).requires_grad_(f_grad)
    tub = torch.from_numpy(ub).to(dev)
    ta = torch.tensor(_alpha(kind), dtype=torch.float64, device=dev, requires_grad=a_grad)
    return ub, f, tub, tf, ta


def _charbonnier(torch, u, ub):
    return torch.sqrt((u - ub) ** 2 + 1e-4).sum()


@pytest.mark.parametrize("reg", [0, 1])
@pytest.mark.parametrize("kind", KINDS)
def test_forward_and_backward_are_the_solvers_bitwise(torch_cuda, gpu_solver_cls, kind, reg):
    """Charbonnier loss: torch's cotangent (u - ubar) / sqrt((u - ubar)^2 + eps) handed to sumregs_vjp_each gives the
    layer's f.grad and alpha.grad bit for bit."""
    torch = torch_cuda
    from bpldenoising_amd.torch_layer import sumregs_denoise_each
    ub, f, tub, tf, ta = _tensors(torch, kind)
    u = sumregs_denoise_each(tf, ta, reg=bool(reg), maxiter=MAXITER)
    _charbonnier(torch, u, tub).backward()
    ud = u.detach().clone().requires_grad_(True)   # the cotangent torch computed, from the same graph of operations
    _charbonnier(torch, ud, tub).backward()
    gu = ud.grad.cpu().numpy()
    s = gpu_solver_cls(M, N, O)
    s.set_data(ub, f)
    a = _alpha(kind)
    ue = s.sumregs_denoise_each(a, maxiter=MAXITER)
    gf, ga = s.sumregs_vjp_each(ue, a, gu, reg=reg)
    s.close()
    assert np.array_equal(u.detach().cpu().numpy(), ue)
    assert ta.grad.shape == ta.shape and tf.grad.shape == tf.shape
    assert np.array_equal(ta.grad.cpu().numpy(), ga)
    assert np.array_equal(tf.grad.cpu().numpy(), gf)


@pytest.mark.parametrize("kind", KINDS)
def test_needs_input_grad_combinations_skip_the_unused_output(torch_cuda, kind, monkeypatch):
    torch = torch_cuda
    from bpldenoising_amd import torch_layer
    from bpldenoising_amd.learning_function import TVSolver
    calls = []
    real = TVSolver.sumregs_vjp_each_device

    def spy(self, u_ptr, alphas_ptr, am, an, gu_ptr, grad_f_ptr, grad_alphas_ptr, **kw):
        calls.append((grad_f_ptr is not None, grad_alphas_ptr is not None))
        return real(self, u_ptr, alphas_ptr, am, an, gu_ptr, grad_f_ptr, grad_alphas_ptr, **kw)

    monkeypatch.setattr(TVSolver, "sumregs_vjp_each_device", spy)
    both = None
    for f_grad, a_grad in ((True, True), (True, False), (False, True)):
        ub, f, tub, tf, ta = _tensors(torch, kind, seed=63, f_grad=f_grad, a_grad=a_grad)
        u = torch_layer.sumregs_denoise_each(tf, ta, maxiter=MAXITER)
        _charbonnier(torch, u, tub).backward()
        assert calls[-1] == (f_grad, a_grad)
        assert (tf.grad is not None) == f_grad and (ta.grad is not None) == a_grad
        if both is None:
            both = (tf.grad.clone(), ta.grad.clone())
        if f_grad:
            assert torch.equal(tf.grad, both[0])
        if a_grad:
            assert torch.equal(ta.grad, both[1])
    n = len(calls)
    ub, f, tub, tf, ta = _tensors(torch, kind, seed=63, f_grad=False, a_grad=False)
    u = torch_layer.sumregs_denoise_each(tf, ta, maxiter=MAXITER)
    assert not u.requires_grad and len(calls) == n


@pytest.mark.parametrize("kind", ["vector", "map"])
def test_a_small_network_predicting_the_weights_trains(torch_cuda, kind):
    """alpha = softplus(net(f)): a two-layer net outputs three positive weights per image -- (B, 3) through a pooled
    head, or (B, 3, H, W) maps -- and a few Adam steps through the layer bring the loss down."""
    torch = torch_cuda
    from bpldenoising_amd.torch_layer import sumregs_denoise_each
    torch.manual_seed(0)
    dev = torch.device("cuda", 0)
    ub, f = synth_batch(O, N, M, seed=62)
    tf, tub = torch.from_numpy(f).to(dev), torch.from_numpy(ub).to(dev)
    net = torch.nn.Sequential(torch.nn.Conv2d(1, 4, 3, padding=1), torch.nn.Tanh(),
                              torch.nn.Conv2d(4, 3, 3, padding=1)).to(dev, torch.float64)

    def weights():
        a = 1e-3 + 0.05 * torch.nn.functional.softplus(net(tf[:, None]))   # (B, 3, H, W), every entry > 0
        return a.mean(dim=(2, 3)) if kind == "vector" else a

    opt = torch.optim.Adam(net.parameters(), lr=2e-3)   # steps of about lr per weight, whatever the gradient's scale
    losses = []
    for step in range(4):
        alpha = weights()
        assert alpha.shape == ((O, 3) if kind == "vector" else (O, 3, N, M))
        u = sumregs_denoise_each(tf, alpha, maxiter=MAXITER)
        loss = 0.5 * ((u - tub) ** 2).sum()
        losses.append(float(loss))
        opt.zero_grad()
        loss.backward()
        for p in net.parameters():
            assert p.grad is not None and torch.isfinite(p.grad).all() and p.grad.abs().max() > 0
        opt.step()
    print("training losses (%s):" % kind, losses)
    assert losses[-1] < losses[0], losses
