"""GPU checks of the PyTorch layer of TV-KL denoising (torch_layer.tv_kl_denoise_unrolled, TVKLDenoiseUnrolled): autograd's u and
gradients in f, alpha and w are the C ABI's bit for bit, for one weight plane and for one per image, with and without
checkpoints, also when another forward pass has replaced the handle's f in between; the module trains alpha and w; forward mode
raises; and central differences of the layer's own output confirm alpha.grad and w.grad."""
import numpy as np
import pytest

import kl_ref as kr

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


def _same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b))


@pytest.fixture
def layer(gpu_solver_cls):
    from bpldenoising_amd import torch_layer
    yield torch_layer
    torch_layer.clear_solvers()


def _tensors(name, kind, wkind):
    O, N, M = kr.GPU_SHAPES[name]
    f, gu = kr.gpu_data(name)
    alpha = kr.alpha_of(kind, N, M)
    w = kr.weight_of(wkind, O, N, M)
    ft = torch.tensor(f, device="cuda", requires_grad=True)
    at = torch.tensor(alpha, dtype=torch.float64, device="cuda", requires_grad=True)
    wt = torch.tensor(w, device="cuda", requires_grad=True)
    return f, gu, alpha, w, ft, at, wt, torch.tensor(gu, device="cuda")


@pytest.mark.parametrize("wkind", ["mask", "real"])      # (H, W) and (B, H, W)
@pytest.mark.parametrize("kind", ["scalar", "patch", "map"])
@pytest.mark.parametrize("name", ["2x17x33", "3x40x48"])
def test_backward_is_the_abi_s_vjp(gpu_solver_cls, layer, name, kind, wkind):
    O, N, M = kr.GPU_SHAPES[name]
    f, gu, alpha, w, ft, at, wt, gt = _tensors(name, kind, wkind)
    K = 57
    u = layer.tv_kl_denoise_unrolled(ft, at, wt, maxiter=K)
    assert tuple(u.shape) == (O, N, M)
    (u * gt).sum().backward()
    s = gpu_solver_cls(M, N, O)
    s.set_data(f, f)
    u0 = s.kl_unrolled_denoise(alpha, w, maxiter=K)
    gf0, ga0, gw0 = s.kl_unrolled_vjp(alpha, w, gu, maxiter=K)
    s.close()
    assert _same(u.detach().cpu().numpy(), u0)
    assert _same(ft.grad.cpu().numpy(), gf0)
    assert tuple(at.grad.shape) == tuple(at.shape) and _same(at.grad.cpu().numpy(), ga0)
    assert tuple(wt.grad.shape) == tuple(wt.shape) and _same(wt.grad.cpu().numpy(), gw0)
    # checkpoints instead of the tape, and another forward pass on the shared handle -- another f -- before backward: the same bits
    grads = [t.grad.clone() for t in (ft, at, wt)]
    for t in (ft, at, wt):
        t.grad = None
    u2 = layer.tv_kl_denoise_unrolled(ft, at, wt, maxiter=K, checkpoint_every=5)
    layer.tv_kl_denoise_unrolled(torch.flip(ft.detach(), dims=(1, 2)), at.detach(), wt.detach(), maxiter=K)
    (u2 * gt).sum().backward()
    assert torch.equal(u2, u) and all(torch.equal(t.grad, g) for t, g in zip((ft, at, wt), grads))


def test_only_the_gradients_asked_for_are_computed(layer):
    """... and the sweep installs f again whatever is asked: another forward pass on the shared handle has replaced it."""
    f, gu, alpha, w, ft, at, wt, gt = _tensors("2x17x33", "scalar", "mask")
    (layer.tv_kl_denoise_unrolled(ft, at, wt, maxiter=30) * gt).sum().backward()
    f2, a2 = ft.detach().clone().requires_grad_(True), at.detach().clone().requires_grad_(True)
    loss = (layer.tv_kl_denoise_unrolled(f2, a2, wt.detach(), maxiter=30) * gt).sum()    # no w.grad: a NULL grad_w_out
    layer.tv_kl_denoise_unrolled(torch.flip(ft.detach(), dims=(0,)), at.detach(), wt.detach(), maxiter=30)   # another f in between
    loss.backward()
    assert torch.equal(f2.grad, ft.grad) and torch.equal(a2.grad, at.grad)
    w2 = wt.detach().clone().requires_grad_(True)
    (layer.tv_kl_denoise_unrolled(ft.detach(), at.detach(), w2, maxiter=30) * gt).sum().backward()
    assert torch.equal(w2.grad, wt.grad)


def test_the_module_trains_alpha_and_w_and_forward_mode_raises(layer):
    f, gu, alpha, w, ft, at, wt, gt = _tensors("2x17x33", "map", "real")
    (layer.tv_kl_denoise_unrolled(ft, at, wt, maxiter=30) * gt).sum().backward()
    m = layer.TVKLDenoiseUnrolled(alpha, w, maxiter=30, learn_w=True).to("cuda")
    assert sorted(n for n, _ in m.named_parameters()) == ["alpha", "w"]
    (m(ft.detach()) * gt).sum().backward()
    assert m.alpha.grad is not None and m.w.grad is not None
    assert torch.equal(m.alpha.grad, at.grad) and torch.equal(m.w.grad, wt.grad)
    fixed = layer.TVKLDenoiseUnrolled(alpha, w, maxiter=30).to("cuda")
    assert [n for n, _ in fixed.named_parameters()] == ["alpha"] and fixed.w.device.type == "cuda"
    (fixed(ft.detach()) * gt).sum().backward()
    assert torch.equal(fixed.alpha.grad, at.grad)
    with pytest.raises(ValueError, match="forward mode through the TV-KL iterations does not exist"):
        layer.tv_kl_denoise_unrolled(ft, at, wt, maxiter=30, forward_mode=True)
    bad = ft.detach().clone()
    bad[1, 3, 4] = -0.5
    with pytest.raises(ValueError, match="tv_kl_denoise_unrolled: f must be finite and >= 0"):
        layer.tv_kl_denoise_unrolled(bad, at, wt, maxiter=30)


def test_central_differences_in_alpha_and_in_w(layer):
    """kl_ref.layer_case: 1 x 8 x 9, maxiter = 20, f in [0.1, 1.1], alpha = 0.1, w in [0.05, 0.15] with about 30 % zeros (tests/
    test_kl_abi.py checks on the twin that the projection is active within the 20 iterations): d/dalpha and the directional
    derivative along a random dw on the kept pixels of L = <u, gu>, against central differences of the layer's own output with
    h = 1e-6, to 1e-5 relative."""
    f, alpha, w, K, h, gu, dw = kr.layer_case()
    ft, gt = torch.tensor(f, device="cuda"), torch.tensor(gu, device="cuda")
    at = torch.tensor(alpha, dtype=torch.float64, device="cuda", requires_grad=True)
    wt = torch.tensor(w, device="cuda", requires_grad=True)
    dwt = torch.tensor(dw, device="cuda")
    loss = lambda a, w_: float((layer.tv_kl_denoise_unrolled(ft, a, w_, maxiter=K) * gt).sum())
    (layer.tv_kl_denoise_unrolled(ft, at, wt, maxiter=K) * gt).sum().backward()
    a0, w0 = at.detach(), wt.detach()
    for what, g, fd in (("alpha", float(at.grad), (loss(a0 + h, w0) - loss(a0 - h, w0)) / (2 * h)),
                        ("w", float((wt.grad * dwt).sum()), (loss(a0, w0 + h * dwt) - loss(a0, w0 - h * dwt)) / (2 * h))):
        print("%s: autograd %.10g central difference %.10g rel %.2e" % (what, g, fd, abs(g - fd) / abs(fd)))
        assert fd != 0.0 and abs(g - fd) <= 1e-5 * abs(fd)
