"""GPU checks of the PyTorch layer of weighted channel-coupled TV (torch_layer.tv_denoise_color_weighted_unrolled): autograd's
gradients in f, alpha and w are the C ABI's VJP bit for bit, for one weight plane and for one per channel; a mask per colour
image, expanded over the channels, gets its gradient summed by autograd; checkpoints give the same bits; and central
differences of the layer's own output confirm alpha.grad and w.grad."""
import numpy as np
import pytest

import color_weighted_ref as cw

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
    B, Cc, N, M = cw.SHAPES[name]
    f, gu = cw.gpu_data(name)
    alpha = cw.alpha_of(kind, N, M)
    w = cw.weight_of(wkind, B, Cc, N, M)
    ft = torch.tensor(f.reshape(B, Cc, N, M), device="cuda", requires_grad=True)
    at = torch.tensor(alpha, dtype=torch.float64, device="cuda", requires_grad=True)
    wt = torch.tensor(w if w.ndim == 2 else w.reshape(B, Cc, N, M), device="cuda", requires_grad=True)
    return f, gu, alpha, w, ft, at, wt, torch.tensor(gu.reshape(B, Cc, N, M), device="cuda")


@pytest.mark.parametrize("wkind", ["mask", "real", "mosaic"])      # (H, W), and two of (B, C, H, W)
@pytest.mark.parametrize("kind", ["scalar", "map"])
@pytest.mark.parametrize("name", ["2x3x17x33", "1x3x40x48"])
def test_backward_is_the_abi_s_vjp(gpu_solver_cls, layer, name, kind, wkind):
    B, Cc, N, M = cw.SHAPES[name]
    f, gu, alpha, w, ft, at, wt, gt = _tensors(name, kind, wkind)
    K = 30
    u = layer.tv_denoise_color_weighted_unrolled(ft, at, wt, maxiter=K)
    assert tuple(u.shape) == (B, Cc, N, M)
    (u * gt).sum().backward()
    s = gpu_solver_cls(M, N, B * Cc)
    s.set_data(f, f)
    u0 = s.color_weighted_unrolled_denoise(alpha, Cc, w, maxiter=K)
    gf0, ga0, gw0 = s.color_weighted_unrolled_vjp(alpha, Cc, w, gu, maxiter=K)
    s.close()
    assert _same(u.detach().cpu().numpy().reshape(u0.shape), u0)
    assert _same(ft.grad.cpu().numpy().reshape(gf0.shape), gf0)
    assert tuple(at.grad.shape) == tuple(at.shape) and _same(at.grad.cpu().numpy(), ga0)
    assert tuple(wt.grad.shape) == tuple(wt.shape) and _same(wt.grad.cpu().numpy().reshape(gw0.shape), gw0)
    # checkpoints instead of the tape: the same bits
    grads = [t.grad.clone() for t in (ft, at, wt)]
    for t in (ft, at, wt):
        t.grad = None
    u2 = layer.tv_denoise_color_weighted_unrolled(ft, at, wt, maxiter=K, checkpoint_every=4)
    (u2 * gt).sum().backward()
    assert torch.equal(u2, u) and all(torch.equal(t.grad, g) for t, g in zip((ft, at, wt), grads))


def test_only_the_gradients_asked_for_are_computed(layer):
    f, gu, alpha, w, ft, at, wt, gt = _tensors("2x3x17x33", "scalar", "mask")
    (layer.tv_denoise_color_weighted_unrolled(ft, at, wt, maxiter=30) * gt).sum().backward()
    f2, a2 = ft.detach().clone().requires_grad_(True), at.detach().clone().requires_grad_(True)
    (layer.tv_denoise_color_weighted_unrolled(f2, a2, wt.detach(), maxiter=30) * gt).sum().backward()   # no w.grad: a NULL grad_w_out
    assert torch.equal(f2.grad, ft.grad) and torch.equal(a2.grad, at.grad)
    w2 = wt.detach().clone().requires_grad_(True)
    (layer.tv_denoise_color_weighted_unrolled(ft.detach(), at.detach(), w2, maxiter=30) * gt).sum().backward()
    assert torch.equal(w2.grad, wt.grad)


def test_a_mask_per_colour_image_gets_its_gradient_summed_over_the_channels(gpu_solver_cls, layer):
    name = "2x3x17x33"
    B, Cc, N, M = cw.SHAPES[name]
    f, gu, alpha, _, ft, at, _, gt = _tensors(name, "scalar", "mask")
    m = (np.random.default_rng(31).random((B, 1, N, M)) > 0.3).astype(np.float64)
    mt = torch.tensor(m, device="cuda", requires_grad=True)
    u = layer.tv_denoise_color_weighted_unrolled(ft, at, mt.expand_as(ft).contiguous(), maxiter=30)
    (u * gt).sum().backward()
    w = np.ascontiguousarray(np.broadcast_to(m, (B, Cc, N, M))).reshape(B * Cc, N, M)
    s = gpu_solver_cls(M, N, B * Cc)
    s.set_data(f, f)
    u0 = s.color_weighted_unrolled_denoise(alpha, Cc, w, maxiter=30)
    gf0, ga0, gw0 = s.color_weighted_unrolled_vjp(alpha, Cc, w, gu, maxiter=30)
    s.close()
    assert _same(u.detach().cpu().numpy().reshape(u0.shape), u0) and _same(ft.grad.cpu().numpy().reshape(gf0.shape), gf0)
    assert tuple(mt.grad.shape) == (B, 1, N, M)
    g = torch.tensor(gw0.reshape(B, Cc, N, M)).sum(dim=1, keepdim=True).numpy()      # autograd's reduction, on the ABI's planes
    d = float(np.abs(mt.grad.cpu().numpy() - g).max())
    assert d <= 4 * np.finfo(np.float64).eps * float(np.abs(gw0).max()) * Cc, d      # (a sum of C terms, in either order)


def test_central_differences_in_alpha_and_in_w(layer):
    """1x3x8x9, maxiter = 20, a masked image: d/dalpha and the directional derivative along a random dw on the kept pixels
    (gamma = min w = 0 stays, so the step table does) of L = <u, gu>, against central differences of the layer's own output
    with h = 1e-6, to 1e-5 relative."""
    from conftest import synth_batch
    N, M, Cc, K, h = 8, 9, 3, 20, 1e-6
    _, f = synth_batch(Cc, N, M, seed=14)
    rng = np.random.default_rng(15)
    gu = rng.standard_normal((1, Cc, N, M))
    w = cw.weight_of("mask", 1, Cc, N, M)
    assert w.min() == 0.0 and w.max() == 1.0
    dw = rng.standard_normal((N, M)) * w
    ft, gt = torch.tensor(f.reshape(1, Cc, N, M), device="cuda"), torch.tensor(gu, device="cuda")
    at = torch.tensor(0.08, dtype=torch.float64, device="cuda", requires_grad=True)
    wt = torch.tensor(w, device="cuda", requires_grad=True)
    dwt = torch.tensor(dw, device="cuda")
    loss = lambda a, w_: float((layer.tv_denoise_color_weighted_unrolled(ft, a, w_, maxiter=K) * gt).sum())
    (layer.tv_denoise_color_weighted_unrolled(ft, at, wt, maxiter=K) * gt).sum().backward()
    a0, w0 = at.detach(), wt.detach()
    for what, g, fd in (("alpha", float(at.grad), (loss(a0 + h, w0) - loss(a0 - h, w0)) / (2 * h)),
                        ("w", float((wt.grad * dwt).sum()), (loss(a0, w0 + h * dwt) - loss(a0, w0 - h * dwt)) / (2 * h))):
        print("%s: autograd %.10g central difference %.10g rel %.2e" % (what, g, fd, abs(g - fd) / abs(fd)))
        assert abs(g - fd) <= 1e-5 * abs(fd)
