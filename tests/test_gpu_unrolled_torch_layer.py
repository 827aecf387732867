"""tv_denoise_unrolled / TVDenoiseUnrolled on the GPU: f.grad and alpha.grad of a 50-iteration layer against torch autograd
through a CPU restatement of the same iterations (tests/unrolled_ref.torch_reference), the caller-owned tape (two forward
passes before two backward passes), one optimiser step, and tv_denoise's own implicit gradient left as it was."""
import numpy as np
import pytest
from conftest import synth_batch

import unrolled_ref as ur
from oracle import np_twin as tw

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

O, N, M, K = 2, 17, 33, 50


def _alpha(kind):
    if kind == "scalar":
        return np.float64(0.08)
    if kind == "patch":
        return np.array([[0.05, 0.1, 0.07], [0.12, 0.06, 0.09]])
    return 0.05 + 0.1 * np.random.default_rng(8).random((N, M))


def _case():
    ub, f = synth_batch(O, N, M, seed=5 + M)
    return ub, f


def _run(layer, f, alpha, ub, **kw):
    ft = torch.tensor(f, device="cuda", requires_grad=True)
    at = torch.tensor(alpha, dtype=torch.float64, device="cuda", requires_grad=True)
    u = layer(ft, at, **kw)
    ((u - torch.tensor(ub, device="cuda")) ** 2).sum().backward()
    return u.detach().cpu().numpy(), ft.grad.cpu().numpy(), at.grad.cpu().numpy()


@pytest.mark.parametrize("kind", ["scalar", "patch", "map"])
def test_gradients_match_torch_autograd_through_the_iterations(gpu_solver_cls, kind):
    from bpldenoising_amd.torch_layer import tv_denoise_unrolled, tv_denoise
    ub, f = _case()
    alpha = _alpha(kind)
    amap = tw.alpha_to_map(alpha, M, N)
    u, gf, ga = _run(tv_denoise_unrolled, f, alpha, ub, maxiter=K)
    assert ga.shape == np.shape(alpha)
    u0 = tw.pdhg_denoise(f, alpha, maxiter=K)
    gf0, ga0 = ur.torch_reference(f, amap, K, 2.0 * (u0 - ub))
    # the bound of tests/test_gpu_unrolled.py: per-pixel terms of the reference (summed over the images here) times the
    # number of pixels summed into one entry
    bf = 1e-11 * float(np.abs(gf0).max())
    ba = 1e-11 * float(np.abs(ga0).max()) * ur.pixels_per_entry(alpha, M, N)
    ga_ref = np.asarray(ur.reduce_alpha(ga0[None], alpha))
    df, da = float(np.abs(gf - gf0).max()), float(np.abs(ga - ga_ref).max())
    print("%s: max|du| %.2e grad_f %.2e (bound %.2e) grad_alpha %.2e (bound %.2e)" % (kind, float(np.abs(u - u0).max()), df, bf, da, ba))
    assert float(np.abs(u - u0).max()) <= 1e-13
    assert df <= bf and da <= ba
    # the same forward value as tv_denoise, bit for bit, and another gradient: the implicit one
    u1, gf1, ga1 = _run(tv_denoise, f, alpha, ub, maxiter=K)
    assert np.array_equal(u1, u)
    assert not np.array_equal(ga1, ga)


def test_two_forward_passes_keep_their_own_tapes(gpu_solver_cls):
    from bpldenoising_amd.torch_layer import tv_denoise_unrolled
    ub, f = _case()
    f2 = np.ascontiguousarray(f[::-1])
    a1, a2 = np.float64(0.08), np.float64(0.05)
    sep1 = _run(tv_denoise_unrolled, f, a1, ub, maxiter=K)
    sep2 = _run(tv_denoise_unrolled, f2, a2, ub, maxiter=K)
    ubt = torch.tensor(ub, device="cuda")
    t = [torch.tensor(x, device="cuda", requires_grad=True) for x in (f, a1, f2, a2)]
    u1 = tv_denoise_unrolled(t[0], t[1], maxiter=K)
    u2 = tv_denoise_unrolled(t[2], t[3], maxiter=K)       # the same handle, before the first backward pass
    ((u1 - ubt) ** 2).sum().backward()
    ((u2 - ubt) ** 2).sum().backward()
    assert np.array_equal(t[0].grad.cpu().numpy(), sep1[1]) and np.array_equal(t[1].grad.cpu().numpy(), sep1[2])
    assert np.array_equal(t[2].grad.cpu().numpy(), sep2[1]) and np.array_equal(t[3].grad.cpu().numpy(), sep2[2])


def test_module_takes_an_optimiser_step(gpu_solver_cls):
    from bpldenoising_amd.torch_layer import TVDenoiseUnrolled
    ub, f = _case()
    layer = TVDenoiseUnrolled(0.02, maxiter=K).to("cuda")
    opt = torch.optim.SGD(layer.parameters(), lr=1e-4)
    ft, ubt = torch.tensor(f, device="cuda"), torch.tensor(ub, device="cuda")
    loss0 = ((layer(ft) - ubt) ** 2).sum()
    loss0.backward()
    g = float(layer.alpha.grad)
    assert np.isfinite(g) and g != 0.0
    opt.step()
    assert float(layer.alpha.detach()) == pytest.approx(0.02 - 1e-4 * g, abs=1e-15)
    loss1 = ((layer(ft) - ubt) ** 2).sum()
    assert float(loss1) < float(loss0)          # a small step along the exact gradient of this very map
    import torch.autograd.forward_ad as fwd
    with fwd.dual_level():                      # no forward mode: torch's own "not implemented" error
        with pytest.raises((NotImplementedError, RuntimeError)):
            layer(fwd.make_dual(ft, torch.ones_like(ft)))


def test_tv_denoise_keeps_its_implicit_gradient(gpu_solver_cls):
    """tv_denoise before and after unrolled calls on the same cached handle: the same bits, and bpltv_vjp's own."""
    from bpldenoising_amd.torch_layer import tv_denoise, tv_denoise_unrolled
    ub, f = _case()
    alpha = _alpha("patch")
    before = _run(tv_denoise, f, alpha, ub, maxiter=K)
    _run(tv_denoise_unrolled, f, alpha, ub, maxiter=K)
    after = _run(tv_denoise, f, alpha, ub, maxiter=K)
    for a, b in zip(before, after):
        assert np.array_equal(a, b)
    s = gpu_solver_cls(M, N, O)
    s.set_data(f, f)
    u = s.denoise(alpha, maxiter=K)
    gf, ga = s.vjp(u, alpha, 2.0 * (u - ub), maxiter=K)
    assert np.array_equal(before[0], u) and np.array_equal(before[1], gf) and np.array_equal(before[2], ga)
    s.close()
