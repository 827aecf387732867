"""sumregs_denoise_unrolled, sumregs_denoise_unrolled_each and SumRegsDenoiseUnrolled on the GPU: loss.backward() gives the
solver calls' gradients bit for bit, a directional finite-difference check on the 24 x 28 case, two forward passes in one
graph keep their own tapes, a few Adam steps reduce the loss, and forward_mode=True raises."""
import numpy as np
import pytest
from conftest import synth_batch

import sumregs_unrolled_ref as sur

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

O, N, M, K = 2, 17, 33, 30


def _run(layer, f, alpha, ub, **kw):
    ft = torch.tensor(f, device="cuda", requires_grad=True)
    at = torch.tensor(alpha, dtype=torch.float64, device="cuda", requires_grad=True)
    u = layer(ft, at, **kw)
    (0.5 * (u - torch.tensor(ub, device="cuda")) ** 2).sum().backward()
    return u.detach().cpu().numpy(), ft.grad.cpu().numpy(), at.grad.cpu().numpy()


@pytest.mark.parametrize("kind", ["vector", "patch", "map", "zero"])
def test_backward_is_the_solver_s_vjp_bitwise(gpu_solver_cls, kind):
    from bpldenoising_amd.torch_layer import SumRegsDenoiseUnrolled, sumregs_denoise, sumregs_denoise_unrolled
    ub, f = synth_batch(O, N, M, seed=5 + M)
    alpha = sur.alpha_of(kind, N, M)
    u, gf, ga = _run(sumregs_denoise_unrolled, f, alpha, ub, maxiter=K)
    s = gpu_solver_cls(M, N, O)
    s.set_data(ub, f)
    u0 = s.sumregs_unrolled_denoise(alpha, maxiter=K)
    gf0, ga0 = s.sumregs_unrolled_vjp(alpha, u0 - ub, maxiter=K)
    s.close()
    assert np.array_equal(u, u0) and np.array_equal(gf, gf0) and np.array_equal(ga, ga0) and ga.shape == alpha.shape
    # the module: the same numbers through an nn.Parameter
    m = SumRegsDenoiseUnrolled(alpha, maxiter=K).to("cuda")
    ft = torch.tensor(f, device="cuda", requires_grad=True)
    um = m(ft)
    (0.5 * (um - torch.tensor(ub, device="cuda")) ** 2).sum().backward()
    assert np.array_equal(um.detach().cpu().numpy(), u0) and np.array_equal(m.alpha.grad.cpu().numpy(), ga0)
    assert np.array_equal(ft.grad.cpu().numpy(), gf0)
    # the same forward value as the implicit layer, bit for bit, and another gradient
    if kind != "zero":
        u1, _, ga1 = _run(sumregs_denoise, f, alpha, ub, maxiter=K)
        assert np.array_equal(u1, u) and not np.array_equal(ga1, ga)


@pytest.mark.parametrize("kind", ["vector", "patch"])
def test_each_backward_is_the_solver_s_vjp_each_bitwise(gpu_solver_cls, kind):
    from bpldenoising_amd.torch_layer import sumregs_denoise_unrolled_each
    ub, f = synth_batch(O, N, M, seed=5 + M)
    a0 = sur.alpha_of(kind, N, M)
    blocks = np.stack([a0, 1.5 * a0])
    u, gf, ga = _run(sumregs_denoise_unrolled_each, f, blocks, ub, maxiter=K)
    s = gpu_solver_cls(M, N, O)
    s.set_data(ub, f)
    u0 = s.sumregs_unrolled_denoise_each(blocks, maxiter=K)
    gf0, ga0 = s.sumregs_unrolled_vjp_each(blocks, u0 - ub, maxiter=K)
    s.close()
    assert np.array_equal(u, u0) and np.array_equal(gf, gf0) and np.array_equal(ga, ga0) and ga.shape == blocks.shape
    assert not np.array_equal(ga[0], ga[1])


@pytest.mark.parametrize("Kfd", [30, 300])
def test_directional_finite_differences(gpu_solver_cls, Kfd):
    """d/dt loss(f + t df, alpha + t da) on the 24 x 28 case, h = 1e-7, against <f.grad, df> + <alpha.grad, da>: relative 1e-5,
    the margin of tests/test_gpu_sumregs_unrolled.py's device check."""
    from bpldenoising_amd.torch_layer import sumregs_denoise_unrolled
    ub, f, alpha, h = sur.fd_case()
    rng = np.random.default_rng(31)
    df, da = rng.standard_normal(f.shape), np.array([0.6, -0.8, 0.5])
    ubt = torch.tensor(ub, device="cuda")

    def loss(ff, aa):
        with torch.no_grad():
            u = sumregs_denoise_unrolled(torch.tensor(ff, device="cuda"), torch.tensor(aa, device="cuda"), maxiter=Kfd)
            return float((0.5 * (u - ubt) ** 2).sum())
    _, gf, ga = _run(sumregs_denoise_unrolled, f, alpha, ub, maxiter=Kfd)
    for what, g, fd in (("alpha", float((ga * da).sum()), (loss(f, alpha + h * da) - loss(f, alpha - h * da)) / (2 * h)),
                        ("f", float((gf * df).sum()), (loss(f + h * df, alpha) - loss(f - h * df, alpha)) / (2 * h))):
        rel = abs(g - fd) / abs(fd)
        print("K %d, along d%s: backward %.10g central difference %.10g rel %.2e" % (Kfd, what, g, fd, rel))
        assert rel <= 1e-5, what


def test_two_forward_passes_keep_their_own_tapes(gpu_solver_cls):
    from bpldenoising_amd.torch_layer import sumregs_denoise_unrolled
    ub, f = synth_batch(O, N, M, seed=5 + M)
    a1, a2 = sur.alpha_of("vector", N, M), 0.5 * sur.alpha_of("vector", N, M)[::-1].copy()
    f2 = np.ascontiguousarray(f[::-1])
    sep1 = _run(sumregs_denoise_unrolled, f, a1, ub, maxiter=K)
    sep2 = _run(sumregs_denoise_unrolled, f2, a2, ub, maxiter=K)
    ubt = torch.tensor(ub, device="cuda")
    t = [torch.tensor(x, device="cuda", requires_grad=True) for x in (f, a1, f2, a2)]
    u1 = sumregs_denoise_unrolled(t[0], t[1], maxiter=K)
    u2 = sumregs_denoise_unrolled(t[2], t[3], maxiter=K)       # the same handle, before the first backward pass
    (0.5 * (u1 - ubt) ** 2).sum().backward()
    (0.5 * (u2 - ubt) ** 2).sum().backward()
    assert np.array_equal(t[0].grad.cpu().numpy(), sep1[1]) and np.array_equal(t[1].grad.cpu().numpy(), sep1[2])
    assert np.array_equal(t[2].grad.cpu().numpy(), sep2[1]) and np.array_equal(t[3].grad.cpu().numpy(), sep2[2])


def test_a_few_adam_steps_reduce_the_loss(gpu_solver_cls):
    from bpldenoising_amd.torch_layer import SumRegsDenoiseUnrolled
    ub, f = synth_batch(2, 16, 16, seed=3)
    ft, ubt = torch.tensor(f, device="cuda"), torch.tensor(ub, device="cuda")
    m = SumRegsDenoiseUnrolled([0.005, 0.005, 0.005], maxiter=30).to("cuda")
    opt = torch.optim.Adam(m.parameters(), lr=5e-3)
    losses = []
    for _ in range(6):
        opt.zero_grad()
        loss = (0.5 * (m(ft) - ubt) ** 2).sum()
        loss.backward()
        opt.step()
        with torch.no_grad():
            m.alpha.clamp_(min=0.0)
        losses.append(float(loss))
    print("losses", losses)
    assert losses[-1] < losses[0] and np.isfinite(losses).all()


def test_forward_mode_raises_a_value_error(gpu_solver_cls):
    from bpldenoising_amd.torch_layer import sumregs_denoise_unrolled, sumregs_denoise_unrolled_each
    ft = torch.zeros(2, 8, 6, dtype=torch.float64, device="cuda")
    a = torch.tensor([0.03, 0.02, 0.04], dtype=torch.float64, device="cuda")
    for call in (lambda: sumregs_denoise_unrolled(ft, a, maxiter=5, forward_mode=True),
                 lambda: sumregs_denoise_unrolled_each(ft, a.expand(2, 3).contiguous(), maxiter=5, forward_mode=True)):
        with pytest.raises(ValueError, match="forward_mode=True") as e:
            call()
        assert not isinstance(e.value, NotImplementedError)
