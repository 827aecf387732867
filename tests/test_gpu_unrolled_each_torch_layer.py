"""tv_denoise_unrolled_each on the GPU: f.grad and alpha.grad of a 30-iteration layer with one parameter per sample against
torch autograd through a CPU restatement of the same iterations (tests/unrolled_ref.torch_reference), sample by sample;
alpha.grad[k] independent of the other samples; the caller-owned tapes; forward mode; one Adam step of a small network that
predicts the parameters; and tv_denoise_unrolled / tv_denoise_each left as they were."""
import numpy as np
import pytest
from conftest import synth_batch

import unrolled_each_ref as ue
import unrolled_ref as ur
from oracle import np_twin as tw

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
fwd = pytest.importorskip("torch.autograd.forward_ad")

O, N, M, K = 2, 17, 33, 30


def _case(kind="scalar"):
    ub, f = synth_batch(O, N, M, seed=5 + M)
    return ub, f, ue.alphas_of(kind, O, N, M)


def _run(layer, f, alpha, ub, **kw):
    ft = torch.tensor(f, device="cuda", requires_grad=True)
    at = torch.tensor(alpha, dtype=torch.float64, device="cuda", requires_grad=True)
    u = layer(ft, at, **kw)
    ((u - torch.tensor(ub, device="cuda")) ** 2).sum().backward()
    return u.detach().cpu().numpy(), ft.grad.cpu().numpy(), at.grad.cpu().numpy()


@pytest.mark.parametrize("kind", ["scalar", "patch", "map"])
def test_gradients_match_torch_autograd_per_sample(gpu_solver_cls, kind):
    """The bounds of tests/test_gpu_unrolled_torch_layer.py, per sample: 1e-13 on u, 1e-11 * max|ref| on grad_f and
    1e-11 * max|ref per-pixel term| * pixels per entry on alpha.grad[k]."""
    from bpldenoising_amd.torch_layer import tv_denoise_unrolled_each, tv_denoise_each
    ub, f, alphas = _case(kind)
    u, gf, ga = _run(tv_denoise_unrolled_each, f, alphas, ub, maxiter=K)
    assert ga.shape == alphas.shape
    for k in range(O):
        a = alphas[k]
        amap = tw.alpha_to_map(a, M, N)
        u0 = tw.pdhg_denoise(f[k:k + 1], a, maxiter=K)
        gf0, ga0 = ur.torch_reference(f[k:k + 1], amap, K, 2.0 * (u0 - ub[k:k + 1]))
        bf = 1e-11 * float(np.abs(gf0).max())
        ba = 1e-11 * float(np.abs(ga0).max()) * ur.pixels_per_entry(a, M, N)
        ga_ref = np.asarray(ur.reduce_alpha(ga0[None], a))
        du, df, da = float(np.abs(u[k] - u0[0]).max()), float(np.abs(gf[k] - gf0[0]).max()), float(np.abs(ga[k] - ga_ref).max())
        print("%s sample %d: max|du| %.2e grad_f %.2e (bound %.2e) grad_alpha %.2e (bound %.2e)" % (kind, k, du, df, bf, da, ba))
        assert du <= 1e-13
        assert df <= bf and da <= ba
    # the same forward value as tv_denoise_each, bit for bit, and another gradient: the implicit one
    u1, _, ga1 = _run(tv_denoise_each, f, alphas, ub, maxiter=K)
    assert np.array_equal(u1, u)
    assert not np.array_equal(ga1, ga)


def test_a_sample_s_gradient_does_not_depend_on_the_other_samples(gpu_solver_cls):
    from bpldenoising_amd.torch_layer import tv_denoise_unrolled_each
    ub, f, alphas = _case("patch")
    _, gf, ga = _run(tv_denoise_unrolled_each, f, alphas, ub, maxiter=K)
    f2, ub2 = f.copy(), ub.copy()
    f2[1] = f[1, ::-1]            # another image in sample 1 ...
    _, gf2, ga2 = _run(tv_denoise_unrolled_each, f2, alphas, ub, maxiter=K)
    ub2[1] = 1.0 - ub[1]          # ... or another cotangent
    _, gf3, ga3 = _run(tv_denoise_unrolled_each, f, alphas, ub2, maxiter=K)
    for g in ((gf2, ga2), (gf3, ga3)):
        assert np.array_equal(g[0][0], gf[0]) and np.array_equal(g[1][0], ga[0])
        assert not np.array_equal(g[0][1], gf[1]) and not np.array_equal(g[1][1], ga[1])


def test_two_forward_passes_keep_their_own_tapes(gpu_solver_cls):
    from bpldenoising_amd.torch_layer import tv_denoise_unrolled_each
    ub, f, a1 = _case("scalar")
    f2 = np.ascontiguousarray(f[::-1])
    a2 = np.ascontiguousarray(a1[::-1]) * 0.5
    sep1 = _run(tv_denoise_unrolled_each, f, a1, ub, maxiter=K)
    sep2 = _run(tv_denoise_unrolled_each, f2, a2, ub, maxiter=K)
    ubt = torch.tensor(ub, device="cuda")
    t = [torch.tensor(x, device="cuda", requires_grad=True) for x in (f, a1, f2, a2)]
    u1 = tv_denoise_unrolled_each(t[0], t[1], maxiter=K)
    u2 = tv_denoise_unrolled_each(t[2], t[3], maxiter=K)       # the same handle, before the first backward pass
    ((u1 - ubt) ** 2).sum().backward()
    ((u2 - ubt) ** 2).sum().backward()
    assert np.array_equal(t[0].grad.cpu().numpy(), sep1[1]) and np.array_equal(t[1].grad.cpu().numpy(), sep1[2])
    assert np.array_equal(t[2].grad.cpu().numpy(), sep2[1]) and np.array_equal(t[3].grad.cpu().numpy(), sep2[2])


@pytest.mark.parametrize("kind", ["scalar", "map"])
def test_forward_mode_is_the_library_s_tangent_sweep_and_backward_still_works(gpu_solver_cls, kind):
    from bpldenoising_amd.torch_layer import tv_denoise_unrolled_each
    ub, f, alphas = _case(kind)
    rng = np.random.default_rng(77)
    df, da = rng.standard_normal(f.shape), rng.standard_normal(alphas.shape)
    s = gpu_solver_cls(M, N, O)
    s.set_data(f, f)

    def dual(x, t):
        xt = torch.tensor(x, dtype=torch.float64, device="cuda")
        return xt if t is None else fwd.make_dual(xt, torch.tensor(t, dtype=torch.float64, device="cuda"))
    for tf, ta in ((df, da), (df, None), (None, da)):
        with fwd.dual_level():
            up, du = fwd.unpack_dual(tv_denoise_unrolled_each(dual(f, tf), dual(alphas, ta), forward_mode=True, maxiter=K))
            up, du = up.cpu().numpy(), du.cpu().numpy()
        du_lib, u_lib = s.unrolled_jvp_each(alphas, df=tf, dalphas=ta, want_u=True, maxiter=K)
        assert np.array_equal(up, u_lib) and np.array_equal(du, du_lib)
    s.close()
    for a, b in zip(_run(tv_denoise_unrolled_each, f, alphas, ub, maxiter=K),
                    _run(tv_denoise_unrolled_each, f, alphas, ub, forward_mode=True, maxiter=K)):
        assert np.array_equal(a, b)


def test_the_default_function_has_no_forward_mode(gpu_solver_cls):
    from bpldenoising_amd.torch_layer import tv_denoise_unrolled_each
    _, f, alphas = _case("scalar")
    ft, at = torch.tensor(f, device="cuda"), torch.tensor(alphas, device="cuda")
    with fwd.dual_level():
        with pytest.raises((NotImplementedError, RuntimeError)):
            tv_denoise_unrolled_each(fwd.make_dual(ft, torch.ones_like(ft)), at, maxiter=K)
        with pytest.raises((NotImplementedError, RuntimeError)):
            tv_denoise_unrolled_each(ft, fwd.make_dual(at, torch.ones_like(at)), maxiter=K)


def test_a_network_that_predicts_the_parameters_takes_an_adam_step(gpu_solver_cls):
    from bpldenoising_amd.torch_layer import tv_denoise_unrolled_each
    ub, f, _ = _case()
    torch.manual_seed(3)
    net = torch.nn.Sequential(torch.nn.Conv2d(1, 4, 3, padding=1), torch.nn.Tanh(), torch.nn.Conv2d(4, 1, 3, padding=1)).double().to("cuda")
    opt = torch.optim.Adam(net.parameters(), lr=1e-3)
    ft, ubt = torch.tensor(f, device="cuda"), torch.tensor(ub, device="cuda")
    before = [p.detach().clone() for p in net.parameters()]
    alpha = 0.1 * torch.nn.functional.softplus(net(ft[:, None]).mean(dim=(1, 2, 3)))     # (B,): one parameter per sample
    assert alpha.shape == (O,)
    loss = ((tv_denoise_unrolled_each(ft, alpha, maxiter=K) - ubt) ** 2).sum()
    loss.backward()
    assert np.isfinite(float(loss.detach()))
    for p in net.parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and bool(p.grad.any())
    opt.step()
    assert all(not torch.equal(p.detach(), b) for p, b in zip(net.parameters(), before))


def test_the_other_layers_keep_their_results(gpu_solver_cls):
    """tv_denoise_unrolled and tv_denoise_each before and after per-image unrolled calls on the same cached handle."""
    from bpldenoising_amd.torch_layer import tv_denoise_each, tv_denoise_unrolled, tv_denoise_unrolled_each
    ub, f, alphas = _case("patch")
    shared = alphas[0]
    before = _run(tv_denoise_unrolled, f, shared, ub, maxiter=K), _run(tv_denoise_each, f, alphas, ub, maxiter=K)
    _run(tv_denoise_unrolled_each, f, alphas, ub, maxiter=K)
    after = _run(tv_denoise_unrolled, f, shared, ub, maxiter=K), _run(tv_denoise_each, f, alphas, ub, maxiter=K)
    for x, y in zip(before, after):
        for a, b in zip(x, y):
            assert np.array_equal(a, b)
    s = gpu_solver_cls(M, N, O)          # ... and they are the library's own calls
    s.set_data(f, f)
    u = s.unrolled_denoise(shared, maxiter=K)
    gf, ga = s.unrolled_vjp(shared, 2.0 * (u - ub), maxiter=K)
    assert np.array_equal(before[0][0], u) and np.array_equal(before[0][1], gf) and np.array_equal(before[0][2], ga)
    s.close()
