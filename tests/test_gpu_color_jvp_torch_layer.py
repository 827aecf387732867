"""tv_denoise_color_unrolled(..., forward_mode=True) / TVDenoiseColorUnrolled(alpha, forward_mode=True) on the GPU: under
torch.autograd.forward_ad the primal is the default path's bit for bit and the tangent TVSolver.color_unrolled_jvp's, for a
scalar, a patch and a map, (B, C, H, W) and (C, H, W) input, a tangent on f only, on alpha only and on both; backward of the same
function is the default path's; and the module works the same way."""
import numpy as np
import pytest

import color_jvp_ref as cj
import color_ref as cr

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
import torch.autograd.forward_ad as fwd  # noqa: E402

NAME, K = "2x3x17x33", 50


def _same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b))


@pytest.fixture
def layer(gpu_solver_cls):
    from bpldenoising_amd import torch_layer
    yield torch_layer
    torch_layer.clear_solvers()


def _dual(x, t):
    xt = torch.tensor(x, dtype=torch.float64, device="cuda")
    return xt if t is None else fwd.make_dual(xt, torch.tensor(t, dtype=torch.float64, device="cuda"))


@pytest.mark.parametrize("batched", [True, False])
@pytest.mark.parametrize("kind", cr.KINDS)
def test_forward_mode_is_the_library_s_tangent_sweep(gpu_solver_cls, layer, kind, batched):
    B, Cc, N, M = cr.SHAPES[NAME]
    f, _ = cr.gpu_data(NAME)
    df, da, _ = cj.tangents(NAME, kind)
    alpha = cr.alpha_of(kind, N, M)
    if not batched:                       # (C, H, W): the batch of one
        B, f, df = 1, f[:Cc], df[:Cc]
    shape = (B, Cc, N, M) if batched else (Cc, N, M)
    s = gpu_solver_cls(M, N, B * Cc)
    s.set_data(f, f)
    u_def = layer.tv_denoise_color_unrolled(torch.tensor(f.reshape(shape), device="cuda"),
                                            torch.tensor(alpha, dtype=torch.float64, device="cuda"), maxiter=K).cpu().numpy()
    for tf, ta in ((df, da), (df, None), (None, da)):
        with fwd.dual_level():
            u = layer.tv_denoise_color_unrolled(_dual(f.reshape(shape), None if tf is None else tf.reshape(shape)), _dual(alpha, ta),
                                                maxiter=K, forward_mode=True)
            up, du = fwd.unpack_dual(u)
            assert tuple(up.shape) == shape and tuple(du.shape) == shape
            up, du = up.cpu().numpy(), du.cpu().numpy()
        du_lib = s.color_unrolled_jvp(alpha, Cc, df=tf, dalpha=ta, maxiter=K)
        assert _same(up, u_def)
        assert _same(du.reshape(du_lib.shape), du_lib)
    s.close()


def test_backward_is_the_default_path_s_and_the_module_works_the_same_way(gpu_solver_cls, layer):
    B, Cc, N, M = cr.SHAPES[NAME]
    f, gu = cr.gpu_data(NAME)
    alpha = cr.alpha_of("patch", N, M)
    gt = torch.tensor(gu.reshape(B, Cc, N, M), device="cuda")

    def run(**kw):
        ft = torch.tensor(f.reshape(B, Cc, N, M), device="cuda", requires_grad=True)
        at = torch.tensor(alpha, dtype=torch.float64, device="cuda", requires_grad=True)
        u = layer.tv_denoise_color_unrolled(ft, at, maxiter=K, **kw)
        (u * gt).sum().backward()
        return u.detach().cpu().numpy(), ft.grad.cpu().numpy(), at.grad.cpu().numpy()
    for a, b in zip(run(), run(forward_mode=True)):
        assert _same(a, b)
    # the module: backward, and forward mode with a tangent on f and on its parameter
    mod = layer.TVDenoiseColorUnrolled(alpha, maxiter=K, forward_mode=True).to("cuda")
    ft = torch.tensor(f.reshape(B, Cc, N, M), device="cuda", requires_grad=True)
    (mod(ft) * gt).sum().backward()
    u0, gf0, ga0 = run()
    assert _same(ft.grad.cpu().numpy(), gf0) and _same(mod.alpha.grad.cpu().numpy(), ga0)
    df, da, _ = cj.tangents(NAME, "patch")
    s = gpu_solver_cls(M, N, B * Cc)
    s.set_data(f, f)
    du_lib = s.color_unrolled_jvp(alpha, Cc, df=df, maxiter=K)
    s.close()
    with fwd.dual_level():
        up, du = fwd.unpack_dual(mod(_dual(f.reshape(B, Cc, N, M), df.reshape(B, Cc, N, M))))
        assert _same(up.detach().cpu().numpy(), u0) and _same(du.detach().cpu().numpy().reshape(du_lib.shape), du_lib)
