"""tv_denoise_unrolled(..., forward_mode=True) / TVDenoiseUnrolled(alpha, forward_mode=True) on the GPU: the tangent under
torch.autograd.forward_ad is TVSolver.unrolled_jvp_device's bit for bit and agrees with torch forward-mode AD through a CPU
restatement of the same iterations (tests/unrolled_jvp_ref.torch_forward_reference); backward of the same layer is the default
layer's; a missing tangent reaches the library as NULL; and the default layer still carries no jvp."""
import numpy as np
import pytest
from conftest import synth_batch

import unrolled_jvp_ref as uj
from oracle import np_twin as tw

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
import torch.autograd.forward_ad as fwd  # noqa: E402

O, N, M, K = 2, 17, 33, 50


def _alpha(kind):
    if kind == "scalar":
        return np.float64(0.08)
    if kind == "patch":
        return np.array([[0.05, 0.1, 0.07], [0.12, 0.06, 0.09]])
    return 0.05 + 0.1 * np.random.default_rng(8).random((N, M))


def _case(kind):
    ub, f = synth_batch(O, N, M, seed=5 + M)
    alpha = _alpha(kind)
    rng = np.random.default_rng(77)
    return ub, f, alpha, rng.standard_normal(f.shape), rng.standard_normal(np.shape(alpha))


def _dual(x, t):
    xt = torch.tensor(x, dtype=torch.float64, device="cuda")
    return xt if t is None else fwd.make_dual(xt, torch.tensor(t, dtype=torch.float64, device="cuda"))


@pytest.mark.parametrize("kind", ["scalar", "patch", "map"])
def test_forward_mode_is_the_library_s_tangent_sweep(gpu_solver_cls, kind):
    from bpldenoising_amd.torch_layer import tv_denoise_unrolled
    _, f, alpha, df, da = _case(kind)
    amap = tw.alpha_to_map(alpha, M, N)
    dam = np.full((N, M), float(da)) if kind == "scalar" else tw.alpha_to_map(da, M, N)
    s = gpu_solver_cls(M, N, O)
    s.set_data(f, f)
    for tf, ta, tam in ((df, da, dam), (df, None, None), (None, da, dam)):
        with fwd.dual_level():
            u = tv_denoise_unrolled(_dual(f, tf), _dual(alpha, ta), forward_mode=True, maxiter=K)
            up, du = fwd.unpack_dual(u)
            up, du = up.cpu().numpy(), du.cpu().numpy()
        du_lib, u_lib = s.unrolled_jvp(alpha, df=tf, dalpha=ta, want_u=True, maxiter=K)
        assert np.array_equal(up, u_lib) and np.array_equal(du, du_lib)
        _, du0 = uj.torch_forward_reference(f, amap, K, tf, tam)
        d, b = float(np.abs(du - du0).max()), 1e-11 * float(np.abs(du0).max())
        print("%s df %d dalpha %d: du %.2e (bound %.2e)" % (kind, tf is not None, ta is not None, d, b))
        assert d <= b
    s.close()


def test_a_missing_tangent_reaches_the_library_as_null(gpu_solver_cls, monkeypatch):
    from bpldenoising_amd import TVSolver
    from bpldenoising_amd.torch_layer import tv_denoise_unrolled
    _, f, alpha, df, da = _case("patch")
    seen = []
    real = TVSolver.unrolled_jvp_device

    def spy(self, alpha_ptr, am, an, df_ptr, dalpha_ptr, du_ptr, u_ptr=None, **kw):
        seen.append((df_ptr is None, dalpha_ptr is None, kw))
        return real(self, alpha_ptr, am, an, df_ptr, dalpha_ptr, du_ptr, u_ptr, **kw)
    monkeypatch.setattr(TVSolver, "unrolled_jvp_device", spy)
    with fwd.dual_level():
        for tf, ta in ((df, None), (None, da), (df, da)):
            du = fwd.unpack_dual(tv_denoise_unrolled(_dual(f, tf), _dual(alpha, ta), forward_mode=True, maxiter=K)).tangent
            assert du is not None and bool(du.any())
        u = tv_denoise_unrolled(_dual(f, None), _dual(alpha, None), forward_mode=True, maxiter=K)   # no tangent at all
        assert fwd.unpack_dual(u).tangent is None
    assert [(a, b) for a, b, _ in seen] == [(False, True), (True, False), (False, False)]
    assert all(kw == {"ndir": 1, "maxiter": K} for _, _, kw in seen)      # forward_mode is no solver parameter


def test_backward_is_the_default_layer_s(gpu_solver_cls):
    from bpldenoising_amd.torch_layer import TVDenoiseUnrolled, tv_denoise_unrolled
    ub, f, alpha, _, _ = _case("patch")
    ubt = torch.tensor(ub, device="cuda")

    def run(**kw):
        ft = torch.tensor(f, device="cuda", requires_grad=True)
        at = torch.tensor(alpha, dtype=torch.float64, device="cuda", requires_grad=True)
        u = tv_denoise_unrolled(ft, at, maxiter=K, **kw)
        ((u - ubt) ** 2).sum().backward()
        return u.detach().cpu().numpy(), ft.grad.cpu().numpy(), at.grad.cpu().numpy()
    for a, b in zip(run(), run(forward_mode=True)):
        assert np.array_equal(a, b)
    layer = TVDenoiseUnrolled(0.02, forward_mode=True, maxiter=K).to("cuda")
    ft = torch.tensor(f, device="cuda")
    ((layer(ft) - ubt) ** 2).sum().backward()
    g = float(layer.alpha.grad)
    assert np.isfinite(g) and g != 0.0
    with fwd.dual_level():                       # the module under forward mode: a tangent in f only
        du = fwd.unpack_dual(layer(fwd.make_dual(ft, torch.ones_like(ft)))).tangent
    assert du is not None and bool(torch.isfinite(du).all()) and bool(du.any())


def test_the_default_layer_still_has_no_forward_mode(gpu_solver_cls):
    from bpldenoising_amd.torch_layer import TVDenoiseUnrolled, tv_denoise_unrolled
    _, f, alpha, df, _ = _case("scalar")
    ft = torch.tensor(f, device="cuda")
    with fwd.dual_level():
        with pytest.raises((NotImplementedError, RuntimeError)):
            tv_denoise_unrolled(fwd.make_dual(ft, torch.tensor(df, device="cuda")), torch.tensor(alpha, device="cuda"), maxiter=K)
        with pytest.raises((NotImplementedError, RuntimeError)):
            TVDenoiseUnrolled(0.02, maxiter=K).to("cuda")(fwd.make_dual(ft, torch.ones_like(ft)))
