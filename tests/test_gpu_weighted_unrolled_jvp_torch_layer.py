"""tv_denoise_weighted_unrolled(..., forward_mode=True) on the GPU, with a mask for w: the tangent under
torch.autograd.forward_ad -- in f, alpha and w, singly and together -- is TVSolver.weighted_unrolled_jvp_device's bit for bit;
a missing tangent reaches the library as NULL; backward of the same function is the default function's; checkpoint_every
does not reach the tangent sweep; and the default function still carries no jvp."""
import numpy as np
import pytest

import weighted_unrolled_ref as wur

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
import torch.autograd.forward_ad as fwd  # noqa: E402

NAME, K = "2x17x33", 50
O, N, M = wur.GPU_SHAPES[NAME]


def _case(kind):
    """(f, gu, alpha, w, df, dalpha, dw): w a mask (one plane), standard-normal tangents."""
    f, gu = wur.gpu_data(NAME)
    alpha = np.float64(0.08) if kind == "scalar" else wur.alpha_of(kind, N, M)
    w = wur.weight_of("mask", O, N, M)
    assert w.min() == 0.0 and w.shape == (N, M)
    rng = np.random.default_rng(77)
    return f, gu, alpha, w, rng.standard_normal(f.shape), rng.standard_normal(np.shape(alpha)), rng.standard_normal(w.shape)


def _dual(x, t):
    xt = torch.tensor(x, dtype=torch.float64, device="cuda")
    return xt if t is None else fwd.make_dual(xt, torch.tensor(t, dtype=torch.float64, device="cuda"))


COMBOS = ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 1))


@pytest.mark.parametrize("kind", ["scalar", "patch", "map"])
def test_forward_mode_is_the_library_s_tangent_sweep(gpu_solver_cls, kind):
    from bpldenoising_amd.torch_layer import tv_denoise_weighted_unrolled
    f, _, alpha, w, df, da, dw = _case(kind)
    a = np.atleast_1d(np.asarray(alpha, dtype=np.float64))
    an, am = (1, 1) if kind == "scalar" else a.shape
    s = gpu_solver_cls(M, N, O)
    s.set_data(f, f)
    dev = lambda x: None if x is None else torch.tensor(x, dtype=torch.float64, device="cuda")
    ptr = lambda t: None if t is None else t.data_ptr()
    at, wt = dev(a), dev(w)
    for cf, ca, cw in COMBOS:
        tf, ta, tw_ = (df if cf else None), (da if ca else None), (dw if cw else None)
        with fwd.dual_level():
            u = tv_denoise_weighted_unrolled(_dual(f, tf), _dual(alpha, ta), _dual(w, tw_), maxiter=K, forward_mode=True)
            up, du = fwd.unpack_dual(u)
            up, du = up.cpu().numpy(), du.cpu().numpy()
        dft, dat, dwt = dev(tf), dev(ta), dev(tw_)
        dud, ud = torch.zeros(O, N, M, dtype=torch.float64, device="cuda"), torch.zeros(O, N, M, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        s.weighted_unrolled_jvp_device(wt.data_ptr(), 1, at.data_ptr(), am, an, ptr(dft), ptr(dat), ptr(dwt), dud.data_ptr(),
                                       ud.data_ptr(), ndir=1, maxiter=K)
        assert np.array_equal(up, ud.cpu().numpy()) and np.array_equal(du, dud.cpu().numpy()), (cf, ca, cw)
        assert np.isfinite(du).all() and du.any()
        assert np.array_equal(up, s.weighted_denoise(alpha, w, maxiter=K))
    s.close()


def test_a_missing_tangent_reaches_the_library_as_null_and_checkpoints_do_not_reach_the_sweep(gpu_solver_cls, monkeypatch):
    from bpldenoising_amd import TVSolver
    from bpldenoising_amd.torch_layer import tv_denoise_weighted_unrolled
    f, _, alpha, w, df, da, dw = _case("patch")
    seen = []
    real = TVSolver.weighted_unrolled_jvp_device

    def spy(self, w_ptr, wo, alpha_ptr, am, an, df_ptr, dalpha_ptr, dw_ptr, du_ptr, u_ptr=None, **kw):
        seen.append((df_ptr is None, dalpha_ptr is None, dw_ptr is None, kw))
        return real(self, w_ptr, wo, alpha_ptr, am, an, df_ptr, dalpha_ptr, dw_ptr, du_ptr, u_ptr, **kw)
    monkeypatch.setattr(TVSolver, "weighted_unrolled_jvp_device", spy)
    by_spacing = {}
    with fwd.dual_level():
        for c in (None, 7, -1):
            for cf, ca, cw in COMBOS:
                u = tv_denoise_weighted_unrolled(_dual(f, df if cf else None), _dual(alpha, da if ca else None),
                                                 _dual(w, dw if cw else None), maxiter=K, forward_mode=True, checkpoint_every=c)
                du = fwd.unpack_dual(u).tangent
                assert du is not None and bool(du.any())
                by_spacing.setdefault((cf, ca, cw), []).append(du.cpu().numpy())
        u = tv_denoise_weighted_unrolled(_dual(f, None), _dual(alpha, None), _dual(w, None), maxiter=K, forward_mode=True)
        assert fwd.unpack_dual(u).tangent is None               # no tangent at all: no sweep
    assert [(a, b, c) for a, b, c, _ in seen] == [(not cf, not ca, not cw) for cf, ca, cw in COMBOS] * 3
    assert all(kw == {"ndir": 1, "maxiter": K} for *_, kw in seen)   # neither forward_mode nor checkpoint_every gets there
    for dus in by_spacing.values():                                  # checkpoint_every does not affect the jvp
        assert np.array_equal(dus[0], dus[1]) and np.array_equal(dus[0], dus[2])


def test_backward_is_the_default_function_s(gpu_solver_cls):
    from bpldenoising_amd.torch_layer import tv_denoise_weighted_unrolled
    f, gu, alpha, w, _, _, _ = _case("patch")
    gut = torch.tensor(gu, device="cuda")

    def run(**kw):
        ft = torch.tensor(f, device="cuda", requires_grad=True)
        at = torch.tensor(alpha, dtype=torch.float64, device="cuda", requires_grad=True)
        wt = torch.tensor(w, device="cuda", requires_grad=True)
        u = tv_denoise_weighted_unrolled(ft, at, wt, maxiter=K, **kw)
        (u * gut).sum().backward()
        return u.detach().cpu().numpy(), ft.grad.cpu().numpy(), at.grad.cpu().numpy(), wt.grad.cpu().numpy()
    plain = run()
    assert all(np.isfinite(g).all() and g.any() for g in plain)
    for kw in (dict(forward_mode=True), dict(forward_mode=True, checkpoint_every=7)):
        for a, b in zip(plain, run(**kw)):
            assert np.array_equal(a, b), kw


def test_the_default_function_still_has_no_forward_mode(gpu_solver_cls):
    from bpldenoising_amd.torch_layer import tv_denoise_weighted_unrolled
    f, _, alpha, w, df, _, dw = _case("scalar")
    ft, at, wt = (torch.tensor(x, dtype=torch.float64, device="cuda") for x in (f, alpha, w))
    with fwd.dual_level():
        with pytest.raises((NotImplementedError, RuntimeError)):
            tv_denoise_weighted_unrolled(fwd.make_dual(ft, torch.tensor(df, device="cuda")), at, wt, maxiter=K)
        with pytest.raises((NotImplementedError, RuntimeError)):
            tv_denoise_weighted_unrolled(ft, at, fwd.make_dual(wt, torch.tensor(dw, device="cuda")), maxiter=K, forward_mode=False)
