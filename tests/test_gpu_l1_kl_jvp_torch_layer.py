"""tv_l1_denoise_unrolled_fwd and tv_kl_denoise_unrolled_fwd on the GPU: the tangent under
torch.autograd.forward_ad -- in f, alpha and w, singly and together -- is TVSolver.l1_unrolled_jvp_device's /
kl_unrolled_jvp_device's bit for bit; a missing tangent reaches the library as NULL, and no tangent at all makes no library call;
backward of the _fwd function is the base function's, with and without checkpoint_every; the modules with forward_mode=True work
under forward_ad and still train alpha and w by backward; and the base functions still carry no jvp."""
import numpy as np
import pytest

import l1_kl_jvp_ref as j

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
import torch.autograd.forward_ad as fwd  # noqa: E402

NAME, K = "2x17x33", 50
O, N, M = j.GPU_SHAPES[NAME]
MODELS = j.MODELS


def _fn(model, fwd_mode=True):
    from bpldenoising_amd import torch_layer
    return getattr(torch_layer, "tv_%s_denoise_unrolled%s" % (model, "_fwd" if fwd_mode else ""))


def _case(model, kind):
    """(f, gu, alpha, w, df, dalpha, dw): the model's data on 2 x 17 x 33, w a mask (one plane), standard-normal tangents."""
    ref = j.REF[model]
    f, gu = ref.gpu_data(NAME)
    alpha = np.float64(ref.alpha_of("scalar", N, M)) if kind == "scalar" else ref.alpha_of(kind, N, M)
    w = ref.weight_of("mask", O, N, M)
    assert w.min() == 0.0 and w.shape == (N, M)
    rng = np.random.default_rng(77)
    return f, gu, alpha, w, rng.standard_normal(f.shape), rng.standard_normal(np.shape(alpha)), rng.standard_normal(w.shape)


def _dual(x, t):
    xt = torch.tensor(x, dtype=torch.float64, device="cuda")
    return xt if t is None else fwd.make_dual(xt, torch.tensor(t, dtype=torch.float64, device="cuda"))


COMBOS = ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 1))


@pytest.mark.parametrize("kind", ["scalar", "patch", "map"])
@pytest.mark.parametrize("model", MODELS)
def test_forward_mode_is_the_library_s_tangent_sweep(gpu_solver_cls, model, kind):
    f, _, alpha, w, df, da, dw = _case(model, kind)
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
            u = _fn(model)(_dual(f, tf), _dual(alpha, ta), _dual(w, tw_), maxiter=K)
            up, du = fwd.unpack_dual(u)
            up, du = up.cpu().numpy(), du.cpu().numpy()
        dft, dat, dwt = dev(tf), dev(ta), dev(tw_)
        dud, ud = torch.zeros(O, N, M, dtype=torch.float64, device="cuda"), torch.zeros(O, N, M, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        getattr(s, "%s_unrolled_jvp_device" % model)(wt.data_ptr(), 1, at.data_ptr(), am, an, ptr(dft), ptr(dat), ptr(dwt), dud.data_ptr(),
                                                     ud.data_ptr(), ndir=1, maxiter=K)
        assert np.array_equal(up, ud.cpu().numpy()) and np.array_equal(du, dud.cpu().numpy()), (cf, ca, cw)
        assert np.isfinite(du).all() and du.any()
        assert np.array_equal(up, getattr(s, "%s_denoise" % model)(alpha, w, maxiter=K))
    s.close()


@pytest.mark.parametrize("model", MODELS)
def test_a_missing_tangent_reaches_the_library_as_null_and_checkpoints_do_not_reach_the_sweep(gpu_solver_cls, monkeypatch, model):
    from bpldenoising_amd import TVSolver
    f, _, alpha, w, df, da, dw = _case(model, "patch")
    seen = []
    entry = "%s_unrolled_jvp_device" % model
    real = getattr(TVSolver, entry)

    def spy(self, w_ptr, wo, alpha_ptr, am, an, df_ptr, dalpha_ptr, dw_ptr, du_ptr, u_ptr=None, **kw):
        seen.append((df_ptr is None, dalpha_ptr is None, dw_ptr is None, kw))
        return real(self, w_ptr, wo, alpha_ptr, am, an, df_ptr, dalpha_ptr, dw_ptr, du_ptr, u_ptr, **kw)
    monkeypatch.setattr(TVSolver, entry, spy)
    by_spacing = {}
    with fwd.dual_level():
        for c in (None, 7, -1):
            for cf, ca, cw in COMBOS:
                u = _fn(model)(_dual(f, df if cf else None), _dual(alpha, da if ca else None), _dual(w, dw if cw else None), maxiter=K,
                               checkpoint_every=c)
                du = fwd.unpack_dual(u).tangent
                assert du is not None and bool(du.any())
                by_spacing.setdefault((cf, ca, cw), []).append(du.cpu().numpy())
        n = len(seen)
        u = _fn(model)(_dual(f, None), _dual(alpha, None), _dual(w, None), maxiter=K)
        assert fwd.unpack_dual(u).tangent is None and len(seen) == n      # no tangent at all: no sweep, no library call
    assert [(a, b, c) for a, b, c, _ in seen] == [(not cf, not ca, not cw) for cf, ca, cw in COMBOS] * 3
    assert all(kw == {"ndir": 1, "maxiter": K} for *_, kw in seen)        # checkpoint_every does not get there
    for dus in by_spacing.values():                                       # ... and does not affect the jvp
        assert np.array_equal(dus[0], dus[1]) and np.array_equal(dus[0], dus[2])


def test_no_tangent_at_all_returns_zeros_without_a_library_call(gpu_solver_cls, monkeypatch):
    """The jvp itself, handed no tangent: zeros in u's shape, and the solver's entry is never reached."""
    from bpldenoising_amd import TVSolver, torch_layer
    f, _, alpha, w, _, _, _ = _case("l1", "scalar")
    for model, row in (("l1", torch_layer._L1_UNROLLED_FWD), ("kl", torch_layer._KL_UNROLLED_FWD)):
        def refuse(*a, **k):
            raise AssertionError("the library was called")
        monkeypatch.setattr(TVSolver, row.jvp, refuse)

        class Ctx:
            saved_tensors = tuple(torch.tensor(x, dtype=torch.float64, device="cuda") for x in (np.abs(f), alpha, w))
        out = torch_layer._jvp(row, Ctx, None, None, None)
        assert out.shape == (O, N, M) and not bool(out.any())


@pytest.mark.parametrize("model", MODELS)
def test_backward_is_the_base_function_s(gpu_solver_cls, model):
    f, gu, alpha, w, _, _, _ = _case(model, "patch")
    gut = torch.tensor(gu, device="cuda")

    def run(fwd_mode, **kw):
        ft = torch.tensor(f, device="cuda", requires_grad=True)
        at = torch.tensor(alpha, dtype=torch.float64, device="cuda", requires_grad=True)
        wt = torch.tensor(w, device="cuda", requires_grad=True)
        u = _fn(model, fwd_mode)(ft, at, wt, maxiter=K, **kw)
        (u * gut).sum().backward()
        return u.detach().cpu().numpy(), ft.grad.cpu().numpy(), at.grad.cpu().numpy(), wt.grad.cpu().numpy()
    plain = run(False)
    assert all(np.isfinite(g).all() and g.any() for g in plain)
    for kw in (dict(), dict(checkpoint_every=7)):
        for a, b in zip(plain, run(True, **kw)):
            assert np.array_equal(a, b), kw
        for a, b in zip(plain, run(False, **kw)):
            assert np.array_equal(a, b), kw


@pytest.mark.parametrize("model", MODELS)
def test_the_module_with_forward_mode_works_under_forward_ad_and_still_trains(gpu_solver_cls, model):
    from bpldenoising_amd import torch_layer
    f, gu, alpha, w, df, _, _ = _case(model, "scalar")
    cls = torch_layer.TVL1DenoiseUnrolled if model == "l1" else torch_layer.TVKLDenoiseUnrolled
    mod = cls(float(alpha), w, maxiter=K, learn_w=True, forward_mode=True).to("cuda")
    base = cls(float(alpha), w, maxiter=K, learn_w=True).to("cuda")
    ft = torch.tensor(f, device="cuda")
    gut = torch.tensor(gu, device="cuda")
    with fwd.dual_level():
        u = mod(fwd.make_dual(ft, torch.tensor(df, device="cuda")))
        up, du = fwd.unpack_dual(u)
        assert du is not None and bool(du.any()) and bool(torch.isfinite(du).all())
        with torch.no_grad():
            assert torch.equal(up, _fn(model)(ft, mod.alpha, mod.w, maxiter=K))
        with pytest.raises((NotImplementedError, RuntimeError)):   # the module without the flag runs the base function: no jvp
            base(fwd.make_dual(ft, torch.tensor(df, device="cuda")))
    grads = []
    for m in (mod, base):
        (m(ft) * gut).sum().backward()
        assert m.alpha.grad is not None and m.w.grad is not None
        grads.append((m.alpha.grad.cpu().numpy(), m.w.grad.cpu().numpy()))
    for a, b in zip(*grads):
        assert np.array_equal(a, b) and np.isfinite(a).all() and a.any()
    opt = torch.optim.SGD(mod.parameters(), lr=1e-3)
    a0, w0 = mod.alpha.detach().clone(), mod.w.detach().clone()
    opt.step()
    assert not torch.equal(mod.alpha.detach(), a0) and not torch.equal(mod.w.detach(), w0)


@pytest.mark.parametrize("model", MODELS)
def test_the_base_function_still_has_no_forward_mode(gpu_solver_cls, model):
    f, _, alpha, w, df, _, dw = _case(model, "scalar")
    ft, at, wt = (torch.tensor(x, dtype=torch.float64, device="cuda") for x in (f, alpha, w))
    with fwd.dual_level():
        with pytest.raises((NotImplementedError, RuntimeError)):
            _fn(model, False)(fwd.make_dual(ft, torch.tensor(df, device="cuda")), at, wt, maxiter=K)
        with pytest.raises((NotImplementedError, RuntimeError)):
            _fn(model, False)(ft, at, fwd.make_dual(wt, torch.tensor(dw, device="cuda")), maxiter=K, forward_mode=False)
    with pytest.raises(ValueError, match="does not exist; tv_%s_denoise_unrolled_fwd" % model):
        _fn(model, False)(ft, at, wt, maxiter=K, forward_mode=True)
