"""tv_denoise_weighted_unrolled on the GPU: f.grad, alpha.grad and w.grad of a 50-iteration weighted layer -- with a real
weight and with a mask -- against torch autograd through a CPU restatement of the same iterations
(tests/weighted_unrolled_ref.torch_reference), the needs_input_grad subsets, the caller-owned tape (two forward passes before
two backward passes), and a few optimiser steps on alpha, f and w through a masked solve."""
import numpy as np
import pytest
from conftest import synth_batch

import unrolled_ref as ur
import weighted_ref as wr
import weighted_unrolled_ref as wur
from oracle import np_twin as tw

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

O, N, M, K = 2, 17, 33, 50


def _case():
    return synth_batch(O, N, M, seed=5 + M)


def _weight(wkind, per_image):
    """real / mask, as (H, W) or (B, H, W) (the mask then differs from image to image)."""
    if wkind == "real":
        w = wur.weight_of("real", O, N, M)
        return w if per_image else np.ascontiguousarray(w[0])
    if per_image:
        return (np.random.default_rng(12).random((O, N, M)) > 0.3).astype(np.float64)
    return wur.weight_of("mask", O, N, M)


def _run(f, alpha, w, ub, need=(True, True, True), **kw):
    from bpldenoising_amd.torch_layer import tv_denoise_weighted_unrolled
    ft = torch.tensor(f, device="cuda", requires_grad=need[0])
    at = torch.tensor(alpha, dtype=torch.float64, device="cuda", requires_grad=need[1])
    wt = torch.tensor(w, device="cuda", requires_grad=need[2])
    u = tv_denoise_weighted_unrolled(ft, at, wt, **kw)
    ((u - torch.tensor(ub, device="cuda")) ** 2).sum().backward()
    return (u.detach().cpu().numpy(),) + tuple(t.grad.cpu().numpy() if t.grad is not None else None for t in (ft, at, wt))


@pytest.mark.parametrize("per_image", [False, True])
@pytest.mark.parametrize("wkind", ["real", "mask"])
@pytest.mark.parametrize("kind", ["scalar", "map"])
def test_gradients_match_torch_autograd_through_the_iterations(gpu_solver_cls, kind, wkind, per_image):
    ub, f = _case()
    alpha = np.float64(0.08) if kind == "scalar" else wur.alpha_of("map", N, M)
    w = _weight(wkind, per_image)
    amap = tw.alpha_to_map(alpha, M, N)
    u, gf, ga, gw = _run(f, alpha, w, ub, maxiter=K)
    assert ga.shape == np.shape(alpha) and gw.shape == w.shape
    u0 = wr.pdhg(f, alpha, w, K)
    gf0, ga0, gw0 = wur.torch_reference(f, amap, w, K, 2.0 * (u0 - ub))
    # the twin bounds of tests/test_gpu_weighted_unrolled.py; the reference's grad_alpha and one-plane grad_w are already
    # summed over the images
    bf = 1e-11 * float(np.abs(gf0).max())
    ba = 1e-11 * float(np.abs(ga0).max()) * ur.pixels_per_entry(alpha, M, N)
    bw = 1e-11 * float(np.abs(gw0).max())
    ga_ref = np.asarray(ur.reduce_alpha(ga0[None], alpha))
    du, df, da, dw = (float(np.abs(a - b).max()) for a, b in ((u, u0), (gf, gf0), (ga, ga_ref), (gw, gw0)))
    print("%s %s %s: max|du| %.2e grad_f %.2e (bound %.2e) grad_alpha %.2e (bound %.2e) grad_w %.2e (bound %.2e)"
          % (kind, wkind, "(B,H,W)" if per_image else "(H,W)", du, df, bf, da, ba, dw, bw))
    assert du <= 1e-13
    assert df <= bf and da <= ba and dw <= bw
    if wkind == "real":   # the same forward value as tv_denoise_weighted, bit for bit
        from bpldenoising_amd.torch_layer import tv_denoise_weighted
        u1 = tv_denoise_weighted(torch.tensor(f, device="cuda"), torch.tensor(alpha, dtype=torch.float64, device="cuda"),
                                 torch.tensor(w, device="cuda"), maxiter=K)
        assert np.array_equal(u1.cpu().numpy(), u)


def test_needs_input_grad_subsets(gpu_solver_cls):
    ub, f = _case()
    alpha, w = np.float64(0.08), _weight("mask", False)
    full = _run(f, alpha, w, ub, maxiter=K)
    for need in ((True, False, False), (False, True, False), (False, False, True), (True, True, False), (False, True, True)):
        got = _run(f, alpha, w, ub, need=need, maxiter=K)
        assert np.array_equal(got[0], full[0])
        for wanted, g, g0 in zip(need, got[1:], full[1:]):
            assert (g is not None) == wanted
            if wanted:
                assert np.array_equal(g, g0), need
    from bpldenoising_amd.torch_layer import tv_denoise_weighted_unrolled
    t = [torch.tensor(x, device="cuda") for x in (f, alpha, w)]
    assert not tv_denoise_weighted_unrolled(*t, maxiter=K).requires_grad      # nothing asked for: no backward at all
    assert np.array_equal(tv_denoise_weighted_unrolled(*t).cpu().numpy(), full[0])   # maxiter defaults to 50


def test_two_forward_passes_keep_their_own_tapes(gpu_solver_cls):
    from bpldenoising_amd.torch_layer import tv_denoise_weighted_unrolled
    ub, f = _case()
    f2 = np.ascontiguousarray(f[::-1])
    a1, a2 = np.float64(0.08), np.float64(0.05)
    w1, w2 = _weight("mask", False), _weight("real", True)
    sep1 = _run(f, a1, w1, ub, maxiter=K)
    sep2 = _run(f2, a2, w2, ub, maxiter=K)
    ubt = torch.tensor(ub, device="cuda")
    t = [torch.tensor(x, device="cuda", requires_grad=True) for x in (f, a1, w1, f2, a2, w2)]
    u1 = tv_denoise_weighted_unrolled(t[0], t[1], t[2], maxiter=K)
    u2 = tv_denoise_weighted_unrolled(t[3], t[4], t[5], maxiter=K)       # the same handle, before the first backward pass
    ((u1 - ubt) ** 2).sum().backward()                                   # (its grad_w reads f, not the f2 now resident)
    ((u2 - ubt) ** 2).sum().backward()
    for k in range(3):
        assert np.array_equal(t[k].grad.cpu().numpy(), sep1[1 + k]), k
        assert np.array_equal(t[3 + k].grad.cpu().numpy(), sep2[1 + k]), k


def test_alpha_f_and_w_train_through_a_masked_solve(gpu_solver_cls):
    """Inpainting: a few SGD steps on alpha, f and the fidelity of the kept pixels lower the loss of this very map."""
    from bpldenoising_amd.torch_layer import tv_denoise_weighted_unrolled
    ub, f = _case()
    ubt = torch.tensor(ub, device="cuda")
    mask = torch.tensor(_weight("mask", False), device="cuda")
    ft = torch.tensor(f, device="cuda", requires_grad=True)
    at = torch.tensor(0.02, dtype=torch.float64, device="cuda", requires_grad=True)
    wt = mask.clone().requires_grad_(True)
    opt = torch.optim.SGD([{"params": [at], "lr": 1e-5}, {"params": [ft, wt], "lr": 1e-2}])
    losses = []
    for _ in range(4):
        opt.zero_grad()
        loss = ((tv_denoise_weighted_unrolled(ft, at, wt, maxiter=K) - ubt) ** 2).sum()
        loss.backward()
        for t in (ft, at, wt):
            assert t.grad is not None and bool(torch.isfinite(t.grad).all()) and bool((t.grad != 0).any())
        wt.grad *= mask                       # the masked pixels stay masked (w = 0: gamma = 0 throughout)
        losses.append(float(loss.detach()))
        opt.step()
        with torch.no_grad():
            wt.clamp_(min=0.0)
            at.clamp_(min=0.0)
    print("losses", losses)
    assert all(b < a for a, b in zip(losses, losses[1:]))
