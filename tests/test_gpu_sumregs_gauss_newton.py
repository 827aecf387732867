"""GPU checks of bpltv_sumregs_gauss_newton: grad = J^T (u - ubar) and H = J^T J of the loss 0.5||u(x) - ubar||^2 for the
sum-of-regularisers model, J the P = 3*am*an columns du/dx_j solved against one factorisation.  H is the Gram matrix of
the columns bpltv_sumregs_jvp returns for single unit directions, grad is bpltv_sumregs_vjp's parameter gradient for the
cotangent u - ubar by the transpose identity."""
import functools

import numpy as np
import pytest
from conftest import synth_batch

from test_gpu_sumregs_vjp import A3, P22

pytestmark = pytest.mark.gpu

E_UNSUPPORTED = 6
SHAPES = [(3, 48, 40), (2, 3, 5)]
PARAMS = {"vector": A3, "patch22": P22}


@functools.lru_cache(maxsize=None)
def _case(shape, kind):
    """(ubar, x, u): u from a 300-iteration sumregs_denoise of the library."""
    from bpldenoising_amd import TVSolver
    O, N, M = shape
    ub, f = synth_batch(O, N, M, seed=90 + M)
    x = PARAMS[kind]
    s = TVSolver(M, N, O)
    s.set_data(ub, f)
    u = s.sumregs_denoise(x, maxiter=300)
    s.close()
    return ub, x, u


@pytest.mark.parametrize("reg", [0, 1])
@pytest.mark.parametrize("kind", list(PARAMS))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_sumregs_gauss_newton_gradient_and_hessian(gpu_solver_cls, shape, kind, reg):
    O, N, M = shape
    ub, x, u = _case(shape, kind)
    P = np.size(x)
    s = gpu_solver_cls(M, N, O)
    grad, H = s.sumregs_gauss_newton(u, ub, x, reg=reg)
    st = s.stats()
    assert H.shape == (P, P) and np.shape(grad) == np.shape(x) and st["reg_gradient_used"] == reg
    assert np.array_equal(H, H.T)
    # the columns, one single-direction call each, in the order of the parameter layout
    eye = np.eye(P).reshape((P,) + np.shape(x))
    J = np.stack([s.sumregs_jvp(u, x, dalpha=eye[j], reg=reg) for j in range(P)]).reshape(P, -1)
    H0 = J @ J.T
    eh = np.abs(H - H0).max() / np.abs(H0).max()
    print("%s %s reg %d: H err %.3e of max|H|" % (shape, kind, reg, eh))
    assert eh <= 1e-12     # the same columns, summed in another order
    assert np.abs(np.ravel(grad) - J @ (u - ub).ravel()).max() <= 1e-12 * np.abs(grad).max()
    g0 = s.sumregs_vjp(u, x, u - ub, reg=reg, want_f=False)[1]
    eg = np.abs(grad - g0).max() / np.abs(g0).max()
    print("   grad %s, vjp %s, err %.3e of max|g|" % (np.ravel(grad)[:3], np.ravel(g0)[:3], eg))
    assert eg <= 1e-6
    w = np.linalg.eigvalsh(H)
    assert w.min() >= -1e-12 * w.max()
    g2, H2 = s.sumregs_gauss_newton(u, ub, x, reg=reg)
    assert np.array_equal(H2, H) and np.array_equal(g2, grad)
    s.close()


@pytest.mark.parametrize("kind", list(PARAMS))
def test_sumregs_gauss_newton_on_shards_of_one_device(gpu_solver_cls, kind):
    """The shards' [grad, H] added on the host in shard order: a single handle's result to 1e-12."""
    shape = (3, 48, 40)
    O, N, M = shape
    ub, x, u = _case(shape, kind)
    s = gpu_solver_cls(M, N, O)
    m = gpu_solver_cls(M, N, O, devices=[0, 0])
    for reg in (0, 1):
        g, H = s.sumregs_gauss_newton(u, ub, x, reg=reg)
        gm, Hm = m.sumregs_gauss_newton(u, ub, x, reg=reg)
        assert m.stats()["shards"] == 2
        assert np.abs(gm - g).max() <= 1e-12 * np.abs(g).max() and np.abs(Hm - H).max() <= 1e-12 * np.abs(H).max()
        assert np.array_equal(Hm, Hm.T)
    m.close()
    s.close()


def test_sumregs_gauss_newton_refuses_a_map_and_a_large_patch(gpu_solver_cls):
    """P = 3*am*an > 16 (the 3 x 5 patch, P = 45) and a pixel map: BPLTV_E_UNSUPPORTED, and the handle stays as it was."""
    import torch
    from bpldenoising_amd._lib import BpltvError
    O, N, M = 3, 48, 40
    ub, f = synth_batch(O, N, M, seed=90 + M)
    s = gpu_solver_cls(M, N, O)
    s.set_data(ub, f)
    u = s.sumregs_denoise(P22, maxiter=200)
    buf = torch.empty(O * N * M, dtype=torch.float64, device="cuda")
    s.copy_u_device(buf.data_ptr())
    snap_u, snap_gap = buf.cpu().numpy(), s.duality_gap()
    ref = s.sumregs_gauss_newton(u, ub, P22)
    for x in (np.full((3, 5, 3), 0.03), np.full((3, N, M), 0.03), np.full((3, 2, 3), 0.03)):
        with pytest.raises(BpltvError) as e:
            s.sumregs_gauss_newton(u, ub, x)
        assert e.value.code == E_UNSUPPORTED, str(e.value)
    g15, H15 = s.sumregs_gauss_newton(u, ub, np.full((3, 5, 1), 0.03))   # P = 15: the 1 x 5 patch fits
    assert H15.shape == (15, 15) and np.array_equal(H15, H15.T) and g15.shape == (3, 5, 1)
    with pytest.raises(BpltvError) as e:
        s.sumregs_gauss_newton(u, ub, -P22)
    assert e.value.code == 1
    s.copy_u_device(buf.data_ptr())
    assert np.array_equal(buf.cpu().numpy(), snap_u) and np.array_equal(s.duality_gap(), snap_gap)
    again = s.sumregs_gauss_newton(u, ub, P22)
    assert np.array_equal(again[0], ref[0]) and np.array_equal(again[1], ref[1])
    assert np.array_equal(s.sumregs_denoise(P22, maxiter=200), u)
    s.close()
