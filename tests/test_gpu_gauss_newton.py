"""GPU checks of bpltv_gauss_newton: grad = J^T (u - ubar) and H = J^T J of the loss 0.5||u(alpha) - ubar||^2, J the
P columns du/dalpha_j solved against one factorisation.  grad is bpltv_gradient's result by the transpose identity, H
the Gram matrix of the columns bpltv_jvp returns for the unit directions."""
import numpy as np
import pytest

from test_gpu_vjp import P22, _case

pytestmark = pytest.mark.gpu

E_UNSUPPORTED = 6
CASES = [(10, 128, 128, "scalar"), (3, 48, 40, "scalar"), (3, 48, 40, "patch22")]
IDS = ["10x128_scalar", "3x48x40_scalar", "3x48x40_patch22"]


def _columns(s, u, alpha, reg):
    """(P, O, N, M): du/dalpha_j for the entries of alpha in the library's (column-major) order."""
    if np.ndim(alpha) == 0:
        return s.jvp(u, alpha, dalpha=np.ones(1), reg=reg)
    an, am = np.shape(alpha)
    P = am * an
    return s.jvp(u, alpha, dalpha=np.eye(P).reshape(P, an, am), reg=reg)


@pytest.mark.parametrize("reg", [0, 1])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_gauss_newton_gradient_and_hessian(gpu_solver_cls, case, reg):
    O, N, M, kind = case
    ub, _, alpha, u = _case(*case)
    s = gpu_solver_cls(M, N, O)
    grad, H = s.gauss_newton(u, ub, alpha, reg=reg)
    P = 1 if kind == "scalar" else 4
    assert H.shape == (P, P) and np.shape(grad) == np.shape(alpha)
    g0 = s.gradient(u, ub, alpha, reg=reg)
    print("%s reg %d: grad %s gradient %s" % (kind, reg, np.ravel(grad), np.ravel(g0)))
    assert np.allclose(grad, g0, rtol=1e-6, atol=0)
    J = _columns(s, u, alpha, reg).reshape(P, -1)
    H0 = J @ J.T
    print("H rel err %.3e" % (np.abs(H - H0).max() / np.abs(H0).max()))
    assert np.allclose(H, H0, rtol=1e-10, atol=0)
    assert np.allclose(np.ravel(grad), J @ (u - ub).ravel(), rtol=1e-10, atol=0)
    assert np.array_equal(H, H.T)
    w = np.linalg.eigvalsh(H)
    assert w.min() >= -1e-12 * w.max()
    if P == 1:
        assert np.isclose(H[0, 0], np.sum(J * J), rtol=1e-10)
    # the same bits from a second call and from image groups of one image
    g2, H2 = s.gauss_newton(u, ub, alpha, reg=reg)
    assert np.array_equal(H2, H) and np.array_equal(g2, grad)
    s.close()


@pytest.mark.parametrize("kind", ["scalar", "patch22"])
def test_gauss_newton_on_shards_of_one_device(gpu_solver_cls, kind):
    """The shards' [grad, H] added on the host in shard order: a single handle's result to rounding."""
    case = (3, 48, 40, kind)
    O, N, M, _ = case
    ub, _, alpha, u = _case(*case)
    s = gpu_solver_cls(M, N, O)
    m = gpu_solver_cls(M, N, O, devices=[0, 0])
    for reg in (0, 1):
        g, H = s.gauss_newton(u, ub, alpha, reg=reg)
        gm, Hm = m.gauss_newton(u, ub, alpha, reg=reg)
        assert m.stats()["shards"] == 2
        assert np.allclose(gm, g, rtol=1e-13, atol=0) and np.allclose(Hm, H, rtol=1e-13, atol=0)
        assert np.array_equal(Hm, Hm.T)
    m.close()
    s.close()


def test_gauss_newton_refuses_a_map_and_a_large_patch(gpu_solver_cls):
    from bpldenoising_amd._lib import BpltvError
    O, N, M = 3, 48, 40
    ub, _, _, u = _case(O, N, M, "scalar")
    s = gpu_solver_cls(M, N, O)
    ref = s.gauss_newton(u, ub, P22)
    for alpha in (np.full((N, M), 0.1), np.full((5, 5), 0.1), np.full((1, 17), 0.1)):
        with pytest.raises(BpltvError) as e:
            s.gauss_newton(u, ub, alpha)
        assert e.value.code == E_UNSUPPORTED, str(e.value)
    g16, H16 = s.gauss_newton(u, ub, np.full((4, 4), 0.1))   # P = 16 is the largest
    assert H16.shape == (16, 16) and np.array_equal(H16, H16.T)
    with pytest.raises(BpltvError) as e:
        s.gauss_newton(u, ub, -P22)
    assert e.value.code == 1
    again = s.gauss_newton(u, ub, P22)
    assert np.array_equal(again[0], ref[0]) and np.array_equal(again[1], ref[1])
    s.close()
