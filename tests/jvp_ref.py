"""CPU reference of the Jacobian-vector product of u = denoise(f, alpha), built on the oracle alone.

The tangent right-hand side is assembled here in numpy from oracle.grad_fwd / grad_fwd_T and the reference's thresholds
(1e-12 for the active set of gradient, 1/1e8 for gradient_reg), so it does not share code with the library's
adj_tangent_rhs_kernel.  A^-1 comes from oracle.gradient_image(u, u - r, ...), whose adjoint state is
    p =  A^-1 r                        reg = 0
    p = -A^-1 r                        reg = 1, scalar
    p = -S A_s^-1 S^-1 (u - ubar)      reg = 1, array parameter (S = diag(sqrt(alpha))):  ubar = u - alpha o r gives
                                       p = -S A_s^-1 S r, so du = S^-1 A_s^-1 S r = -p / alpha.
tests/test_jvp_abi.py pins this reference to the oracle's own vector-Jacobian product by the transpose identity."""
import numpy as np

ACT_TOL = 1e-12   # |grad u| below: active set of gradient
GAMMA = 1e8       # gradient_reg


def h_plane(oracle, u, reg):
    """(h1, h2): the per-pixel plane the parameter gradient pairs with G p."""
    g1, g2 = oracle.grad_fwd(u)
    ng = np.sqrt(g1 * g1 + g2 * g2)
    safe = np.where(ng > 0, ng, 1.0)
    if not reg:
        on = ng >= ACT_TOL
        return np.where(on, g1 / safe, 0.0), np.where(on, g2 / safe, 0.0)
    on = ng > 1.0 / GAMMA
    return np.where(on, g1 / safe, GAMMA * g1), np.where(on, g2 / safe, GAMMA * g2)


def jvp_image(oracle, u, alpha, df, dalpha, reg):
    """du of one (N, M) image for the tangents df ((N, M) or None) and dalpha (shaped like alpha, or None)."""
    N, M = u.shape
    patch = np.ndim(alpha) != 0
    amap = oracle.patch_upsample(alpha, M, N)
    da = oracle.patch_upsample(dalpha, M, N) if dalpha is not None else np.zeros((N, M))
    r = np.zeros((N, M)) if df is None else np.array(df, dtype=np.float64)
    h1, h2 = h_plane(oracle, u, reg)
    if not (reg and patch):
        r = r - oracle.grad_fwd_T(h1 * da, h2 * da)
        _, p, _ = oracle.gradient_image(u, u - r, amap, patch=patch, reg=bool(reg))
        return -p if reg else p
    r = r - oracle.grad_fwd_T(h1, h2) * da
    _, p, _ = oracle.gradient_image(u, u - amap * r, amap, patch=True, reg=True)
    return -p / amap


def vjp_image(oracle, u, alpha, gu, reg):
    """(grad_f, grad_alpha) of one image from the oracle, as tests/test_gpu_vjp.py takes them."""
    N, M = u.shape
    patch = np.ndim(alpha) != 0
    amap = oracle.patch_upsample(alpha, M, N)
    gpix, p, _ = oracle.gradient_image(u, u - gu, amap, patch=patch, reg=bool(reg))
    gf = -p if reg else p
    if not patch:
        return gf, float(gpix.sum())
    an, am = np.shape(alpha)
    return gf, (gpix if (an, am) == (N, M) else oracle.patch_adjoint(gpix, am, an))
