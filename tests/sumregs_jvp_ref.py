"""CPU reference of the Jacobian-vector product of u = sumregs_denoise(f, x), built on the oracle alone.

One image at a time.  With k = forward, backward, centred, (g1, g2) = G_k u from oracle.sr_grad and the reference's
thresholds (|G_k u| < 1e-12: active set of sumregs_gradient; |G_k u| <= 1/gamma, gamma = 1e3 for a vector and 1e8 for an
array parameter: the smoothed branch of sumregs_gradient_reg) the planes are
    h_k = G_k u / |G_k u| where the element is "on", else 0 (reg = 0) or gamma G_k u (reg = 1),
    w_k = G_k^T h_k            (oracle.sr_gradT),
    r   = df - sum_k w_k o up(dx_k),
and the reduced system is assembled with scipy.sparse from oracle.np_twin_sumregs.grad_matrix:
    K_k = G_k^T W_k G_k,   W_k per element = c t t^T + kap I,   t = (-g2, g1) / |G_k u|,
    reg = 0:                    c = x_k / |G_k u| on,   kap = 1e14 off  (the cap of the library and the C oracle on 1/eps)
    reg = 1, vector:            c = x_k / |G_k u| on,   kap = x_k gamma off
    reg = 1, patch or map:      c = 1 / |G_k u| on,     kap = gamma off,  A = I + sum_k diag(up(x_k)) K_k  (row-scaled)
    otherwise                   A = I + sum_k K_k.
du = A^-T r by scipy's sparse LU (jvp_image); for images of a few dozen pixels, where kap = 1e14 can push cond(A) past
what double precision resolves, by a rational solve of the same system (jvp_image_exact, jvp_image_small).  Nothing here
shares code with the library's kernels.  tests/test_sumregs_jvp_abi.py pins this reference to the oracle's own gradients
by the transpose identity, and the rational solve to scipy's where the system is well conditioned.  On images with a
real active set (flat regions of more than a few pixels) jvp_image is off by 1e-4 of max|du| and more; the reference there
is the literal unreduced system of tests/sumregs_active_ref.py."""
import numpy as np

ACT_TOL = 1e-12
KAPPA = 1e14


def _sp():
    import scipy.sparse as sp
    import scipy.sparse.linalg as spla
    return sp, spla


def _oracle():
    from oracle import c_oracle
    c_oracle.build()
    return c_oracle


def _maps(x, M, N):
    from oracle import np_twin_sumregs as TS
    return TS.alpha_maps(np.asarray(x, dtype=np.float64), M, N)


def is_array(x):
    """A patch or map parameter; (3, 1, 1) is the vector [a1; a2; a3], as the library and the reference's dispatch see it."""
    return np.ndim(x) == 3 and np.size(x) > 3


def planes(u, x, reg):
    """Per operator k: (h1, h2, c, kap, t1, t2) as (N, M) arrays; c carries x_k unless the system is row-scaled."""
    N, M = u.shape
    patch = is_array(x)
    gamma = 1e8 if patch else 1e3
    amap = _maps(x, M, N)
    out = []
    for k in range(3):
        g1, g2 = _oracle().sr_grad(k, u)
        ng = np.sqrt(g1 * g1 + g2 * g2)
        on = (ng > 1.0 / gamma) if reg else ~(ng < ACT_TOL)
        safe = np.where(on, ng, 1.0)
        a = amap[k]
        if not reg:
            h1, h2 = np.where(on, g1 / safe, 0.0), np.where(on, g2 / safe, 0.0)
            c, kap = np.where(on, a / safe, 0.0), np.where(on, 0.0, KAPPA)
        else:
            h1, h2 = np.where(on, g1 / safe, gamma * g1), np.where(on, g2 / safe, gamma * g2)
            c = np.where(on, (1.0 if patch else a) / safe, 0.0)
            kap = np.where(on, 0.0, gamma if patch else a * gamma)
        t1, t2 = np.where(on, -g2 / safe, 0.0), np.where(on, g1 / safe, 0.0)
        out.append((h1, h2, c, kap, t1, t2))
    return out


def matrix(u, x, reg):
    """A of the module docstring (scipy CSR, column-major pixel order q = i + M j == numpy (N, M).reshape(-1))."""
    from oracle import np_twin_sumregs as TS
    sp, _ = _sp()
    N, M = u.shape
    n = N * M
    rowsc = bool(reg) and is_array(x)
    amap = _maps(x, M, N)
    A = sp.identity(n, format="csr")
    for k, (_, _, c, kap, t1, t2) in enumerate(planes(u, x, reg)):
        G = TS.grad_matrix(k, M, N)
        c, kap, t1, t2 = (v.reshape(-1) for v in (c, kap, t1, t2))
        W = sp.bmat([[sp.diags(c * t1 * t1 + kap), sp.diags(c * t1 * t2)],
                     [sp.diags(c * t1 * t2), sp.diags(c * t2 * t2 + kap)]], format="csr")
        K = G.T @ W @ G
        A = A + (sp.diags(amap[k].reshape(-1)) @ K if rowsc else K)
    return A.tocsr()


def rhs(u, x, df, dx, reg):
    N, M = u.shape
    r = np.zeros((N, M)) if df is None else np.array(df, dtype=np.float64)
    if dx is not None:
        dmap = _maps(dx, M, N)
        for k, (h1, h2, *_rest) in enumerate(planes(u, x, reg)):
            r = r - _oracle().sr_gradT(k, h1, h2) * dmap[k]
    return r


def factor(u, x, reg, transposed=True):
    """scipy's sparse LU of A^T (of A: transposed = False) for one image: several directions against one factorisation."""
    _, spla = _sp()
    A = matrix(u, x, reg)
    return spla.splu((A.T if transposed else A).tocsc())


def jvp_image(u, x, df, dx, reg, transposed=True, lu=None):
    """du of one (N, M) image for the tangents df ((N, M) or None) and dx (shaped like x, or None).  transposed = False
    solves with A instead of A^T: what an untransposed factor would return (they differ on the row-scaled system only).
    lu: factor(u, x, reg, transposed) of an earlier call."""
    if lu is None:
        lu = factor(u, x, reg, transposed)
    return lu.solve(rhs(u, x, df, dx, reg).reshape(-1)).reshape(u.shape)


def jvp_image_exact(u, x, df, dx, reg, transposed=True):
    """The same du with the system formed and solved in rational arithmetic (fractions.Fraction) from the same double
    planes: for images of a few dozen pixels.  Where active elements (kap = 1e14) connect most of a small image, the
    assembled double matrix has lost the identity under kap (1 + 2e14 rounds in steps of 0.03) and its LU, scipy's
    included, returns the component means of du to two or three digits only; the library refines against the
    matrix-free operator, whose differences of neighbouring values are exact, and does not share that loss."""
    from fractions import Fraction as Fr
    from oracle import np_twin_sumregs as TS
    N, M = u.shape
    n = N * M
    rowsc = bool(reg) and is_array(x)
    amap = _maps(x, M, N)
    A = [[Fr(int(i == j)) for j in range(n)] for i in range(n)]
    for k, (_, _, c, kap, t1, t2) in enumerate(planes(u, x, reg)):
        G = TS.grad_matrix(k, M, N).toarray()
        c, kap, t1, t2 = ([Fr(float(v)) for v in p.reshape(-1)] for p in (c, kap, t1, t2))
        xs = [Fr(float(v)) for v in amap[k].reshape(-1)]
        for e in range(n):   # element e: rows e and n + e of G_k, W_e = c t t^T + kap I
            r1 = {j: Fr(float(G[e, j])) for j in np.nonzero(G[e])[0]}
            r2 = {j: Fr(float(G[n + e, j])) for j in np.nonzero(G[n + e])[0]}
            w11, w12, w22 = c[e] * t1[e] * t1[e] + kap[e], c[e] * t1[e] * t2[e], c[e] * t2[e] * t2[e] + kap[e]
            for ra, wa1, wa2 in ((r1, w11, w12), (r2, w12, w22)):
                for i, gi in ra.items():
                    for rb, w in ((r1, wa1), (r2, wa2)):
                        for j, gj in rb.items():
                            A[i][j] += (xs[i] if rowsc else 1) * gi * w * gj
    if transposed:
        A = [list(col) for col in zip(*A)]
    b = [Fr(float(v)) for v in rhs(u, x, df, dx, reg).reshape(-1)]
    # every entry is a dyadic rational: scale to integers and eliminate fraction-free (Bareiss), which keeps them small
    scale = 1
    for row in A + [b]:
        for v in row:
            scale = max(scale, v.denominator)
    T = [[int(v * scale) for v in row] + [int(b[i] * scale)] for i, row in enumerate(A)]
    prev = 1
    for col in range(n - 1):
        piv = next(r for r in range(col, n) if T[r][col] != 0)
        if piv != col:
            T[col], T[piv] = T[piv], T[col]
        for r in range(col + 1, n):
            T[r] = [0] * (col + 1) + [(T[r][j] * T[col][col] - T[r][col] * T[col][j]) // prev for j in range(col + 1, n + 1)]
        prev = T[col][col]
    sol = [Fr(0)] * n
    for i in reversed(range(n)):
        sol[i] = (T[i][n] - sum(T[i][j] * sol[j] for j in range(i + 1, n))) / Fr(T[i][i])
    return np.array([float(v) for v in sol]).reshape(N, M)


def jvp_image_small(u, x, df, dx, reg):
    """jvp_image for an image of a few dozen pixels, with a reference that is good to 1e-8 either way: scipy's LU where
    cond(A) eps <= 1e-8 bounds its error, the rational solve where it does not (cond(A) > 1e8 / 2.2)."""
    cond = np.linalg.cond(matrix(u, x, reg).toarray())
    if cond * np.finfo(np.float64).eps <= 1e-8:
        return jvp_image(u, x, df, dx, reg)
    return jvp_image_exact(u, x, df, dx, reg)
