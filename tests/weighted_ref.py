"""numpy / scipy reference of the TV model with a per-pixel data-fidelity weight -- TEST INFRASTRUCTURE ONLY.

    min_u 0.5 sum w (u - f)^2 + sum alpha |G u|,   w >= 0

* pdhg: the recurrence of include/bpltv.h's bpltv_weighted_denoise, restated with oracle.np_twin's operators (numpy has no
  fma: it agrees with the library to a few ulp per iteration, not bit for bit),
* gap: the duality gap of that model (min w > 0),
* vjp_image: the vector-Jacobian product from the LITERAL system diag(w) + K, assembled with scipy.sparse from
  oracle.np_twin.grad_matrix in the reference's unreduced (saddle-point) form and solved by a sparse LU;
  vjp_image_scaled solves the node-scaled form (I + S K S) q = S gu, S = diag(w)^-1/2, the library's formulation, for
  the identity test.
Arrays are (O, N, M) / (N, M) as everywhere in tests/; nothing here shares code with the library's kernels.
"""
import math

import numpy as np

from oracle import np_twin as tw


def weight_planes(w, shape):
    """w as an array broadcastable against a batch of `shape` = (O, N, M)."""
    w = np.asarray(w, dtype=np.float64)
    assert w.shape == shape[-2:] or w.shape == tuple(shape), (w.shape, shape)
    return w


def step_table(maxiter, gamma, tau0=5.0, sigma0=0.99 / 5, accel=True, opnorm=0.0):
    L = opnorm if opnorm > 0 else math.sqrt(8.0)
    tau, sigma = tau0 / L, sigma0 / L
    tab = np.empty((maxiter, 3))
    for k in range(maxiter):
        omega = 1.0 / math.sqrt(1.0 + 2.0 * gamma * tau) if accel else 1.0
        tab[k] = (tau, sigma, omega)
        if accel:
            tau, sigma = tau * omega, sigma / omega
    return tab


def pdhg(f, alpha, w, maxiter, tau0=5.0, sigma0=0.99 / 5, accel=True, opnorm=0.0, return_dual=False, dtype=np.float64):
    """x = f, y = 0; per iteration: t = div - w f; x = (x - tau t) / (1 + tau w); xbar, dual ascent and the projection on
    the alpha-ball as np_twin.pdhg_denoise; gamma = min over ALL entries of w.
    dtype = np.longdouble: the same recurrence on the same (double) step table in extended precision, with 1 / sqrt for the
    Newton rsqrt -- what tests/test_weighted_abi.py measures this twin's own rounding against."""
    f = np.asarray(f, dtype=np.float64)
    N, M = f.shape[-2:]
    w = weight_planes(w, f.shape if f.ndim == 3 else (1,) + f.shape)
    amap = tw.alpha_to_map(alpha, M, N)
    tab = step_table(maxiter, float(w.min()), tau0, sigma0, accel, opnorm)
    rsqrt = tw.rsqrt_nr
    if dtype is not np.float64:
        f, w, amap, tab = (a.astype(dtype) for a in (f, w, amap, tab))
        rsqrt = lambda v: 1.0 / np.sqrt(v)
    x = f.copy()
    y1 = np.zeros_like(f)
    y2 = np.zeros_like(f)
    a2 = amap * amap
    for k in range(maxiter):
        tau, sigma, omega = tab[k]
        div = tw.grad_fwd_T(y1, y2)
        xo = x
        x = (x - tau * (div - w * f)) * (1.0 / (1.0 + tau * w))
        xb = (1.0 + omega) * x - omega * xo
        d1, d2 = tw.grad_fwd(xb)
        y1 = y1 + sigma * d1
        y2 = y2 + sigma * d2
        n2 = y1 * y1 + y2 * y2
        with np.errstate(all="ignore"):
            v = np.where(n2 > a2, amap * rsqrt(np.where(n2 > a2, n2, 1.0)), 1.0)
        y1 = y1 * v
        y2 = y2 * v
    if return_dual:
        return x, y1, y2
    return x


def primal_energy(u, f, alpha, w):
    N, M = f.shape[-2:]
    amap = tw.alpha_to_map(alpha, M, N)
    d1, d2 = tw.grad_fwd(u)
    return 0.5 * np.sum(w * (u - f) ** 2, axis=(-1, -2)) + np.sum(amap * np.sqrt(d1 * d1 + d2 * d2), axis=(-1, -2))


def gap(u, y1, y2, f, alpha, w):
    """Per image: 0.5 sum w (u-f)^2 + sum alpha |G u| - sum (d f - d^2 / (2 w)), d = G^T y  (min w > 0)."""
    d = tw.grad_fwd_T(y1, y2)
    return primal_energy(u, f, alpha, w) - np.sum(d * f - d * d / (2.0 * w), axis=(-1, -2))


def kappa_default(alpha, cap=1e14):
    """The active-set weight bpltv_vjp uses before any retry (stats.kappa_used reports the one actually used)."""
    scalar = np.ndim(alpha) == 0
    return min(1.0 / (tw.EPS if scalar else math.sqrt(tw.EPS)), cap)


def _system(u, alpha, kappa):
    """The pieces of (diag(w) + K) p = gu, K = G^T (alpha T_inactive + kappa I_active) G, for one (N, M) image, in the
    unreduced form the reference writes its adjoint systems in (/root/reference/src/TVLearningFunctionVec.jl:98-135):
        [ diag(w)                                  -G^T                  ] [ p   ]   [ gu ]
        [ Act G + Inact alpha (Den - P) G           Inact + (1/kappa) Act ] [ lam ] = [ 0  ]
    Eliminating lam gives diag(w) + K exactly; written this way kappa enters as 1/kappa next to entries of order one,
    and a double-precision LU resolves it (assembled, diag(w) + 4 kappa would round w away at kappa = 1e14)."""
    sp, _ = tw._sp()
    N, M = u.shape
    G = tw.grad_matrix(M, N)
    Gu = G @ u.reshape(-1)
    nGu = tw.xi(Gu)
    act = (nGu < 1e-12).astype(np.float64)
    inact = 1.0 - act
    den = inact * nGu + act
    av = tw.alpha_to_map(alpha, M, N).reshape(-1)
    A2 = sp.diags(np.concatenate([av, av]))
    low = sp.diags(act) @ G + sp.diags(inact) @ A2 @ (sp.diags(1.0 / den) - tw.prodesc(Gu / den ** 3, Gu)) @ G
    corner = sp.diags(inact + act / kappa)
    return G, low, corner, inact * Gu / den


def _solve(A, b, refine):
    _, spla = tw._sp()
    return tw.solve_refined(A, b, refine) if refine else spla.spsolve(A.tocsc(), b)


def vjp_image(u, f, alpha, w, gu, kappa, refine=0):
    """(grad_f, grad_alpha per pixel, grad_w, p) of one image from the literal system (diag(w) + K) p = gu."""
    sp, _ = tw._sp()
    N, M = u.shape
    n = N * M
    G, low, corner, h = _system(u, alpha, kappa)
    A = sp.bmat([[sp.diags(w.reshape(-1)), -G.T], [low, corner]], format="csc")
    p = _solve(A, np.concatenate([gu.reshape(-1), np.zeros(2 * n)]), refine)[:n]
    gpix = -tw.scalarprod(G @ p, h)
    pm = p.reshape(N, M)
    return w * pm, gpix.reshape(N, M), -(u - f) * pm, pm


def vjp_image_scaled(u, alpha, w, gu, kappa, refine=0):
    """p = S q of the node-scaled system (I + S K S) q = S gu, S = diag(w)^-1/2: the form the library factors."""
    sp, _ = tw._sp()
    N, M = u.shape
    n = N * M
    G, low, corner, _ = _system(u, alpha, kappa)
    s = 1.0 / np.sqrt(w.reshape(-1))
    S = sp.diags(s)
    A = sp.bmat([[sp.identity(n), -(S @ G.T)], [low @ S, corner]], format="csc")
    q = _solve(A, np.concatenate([s * gu.reshape(-1), np.zeros(2 * n)]), refine)[:n]
    return (s * q).reshape(N, M)


def vjp(u, f, alpha, w, gu, kappa, refine=0):
    """Batch (O, N, M): grad_f (O, N, M), grad_alpha in alpha's shape (summed over the images), grad_w in w's shape
    (summed over the images for an (N, M) weight), and p."""
    O, N, M = u.shape
    w = weight_planes(w, u.shape)
    wk = (lambda k: w) if w.ndim == 2 else (lambda k: w[k])
    gf, gw, pp = np.empty_like(u), np.empty_like(u), np.empty_like(u)
    gpix = np.zeros((N, M))
    for k in range(O):
        gf[k], g, gw[k], pp[k] = vjp_image(u[k], f[k], alpha, wk(k), gu[k], kappa, refine)
        gpix += g
    a = np.asarray(alpha, dtype=np.float64)
    if a.ndim == 0:
        ga = float(gpix.sum())
    elif a.shape == (N, M):
        ga = gpix
    else:
        ga = tw.patch_adjoint(gpix, a.shape[1], a.shape[0])
    return gf, ga, (gw.sum(axis=0) if w.ndim == 2 else gw), pp


# the shapes tests/test_gpu_weighted_shapes.py runs every factorisation on (tests/test_weighted_abi.py pins the reference
# on each): several tiles and fronts, odd sizes with N > M, the denoise tests' largest, and the only one with M > 138 (the
# band in HBM instead of LDS; no block cyclic reduction)
VJP_SHAPES = [(2, 40, 48), (3, 33, 17), (2, 70, 72), (1, 12, 140)]


def vjp_case(alpha, seed, O=2, N=16, M=20, iters=60, per_image=True):
    """(f, w, u, gu) for the VJP tests: w random in [0.25, 4], u the twin's iterate after `iters` iterations with two
    flat blocks planted (an active set |G u| < 1e-12 the kappa weight acts on), gu random.  A VJP takes any u; this
    one keeps the reference trustworthy: after 60 iterations the smallest inactive |G u| is ~1e-9 and the sparse LU
    agrees with its extended-precision refinement to 1e-11, while on a converged u (|G u| down to 1e-12 next to the
    active set) the two differ by up to 2e-6 -- more than the tolerance the library is held to."""
    from conftest import synth_batch
    assert N >= 12 and M >= 16, "the planted blocks sit at rows 3:6 / 10:12 and columns 4:8 / 15:"
    _, f = synth_batch(O, N, M, seed=seed)
    rng = np.random.default_rng(seed + 1)
    w = 0.25 + 3.75 * rng.random((O, N, M) if per_image else (N, M))
    u = pdhg(f, alpha, w, iters)
    u[0, 3:6, 4:8] = u[0, 3, 4]
    u[-1, 10:12, 15:] = u[-1, 10, 15]
    return f, w, u, rng.standard_normal(u.shape)
