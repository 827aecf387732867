"""Unweighted TV adjoint on images with a real active set -- TEST INFRASTRUCTURE ONLY.

The reference is tests/weighted_ref.py's literal (unreduced) system with w = 1: vjp / vjp_each wrap weighted_ref.vjp, jvp solves
the same matrix with the tangent right-hand side df - G^T (dalpha o h).  tv_case makes the inputs: the numpy twin's iterate after
60 iterations (inactive |G u| >= 3.6e-9, on which the sparse LU agrees with ten extended-precision sweeps to 4e-11; see
weighted_ref.vjp_case) with flat regions planted, so that |G u| is exactly zero on many elements: the active set the kappa weight
acts on.  tests/test_tv_active_ref.py pins all of it on the CPU; tests/test_gpu_tv_active_set.py holds the library to it."""
import functools

import numpy as np

from oracle import np_twin as tw

import weighted_ref as wr

LAYOUTS = ("blocks", "strips", "flat")


def _blocks(img_a, img_b):
    """The two blocks of weighted_ref.vjp_case: 3 x 4 inside img_a, 2 rows that reach the right border in img_b."""
    img_a[3:6, 4:8] = img_a[3, 4]
    img_b[10:12, 15:] = img_b[10, 15]


def plant(u, layout):
    """Flat regions in the batch u (O, N, M), in place.
    blocks: one block in the first image, one that reaches the right border in the last;
    strips: image 0, rows 18:22 over the full width and columns 30:34 over the full height, one value (they cross);
    flat:   image 0 constant, image 1 with both blocks, the last image untouched (O >= 3)."""
    O, N, M = u.shape
    assert N >= 12 and M >= 16, "the planted blocks sit at rows 3:6 / 10:12 and columns 4:8 / 15:"
    if layout == "blocks":
        _blocks(u[0], u[-1])
    elif layout == "strips":
        assert N >= 24 and M >= 36
        c = u[0, 18, 30]
        u[0, 18:22, :] = c
        u[0, :, 30:34] = c
    elif layout == "flat":
        assert O >= 3
        u[0] = u[0, 0, 0]
        _blocks(u[1], u[1])
    else:
        raise ValueError(layout)
    return u


def tv_case(alpha, seed, O, N, M, layout="blocks", iters=60):
    """(f, u, gu, df, dalpha): f from synth_batch, u the twin's iterate after `iters` iterations with `layout` planted, the
    cotangent gu, the tangent df and the parameter tangent dalpha (shaped like alpha; a float for a scalar) standard normal."""
    from conftest import synth_batch
    _, f = synth_batch(O, N, M, seed=seed)
    rng = np.random.default_rng(seed + 1)
    u = plant(tw.pdhg_denoise(f, alpha, maxiter=iters), layout)
    gu, df = rng.standard_normal(u.shape), rng.standard_normal(u.shape)
    da = rng.standard_normal(np.shape(alpha))
    return f, u, gu, df, (float(da) if da.ndim == 0 else da)


def grad_norm(u):
    """|G u| per element, (O, N, M)."""
    d1, d2 = tw.grad_fwd(u)
    return np.sqrt(d1 * d1 + d2 * d2)


def active_counts(u, tol=1e-12):
    """Per image: the elements with |G u| < tol, without the last pixel (both its forward differences are zero by the
    boundary rule, on any image)."""
    act = grad_norm(u) < tol
    assert act[:, -1, -1].all()
    return act.reshape(len(u), -1).sum(axis=1) - 1


def vjp(u, alpha, gu, kappa, refine=0):
    """(grad_f, grad_alpha, p) of the batch: weighted_ref.vjp with w = 1 (grad_f = p)."""
    gf, ga, _, p = wr.vjp(u, u, alpha, np.ones(u.shape), gu, kappa, refine)
    return gf, ga, p


def vjp_each(u, alphas, gu, kappa, refine=0):
    """Image k with its own parameter alphas[k]: (grad_f (O, N, M), grad_alphas shaped like alphas, p)."""
    out = [vjp(u[k:k + 1], (float(a) if np.ndim(a) == 0 else a), gu[k:k + 1], kappa, refine) for k, a in enumerate(alphas)]
    return np.concatenate([o[0] for o in out]), np.array([o[1] for o in out]), np.concatenate([o[2] for o in out])


def jvp_image(u, alpha, df, dalpha, kappa, refine=0):
    """du of one (N, M) image: the matrix of weighted_ref.vjp_image (w = 1), right-hand side df - G^T (dalpha_map o h)."""
    sp, _ = tw._sp()
    N, M = u.shape
    n = N * M
    G, low, corner, h = wr._system(u, alpha, kappa)
    A = sp.bmat([[sp.identity(n), -G.T], [low, corner]], format="csc")
    r = np.zeros(n) if df is None else np.array(df, dtype=np.float64).reshape(-1)
    if dalpha is not None:
        da = tw.alpha_to_map(dalpha, M, N).reshape(-1)
        r = r - G.T @ (np.concatenate([da, da]) * h)
    return wr._solve(A, np.concatenate([r, np.zeros(2 * n)]), refine)[:n].reshape(N, M)


def jvp(u, alpha, df, dalpha, kappa, refine=0):
    """du (O, N, M) for the tangents df ((O, N, M) or None) and dalpha (shaped like alpha, or None)."""
    return np.stack([jvp_image(u[k], alpha, None if df is None else df[k], dalpha, kappa, refine) for k in range(len(u))])


def jvp_each(u, alphas, df, dalphas, kappa, refine=0):
    """Image k with its own alphas[k] and dalphas[k]."""
    pick = lambda x, k: None if x is None else (float(x[k]) if np.ndim(x[k]) == 0 else x[k])
    return np.stack([jvp_image(u[k], pick(alphas, k), None if df is None else df[k], pick(dalphas, k), kappa, refine)
                     for k in range(len(u))])


def gauss_newton(u, ubar, alpha, kappa, refine=0):
    """(J^T (u - ubar) shaped like alpha, J^T J) from one jvp per parameter entry, entries in alpha.ravel() order."""
    a = np.asarray(alpha, dtype=np.float64)
    cols = []
    for e in range(max(a.size, 1)):
        da = np.zeros(a.size)
        da[e] = 1.0
        cols.append(jvp(u, alpha, None, (1.0 if a.ndim == 0 else da.reshape(a.shape)), kappa, refine).reshape(-1))
    J = np.stack(cols, axis=1)
    g = J.T @ (u - ubar).reshape(-1)
    return (float(g[0]) if a.ndim == 0 else g.reshape(a.shape)), J.T @ J


def alpha_kind(kind, N, M):
    """The parameters of tests/test_gpu_weighted.py: scalar 0.1, the 2 x 2 patch, a map."""
    if kind == "scalar":
        return 0.1
    if kind == "patch":
        return np.array([[0.08, 0.12], [0.1, 0.05]])
    return 0.05 + 0.1 * np.random.default_rng(8).random((N, M))


KINDS = ("scalar", "patch", "map")
SEED = 21
# (shape, layout) of every case tests/test_gpu_tv_active_set.py runs; each with every parameter kind
CASES = [(shape, "blocks") for shape in wr.VJP_SHAPES] + [((2, 40, 48), "strips"), ((3, 40, 48), "flat"), ((3, 33, 17), "flat")]


def case_id(shape, layout, kind=None):
    return "x".join(str(n) for n in shape) + "-" + layout + ("-" + kind if kind else "")


def _frozen(*arrays):
    for a in arrays:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def case(shape, kind, layout):
    """(alpha, f, u, gu, df, dalpha) of tv_case at SEED: computed once, shared by the tests, read-only."""
    O, N, M = shape
    alpha = alpha_kind(kind, N, M)
    return _frozen(alpha, *tv_case(alpha, SEED, O, N, M, layout))


@functools.lru_cache(maxsize=None)
def vjp_ref(shape, kind, layout, kappa, refine=10):
    """(grad_f, grad_alpha, max|p|) of the literal system with weight kappa: solved once per (case, kappa), shared, read-only."""
    alpha, f, u, gu, df, da = case(shape, kind, layout)
    gf, ga, p = vjp(u, alpha, gu, kappa, refine)
    return _frozen(gf, ga) + (float(np.abs(p).max()),)


@functools.lru_cache(maxsize=None)
def jvp_ref(shape, kind, layout, kappa, which="both", refine=10):
    """du of the literal system for both tangents of the case, or `df` / `dalpha` alone."""
    alpha, f, u, gu, df, da = case(shape, kind, layout)
    return _frozen(jvp(u, alpha, None if which == "dalpha" else df, None if which == "df" else da, kappa, refine))[0]
