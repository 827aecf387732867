"""Sum-of-regularisers adjoint on images with a real active set -- TEST INFRASTRUCTURE ONLY.

The reference is the literal unreduced 7n^2 saddle system of oracle/np_twin_sumregs.gradient_image, per image
    [ I                                   -G_f^T  -G_b^T  -G_c^T ] [ p     ]   [ r ]
    [ Act_k G_k + Inact_k X_k (Den_k - P_k) G_k    Inact_k + (1/kappa) Act_k  ] [ lam_k ] = [ 0 ]      k = f, b, c
with the active-set weight kappa an argument (the twin writes eps()), solved by np_twin.solve_refined: a sparse LU and ten
sweeps of refinement with the residual in extended precision.  Eliminating lam_k gives I + sum_k G_k^T W_k G_k exactly;
written this way kappa enters as 1/kappa beside entries of order one and double precision resolves it, where the assembled
matrix (tests/sumregs_jvp_ref.py) has lost the identity under 1e14.  r = gu gives the vector-Jacobian product (grad_f = p,
grad_x_k = -<p, G_k^T h_k>, per pixel for an array parameter), r = sumregs_jvp_ref.rhs(u, x, df, dx, 0) the Jacobian-vector
product du = p: the reduced matrix is symmetric without regularisation, so both solve the same system.

case() makes the inputs: the numpy twin's iterate after 60 iterations (every inactive |G_k u| >= 1e-9, so that the system
is one a sparse LU resolves) with a layout planted, so that |G_k u| is exactly zero on many elements:
    blocks    a 4 x 5 flat block inside image 0, a 3-row block that reaches the right border in the last image.  Inside
              them all three operators are active, on their rims only the forward or only the backward one.  On one
              40 x 48 image with both blocks: 25 forward, 23 backward, 11 centred active elements (forced border rows
              included: the last pixel for forward, the first for backward differences)
    stripes   rows 14:30, columns 6:M-2 of image 0 set to a 2 x 2-periodic pattern of four values of u: G_c u = 0 exactly
              in the window's interior (14 x 38 = 532 elements at 40 x 48) while the forward and backward operators keep
              only their forced corner.  The window crosses the two-pixel separators of the dissection
    cross     image 0, rows 18:22 over the full width and columns 30:34 over the full height, one value
    flat      image 0 constant, image 1 with both blocks, the last image untouched (O >= 3)
tests/test_sumregs_active_ref.py pins all of it on the CPU; tests/test_gpu_sumregs_active_set.py holds the library to it.
Nothing here shares code with the library's kernels."""
import functools

import numpy as np

from oracle import np_twin as tw
from oracle import np_twin_sumregs as ts

import sumregs_jvp_ref as jr
import weighted_ref as wr

ACT_TOL = 1e-12
SEED = 21
KAPPA = 1e14    # the library's weight before any retry: min(1 / eps(), kappa_cap = 1e14), for every parameter kind
A3 = np.array([0.03, 0.02, 0.05])
P22 = np.stack([np.array([[0.03, 0.05], [0.02, 0.04]]), np.array([[0.02, 0.03], [0.05, 0.02]]),
                np.array([[0.04, 0.02], [0.03, 0.06]])])
KINDS = ("vector", "vector-off", "patch22", "map")
LAYOUTS = ("blocks", "stripes", "cross", "flat")
# (shape, layout) of every case tests/test_gpu_sumregs_active_set.py runs; each with every parameter kind
CASES = ([(shape, "blocks") for shape in wr.VJP_SHAPES]
         + [((2, 40, 48), "stripes"), ((2, 70, 72), "stripes"), ((2, 40, 48), "cross"), ((2, 70, 72), "cross"),
            ((3, 40, 48), "flat"), ((3, 33, 17), "flat")])


def x_kind(kind, N, M):
    """The parameters of tests/test_gpu_sumregs_vjp.py: the vector A3, the same with x_2 = 0 (the backward operator switched
    off; sumregs_gradient only), the 2 x 2 patch P22, a map."""
    if kind == "vector":
        return A3.copy()
    if kind == "vector-off":
        return np.array([A3[0], 0.0, A3[2]])
    if kind == "patch22":
        return P22.copy()
    if kind == "map":
        return 0.02 + 0.04 * np.random.default_rng(32).random((3, N, M))
    raise ValueError(kind)


def case_id(shape, layout, kind=None):
    return "x".join(str(n) for n in shape) + "-" + layout + ("-" + kind if kind else "")


# ---- planted layouts ----------------------------------------------------------------------------------------------------
def _regions(shape, layout):
    """[(image, row slice, column slice)] of the flat regions of `layout` (stripes: the window)."""
    O, N, M = shape
    blocks = lambda a, b: [(a, slice(3, 7), slice(4, 9)), (b, slice(10, 13), slice(M - 6, M))]
    if layout == "blocks":
        return blocks(0, O - 1)
    if layout == "stripes":
        assert N >= 32 and M >= 32
        return [(0, slice(14, 30), slice(6, M - 2))]
    if layout == "cross":
        assert N >= 24 and M >= 36
        return [(0, slice(18, 22), slice(0, M)), (0, slice(0, N), slice(30, 34))]
    if layout == "flat":
        assert O >= 3
        return [(0, slice(0, N), slice(0, M))] + blocks(1, 1)
    raise ValueError(layout)


def plant(u, layout):
    """The layout in the batch u (O, N, M), in place."""
    O, N, M = u.shape
    assert N >= 12 and M >= 16, "the planted blocks sit at rows 3:7 / 10:13 and columns 4:9 / M-6:"
    reg = _regions(u.shape, layout)
    if layout == "stripes":
        k, rows, cols = reg[0]
        vals = u[k, 14:16, 20:22].copy()      # four values of u itself, at even / odd offsets of the window
        win = u[k, rows, cols]
        for a in (0, 1):
            for b in (0, 1):
                win[a::2, b::2] = vals[a, b]
    elif layout == "cross":
        for k, rows, cols in reg:
            u[k, rows, cols] = u[0, 18, 30]
    else:
        for k, rows, cols in reg:
            u[k, rows, cols] = u[k, rows.start, cols.start]
    return u


def labels(shape, layout):
    """An integer per pixel, equal on two pixels exactly where the layout makes u equal there by construction: what
    expected_counts counts the active elements from, without looking at u."""
    O, N, M = shape
    lab = np.arange(1, O * N * M + 1).reshape(shape)
    for r, (k, rows, cols) in enumerate(_regions(shape, layout)):
        if layout == "stripes":
            win = lab[k, rows, cols]
            for a in (0, 1):
                for b in (0, 1):
                    win[a::2, b::2] = -(1 + 2 * a + b)
        else:
            lab[k, rows, cols] = -1 if layout == "cross" else -(1 + r)
    return lab


def expected_counts(shape, layout):
    """(O, 3): per image and operator (forward, backward, centred) the elements both of whose differences vanish by the
    layout's construction or by the operator's boundary rule (forward: zero row at the far border, backward: at the near
    border, centred: mirrored border, no zero row).  The forced ones are included: the last pixel (forward), the first
    (backward)."""
    O, N, M = shape
    lab = labels(shape, layout)
    ii, jj = np.arange(M), np.arange(N)
    out = np.zeros((O, 3), dtype=int)
    for k in range(O):
        L = lab[k]
        f1 = L[:, np.minimum(ii + 1, M - 1)] == L             # the far border compares a pixel with itself: zero row
        f2 = L[np.minimum(jj + 1, N - 1), :] == L
        b1 = L == L[:, np.maximum(ii - 1, 0)]
        b2 = L == L[np.maximum(jj - 1, 0), :]
        c1 = L[:, np.minimum(ii + 1, M - 1)] == L[:, np.maximum(ii - 1, 0)]
        c2 = L[np.minimum(jj + 1, N - 1), :] == L[np.maximum(jj - 1, 0), :]
        out[k] = [(f1 & f2).sum(), (b1 & b2).sum(), (c1 & c2).sum()]
    return out


def grad_norms(u):
    """|G_k u| per operator and element of one (N, M) image: (3, N, M), from the sparse operators the system is built from."""
    N, M = u.shape
    return np.stack([tw.xi(ts.grad_matrix(k, M, N) @ u.reshape(-1))[:N * M].reshape(N, M) for k in range(3)])


def active_counts(u):
    """(O, 3): elements with |G_k u| < 1e-12 per image and operator, the forced border rows included."""
    return np.array([(grad_norms(img) < ACT_TOL).reshape(3, -1).sum(axis=1) for img in u])


# ---- the literal system ---------------------------------------------------------------------------------------------------
def system(u, x, kappa):
    """(A, pieces) of one (N, M) image: np_twin_sumregs.gradient_image's saddle matrix with 1/kappa in place of eps()."""
    sp, _ = ts._sp()
    N, M = u.shape
    n = N * M
    maps = ts.alpha_maps(np.asarray(x, dtype=np.float64), M, N)
    pcs = [ts._pieces(k, u, tol=ACT_TOL) for k in range(3)]
    Z = sp.csr_matrix((2 * n, 2 * n))
    top, lower = [sp.identity(n)], []
    for k, (G, Gu, act, inact, den, P) in enumerate(pcs):
        top.append(-G.T)
        X = sp.diags(np.concatenate([maps[k].reshape(-1)] * 2))
        row = [sp.diags(act) @ G + sp.diags(inact) @ X @ (sp.diags(1.0 / den) - P) @ G] + [Z] * 3
        row[1 + k] = sp.diags(inact + act / kappa)
        lower.append(row)
    return sp.bmat([top] + lower, format="csc"), pcs


def solve(A, r, refine=10):
    """p (the first block) of A [p; lam] = [r; 0].  refine = 0: the plain sparse LU."""
    _, spla = ts._sp()
    n = r.size
    b = np.concatenate([np.asarray(r, dtype=np.float64).reshape(-1), np.zeros(A.shape[0] - n)])
    return (tw.solve_refined(A, b, refine) if refine else spla.spsolve(A, b))[:n]


def vjp_image(u, x, gu, kappa, refine=10):
    """(p (N, M), g): g the three numbers -<p, G_k^T h_k> for a vector x, the three (N, M) maps -p o G_k^T h_k otherwise."""
    N, M = u.shape
    A, pcs = system(u, x, kappa)
    p = solve(A, gu, refine)
    vec = np.ndim(x) == 1
    g = []
    for G, Gu, act, inact, den, P in pcs:
        w = G.T @ (inact * Gu / den)
        g.append(-float(p @ w) if vec else -(p * w).reshape(N, M))
    return p.reshape(N, M), np.array(g)


def _to_x(g, x):
    """Pixel maps (3, N, M) to the shape of the array parameter x: calc_adjoint per slice."""
    _, n, m = np.shape(x)
    return np.stack([tw.patch_adjoint(g[s], m, n) for s in range(3)])


def vjp(u, x, gu, kappa, refine=10):
    """(grad_f = p (O, N, M), grad_x shaped like x and summed over the images as batch_gradient does, max|p|)."""
    out = [vjp_image(u[k], x, gu[k], kappa, refine) for k in range(len(u))]
    p = np.stack([o[0] for o in out])
    g = sum(o[1] for o in out)
    return p, (g if np.ndim(x) == 1 else _to_x(g, x)), float(np.abs(p).max())


def vjp_each(u, xs, gu, kappa, refine=10):
    """Image k with its own block xs[k]: (grad_f, grad_xs shaped like xs, nothing summed over images, max|p| per image)."""
    out = [vjp_image(u[k], xs[k], gu[k], kappa, refine) for k in range(len(u))]
    p = np.stack([o[0] for o in out])
    g = np.stack([o[1] if np.ndim(xs[k]) == 1 else _to_x(o[1], xs[k]) for k, o in enumerate(out)])
    return p, g, np.abs(p).reshape(len(u), -1).max(axis=1)


def jvp_image(u, x, df, dx, kappa, refine=10):
    """du of one (N, M) image: the same matrix, right-hand side df - sum_k (G_k^T h_k) o up(dx_k) (sumregs_jvp_ref.rhs)."""
    A, _ = system(u, x, kappa)
    return solve(A, jr.rhs(u, x, df, dx, 0), refine).reshape(u.shape)


def jvp(u, x, df, dx, kappa, refine=10):
    """du (O, N, M) for the tangents df ((O, N, M) or None) and dx (shaped like x, or None)."""
    return np.stack([jvp_image(u[k], x, None if df is None else df[k], dx, kappa, refine) for k in range(len(u))])


def jvp_each(u, xs, df, dxs, kappa, refine=10):
    """Image k with its own xs[k] and dxs[k]."""
    return np.stack([jvp_image(u[k], xs[k], None if df is None else df[k], None if dxs is None else dxs[k], kappa, refine)
                     for k in range(len(u))])


def gauss_newton(u, ubar, x, kappa, refine=10):
    """(J^T (u - ubar) shaped like x, J^T J) from one jvp per parameter entry, entries in x.ravel() order."""
    x = np.asarray(x, dtype=np.float64)
    eye = np.eye(x.size).reshape((x.size,) + x.shape)
    J = np.empty((u.size, x.size))
    for k, img in enumerate(u):   # one assembly per image, one refined solve per column
        A, _ = system(img, x, kappa)
        for e in range(x.size):
            J[k * img.size:(k + 1) * img.size, e] = solve(A, jr.rhs(img, x, None, eye[e], 0), refine)
    return (J.T @ (u - ubar).reshape(-1)).reshape(x.shape), J.T @ J


# ---- cases ----------------------------------------------------------------------------------------------------------------
def _frozen(*arrays):
    for a in arrays:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def case(shape, kind, layout):
    """(x, f, u, gu, df, dx): f from synth_batch at SEED, u the twin's iterate after 60 iterations with `layout` planted,
    the cotangent gu and the tangents df, dx (shaped like x) standard normal.  Computed once, shared, read-only."""
    from conftest import synth_batch
    O, N, M = shape
    x = x_kind(kind, N, M)
    _, f = synth_batch(O, N, M, seed=SEED)
    rng = np.random.default_rng(SEED + 1)
    u = plant(ts.pdhg(f, x, maxiter=60), layout)
    gu, df = rng.standard_normal(u.shape), rng.standard_normal(u.shape)
    return _frozen(x, f, u, gu, df, rng.standard_normal(x.shape))


@functools.lru_cache(maxsize=None)
def vjp_ref(shape, kind, layout, kappa, refine=10):
    """(grad_f, grad_x, max|p|) of the literal system with weight kappa: solved once per (case, kappa), shared, read-only."""
    x, f, u, gu, df, dx = case(shape, kind, layout)
    gf, gx, pmax = vjp(u, x, gu, kappa, refine)
    return _frozen(gf, gx) + (pmax,)


@functools.lru_cache(maxsize=None)
def jvp_ref(shape, kind, layout, kappa, which="both", refine=10):
    """du of the literal system for both tangents of the case, or `df` / `dx` alone."""
    x, f, u, gu, df, dx = case(shape, kind, layout)
    return _frozen(jvp(u, x, None if which == "dx" else df, None if which == "df" else dx, kappa, refine))[0]
