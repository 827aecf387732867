"""numpy twin of reverse mode through the PDHG iterations of the sum-of-regularisers model -- TEST
INFRASTRUCTURE ONLY.

fwd_tape is oracle/np_twin_sumregs.pdhg's loop, operation for operation, that also records the six dual components before
their projection; reverse runs the recorded iterations backwards with the transposes of the same three sparse matrices
(np_twin_sumregs.grad_matrix: the border rules come from there); torch_reference restates the forward loop in torch ops on
the CPU and lets autograd differentiate it.  Arrays follow np_twin_sumregs: batches are (O, N, M), the parameter is (3,) or
(3, n, m), parameter maps are (3, N, M); a tape is (K, 6, O, N, M) with the components f1, f2, b1, b2, c1, c2."""
import math

import numpy as np

from oracle import np_twin as T
from oracle import np_twin_sumregs as sr


def _batch(f):
    f = np.asarray(f, dtype=np.float64)
    return f if f.ndim == 3 else f[None]


def fwd_tape(f, alpha, K, accel=True, tau0=5.0, sigma0=0.99 / 5):
    """(u, tape, tab): u = np_twin_sumregs.pdhg(f, alpha, K) bit for bit, tape[k, 2r:2r+2] = z_k^(r) = y_k^(r) + sigma_k G_r
    xbar_k, tab[k] = (tau_k, sigma_k, omega_k).  alpha: (3,), (3, n, m), or (O, 3) / (O, 3, n, m) for one block per image."""
    fb = _batch(f)
    O, N, M = fb.shape
    n = N * M
    a = np.asarray(alpha, dtype=np.float64)
    each = a.ndim in (2, 4)
    G = [sr.grad_matrix(k, M, N) for k in range(3)]
    u = np.empty_like(fb)
    tape = np.empty((K, 6, O, N, M))
    tab = np.empty((K, 3))
    for o in range(O):
        am = sr.alpha_maps(a[o] if each else a, M, N)
        fo = fb[o].reshape(-1)
        x = fo.copy()
        y = [np.zeros(2 * n) for _ in range(3)]
        tau, sigma = tau0 / sr.SR_L, sigma0 / sr.SR_L
        for k in range(K):
            omega = 1.0 / math.sqrt(1.0 + 2.0 * tau) if accel else 1.0
            tab[k] = (tau, sigma, omega)
            div = (G[0].T @ y[0] + G[1].T @ y[1]) + G[2].T @ y[2]
            xo = x
            x = (x - tau * (div - fo)) / (1.0 + tau)
            xb = (1.0 + omega) * x - omega * xo
            for r in range(3):
                yk = y[r] + sigma * (G[r] @ xb)
                tape[k, 2 * r, o] = yk[:n].reshape(N, M)
                tape[k, 2 * r + 1, o] = yk[n:].reshape(N, M)
                ar = am[r].reshape(-1)
                nrm = np.sqrt(yk[:n] ** 2 + yk[n:] ** 2)
                sc = np.where(nrm > ar, ar / np.where(nrm > ar, nrm, 1.0), 1.0)
                y[r] = yk * np.concatenate([sc, sc])
            if accel:
                tau, sigma = tau * omega, sigma / omega
        u[o] = x.reshape(N, M)
    return u.reshape(np.shape(f)), tape, tab


def maps_of(alpha, O, N, M):
    """(3, O, N, M) parameter maps of a shared parameter or of O per-image blocks."""
    a = np.asarray(alpha, dtype=np.float64)
    if a.ndim in (2, 4):
        return np.stack([sr.alpha_maps(a[o], M, N) for o in range(O)], axis=1)
    return np.repeat(sr.alpha_maps(a, M, N)[:, None], O, axis=1)


def reverse(gu, tape, tab, alpha_maps):
    """(grad_f, ga): dL/df (O, N, M) and the per-pixel, per-image terms (3, O, N, M) of dL/dalpha, for gu = dL/du.
    alpha_maps: (3, N, M), or (3, O, N, M) for one block per image."""
    gub = _batch(gu)
    O, N, M = gub.shape
    n = N * M
    K = tape.shape[0]
    amaps = np.asarray(alpha_maps, dtype=np.float64)
    if amaps.ndim == 3:
        amaps = np.repeat(amaps[:, None], O, axis=1)
    G = [sr.grad_matrix(k, M, N) for k in range(3)]
    grad_f = np.empty_like(gub)
    ga = np.zeros((3, O, N, M))
    for o in range(O):
        gx = gub[o].reshape(-1).copy()
        gy = [np.zeros(2 * n) for _ in range(3)]
        gf = np.zeros(n)
        for k in range(K - 1, -1, -1):
            tau, sigma, omega = tab[k]
            gz = []
            for r in range(3):
                a = amaps[r, o].reshape(-1)
                z1 = tape[k, 2 * r, o].reshape(-1)
                z2 = tape[k, 2 * r + 1, o].reshape(-1)
                nrm = np.sqrt(z1 ** 2 + z2 ** 2)      # the twin forward's expression on the taped values: the same decision
                out = nrm > a
                q = 1.0 / np.where(out, nrm, 1.0)
                e1, e2 = z1 * q, z2 * q
                g1, g2 = gy[r][:n], gy[r][n:]
                dot = e1 * g1 + e2 * g2
                gz.append(np.concatenate([np.where(out, (a * q) * (g1 - e1 * dot), g1),
                                          np.where(out, (a * q) * (g2 - e2 * dot), g2)]))
                ga[r, o] += np.where(out, dot, 0.0).reshape(N, M)
            gxb = sigma * ((G[0].T @ gz[0] + G[1].T @ gz[1]) + G[2].T @ gz[2])
            gxn = gx + (1.0 + omega) * gxb
            h = gxn / (1.0 + tau)
            gf = gf + tau * h
            for r in range(3):
                gy[r] = gz[r] - tau * (G[r] @ h)
            gx = h - omega * gxb
        grad_f[o] = (gf + gx).reshape(N, M)
    return grad_f.reshape(np.shape(gu)), ga


def reduce_alpha(ga, alpha):
    """dL/dalpha in the shape of alpha from the per-pixel, per-image terms (3, O, N, M): a shared parameter sums over the
    images in image order, then over all pixels (vector) or each patch (np_twin.patch_adjoint); per-image blocks keep image
    k's own terms."""
    a = np.asarray(alpha, dtype=np.float64)
    _, O, N, M = ga.shape

    def block(g3, shape):   # g3: (3, N, M)
        if len(shape) == 1:
            return np.array([g3[r].sum() for r in range(3)])
        _, n, m = shape
        return np.stack([T.patch_adjoint(g3[r], m, n) for r in range(3)])

    if a.ndim in (2, 4):
        return np.stack([block(ga[:, o], a.shape[1:]) for o in range(O)])
    g = np.zeros((3, N, M))
    for o in range(O):
        g = g + ga[:, o]
    return block(g, a.shape)


def min_decision_margin(tape, alpha_maps):
    """min | |z|^2 - a^2 | / a^2 over all pixels, iterations and regularisers of a tape: how far every projection decision
    is from flipping.  Slices whose entry is 0 are skipped (|z|^2 > 0 decides there, at any rounding)."""
    amaps = np.asarray(alpha_maps, dtype=np.float64)
    if amaps.ndim == 3:
        amaps = amaps[:, None]
    worst = np.inf
    for r in range(3):
        a2 = amaps[r] * amaps[r]
        n2 = tape[:, 2 * r] ** 2 + tape[:, 2 * r + 1] ** 2
        a2b = np.broadcast_to(a2, n2.shape)
        pos = a2b > 0
        if pos.any():
            worst = min(worst, float((np.abs(n2 - a2b)[pos] / a2b[pos]).min()))
    return worst


def torch_reference(f, alpha_maps, K, gu, accel=True, tau0=5.0, sigma0=0.99 / 5):
    """(grad_f, ga (3, O, N, M)) by torch autograd through a torch restatement of np_twin_sumregs.pdhg on the CPU, with the
    projection factor a / sqrt(n2) and the step sizes as constants.  alpha_maps: (3, N, M) or (3, O, N, M)."""
    import torch
    fb = _batch(f)
    O, N, M = fb.shape
    n = N * M
    amaps = np.asarray(alpha_maps, dtype=np.float64)
    if amaps.ndim == 3:
        amaps = np.repeat(amaps[:, None], O, axis=1)

    def sparse(m):
        c = m.tocoo()
        return torch.sparse_coo_tensor(np.vstack([c.row, c.col]), c.data, c.shape, dtype=torch.float64).coalesce()

    G = [sparse(sr.grad_matrix(k, M, N)) for k in range(3)]
    GT = [sparse(sr.grad_matrix(k, M, N).T) for k in range(3)]
    ft = torch.tensor(fb.reshape(O, n).T.copy(), dtype=torch.float64, requires_grad=True)            # (n, O)
    at = torch.tensor(amaps.reshape(3, O, n).transpose(0, 2, 1).copy(), dtype=torch.float64, requires_grad=True)   # (3, n, O)
    x = ft
    y = [torch.zeros(2 * n, O, dtype=torch.float64) for _ in range(3)]
    tau, sigma = tau0 / sr.SR_L, sigma0 / sr.SR_L
    for _ in range(K):
        omega = 1.0 / math.sqrt(1.0 + 2.0 * tau) if accel else 1.0
        div = (torch.sparse.mm(GT[0], y[0]) + torch.sparse.mm(GT[1], y[1])) + torch.sparse.mm(GT[2], y[2])
        xo = x
        x = (x - tau * (div - ft)) / (1.0 + tau)
        xb = (1.0 + omega) * x - omega * xo
        for r in range(3):
            yk = y[r] + sigma * torch.sparse.mm(G[r], xb)
            n2 = yk[:n] ** 2 + yk[n:] ** 2
            out = torch.sqrt(n2) > at[r]
            sc = torch.where(out, at[r] / torch.sqrt(torch.where(out, n2, torch.ones_like(n2))), torch.ones_like(n2))
            y[r] = yk * torch.cat([sc, sc])
        if accel:
            tau, sigma = tau * omega, sigma / omega
    gut = torch.tensor(_batch(gu).reshape(O, n).T.copy(), dtype=torch.float64)
    (x * gut).sum().backward()
    grad_f = ft.grad.numpy().T.reshape(O, N, M)
    ga = at.grad.numpy().transpose(0, 2, 1).reshape(3, O, N, M) if at.grad is not None else np.zeros((3, O, N, M))
    return grad_f.reshape(np.shape(gu)), ga


# ---- the cases tests/test_gpu_sumregs_unrolled.py runs (tests/test_sumregs_unrolled_abi.py checks their margins) ----
GPU_SHAPES = {"2x40x48": (2, 40, 48), "2x17x33": (2, 17, 33), "1x1x9": (1, 1, 9), "1x9x1": (1, 9, 1), "1x2x2": (1, 2, 2),
              "2x70x72": (2, 70, 72)}
GRADIENT_SHAPES = ["2x40x48", "2x17x33", "1x1x9", "1x9x1", "1x2x2"]
GRADIENT_K = (50, 203)
ALPHA_KINDS = ("vector", "patch", "map", "zero")
SEEDS = {}   # (shape name, alpha kind) -> data seed, where the default (5) leaves a decision closer than 1e-9


def alpha_of(kind, N, M):
    """vector; three 2 x 3 patches (cut down on a single row / column); three maps; the vector with a zero slice."""
    if kind == "vector":
        return np.array([0.03, 0.02, 0.04])
    if kind == "zero":
        return np.array([0.03, 0.0, 0.04])
    if kind == "patch":
        p = np.array([[0.03, 0.05, 0.02], [0.04, 0.025, 0.035]])[:min(2, N), :min(3, M)]
        return np.stack([p, 0.7 * p, 1.3 * p])
    return 0.02 + 0.04 * np.random.default_rng(8).random((3, N, M))


def gpu_data(name, kind="vector"):
    """(f, gu) of a GPU case: tests/test_gpu_unrolled.py's _data, with the seed of SEEDS."""
    from conftest import synth_batch
    O, N, M = GPU_SHAPES[name]
    seed = SEEDS.get((name, kind), 5)
    _, f = synth_batch(O, N, M, seed=seed + M)
    gu = np.random.default_rng(seed + 100).standard_normal(f.shape)
    return f, gu


def fd_case():
    """The central-difference case: (ubar, f, alpha, h), loss 0.5 ||u_K - ubar||^2, K = 30 and 300."""
    from conftest import synth_batch
    ubar, f = synth_batch(1, 24, 28, seed=9)
    return ubar, f, np.array([0.03, 0.02, 0.04]), 1e-7
