"""numpy twin of reverse mode through the PDHG iterations of the weighted model -- TEST
INFRASTRUCTURE ONLY.

fwd_tape is weighted_ref.pdhg's loop, operation for operation, that also records the dual before every projection and the
new primal iterate; reverse runs the recorded iterations backwards, the step table (gamma = min w) held fixed;
torch_reference restates the forward loop in torch ops on the CPU, on the same fixed table, and lets autograd differentiate
it.  Arrays follow np_twin: batches are (O, N, M), a parameter map is (N, M), a weight is (N, M) or (O, N, M)."""
import numpy as np

import weighted_ref as wr
from oracle import np_twin as tw


def fwd_tape(f, amap, w, K, accel=True, tau0=5.0, sigma0=0.99 / 5):
    """(u, tape, tab): u = weighted_ref.pdhg(f, amap, w, K) bit for bit, tape[k] = (z1, z2, x) with z = y_k + sigma_k G xbar_k
    and x = x_{k+1} of iteration k, tab = weighted_ref.step_table with gamma = min w."""
    f = np.asarray(f, dtype=np.float64)
    w = wr.weight_planes(w, f.shape)
    tab = wr.step_table(K, float(w.min()), tau0, sigma0, accel)
    x = f.copy()
    y1 = np.zeros_like(f)
    y2 = np.zeros_like(f)
    a2 = amap * amap
    tape = np.empty((K, 3) + f.shape)
    for k in range(K):
        tau, sigma, omega = tab[k]
        div = tw.grad_fwd_T(y1, y2)
        xo = x
        x = (x - tau * (div - w * f)) * (1.0 / (1.0 + tau * w))
        xb = (1.0 + omega) * x - omega * xo
        d1, d2 = tw.grad_fwd(xb)
        y1 = y1 + sigma * d1
        y2 = y2 + sigma * d2
        tape[k, 0] = y1
        tape[k, 1] = y2
        tape[k, 2] = x
        n2 = y1 * y1 + y2 * y2
        with np.errstate(all="ignore"):
            v = np.where(n2 > a2, amap * tw.rsqrt_nr(np.where(n2 > a2, n2, 1.0)), 1.0)
        y1 = y1 * v
        y2 = y2 * v
    return x, tape, tab


def reverse(gu, tape, tab, amap, w, f):
    """(grad_f, ga, gw): dL/df, and the per-pixel, per-image terms (O, N, M) of dL/dalpha and dL/dw, for gu = dL/du."""
    gx = np.array(gu, dtype=np.float64)
    w = wr.weight_planes(w, gx.shape)
    gy1 = np.zeros_like(gx)
    gy2 = np.zeros_like(gx)
    gf = np.zeros_like(gx)
    ga = np.zeros_like(gx)
    gw = np.zeros_like(gx)
    a2 = amap * amap
    for k in range(tape.shape[0] - 1, -1, -1):
        tau, sigma, omega = tab[k]
        z1, z2, xp = tape[k]
        n2 = z1 * z1 + z2 * z2          # the twin forward's expression on the taped values: the same decision
        out = n2 > a2
        q = tw.rsqrt_nr(np.where(out, n2, 1.0))
        e1 = z1 * q
        e2 = z2 * q
        dot = e1 * gy1 + e2 * gy2
        gz1 = np.where(out, (amap * q) * (gy1 - e1 * dot), gy1)
        gz2 = np.where(out, (amap * q) * (gy2 - e2 * dot), gy2)
        ga = ga + np.where(out, dot, 0.0)
        gxb = sigma * tw.grad_fwd_T(gz1, gz2)
        gxn = gx + (1.0 + omega) * gxb
        h = gxn * (1.0 / (1.0 + tau * w))
        gf = gf + tau * (w * h)
        gw = gw + tau * ((f - xp) * h)
        d1, d2 = tw.grad_fwd(h)
        gy1 = gz1 - tau * d1
        gy2 = gz2 - tau * d2
        gx = h - omega * gxb
    return gf + gx, ga, gw


def reduce_w(gw, w):
    """dL/dw in the shape of w: per image, or for one plane the sum over the images in image order."""
    if np.ndim(w) == 3:
        return gw
    g = np.zeros(gw.shape[-2:])
    for k in range(gw.shape[0]):
        g = g + gw[k]
    return g


def min_decision_margin(tape, amap):
    """min |n2 - alpha^2| / alpha^2 over all pixels and iterations of a tape: how far every projection decision is from
    flipping."""
    a2 = amap * amap
    n2 = tape[:, 0] * tape[:, 0] + tape[:, 1] * tape[:, 1]
    return float((np.abs(n2 - a2) / a2).min())


def torch_reference(f, amap, w, K, gu, accel=True):
    """(grad_f, ga summed over the images (N, M), grad_w in w's shape) by torch autograd through a torch restatement of
    weighted_ref.pdhg on the CPU, with the projection factor alpha / sqrt(n2) and the step table of gamma = min w as
    constants."""
    import torch
    w = np.asarray(w, dtype=np.float64)
    tab = wr.step_table(K, float(w.min()), accel=accel)
    ft = torch.tensor(np.asarray(f), dtype=torch.float64, requires_grad=True)
    at = torch.tensor(np.asarray(amap), dtype=torch.float64, requires_grad=True)
    wt = torch.tensor(w, dtype=torch.float64, requires_grad=True)
    N, M = ft.shape[-2:]

    def G(x):
        d1 = torch.zeros_like(x)
        d2 = torch.zeros_like(x)
        if M > 1:
            d1 = torch.cat([x[..., :, 1:] - x[..., :, :-1], torch.zeros_like(x[..., :, :1])], dim=-1)
        if N > 1:
            d2 = torch.cat([x[..., 1:, :] - x[..., :-1, :], torch.zeros_like(x[..., :1, :])], dim=-2)
        return d1, d2

    def GT(y1, y2):
        r = torch.zeros_like(y1)
        if M > 1:
            z = torch.zeros_like(y1[..., :, :1])
            r = r + torch.cat([z, y1[..., :, :-1]], dim=-1) - torch.cat([y1[..., :, :-1], z], dim=-1)
        if N > 1:
            z = torch.zeros_like(y2[..., :1, :])
            r = r + torch.cat([z, y2[..., :-1, :]], dim=-2) - torch.cat([y2[..., :-1, :], z], dim=-2)
        return r

    x = ft
    y1 = torch.zeros_like(ft)
    y2 = torch.zeros_like(ft)
    for k in range(K):
        tau, sigma, omega = (float(t) for t in tab[k])
        div = GT(y1, y2)
        xo = x
        x = (x - tau * (div - wt * ft)) * (1.0 / (1.0 + tau * wt))
        xb = (1.0 + omega) * x - omega * xo
        d1, d2 = G(xb)
        y1 = y1 + sigma * d1
        y2 = y2 + sigma * d2
        n2 = y1 * y1 + y2 * y2
        out = n2 > at * at
        v = torch.where(out, at / torch.sqrt(torch.where(out, n2, torch.ones_like(n2))), torch.ones_like(n2))
        y1 = y1 * v
        y2 = y2 * v
    (x * torch.tensor(np.asarray(gu), dtype=torch.float64)).sum().backward()
    ga = at.grad.numpy() if at.grad is not None else np.zeros((N, M))
    return ft.grad.numpy(), ga, wt.grad.numpy()


# ---- the cases tests/test_gpu_weighted_unrolled.py runs (tests/test_weighted_unrolled_abi.py checks their margins) ----
GPU_SHAPES = {"3x40x48": (3, 40, 48), "2x17x33": (2, 17, 33), "1x1x9": (1, 1, 9), "1x9x1": (1, 9, 1), "2x70x72": (2, 70, 72)}
GRADIENT_SHAPES = ["3x40x48", "2x17x33", "1x1x9", "1x9x1"]
GRADIENT_K = (50, 203)


def alpha_of(kind, N, M):
    """tests/test_gpu_unrolled.py's _alpha: scalar, a 2 x 3 patch (cut down on a single row / column), or a map."""
    if kind == "scalar":
        return 0.08
    if kind == "patch":
        return np.array([[0.05, 0.1, 0.07], [0.12, 0.06, 0.09]])[:min(2, N), :min(3, M)].copy()
    return 0.05 + 0.1 * np.random.default_rng(8).random((N, M))


def weight_of(wkind, O, N, M):
    """real: (O, N, M) in [0.25, 4]; mask: one plane in {0, 1}, about 30 % zeros; ones: one plane."""
    if wkind == "real":
        return 0.25 + 3.75 * np.random.default_rng(11).random((O, N, M))
    if wkind == "mask":
        return (np.random.default_rng(12).random((N, M)) > 0.3).astype(np.float64)
    return np.ones((N, M))


def gpu_data(name, seed=5):
    """(f, gu) of a GPU case: tests/test_gpu_unrolled.py's _data."""
    from conftest import synth_batch
    O, N, M = GPU_SHAPES[name]
    _, f = synth_batch(O, N, M, seed=seed + M)
    gu = np.random.default_rng(seed + 100).standard_normal(f.shape)
    return f, gu
