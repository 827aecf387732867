"""numpy twin of TV-L1 denoising and of reverse mode through its iterations -- TEST INFRASTRUCTURE
ONLY.

fwd_tape is weighted_unrolled_ref.fwd_tape's loop with the L1 primal step, a soft threshold around f, on the step table of
gamma = 0 (whatever w is); reverse is weighted_unrolled_ref.reverse with the L1 tail, which decides on the tape alone;
torch_reference restates the forward loop in torch ops on the CPU and lets autograd differentiate it.  Arrays follow np_twin:
batches are (O, N, M), a parameter map is (N, M), a weight is (N, M) or (O, N, M)."""
import functools

import numpy as np

import weighted_ref as wr
import weighted_unrolled_ref as wur
from oracle import np_twin as tw


def step_table(K, tau0=5.0, sigma0=0.99 / 5, accel=True):
    """weighted_ref.step_table with gamma = 0: omega = 1 and constant steps, with or without the acceleration."""
    return wr.step_table(K, 0.0, tau0, sigma0, accel)


def fwd_tape(f, amap, w, K, accel=True, tau0=5.0, sigma0=0.99 / 5, stats=None):
    """(u, tape, tab): K iterations from x = f, y = 0; tape[k] = (z1, z2, x+) of iteration k.  stats (a dict, optional) receives
    the smallest threshold margin min |m| / max(tau w, |d|) over the pixels with w > 0 and all iterations, the share of
    pixel-iterations in which the threshold let the step through (m > 0), and min |d| over the pixels with w = 0 in the iterations
    whose div there is not exactly zero (it is in iteration 0, where y = 0): the sign of d is grad_w's there."""
    f = np.asarray(f, dtype=np.float64)
    w = wr.weight_planes(w, f.shape)
    tab = step_table(K, tau0, sigma0, accel)
    x = f.copy()
    y1 = np.zeros_like(f)
    y2 = np.zeros_like(f)
    a2 = amap * amap
    tape = np.empty((K, 3) + f.shape)
    margin, active, nodata = np.inf, 0, np.inf
    for k in range(K):
        tau, sigma, omega = tab[k]
        div = tw.grad_fwd_T(y1, y2)
        xo = x
        v = x - tau * div
        d = v - f
        s = tau * w
        m = np.abs(d) - s
        x = np.where(m > 0, f + np.copysign(m, d), f)
        if stats is not None:
            pos = np.broadcast_to(w > 0, f.shape)
            if pos.any():
                margin = min(margin, float((np.abs(m[pos]) / np.maximum(np.broadcast_to(s, f.shape)[pos], np.abs(d[pos]))).min()))
            active += int((m > 0).sum())
            free = np.broadcast_to(w == 0, f.shape) & (div != 0)
            if free.any():
                nodata = min(nodata, float(np.abs(d[free]).min()))
        xb = (1.0 + omega) * x - omega * xo
        d1, d2 = tw.grad_fwd(xb)
        y1 = y1 + sigma * d1
        y2 = y2 + sigma * d2
        tape[k, 0] = y1
        tape[k, 1] = y2
        tape[k, 2] = x
        n2 = y1 * y1 + y2 * y2
        with np.errstate(all="ignore"):
            p = np.where(n2 > a2, amap * tw.rsqrt_nr(np.where(n2 > a2, n2, 1.0)), 1.0)
        y1 = y1 * p
        y2 = y2 * p
    if stats is not None:
        stats["threshold_margin"] = margin
        stats["active_share"] = active / float(K * f.size)
        stats["nodata_margin"] = nodata
    return x, tape, tab


def reverse(gu, tape, tab, amap, w, f):
    """(grad_f, ga, gw): dL/df, and the per-pixel, per-image terms (O, N, M) of dL/dalpha and dL/dw, for gu = dL/du.  act and the
    sign are read off the tape (x+ and f); of w only where it is zero: there the threshold is the identity whatever d is."""
    gx = np.array(gu, dtype=np.float64)
    f = np.asarray(f, dtype=np.float64)
    nodata = np.broadcast_to(wr.weight_planes(w, gx.shape) == 0, gx.shape)
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
        act = (xp != f) | nodata
        sg = np.sign(xp - f)
        h = np.where(act, gxn, 0.0)
        gf = gf + np.where(act, 0.0, gxn)
        gw = gw + (-tau) * (sg * h)
        d1, d2 = tw.grad_fwd(h)
        gy1 = gz1 - tau * d1
        gy2 = gz2 - tau * d2
        gx = h - omega * gxb
    return gf + gx, ga, gw


reduce_w = wur.reduce_w
min_decision_margin = wur.min_decision_margin


def torch_reference(f, amap, w, K, gu, accel=True):
    """(grad_f, ga summed over the images (N, M), grad_w in w's shape) by torch autograd through a torch restatement of
    fwd_tape on the CPU, with the projection factor alpha / sqrt(n2) and the soft threshold as relu(|d| - tau w) sign(d), plus d
    where w = 0 and d = 0 -- the same value, zero; it carries the identity's derivative there, which autograd's sign(0) = 0 cuts."""
    import torch
    w = np.asarray(w, dtype=np.float64)
    tab = step_table(K, accel=accel)
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
        d = (x - tau * div) - ft
        x = ft + torch.sign(d) * torch.relu(torch.abs(d) - tau * wt) + torch.where((wt == 0) & (d == 0), d, torch.zeros_like(d))
        xb = (1.0 + omega) * x - omega * xo
        d1, d2 = G(xb)
        y1 = y1 + sigma * d1
        y2 = y2 + sigma * d2
        n2 = y1 * y1 + y2 * y2
        out = n2 > at * at
        p = torch.where(out, at / torch.sqrt(torch.where(out, n2, torch.ones_like(n2))), torch.ones_like(n2))
        y1 = y1 * p
        y2 = y2 * p
    (x * torch.tensor(np.asarray(gu), dtype=torch.float64)).sum().backward()
    ga = at.grad.numpy() if at.grad is not None else np.zeros((N, M))
    return ft.grad.numpy(), ga, wt.grad.numpy()


# ---- the cases tests/test_gpu_l1.py runs (tests/test_l1_abi.py checks their margins and that both branches are taken) ----
GPU_SHAPES = wur.GPU_SHAPES
GRADIENT_SHAPES = wur.GRADIENT_SHAPES
GRADIENT_K = wur.GRADIENT_K
KINDS = ("scalar", "patch", "map")
WEIGHTS = ("real", "mask", "ones")


def gpu_data(name):
    """(f, gu) of a GPU case: weighted_unrolled_ref.gpu_data's, with f taken off its grid of 1 / 255 by Gaussian noise of 1e-3: on
    the grid the four differences around a pixel cancel exactly at about one pixel in a hundred, div is then zero up to rounding
    for many iterations, and at a pixel without data (w = 0) the sign of d, which grad_w reads, is that rounding.  A single row or
    column of nine pixels is nearly a ramp there, on which the threshold lets next to nothing through in 50 iterations; it gets
    salt-and-pepper noise on about 30 % of its pixels, the noise this model is for."""
    f, gu = wur.gpu_data(name)
    O, N, M = GPU_SHAPES[name]
    f = f + 1e-3 * np.random.default_rng(45).standard_normal(f.shape)
    if min(N, M) == 1:
        rng = np.random.default_rng(44)
        hit = rng.random(f.shape) < 0.3
        f[hit] = (rng.random(f.shape) < 0.5)[hit].astype(np.float64)
    return f, gu


def alpha_of(kind, N, M):
    """scalar, a 2 x 3 patch (cut down on a single row / column), or a map -- around 0.5 ... 1, where with w near 1 both
    branches of the threshold are taken (at the quadratic models' 0.08 nearly every pixel stays at f); 1.5 times that on a
    single row or column, where a pixel has two neighbours, not four."""
    c = 1.5 if min(N, M) == 1 else 1.0
    if kind == "scalar":
        return c * 0.7
    if kind == "patch":
        return c * np.array([[0.5, 0.9, 0.65], [1.0, 0.55, 0.8]])[:min(2, N), :min(3, M)].copy()
    return c * (0.5 + 0.5 * np.random.default_rng(8).random((N, M)))


def weight_of(wkind, O, N, M):
    """real: (O, N, M) in [0.5, 2]; mask: one plane in {0, 1}, about 30 % zeros; ones: one plane."""
    if wkind == "real":
        return 0.5 + 1.5 * np.random.default_rng(11).random((O, N, M))
    if wkind == "mask":
        return (np.random.default_rng(12).random((N, M)) > 0.3).astype(np.float64)
    assert wkind == "ones"
    return np.ones((N, M))


def spikes():
    """(f, heights): the constant plane 0.5 of 17 x 33 with four isolated spikes.  With w = 1, removing a spike of height h costs
    w h and saves (2 + sqrt 2) alpha h: for alpha >= 0.35 the solution is the constant, for alpha = 0.2 it is f."""
    f = np.full((1, 17, 33), 0.5)
    heights = {(4, 6): 0.4, (11, 9): -0.3, (7, 20): 0.25, (13, 28): -0.45}
    for (n, m), h in heights.items():
        f[0, n, m] += h
    return f, heights


@functools.lru_cache(maxsize=8)
def twin_case(name, kind, wkind, K):
    """(u0, gf0, ga0, gw0, stats) of a case by the twin, computed once and shared (read-only); stats: fwd_tape's, and
    decision_margin = min |n2 - alpha^2| / alpha^2."""
    O, N, M = GPU_SHAPES[name]
    f, gu = gpu_data(name)
    amap = tw.alpha_to_map(alpha_of(kind, N, M), M, N)
    w = weight_of(wkind, O, N, M)
    stats = {}
    u0, tape, tab = fwd_tape(f, amap, w, K, stats=stats)
    stats["decision_margin"] = min_decision_margin(tape, amap)
    gf0, ga0, gw0 = reverse(gu, tape, tab, amap, w, f)
    for a in (u0, gf0, ga0, gw0):
        a.setflags(write=False)
    return u0, gf0, ga0, gw0, stats


CD_ALPHA, CD_K, CD_H = 0.7, 30, 1e-6


def central_difference_case():
    """(ub, f, w, df, dw) of the central-difference checks, on the CPU and on the device: synth_batch(1, 24, 28, seed=9), a mask
    with about 30 % zeros, a random direction of f and one of w that is zero where w = 0."""
    from conftest import synth_batch
    ub, f = synth_batch(1, 24, 28, seed=9)
    rng = np.random.default_rng(21)
    w = weight_of("mask", 1, 24, 28)
    dw = rng.standard_normal(w.shape) * w
    df = rng.standard_normal(f.shape)
    return ub, f, w, df, dw
