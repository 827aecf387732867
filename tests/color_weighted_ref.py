"""numpy twin of channel-coupled TV with a per-pixel fidelity weight and of reverse mode through its iterations (DESIGN.md
section 4.17) -- TEST INFRASTRUCTURE ONLY.

fwd_tape is color_ref.fwd_tape with weighted_unrolled_ref.fwd_tape's primal step and tape (z1, z2, x+ of every plane);
reverse is color_ref.reverse's projection adjoint with weighted_unrolled_ref.reverse's tail, the step table (gamma = min w)
held fixed; torch_reference restates the forward loop in torch ops on the CPU and lets autograd differentiate it.  Arrays
follow color_ref: a batch is (O, N, M) with O = B*C, colour image b owns the planes b*C ... b*C + C-1; a parameter map is
(N, M); a weight is (N, M) -- one plane for every plane of the batch -- or (O, N, M), one per plane (per channel)."""
import functools

import numpy as np

import color_ref as cr
import weighted_ref as wr
from oracle import np_twin as tw


def fwd_tape(f, amap, w, K, C, accel=True, tau0=5.0, sigma0=0.99 / 5):
    """(u, tape, tab): K iterations on the O = B*C planes of f (O, N, M); tape[k] = (z1, z2, x+) of every plane, tab =
    weighted_ref.step_table with gamma = min w.  C = 1 is weighted_unrolled_ref.fwd_tape bit for bit."""
    f = np.asarray(f, dtype=np.float64)
    O, N, M = f.shape
    assert O % C == 0
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
        z1, z2 = y1.reshape(O // C, C, N, M), y2.reshape(O // C, C, N, M)
        n2 = cr._norm2(z1, z2, C)
        with np.errstate(all="ignore"):
            v = np.where(n2 > a2, amap * tw.rsqrt_nr(np.where(n2 > a2, n2, 1.0)), 1.0)
        y1 = (z1 * v).reshape(O, N, M)
        y2 = (z2 * v).reshape(O, N, M)
    return x, tape, tab


def reverse(gu, tape, tab, amap, w, f, C):
    """(grad_f (O, N, M), ga (B, N, M), gw (O, N, M)): dL/df, the per-pixel parameter terms of every colour image and the
    per-pixel, per-plane weight terms for gu = dL/du."""
    gx = np.array(gu, dtype=np.float64)
    O, N, M = gx.shape
    B = O // C
    sh = (B, C, N, M)
    w = wr.weight_planes(w, gx.shape)
    gy1 = np.zeros(sh)
    gy2 = np.zeros(sh)
    gf = np.zeros_like(gx)
    gw = np.zeros_like(gx)
    ga = np.zeros((B, N, M))
    a2 = amap * amap
    for k in range(tape.shape[0] - 1, -1, -1):
        tau, sigma, omega = tab[k]
        z1, z2, xp = tape[k, 0].reshape(sh), tape[k, 1].reshape(sh), tape[k, 2]
        n2 = cr._norm2(z1, z2, C)          # the twin forward's expression on the taped values: the same decision
        out = n2 > a2
        q = tw.rsqrt_nr(np.where(out, n2, 1.0))
        e1 = z1 * q
        e2 = z2 * q
        dot = e1[:, 0] * gy1[:, 0] + e2[:, 0] * gy2[:, 0]
        for c in range(1, C):
            dot = dot + (e1[:, c] * gy1[:, c] + e2[:, c] * gy2[:, c])
        dot = dot[:, None]
        gz1 = np.where(out, (amap * q) * (gy1 - e1 * dot), gy1)
        gz2 = np.where(out, (amap * q) * (gy2 - e2 * dot), gy2)
        ga = ga + np.where(out, dot, 0.0)[:, 0]
        gxb = sigma * tw.grad_fwd_T(gz1.reshape(O, N, M), gz2.reshape(O, N, M))
        gxn = gx + (1.0 + omega) * gxb
        h = gxn * (1.0 / (1.0 + tau * w))
        gf = gf + tau * (w * h)
        gw = gw + tau * ((f - xp) * h)
        d1, d2 = tw.grad_fwd(h)
        gy1 = gz1 - tau * d1.reshape(sh)
        gy2 = gz2 - tau * d2.reshape(sh)
        gx = h - omega * gxb
    return gf + gx, ga, gw


def reduce_w(gw, w):
    """dL/dw in the shape of w: per plane, or for one plane the sum over the planes in plane order."""
    if np.ndim(w) == 3:
        return gw
    g = np.zeros(gw.shape[-2:])
    for k in range(gw.shape[0]):
        g = g + gw[k]
    return g


def torch_reference(f, amap, w, K, gu, C, accel=True):
    """(grad_f, ga summed over the colour images (N, M), grad_w in w's shape) by torch autograd through a torch restatement
    of the forward loop on the CPU, with the projection factor alpha / sqrt(n2) and the step table of gamma = min w as
    constants."""
    import torch
    w = np.asarray(w, dtype=np.float64)
    tab = wr.step_table(K, float(w.min()), accel=accel)
    f = np.asarray(f)
    O, N, M = f.shape
    sh = (O // C, C, N, M)
    ft = torch.tensor(f.reshape(sh), dtype=torch.float64, requires_grad=True)
    at = torch.tensor(np.asarray(amap), dtype=torch.float64, requires_grad=True)
    wt = torch.tensor(w, dtype=torch.float64, requires_grad=True)
    wb = wt if w.ndim == 2 else wt.reshape(sh)

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
        x = (x - tau * (div - wb * ft)) * (1.0 / (1.0 + tau * wb))
        xb = (1.0 + omega) * x - omega * xo
        d1, d2 = G(xb)
        y1 = y1 + sigma * d1
        y2 = y2 + sigma * d2
        n2 = (y1 * y1 + y2 * y2).sum(dim=1, keepdim=True)
        out = n2 > at * at
        v = torch.where(out, at / torch.sqrt(torch.where(out, n2, torch.ones_like(n2))), torch.ones_like(n2))
        y1 = y1 * v
        y2 = y2 * v
    (x * torch.tensor(np.asarray(gu).reshape(sh), dtype=torch.float64)).sum().backward()
    ga = at.grad.numpy() if at.grad is not None else np.zeros((N, M))
    return ft.grad.numpy().reshape(O, N, M), ga, wt.grad.numpy()


def min_decision_margin(tape, amap, C):
    """min | n2 - alpha^2 | / alpha^2 over all pixels and iterations: how far every projection decision is from flipping."""
    return cr.min_decision_margin(tape[:, :2], amap, C)


# ---- the cases tests/test_gpu_color_weighted.py holds against the twin ------------------------------------------------------
SHAPES, KINDS, gpu_data, alpha_of = cr.SHAPES, cr.KINDS, cr.gpu_data, cr.alpha_of
WEIGHTS = ("real", "mask", "mosaic", "ones")
KS = (50, 203)


def weight_of(wkind, B, C, N, M):
    """real: (O, N, M) in [0.25, 4]; mask: one plane in {0, 1}, about 30 % zeros, shared by the channels; mosaic: (O, N, M),
    plane b*C + c is 1 where ((n % 2)*2 + (m % 2)) % C == c and 0 elsewhere (C = 4: one channel kept per pixel); ones: one
    plane."""
    O = B * C
    if wkind == "real":
        return 0.25 + 3.75 * np.random.default_rng(11).random((O, N, M))
    if wkind == "mask":
        return (np.random.default_rng(12).random((N, M)) > 0.3).astype(np.float64)
    if wkind == "mosaic":
        n, m = np.meshgrid(np.arange(N), np.arange(M), indexing="ij")
        cell = ((n % 2) * 2 + (m % 2)) % C
        w = np.empty((O, N, M))
        for p in range(O):
            w[p] = (cell == p % C)
        return w
    assert wkind == "ones"
    return np.ones((N, M))


@functools.lru_cache(maxsize=4)   # (a tape of K = 203 on 2x4x33x70 is 90 MB: the tests use a case, then move on)
def twin_case(name, kind, wkind, K):
    """(u0, tape, tab, gf0, ga0, gw0) of a case by the twin, computed once and shared (read-only)."""
    B, C, N, M = SHAPES[name]
    f, gu = gpu_data(name)
    amap = tw.alpha_to_map(alpha_of(kind, N, M), M, N)
    w = weight_of(wkind, B, C, N, M)
    u0, tape, tab = fwd_tape(f, amap, w, K, C)
    gf0, ga0, gw0 = reverse(gu, tape, tab, amap, w, f, C)
    for a in (u0, tape, gf0, ga0, gw0):
        a.setflags(write=False)
    return u0, tape, tab, gf0, ga0, gw0
