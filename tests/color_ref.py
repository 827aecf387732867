"""numpy twin of channel-coupled (vectorial) TV and of reverse mode through its iterations -- TEST
INFRASTRUCTURE ONLY.

fwd_tape is unrolled_ref.fwd_tape's loop per plane, with the projection taken per pixel of a colour image over its C planes
in channel order; reverse runs the recorded iterations backwards; torch_reference restates the forward loop in torch ops on
the CPU and lets autograd differentiate it.  Arrays follow np_twin: a batch is (O, N, M) with O = B*C, colour image b owns
the planes b*C ... b*C + C-1; a parameter map is (N, M), shared by the batch and the channels."""
import functools

import numpy as np

from oracle import np_twin as tw


def _norm2(y1, y2, C):
    """(B, 1, N, M): z1_0^2, + z2_0^2, + z1_1^2, ... in channel order (y: (B, C, N, M))."""
    n2 = y1[:, 0] * y1[:, 0]
    n2 = n2 + y2[:, 0] * y2[:, 0]
    for c in range(1, C):
        n2 = n2 + y1[:, c] * y1[:, c]
        n2 = n2 + y2[:, c] * y2[:, c]
    return n2[:, None]


def fwd_tape(f, amap, K, C, accel=True, tau0=5.0, sigma0=0.99 / 5):
    """(u, tape, tab): K iterations on the O = B*C planes of f (O, N, M); tape[k] = (z1, z2) of every plane before the
    projection, tab = np_twin.step_table.  C = 1 is unrolled_ref.fwd_tape bit for bit."""
    f = np.asarray(f, dtype=np.float64)
    O, N, M = f.shape
    assert O % C == 0
    tab = tw.step_table(K, tau0, sigma0, accel)
    x = f.copy()
    y1 = np.zeros_like(f)
    y2 = np.zeros_like(f)
    a2 = amap * amap
    tape = np.empty((K, 2) + f.shape)
    for k in range(K):
        tau, sigma, omega = tab[k]
        div = tw.grad_fwd_T(y1, y2)
        xo = x
        x = (x - tau * (div - f)) / (1.0 + tau)
        xb = (1.0 + omega) * x - omega * xo
        d1, d2 = tw.grad_fwd(xb)
        y1 = y1 + sigma * d1
        y2 = y2 + sigma * d2
        tape[k, 0] = y1
        tape[k, 1] = y2
        z1, z2 = y1.reshape(O // C, C, N, M), y2.reshape(O // C, C, N, M)
        n2 = _norm2(z1, z2, C)
        with np.errstate(all="ignore"):
            v = np.where(n2 > a2, amap * tw.rsqrt_nr(np.where(n2 > a2, n2, 1.0)), 1.0)
        y1 = (z1 * v).reshape(O, N, M)
        y2 = (z2 * v).reshape(O, N, M)
    return x, tape, tab


def reverse(gu, tape, tab, amap, C):
    """(grad_f (O, N, M), ga (B, N, M)): dL/df and the per-pixel parameter terms of every colour image for gu = dL/du."""
    gx = np.array(gu, dtype=np.float64)
    O, N, M = gx.shape
    B = O // C
    sh = (B, C, N, M)
    gy1 = np.zeros(sh)
    gy2 = np.zeros(sh)
    gf = np.zeros_like(gx)
    ga = np.zeros((B, N, M))
    a2 = amap * amap
    for k in range(tape.shape[0] - 1, -1, -1):
        tau, sigma, omega = tab[k]
        z1, z2 = tape[k, 0].reshape(sh), tape[k, 1].reshape(sh)
        n2 = _norm2(z1, z2, C)          # the twin forward's expression on the taped values: the same decision
        out = n2 > a2
        r = tw.rsqrt_nr(np.where(out, n2, 1.0))
        e1 = z1 * r
        e2 = z2 * r
        dot = e1[:, 0] * gy1[:, 0] + e2[:, 0] * gy2[:, 0]
        for c in range(1, C):
            dot = dot + (e1[:, c] * gy1[:, c] + e2[:, c] * gy2[:, c])
        dot = dot[:, None]
        gz1 = np.where(out, (amap * r) * (gy1 - e1 * dot), gy1)
        gz2 = np.where(out, (amap * r) * (gy2 - e2 * dot), gy2)
        ga = ga + np.where(out, dot, 0.0)[:, 0]
        gxb = sigma * tw.grad_fwd_T(gz1.reshape(O, N, M), gz2.reshape(O, N, M))
        gxn = gx + (1.0 + omega) * gxb
        c_ = 1.0 / (1.0 + tau)
        gf = gf + tau * c_ * gxn
        d1, d2 = tw.grad_fwd(gxn)
        gy1 = gz1 - tau * c_ * d1.reshape(sh)
        gy2 = gz2 - tau * c_ * d2.reshape(sh)
        gx = c_ * gxn - omega * gxb
    return gf + gx, ga


def torch_reference(f, amap, K, gu, C, accel=True):
    """(grad_f, ga summed over the colour images (N, M)) by torch autograd through a torch restatement of the forward loop on
    the CPU, with the projection factor alpha / sqrt(n2)."""
    import torch
    tab = tw.step_table(K, accel=accel)
    f = np.asarray(f)
    O, N, M = f.shape
    ft = torch.tensor(f.reshape(O // C, C, N, M), dtype=torch.float64, requires_grad=True)
    at = torch.tensor(np.asarray(amap), dtype=torch.float64, requires_grad=True)

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
        x = (x - tau * (div - ft)) / (1.0 + tau)
        xb = (1.0 + omega) * x - omega * xo
        d1, d2 = G(xb)
        y1 = y1 + sigma * d1
        y2 = y2 + sigma * d2
        n2 = (y1 * y1 + y2 * y2).sum(dim=1, keepdim=True)
        out = n2 > at * at
        v = torch.where(out, at / torch.sqrt(torch.where(out, n2, torch.ones_like(n2))), torch.ones_like(n2))
        y1 = y1 * v
        y2 = y2 * v
    (x * torch.tensor(np.asarray(gu).reshape(O // C, C, N, M), dtype=torch.float64)).sum().backward()
    ga = at.grad.numpy() if at.grad is not None else np.zeros((N, M))
    return ft.grad.numpy().reshape(O, N, M), ga


def min_decision_margin(tape, amap, C):
    """min | n2 - alpha^2 | / alpha^2 over all pixels and iterations: how far every projection decision is from flipping."""
    K, _, O, N, M = tape.shape
    sh = (O // C, C, N, M)
    a2 = amap * amap
    worst = np.inf
    for k in range(K):
        n2 = _norm2(tape[k, 0].reshape(sh), tape[k, 1].reshape(sh), C)
        worst = min(worst, float((np.abs(n2 - a2) / a2).min()))
    return worst


# ---- the cases tests/test_gpu_color.py holds against the twin ---------------------------------------------------------------
SHAPES = {"2x3x17x33": (2, 3, 17, 33), "1x3x40x48": (1, 3, 40, 48), "1x2x9x1": (1, 2, 9, 1), "1x4x1x9": (1, 4, 1, 9),
          "1x3x2x2": (1, 3, 2, 2), "2x4x33x70": (2, 4, 33, 70)}   # (B, C, N, M)
KS = (7, 50, 203)
KINDS = ("scalar", "patch", "map")


def alpha_of(kind, N, M):
    """scalar 0.08, a 2 x 3 patch (cut down where the image has fewer rows / columns), or a map in [0.05, 0.11]."""
    if kind == "scalar":
        return 0.08
    if kind == "patch":
        return np.array([[0.05, 0.1, 0.07], [0.12, 0.06, 0.09]])[:min(2, N), :min(3, M)].copy()
    return 0.05 + 0.06 * np.random.default_rng(8).random((N, M))


@functools.lru_cache(maxsize=None)
def gpu_data(name, seed=5):
    """(f (B*C, N, M), gu) of a case, read-only: synth_batch(B*C, N, M, seed + M) and a standard-normal cotangent."""
    from conftest import synth_batch
    B, C, N, M = SHAPES[name]
    _, f = synth_batch(B * C, N, M, seed=seed + M)
    gu = np.random.default_rng(seed + 100).standard_normal(f.shape)
    for a in (f, gu):
        a.setflags(write=False)
    return f, gu


@functools.lru_cache(maxsize=None)
def twin_case(name, kind, K):
    """(u0, tape, tab, gf0, ga0) of a case by the twin, computed once and shared (read-only)."""
    B, C, N, M = SHAPES[name]
    f, gu = gpu_data(name)
    amap = tw.alpha_to_map(alpha_of(kind, N, M), M, N)
    u0, tape, tab = fwd_tape(f, amap, K, C)
    gf0, ga0 = reverse(gu, tape, tab, amap, C)
    for a in (u0, tape, gf0, ga0):
        a.setflags(write=False)
    return u0, tape, tab, gf0, ga0
