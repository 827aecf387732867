"""numpy twin of reverse mode through the PDHG iterations -- TEST INFRASTRUCTURE ONLY.

fwd_tape is oracle.np_twin.pdhg_denoise's loop, operation for operation, that also records the dual before every
projection; reverse runs the recorded iterations backwards; torch_reference restates the forward loop in torch ops on
the CPU and lets autograd differentiate it.  Arrays follow np_twin: batches are (O, N, M), a parameter map is (N, M)."""
import numpy as np

from oracle import np_twin as tw


def fwd_tape(f, amap, K, accel=True, tau0=5.0, sigma0=0.99 / 5):
    """(u, tape, tab): u = np_twin.pdhg_denoise(f, amap, K) bit for bit, tape[k] = (z1, z2) = y_k + sigma_k G xbar_k of
    iteration k, tab = np_twin.step_table."""
    f = np.asarray(f, dtype=np.float64)
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
        n2 = y1 * y1 + y2 * y2
        with np.errstate(all="ignore"):
            v = np.where(n2 > a2, amap * tw.rsqrt_nr(np.where(n2 > a2, n2, 1.0)), 1.0)
        y1 = y1 * v
        y2 = y2 * v
    return x, tape, tab


def reverse(gu, tape, tab, amap):
    """(grad_f, ga): dL/df and the per-pixel, per-image parameter terms (O, N, M) for the cotangent gu = dL/du."""
    gx = np.array(gu, dtype=np.float64)
    gy1 = np.zeros_like(gx)
    gy2 = np.zeros_like(gx)
    gf = np.zeros_like(gx)
    ga = np.zeros_like(gx)
    a2 = amap * amap
    for k in range(tape.shape[0] - 1, -1, -1):
        tau, sigma, omega = tab[k]
        z1, z2 = tape[k]
        n2 = z1 * z1 + z2 * z2          # the twin forward's expression on the taped values: the same decision
        out = n2 > a2
        r = tw.rsqrt_nr(np.where(out, n2, 1.0))
        e1 = z1 * r
        e2 = z2 * r
        dot = e1 * gy1 + e2 * gy2
        gz1 = np.where(out, (amap * r) * (gy1 - e1 * dot), gy1)
        gz2 = np.where(out, (amap * r) * (gy2 - e2 * dot), gy2)
        ga = ga + np.where(out, dot, 0.0)
        gxb = sigma * tw.grad_fwd_T(gz1, gz2)
        gxn = gx + (1.0 + omega) * gxb
        c = 1.0 / (1.0 + tau)
        gf = gf + tau * c * gxn
        d1, d2 = tw.grad_fwd(gxn)
        gy1 = gz1 - tau * c * d1
        gy2 = gz2 - tau * c * d2
        gx = c * gxn - omega * gxb
    return gf + gx, ga


def reduce_alpha(ga, alpha):
    """dL/dalpha in the type / shape of alpha from the per-pixel terms: over the images in image order, then over all
    pixels (scalar), over each patch (calc_adjoint) or not at all (map)."""
    g = np.zeros(ga.shape[-2:])
    for k in range(ga.shape[0]):
        g = g + ga[k]
    a = np.asarray(alpha)
    if a.ndim == 0:
        return float(g.sum())
    if a.shape == g.shape:
        return g
    return tw.patch_adjoint(g, a.shape[1], a.shape[0])


def pixels_per_entry(alpha, M, N):
    """How many per-pixel terms of ONE image are summed into an entry of dL/dalpha (the largest count)."""
    a = np.asarray(alpha)
    if a.ndim == 0:
        return M * N
    if a.shape == (N, M):
        return 1
    return int(tw.patch_adjoint(np.ones((N, M)), a.shape[1], a.shape[0]).max())


def torch_reference(f, amap, K, gu, accel=True):
    """(grad_f, ga summed over the images (N, M)) by torch autograd through a torch restatement of the forward loop on the
    CPU, with the projection factor alpha / sqrt(n2)."""
    import torch
    tab = tw.step_table(K, accel=accel)
    ft = torch.tensor(np.asarray(f), dtype=torch.float64, requires_grad=True)
    at = torch.tensor(np.asarray(amap), dtype=torch.float64, requires_grad=True)
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
        x = (x - tau * (div - ft)) / (1.0 + tau)
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
    return ft.grad.numpy(), ga
