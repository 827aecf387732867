"""numpy twin of forward mode through the PDHG iterations -- TEST INFRASTRUCTURE ONLY.

forward_tangent is unrolled_ref.fwd_tape's loop, operation for operation, that carries the tangent (dx, dy1, dy2) beside
(x, y1, y2) and records nothing: the exact transpose of unrolled_ref.reverse.  torch_forward_reference restates the forward
loop of unrolled_ref.torch_reference as a function and lets torch's forward-mode AD differentiate it.  Arrays follow np_twin:
batches are (O, N, M), a parameter map and its tangent are (N, M)."""
import numpy as np

from oracle import np_twin as tw


def forward_tangent(f, amap, K, df=None, damap=None, accel=True, tau0=5.0, sigma0=0.99 / 5):
    """(u, du): u = np_twin.pdhg_denoise(f, amap, K) bit for bit and du = (du/df) df + (du/dalpha) damap of the K-step map;
    a tangent that is None is zero."""
    f = np.asarray(f, dtype=np.float64)
    df = np.zeros_like(f) if df is None else np.asarray(df, dtype=np.float64)
    da = np.zeros_like(amap) if damap is None else np.asarray(damap, dtype=np.float64)
    tab = tw.step_table(K, tau0, sigma0, accel)
    x = f.copy()
    y1 = np.zeros_like(f)
    y2 = np.zeros_like(f)
    dx = df.copy()
    dy1 = np.zeros_like(f)
    dy2 = np.zeros_like(f)
    a2 = amap * amap
    for k in range(K):
        tau, sigma, omega = tab[k]
        c = 1.0 / (1.0 + tau)
        div = tw.grad_fwd_T(y1, y2)
        xo = x
        x = (x - tau * (div - f)) / (1.0 + tau)
        xb = (1.0 + omega) * x - omega * xo
        ddiv = tw.grad_fwd_T(dy1, dy2)
        dxn = (dx - tau * (ddiv - df)) * c
        dxb = (1.0 + omega) * dxn - omega * dx
        dx = dxn
        d1, d2 = tw.grad_fwd(xb)
        y1 = y1 + sigma * d1
        y2 = y2 + sigma * d2
        dd1, dd2 = tw.grad_fwd(dxb)
        dz1 = dy1 + sigma * dd1
        dz2 = dy2 + sigma * dd2
        n2 = y1 * y1 + y2 * y2
        out = n2 > a2
        with np.errstate(all="ignore"):
            r = tw.rsqrt_nr(np.where(out, n2, 1.0))
        e1 = y1 * r
        e2 = y2 * r
        dot = e1 * dz1 + e2 * dz2
        dy1 = np.where(out, da * e1 + (amap * r) * (dz1 - e1 * dot), dz1)
        dy2 = np.where(out, da * e2 + (amap * r) * (dz2 - e2 * dot), dz2)
        v = np.where(out, amap * r, 1.0)
        y1 = y1 * v
        y2 = y2 * v
    return x, dx


def torch_forward_reference(f, amap, K, df=None, damap=None, accel=True):
    """(u, du) by torch forward-mode AD through unrolled_ref.torch_reference's loop on the CPU, with the projection factor
    alpha / sqrt(n2)."""
    import torch
    tab = tw.step_table(K, accel=accel)
    ft = torch.tensor(np.asarray(f), dtype=torch.float64)
    at = torch.tensor(np.asarray(amap), dtype=torch.float64)
    dft = torch.zeros_like(ft) if df is None else torch.tensor(np.asarray(df), dtype=torch.float64)
    dat = torch.zeros_like(at) if damap is None else torch.tensor(np.asarray(damap), dtype=torch.float64)
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

    def solve(fv, av):
        x = fv
        y1 = torch.zeros_like(fv)
        y2 = torch.zeros_like(fv)
        for k in range(K):
            tau, sigma, omega = (float(t) for t in tab[k])
            div = GT(y1, y2)
            xo = x
            x = (x - tau * (div - fv)) / (1.0 + tau)
            xb = (1.0 + omega) * x - omega * xo
            d1, d2 = G(xb)
            y1 = y1 + sigma * d1
            y2 = y2 + sigma * d2
            n2 = y1 * y1 + y2 * y2
            out = n2 > av * av
            v = torch.where(out, av / torch.sqrt(torch.where(out, n2, torch.ones_like(n2))), torch.ones_like(n2))
            y1 = y1 * v
            y2 = y2 * v
        return x

    u, du = torch.func.jvp(solve, (ft, at), (dft, dat))
    return u.numpy(), du.numpy()
