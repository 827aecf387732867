"""numpy twin of forward mode through the channel-coupled PDHG iterations -- TEST INFRASTRUCTURE ONLY.

forward_tangent is color_ref.fwd_tape's loop, operation for operation, that carries the tangent (dx, dy1, dy2) beside
(x, y1, y2) and records nothing: the exact transpose of color_ref.reverse.  With C = 1 it is
unrolled_jvp_ref.forward_tangent bit for bit.  torch_forward_reference restates the forward loop of
color_ref.torch_reference as a function and lets torch's forward-mode AD differentiate it.  Arrays follow color_ref: a batch is
(O, N, M) with O = B*C, colour image b owns the planes b*C ... b*C + C-1; a parameter map and its tangent are (N, M)."""
import functools

import numpy as np

import color_ref as cr
from oracle import np_twin as tw


def forward_tangent(f, amap, K, C, df=None, damap=None, accel=True, tau0=5.0, sigma0=0.99 / 5):
    """(u, du): u = color_ref.fwd_tape(f, amap, K, C)[0] bit for bit and du = (du/df) df + (du/dalpha) damap of the K-step
    map; a tangent that is None is zero."""
    f = np.asarray(f, dtype=np.float64)
    O, N, M = f.shape
    assert O % C == 0
    sh = (O // C, C, N, M)
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
        c_ = 1.0 / (1.0 + tau)
        div = tw.grad_fwd_T(y1, y2)
        xo = x
        x = (x - tau * (div - f)) / (1.0 + tau)
        xb = (1.0 + omega) * x - omega * xo
        ddiv = tw.grad_fwd_T(dy1, dy2)
        dxn = (dx - tau * (ddiv - df)) * c_
        dxb = (1.0 + omega) * dxn - omega * dx
        dx = dxn
        d1, d2 = tw.grad_fwd(xb)
        y1 = y1 + sigma * d1
        y2 = y2 + sigma * d2
        dd1, dd2 = tw.grad_fwd(dxb)
        dz1 = (dy1 + sigma * dd1).reshape(sh)
        dz2 = (dy2 + sigma * dd2).reshape(sh)
        z1, z2 = y1.reshape(sh), y2.reshape(sh)
        n2 = cr._norm2(z1, z2, C)
        out = n2 > a2
        with np.errstate(all="ignore"):
            r = tw.rsqrt_nr(np.where(out, n2, 1.0))
        e1 = z1 * r
        e2 = z2 * r
        dot = e1[:, 0] * dz1[:, 0] + e2[:, 0] * dz2[:, 0]
        for c in range(1, C):
            dot = dot + (e1[:, c] * dz1[:, c] + e2[:, c] * dz2[:, c])
        dot = dot[:, None]
        dy1 = np.where(out, da * e1 + (amap * r) * (dz1 - e1 * dot), dz1).reshape(O, N, M)
        dy2 = np.where(out, da * e2 + (amap * r) * (dz2 - e2 * dot), dz2).reshape(O, N, M)
        v = np.where(out, amap * r, 1.0)
        y1 = (z1 * v).reshape(O, N, M)
        y2 = (z2 * v).reshape(O, N, M)
    return x, dx


def torch_forward_reference(f, amap, K, C, df=None, damap=None, accel=True):
    """(u, du) by torch.func.jvp through color_ref.torch_reference's forward loop on the CPU, with the projection factor
    alpha / sqrt(n2)."""
    import torch
    tab = tw.step_table(K, accel=accel)
    f = np.asarray(f)
    O, N, M = f.shape
    sh = (O // C, C, N, M)
    ft = torch.tensor(f.reshape(sh), dtype=torch.float64)
    at = torch.tensor(np.asarray(amap), dtype=torch.float64)
    dft = torch.zeros_like(ft) if df is None else torch.tensor(np.asarray(df).reshape(sh), dtype=torch.float64)
    dat = torch.zeros_like(at) if damap is None else torch.tensor(np.asarray(damap), dtype=torch.float64)

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
            n2 = (y1 * y1 + y2 * y2).sum(dim=1, keepdim=True)
            out = n2 > av * av
            v = torch.where(out, av / torch.sqrt(torch.where(out, n2, torch.ones_like(n2))), torch.ones_like(n2))
            y1 = y1 * v
            y2 = y2 * v
        return x

    u, du = torch.func.jvp(solve, (ft, at), (dft, dat))
    return u.numpy().reshape(O, N, M), du.numpy().reshape(O, N, M)


# ---- the tangents of the cases tests/test_gpu_color_jvp.py holds against the twin (color_ref.SHAPES, KINDS, alpha_of) -------
WHICH = ("df", "dalpha", "both")


@functools.lru_cache(maxsize=None)
def tangents(name, kind):
    """(df (O, N, M), dalpha shaped like the case's parameter (a float for the scalar), damap (N, M)), read-only."""
    B, C, N, M = cr.SHAPES[name]
    rng = np.random.default_rng(77 + M)
    df = rng.standard_normal((B * C, N, M))
    alpha = cr.alpha_of(kind, N, M)
    da = float(rng.standard_normal()) if kind == "scalar" else rng.standard_normal(np.shape(alpha))
    damap = tw.alpha_to_map(da, M, N)   # the patch upsampling is linear: the tangent's map is the tangent upsampled
    for a in (df, damap) + (() if kind == "scalar" else (da,)):
        a.setflags(write=False)
    return df, da, damap


@functools.lru_cache(maxsize=None)
def twin_tangent(name, kind, K, which):
    """(u0, du0) of a case by the twin, computed once and shared (read-only)."""
    B, C, N, M = cr.SHAPES[name]
    f, _ = cr.gpu_data(name)
    amap = tw.alpha_to_map(cr.alpha_of(kind, N, M), M, N)
    df, _, damap = tangents(name, kind)
    u0, du0 = forward_tangent(f, amap, K, C, df if which != "dalpha" else None, damap if which != "df" else None)
    for a in (u0, du0):
        a.setflags(write=False)
    return u0, du0
