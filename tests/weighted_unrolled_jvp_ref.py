"""numpy twin of forward mode through the PDHG iterations of the weighted model -- TEST
INFRASTRUCTURE ONLY.

forward_tangent is weighted_unrolled_ref.fwd_tape's loop, operation for operation, that carries the tangent (dx, dy1, dy2)
beside (x, y1, y2) and records nothing: the exact transpose of weighted_unrolled_ref.reverse, the step table (gamma = min w)
held fixed.  torch_forward_reference restates the forward loop of weighted_unrolled_ref.torch_reference as a function of
(f, alpha, w) on that fixed table and lets torch's forward-mode AD differentiate it.  Arrays follow np_twin: batches are
(O, N, M), a parameter map and its tangent are (N, M), a weight and its tangent are (N, M) or (O, N, M)."""
import numpy as np

import weighted_ref as wr
from oracle import np_twin as tw


def forward_tangent(f, amap, w, K, df=None, damap=None, dw=None, accel=True, tau0=5.0, sigma0=0.99 / 5):
    """(u, du): u = weighted_ref.pdhg(f, amap, w, K) bit for bit and du = (du/df) df + (du/dalpha) damap + (du/dw) dw of the
    K-step map; a tangent that is None is zero."""
    f = np.asarray(f, dtype=np.float64)
    w = wr.weight_planes(w, f.shape)
    df = np.zeros_like(f) if df is None else np.asarray(df, dtype=np.float64)
    da = np.zeros_like(amap) if damap is None else np.asarray(damap, dtype=np.float64)
    dw = np.zeros_like(f) if dw is None else wr.weight_planes(dw, f.shape)
    tab = wr.step_table(K, float(w.min()), tau0, sigma0, accel)
    x = f.copy()
    y1 = np.zeros_like(f)
    y2 = np.zeros_like(f)
    dx = df.copy()
    dy1 = np.zeros_like(f)
    dy2 = np.zeros_like(f)
    a2 = amap * amap
    for k in range(K):
        tau, sigma, omega = tab[k]
        r = 1.0 / (1.0 + tau * w)
        div = tw.grad_fwd_T(y1, y2)
        xo = x
        x = (x - tau * (div - w * f)) * r
        xb = (1.0 + omega) * x - omega * xo
        ddiv = tw.grad_fwd_T(dy1, dy2)
        dxn = (dx - tau * ((ddiv - w * df) - dw * (f - x))) * r
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
            q = tw.rsqrt_nr(np.where(out, n2, 1.0))
            v = np.where(out, amap * q, 1.0)
        e1 = y1 * q
        e2 = y2 * q
        dot = e1 * dz1 + e2 * dz2
        dy1 = np.where(out, da * e1 + (amap * q) * (dz1 - e1 * dot), dz1)
        dy2 = np.where(out, da * e2 + (amap * q) * (dz2 - e2 * dot), dz2)
        y1 = y1 * v
        y2 = y2 * v
    return x, dx


def torch_forward_reference(f, amap, w, K, df=None, damap=None, dw=None, accel=True):
    """(u, du) by torch forward-mode AD (torch.func.jvp) through weighted_unrolled_ref.torch_reference's loop on the CPU, with
    the projection factor alpha / sqrt(n2) and the step table of gamma = min w as constants."""
    import torch
    w = np.asarray(w, dtype=np.float64)
    tab = wr.step_table(K, float(w.min()), accel=accel)
    ft = torch.tensor(np.asarray(f), dtype=torch.float64)
    at = torch.tensor(np.asarray(amap), dtype=torch.float64)
    wt = torch.tensor(w, dtype=torch.float64)
    dft = torch.zeros_like(ft) if df is None else torch.tensor(np.asarray(df), dtype=torch.float64)
    dat = torch.zeros_like(at) if damap is None else torch.tensor(np.asarray(damap), dtype=torch.float64)
    dwt = torch.zeros_like(wt) if dw is None else torch.tensor(np.asarray(dw), dtype=torch.float64)
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

    def solve(fv, av, wv):
        x = fv
        y1 = torch.zeros_like(fv)
        y2 = torch.zeros_like(fv)
        for k in range(K):
            tau, sigma, omega = (float(t) for t in tab[k])
            div = GT(y1, y2)
            xo = x
            x = (x - tau * (div - wv * fv)) * (1.0 / (1.0 + tau * wv))
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

    u, du = torch.func.jvp(solve, (ft, at, wt), (dft, dat, dwt))
    return u.numpy(), du.numpy()


# ---- what tests/test_weighted_unrolled_jvp_abi.py settles on the CPU and tests/test_gpu_weighted_unrolled_jvp.py reuses ----
# w == 1 against the TV sweep: the two differ in rounding only ((div - 1*f) * r against (div - f) * c), like either against
# torch's forward mode, which both twins are held to at this bound; the CPU test keeps it a decade above what it measures
UNIT_WEIGHT_RTOL = 1e-11
# central differences: step and relative bound in the maximum norm (at h = 1e-6 the masked K = 300 case flips a projection
# decision)
CD_H, CD_RTOL = 1e-7, 1e-5


def central_difference_case(wkind):
    """(f, alpha, w, directions) of the central-difference checks, here and on the GPU: 1 x 24 x 28, alpha = 0.08, the mask of
    weight_of("mask") or the real weight; one direction each in alpha (dalpha = 1), in f and in w -- the w direction zero where
    w = 0 (the one-sided derivative there is not a central difference's) and, for the real weight, where w attains its minimum
    (gamma, and with it the step table the sweep holds fixed, stays what it is)."""
    from conftest import synth_batch
    import weighted_unrolled_ref as wur
    _, f = synth_batch(1, 24, 28, seed=9)
    w = wur.weight_of(wkind, 1, 24, 28)
    rng = np.random.default_rng(21)
    df = rng.standard_normal(f.shape)
    dw = rng.standard_normal(w.shape) * (w > 0)
    if wkind == "real":
        dw = dw * (w > w.min())
    return f, 0.08, w, (("alpha", None, 1.0, None), ("f", df, None, None), ("w", None, None, dw))
