"""numpy twin of forward mode through the TV-L1 and the TV-KL iterations -- TEST INFRASTRUCTURE ONLY.

forward_tangent is l1_ref.fwd_tape's / kl_ref.fwd_tape's loop, operation for operation, that carries the tangent (dx, dy1, dy2)
beside (x, y1, y2) and records nothing: the exact transpose of the model's reverse, which decides on x+, f and w what this decides
on them, on the step table of gamma = 0.  torch_forward_reference restates the twins' torch_reference loops as functions of
(f, alpha, w) and lets torch's forward-mode AD differentiate them.  Arrays follow np_twin: batches are (O, N, M), a parameter map
and its tangent are (N, M), a weight and its tangent are (N, M) or (O, N, M)."""
import functools

import numpy as np

import kl_ref as kr
import l1_ref as lr
import weighted_ref as wr
from oracle import np_twin as tw

MODELS = ("l1", "kl")
REF = {"l1": lr, "kl": kr}


def forward_tangent(model, f, amap, w, K, df=None, dam=None, dw=None, accel=True, tau0=5.0, sigma0=0.99 / 5):
    """(u, du): u = the model's fwd_tape(f, amap, w, K)[0] bit for bit and du = (du/df) df + (du/dalpha) dam + (du/dw) dw of the
    K-step map; a tangent that is None is zero.  No fma in the tangent."""
    assert model in MODELS
    f = np.asarray(f, dtype=np.float64)
    w = wr.weight_planes(w, f.shape)
    df = np.zeros_like(f) if df is None else np.asarray(df, dtype=np.float64)
    da = np.zeros_like(amap) if dam is None else np.asarray(dam, dtype=np.float64)
    dw = np.zeros_like(f) if dw is None else np.broadcast_to(wr.weight_planes(dw, f.shape), f.shape)
    tab = lr.step_table(K, tau0, sigma0, accel)
    x = f.copy()
    y1 = np.zeros_like(f)
    y2 = np.zeros_like(f)
    dx = df.copy()
    dy1 = np.zeros_like(f)
    dy2 = np.zeros_like(f)
    a2 = amap * amap
    nodata = np.broadcast_to(w == 0, f.shape)
    for k in range(K):
        tau, sigma, omega = tab[k]
        div = tw.grad_fwd_T(y1, y2)
        xo = x
        v = x - tau * div
        dv = dx - tau * tw.grad_fwd_T(dy1, dy2)
        if model == "l1":
            d = v - f
            m = np.abs(d) - tau * w
            x = np.where(m > 0, f + np.copysign(m, d), f)
            act = (x != f) | nodata
            dxn = np.where(act, dv - tau * (np.sign(x - f) * dw), df)
        else:
            t = tau * w
            x = kr.prox(v - t, t * f)
            D = t * f + x * x
            q = np.where(D > 0, x / np.where(D > 0, D, 1.0), 0.0)
            dxn = q * (x * dv + t * df + tau * ((f - x) * dw))
        xb = (1.0 + omega) * x - omega * xo
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
            p = np.where(out, amap * q, 1.0)
        e1 = y1 * q
        e2 = y2 * q
        dot = e1 * dz1 + e2 * dz2
        dy1 = np.where(out, da * e1 + (amap * q) * (dz1 - e1 * dot), dz1)
        dy2 = np.where(out, da * e2 + (amap * q) * (dz2 - e2 * dot), dz2)
        y1 = y1 * p
        y2 = y2 * p
    return x, dx


def torch_forward_reference(model, f, amap, w, K, df=None, dam=None, dw=None, accel=True):
    """(u, du) by torch forward-mode AD (torch.func.jvp) through l1_ref.torch_reference's / kl_ref.torch_reference's loop on the
    CPU: the projection factor alpha / sqrt(n2); the soft threshold as relu(|d| - tau w) sign(d), plus d where w = 0 and d = 0;
    the KL prox as 0.5 (c + sqrt(c^2 + 4 tau w f))."""
    import torch
    w = np.asarray(w, dtype=np.float64)
    tab = lr.step_table(K, accel=accel)
    ft = torch.tensor(np.asarray(f), dtype=torch.float64)
    at = torch.tensor(np.asarray(amap), dtype=torch.float64)
    wt = torch.tensor(w, dtype=torch.float64)
    dft = torch.zeros_like(ft) if df is None else torch.tensor(np.asarray(df), dtype=torch.float64)
    dat = torch.zeros_like(at) if dam is None else torch.tensor(np.asarray(dam), dtype=torch.float64)
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
            if model == "l1":
                d = (x - tau * div) - fv
                x = fv + torch.sign(d) * torch.relu(torch.abs(d) - tau * wv) + torch.where((wv == 0) & (d == 0), d, torch.zeros_like(d))
            else:
                c = (x - tau * div) - tau * wv
                x = 0.5 * (c + torch.sqrt(c * c + 4.0 * (tau * wv * fv)))
            xb = (1.0 + omega) * x - omega * xo
            d1, d2 = G(xb)
            y1 = y1 + sigma * d1
            y2 = y2 + sigma * d2
            n2 = y1 * y1 + y2 * y2
            out = n2 > av * av
            p = torch.where(out, av / torch.sqrt(torch.where(out, n2, torch.ones_like(n2))), torch.ones_like(n2))
            y1 = y1 * p
            y2 = y2 * p
        return x

    u, du = torch.func.jvp(solve, (ft, at, wt), (dft, dat, dwt))
    return u.numpy(), du.numpy()


# ---- the cases tests/test_gpu_l1_kl_jvp.py runs (tests/test_l1_kl_jvp_abi.py settles them on the CPU) ----
GPU_SHAPES = lr.GPU_SHAPES
GRADIENT_SHAPES = lr.GRADIENT_SHAPES
GRADIENT_K = lr.GRADIENT_K
KINDS = lr.KINDS
WEIGHTS = lr.WEIGHTS
DIRECTIONS = ("f", "alpha", "w", "all")

# The dalpha-alone direction of L1 on the single row and the single column at K = 50: where the nine pixels end held at f or flat
# the tangent is identically zero.  (name, kind, wkind); tests/test_l1_kl_jvp_abi.py asserts that the twin gives zeros for exactly
# these and a non-zero du on at least 5 % of the pixels for every other (model, case, depth, single direction).
L1_ZERO_DALPHA_K = 50
L1_ZERO_DALPHA = frozenset({
    ("1x1x9", "scalar", "real"), ("1x1x9", "scalar", "ones"), ("1x1x9", "patch", "real"), ("1x1x9", "patch", "mask"),
    ("1x1x9", "patch", "ones"), ("1x1x9", "map", "real"), ("1x1x9", "map", "ones"),
    ("1x9x1", "scalar", "real"), ("1x9x1", "scalar", "mask"), ("1x9x1", "patch", "real"), ("1x9x1", "map", "real"),
    ("1x9x1", "map", "mask"), ("1x9x1", "map", "ones"),
})


def is_zero_case(model, name, kind, wkind, K, direction):
    """The tangent of this case is identically zero (and is no tangent check)."""
    return model == "l1" and direction == "alpha" and K == L1_ZERO_DALPHA_K and (name, kind, wkind) in L1_ZERO_DALPHA


def tangents_of(name, wkind, kind):
    """(df, dalpha, dam, dw) of a case: standard-normal tangents in the shapes of f, of the parameter (dalpha; dam is its map)
    and of w; read-only."""
    return _tangents_of(name, wkind, kind)


@functools.lru_cache(maxsize=None)
def _tangents_of(name, wkind, kind):
    O, N, M = GPU_SHAPES[name]
    df = np.random.default_rng(305).standard_normal((O, N, M))
    w = lr.weight_of(wkind, O, N, M)
    dw = np.random.default_rng(306).standard_normal(w.shape)
    alpha = lr.alpha_of(kind, N, M)
    g = np.random.default_rng(11).standard_normal(np.shape(alpha))
    dalpha = float(g) if np.ndim(alpha) == 0 else g
    dam = np.full((N, M), dalpha) if np.ndim(dalpha) == 0 else tw.alpha_to_map(dalpha, M, N)
    for a in (df, dw, dam):
        a.setflags(write=False)
    return df, dalpha, dam, dw


def case(model, name, kind, wkind):
    """(f, gu, alpha, amap, w) of a gradient case of a model: the committed helpers' data."""
    ref = REF[model]
    O, N, M = GPU_SHAPES[name]
    f, gu = ref.gpu_data(name)
    alpha = ref.alpha_of(kind, N, M)
    return f, gu, alpha, tw.alpha_to_map(alpha, M, N), ref.weight_of(wkind, O, N, M)


def select(direction, df, dalpha, dam, dw):
    """The tangents of a direction: (df, dalpha, dam, dw) with None for those that are not in it."""
    return (df if direction in ("f", "all") else None, dalpha if direction in ("alpha", "all") else None,
            dam if direction in ("alpha", "all") else None, dw if direction in ("w", "all") else None)


@functools.lru_cache(maxsize=None)
def twin_tangent(model, name, kind, wkind, K, direction):
    """(u0, du0) of a case and direction by the twin, computed once and shared (read-only)."""
    f, _, _, amap, w = case(model, name, kind, wkind)
    tf, _, tam, tw_ = select(direction, *tangents_of(name, wkind, kind))
    u0, du0 = forward_tangent(model, f, amap, w, K, tf, tam, tw_)
    u0.setflags(write=False)
    du0.setflags(write=False)
    return u0, du0



def cross_model_case():
    """(f, alpha, w, K, df, dam, dw) on which the weighted, the L1 and the KL sweep run side by side: kl_ref's 3 x 40 x 48 (f > 0,
    which KL needs), the mask -- min w = 0, so the weighted model's step table is the flat one too and nothing but the kernel
    tells the three apart --, alpha = 0.15, 57 iterations (no multiple of a fusion depth); read-only tangents."""
    name = "3x40x48"
    O, N, M = GPU_SHAPES[name]
    f, _ = kr.gpu_data(name)
    w = lr.weight_of("mask", O, N, M)
    df, _, _, dw = tangents_of(name, "mask", "scalar")
    return f, 0.15, w, 57, df, np.full((N, M), 1.0), dw
