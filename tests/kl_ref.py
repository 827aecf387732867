"""numpy twin of TV-KL denoising and of reverse mode through its iterations -- TEST INFRASTRUCTURE
ONLY.

fwd_tape is l1_ref.fwd_tape's loop with the KL primal step, the closed-form prox of w (u - f log u), on the step table of
gamma = 0 (whatever w is); reverse is l1_ref.reverse with the KL tail, which needs the tape, f, w and tau only;
torch_reference restates the forward loop in torch ops on the CPU, with the plain form of the prox -- another expression for the
same value -- and lets autograd differentiate it.  Arrays follow np_twin: batches are (O, N, M), a parameter map is (N, M), a
weight is (N, M) or (O, N, M)."""
import functools

import numpy as np

import l1_ref as lr
import weighted_ref as wr
import weighted_unrolled_ref as wur
from oracle import np_twin as tw

step_table = lr.step_table      # gamma = 0: omega = 1, constant steps, with or without the acceleration
reduce_w = wur.reduce_w
min_decision_margin = wur.min_decision_margin
weight_of = lr.weight_of        # real: (O, N, M) in [0.5, 2]; mask: one plane in {0, 1}, about 30 % zeros; ones: one plane


def prox(c, g):
    """The positive root of u^2 - c u - g = 0 (g = tau w f >= 0) in the form without cancellation: 0.5 (c + s) for c >= 0,
    2 g / (s - c) for c < 0, s = sqrt(c^2 + 4 g)."""
    s = np.sqrt(c * c + 4.0 * g)
    with np.errstate(all="ignore"):
        return np.where(c >= 0, 0.5 * (c + s), (2.0 * g) / np.where(c >= 0, 1.0, s - c))


def prox_plain(c, g):
    """The same root as 0.5 (c + sqrt(c^2 + 4 g)): cancels for c << 0."""
    return 0.5 * (c + np.sqrt(c * c + 4.0 * g))


def fwd_tape(f, amap, w, K, accel=True, tau0=5.0, sigma0=0.99 / 5, stats=None, plain=False):
    """(u, tape, tab): K iterations from x = f, y = 0; tape[k] = (z1, z2, x+) of iteration k.  stats (a dict, optional) receives
    min x+ over all pixels and iterations, the share of pixel-iterations with c < 0 (the second branch of the prox) and the share
    with the projection active (n2 > alpha^2).  plain: the prox in its plain form."""
    f = np.asarray(f, dtype=np.float64)
    w = wr.weight_planes(w, f.shape)
    tab = step_table(K, tau0, sigma0, accel)
    x = f.copy()
    y1 = np.zeros_like(f)
    y2 = np.zeros_like(f)
    a2 = amap * amap
    tape = np.empty((K, 3) + f.shape)
    xmin, neg, act = np.inf, 0, 0
    for k in range(K):
        tau, sigma, omega = tab[k]
        div = tw.grad_fwd_T(y1, y2)
        xo = x
        v = x - tau * div
        t = tau * w
        c = v - t
        g = t * f
        x = prox_plain(c, g) if plain else prox(c, g)
        xb = (1.0 + omega) * x - omega * xo
        d1, d2 = tw.grad_fwd(xb)
        y1 = y1 + sigma * d1
        y2 = y2 + sigma * d2
        tape[k, 0] = y1
        tape[k, 1] = y2
        tape[k, 2] = x
        n2 = y1 * y1 + y2 * y2
        if stats is not None:
            xmin = min(xmin, float(x.min()))
            neg += int((c < 0).sum())
            act += int((n2 > a2).sum())
        with np.errstate(all="ignore"):
            p = np.where(n2 > a2, amap * tw.rsqrt_nr(np.where(n2 > a2, n2, 1.0)), 1.0)
        y1 = y1 * p
        y2 = y2 * p
    if stats is not None:
        stats["min_x"] = xmin
        stats["neg_share"] = neg / float(K * f.size)
        stats["active_share"] = act / float(K * f.size)
    return x, tape, tab


def reverse(gu, tape, tab, amap, w, f):
    """(grad_f, ga, gw): dL/df, and the per-pixel, per-image terms (O, N, M) of dL/dalpha and dL/dw, for gu = dL/du.  The tail
    reads x+ off the tape: e = gxn / s with s = x+ + t f / x+, and nothing is passed where x+ = 0 exactly (the convention)."""
    gx = np.array(gu, dtype=np.float64)
    f = np.asarray(f, dtype=np.float64)
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
        t = tau * w
        D = t * f + xp * xp
        qd = np.where(D > 0, xp / np.where(D > 0, D, 1.0), 0.0)
        e = qd * gxn
        h = xp * e
        gf = gf + t * e
        gw = gw + tau * ((f - xp) * e)
        d1, d2 = tw.grad_fwd(h)
        gy1 = gz1 - tau * d1
        gy2 = gz2 - tau * d2
        gx = h - omega * gxb
    return gf + gx, ga, gw


def torch_reference(f, amap, w, K, gu, accel=True):
    """(grad_f, ga summed over the images (N, M), grad_w in w's shape) by torch autograd through a torch restatement of
    fwd_tape on the CPU, with the projection factor alpha / sqrt(n2) and the prox as 0.5 (c + sqrt(c^2 + 4 tau w f))."""
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
        c = (x - tau * div) - tau * wt
        x = 0.5 * (c + torch.sqrt(c * c + 4.0 * (tau * wt * ft)))
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


# ---- the cases tests/test_gpu_kl.py runs (tests/test_kl_abi.py checks their margins and that both branches are taken) ----
GPU_SHAPES = wur.GPU_SHAPES
GRADIENT_SHAPES = wur.GRADIENT_SHAPES
GRADIENT_K = wur.GRADIENT_K
KINDS = ("scalar", "patch", "map")
WEIGHTS = ("real", "mask", "ones")
PEAK, BACKGROUND = 30.0, 0.1


def poisson_data(name):
    """(clean, counts / PEAK): weighted_unrolled_ref.gpu_data's f clipped at 0 and scaled to a peak of PEAK counts, and Poisson
    samples of it (fixed seed) divided by PEAK -- photon-limited data, with zero counts."""
    f, _ = wur.gpu_data(name)
    clean = np.clip(f, 0.0, None)
    clean = clean * (PEAK / clean.max())
    return clean / PEAK, np.random.default_rng(31).poisson(clean).astype(np.float64) / PEAK


def gpu_data(name):
    """(f, gu) of a GPU case: poisson_data's samples on a background of BACKGROUND, so that f > 0, every iterate stays clear of
    zero and no gradient check depends on the x+ = 0 convention; gu is weighted_unrolled_ref.gpu_data's."""
    _, gu = wur.gpu_data(name)
    return poisson_data(name)[1] + BACKGROUND, gu


def alpha_of(kind, N, M):
    """scalar 0.15, a 2 x 3 patch (cut down on a single row / column) or a map in [0.08, 0.2]; about half of that on a single row
    or column, where a pixel has two neighbours, not four (at 0.15 the masked 1 x 9 x 1 case never leaves the ball in 50
    iterations)."""
    c = 0.5 if min(N, M) == 1 else 1.0
    if kind == "scalar":
        return 0.08 if min(N, M) == 1 else 0.15
    if kind == "patch":
        return c * np.array([[0.08, 0.2, 0.12], [0.18, 0.1, 0.15]])[:min(2, N), :min(3, M)].copy()
    return c * (0.08 + 0.12 * np.random.default_rng(8).random((N, M)))


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


CD_ALPHA, CD_K, CD_H = 0.15, 30, 1e-6


def central_difference_case():
    """(ub, f, w, df, dw) of the central-difference checks, on the CPU and on the device: l1_ref.central_difference_case's (a
    masked 1 x 24 x 28) with f clipped at 0 plus 0.02."""
    ub, f, w, df, dw = lr.central_difference_case()
    return ub, np.clip(f, 0.0, None) + 0.02, w, df, dw


def layer_case():
    """(f, alpha, w, K, h, gu, dw) of the torch layer's central differences of <u, gu> along alpha and along dw (zero where w = 0): 1 x 8 x 9, f in [0.1, 1.1], alpha = 0.1, w in [0.05, 0.15]
    with about 30 % zeros, 20 iterations.  With weights this small the data term hardly holds the image and the iterations flatten
    it before most duals reach alpha: the projection is active in a few pixel-iterations only (tests/test_kl_abi.py counts them;
    the seed is one of those where there are any)."""
    rng = np.random.default_rng(34)
    f = 0.1 + rng.random((1, 8, 9))
    w = (0.05 + 0.1 * rng.random((8, 9))) * (rng.random((8, 9)) > 0.3)
    gu = np.random.default_rng(3).standard_normal(f.shape)
    dw = np.random.default_rng(4).standard_normal(w.shape) * (w > 0)
    return f, 0.1, w, 20, 1e-6, gu, dw
