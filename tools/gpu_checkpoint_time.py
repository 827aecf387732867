#!/usr/bin/env python3
"""Developer probe: what a checkpointed tape costs against the full one.

    python tools/gpu_checkpoint_time.py [--reps 5] [--iters 5000] [--models tv sumregs] [--spacing -1] [--out DIR]
    python tools/gpu_checkpoint_time.py --large       (8 x 1024^2, a pixel map, 2000 iterations: checkpointed only)

10 x 128^2, a scalar parameter (TV: 0.08; sum of regularisers: (0.03, 0.02, 0.04)), one MI355X.  Per model and iteration
count, after a warm-up of every call (graphs built, workspaces allocated), `reps` rounds in which ONE handle runs in
alternation
    the plain solve (bpltv_denoise_device / bpltv_sumregs_denoise_device, the 32 x 32 kernel)     -> stats.pdhg_ms
    the taped solve on a caller's full tape, and its sweep                                          -> pdhg_ms, adjoint_ms
    the checkpoint solve on a caller's checkpoints (checkpoint_every = spacing), and its sweep     -> pdhg_ms, adjoint_ms
HIP-event medians with min / max, both buffer sizes, the handle's segment workspace, whether u and both gradients are
bitwise equal, and the ratio the scheme predicts to be 1: checkpointed sweep / (full-tape sweep + taped solve).  One JSON
line per case, collected in DIR/checkpoint_time.json.  A count whose full tape does not fit is measured checkpointed only."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

KEYS = ("tile_iters", "tiles", "launches", "launch_chains", "graph_used", "bytes_per_px_iter")


def _stats(xs):
    import numpy as np
    xs = np.asarray(xs, dtype=float)
    return {"median": float(np.median(xs)), "min": float(xs.min()), "max": float(xs.max()), "n": int(xs.size)}


def time_case(model, K, reps, spacing, O=10, n=128, amap=False):
    import torch
    from conftest import synth_batch
    from bpldenoising_amd import TVSolver
    ub, f = synth_batch(O, n, n, seed=5)
    dev = torch.device("cuda", 0)
    tf, tub = torch.from_numpy(f).to(dev), torch.from_numpy(ub).to(dev)
    sr = model == "sumregs"
    base = torch.tensor([0.03, 0.02, 0.04] if sr else [0.08], dtype=torch.float64, device=dev)
    if amap:
        ta = (base.reshape(-1, 1, 1) * (0.75 + 0.5 * torch.rand(n, n, dtype=torch.float64, device=dev))).contiguous()
        am = an = n
    else:
        ta, am, an = base, 1, 1
    s = TVSolver(n, n, O, device=0)
    s.set_data_device(tub.data_ptr(), tf.data_ptr())
    pre = "sumregs_" if sr else ""
    plain = getattr(s, pre + "denoise_device")
    solve = getattr(s, pre + "unrolled_denoise_device")
    sweep = getattr(s, pre + "unrolled_vjp_device")
    doubles = getattr(s, pre + "unrolled_tape_doubles")
    plain_kw = dict(variant=1) if sr else {}
    n_full, n_ck = doubles(maxiter=K), doubles(maxiter=K, checkpoint_every=spacing)
    with_full = 8 * n_full <= 0.7 * torch.cuda.mem_get_info(dev)[0]
    free0 = torch.cuda.mem_get_info(dev)[0]
    full = torch.empty(n_full, dtype=torch.float64, device=dev) if with_full else None
    ck = torch.empty(n_ck, dtype=torch.float64, device=dev)
    u0, u1, u2 = torch.empty_like(tf), torch.empty_like(tf), torch.empty_like(tf)
    gf1, gf2 = torch.empty_like(tf), torch.empty_like(tf)
    ga1, ga2 = torch.empty(ta.numel(), dtype=torch.float64, device=dev), torch.empty(ta.numel(), dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    rows = {k: [] for k in ("plain_pdhg_ms", "taped_pdhg_ms", "full_vjp_ms", "checkpoint_pdhg_ms", "checkpoint_vjp_ms")}
    plans = {}
    for r in range(reps + 1):          # round 0 is the warm-up
        t = {}
        plain(ta.data_ptr(), am, an, maxiter=K, **plain_kw)
        t["plain_pdhg_ms"] = s.stats()["pdhg_ms"]
        s.copy_u_device(u0.data_ptr())
        gu = u0 - tub
        torch.cuda.synchronize()
        if with_full:
            solve(ta.data_ptr(), am, an, tape_ptr=full.data_ptr(), maxiter=K)
            st = s.stats()
            t["taped_pdhg_ms"] = st["pdhg_ms"]
            plans["taped"] = {k: st[k] for k in KEYS}
            s.copy_u_device(u1.data_ptr())
            sweep(full.data_ptr(), ta.data_ptr(), am, an, gu.data_ptr(), gf1.data_ptr(), ga1.data_ptr(), maxiter=K)
            t["full_vjp_ms"] = s.stats()["adjoint_ms"]
        solve(ta.data_ptr(), am, an, tape_ptr=ck.data_ptr(), maxiter=K, checkpoint_every=spacing)
        st = s.stats()
        t["checkpoint_pdhg_ms"] = st["pdhg_ms"]
        plans["checkpoint"] = {k: st[k] for k in KEYS}
        s.copy_u_device(u2.data_ptr())
        sweep(ck.data_ptr(), ta.data_ptr(), am, an, gu.data_ptr(), gf2.data_ptr(), ga2.data_ptr(), maxiter=K, checkpoint_every=spacing)
        t["checkpoint_vjp_ms"] = s.stats()["adjoint_ms"]
        if r:
            for k, v in t.items():
                rows[k].append(v)
    torch.cuda.synchronize()
    nplanes, tape_planes = (7, 6) if sr else (3, 2)
    ceff = s.auto_checkpoint_every(K, model) if spacing == -1 else min(spacing, K)
    out = {"case": "%s %dx%dx%d %s" % (model, O, n, n, "map" if amap else "scalar"), "maxiter": K, "spacing": ceff,
           "full_tape_MB": n_full * 8 / 1e6, "checkpoints_MB": n_ck * 8 / 1e6,
           "segment_workspace_MB": (tape_planes * ceff + 2 * nplanes) * O * n * n * 8 / 1e6,
           "hbm_taken_MB": (free0 - torch.cuda.mem_get_info(dev)[0]) / 1e6, "plans": plans,
           "u_bitwise_equal": bool(torch.equal(u0, u2)) and (not with_full or bool(torch.equal(u0, u1)))}
    if with_full:
        out["gradients_bitwise_equal"] = bool(torch.equal(gf1, gf2)) and bool(torch.equal(ga1, ga2))
    out.update({k: _stats(v) for k, v in rows.items() if v})
    med = lambda k: out[k]["median"]
    if with_full:
        out["ratios"] = {"checkpointed sweep / (full-tape sweep + taped solve)": med("checkpoint_vjp_ms") / (med("full_vjp_ms") + med("taped_pdhg_ms")),
                         "checkpoint solve / taped solve": med("checkpoint_pdhg_ms") / med("taped_pdhg_ms"),
                         "checkpoint solve / plain solve": med("checkpoint_pdhg_ms") / med("plain_pdhg_ms")}
    s.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, nargs="+", default=[5000])
    ap.add_argument("--models", nargs="+", default=["tv", "sumregs"], choices=["tv", "sumregs"])
    ap.add_argument("--spacing", type=int, default=-1)
    ap.add_argument("--large", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "results"))
    a = ap.parse_args()
    res = []
    if a.large:
        res.append(time_case("tv", 2000, min(a.reps, 2), a.spacing, O=8, n=1024, amap=True))
        print(json.dumps(res[-1]), flush=True)
    else:
        for model in a.models:
            for K in a.iters:
                res.append(time_case(model, K, a.reps, a.spacing))
                print(json.dumps(res[-1]), flush=True)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "checkpoint_time_large.json" if a.large else "checkpoint_time.json"), "w") as fh:
        json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
