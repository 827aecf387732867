#!/usr/bin/env python3
"""Developer probe: what the channel coupling costs against channel-by-channel TV on the same planes.

    python tools/gpu_color_time.py [--reps 7] [--out DIR]

10 x 3 x 128^2 (30 planes), alpha = 0.08, one MI355X, ONE handle.  After a warm-up of every call (graphs built, workspaces
allocated), `reps` rounds in which the calls of a pair alternate:
    K = 5000:  bpltv_denoise_device                  against  bpltv_color_denoise_device, channels = 3         -> stats.pdhg_ms
    K = 50:    bpltv_unrolled_denoise_device + bpltv_unrolled_vjp_device  against  the bpltv_color_unrolled_* pair, each on a
               caller's tape                                                    -> stats.pdhg_ms, stats.adjoint_ms
HIP-event medians with min / max and the ratios colour / channel-wise, per plane-iteration; one JSON line per pair, both
collected in DIR/color_time.json."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

PLAN = ("tile_iters", "tiles", "launches", "launch_chains", "graph_used", "bytes_per_px_iter")


def _stats(xs):
    import numpy as np
    xs = np.asarray(xs, dtype=float)
    return {"median": float(np.median(xs)), "min": float(xs.min()), "max": float(xs.max()), "n": int(xs.size)}


def _setup(B, C, n):
    import torch
    from conftest import synth_batch
    from bpldenoising_amd import TVSolver
    ub, f = synth_batch(B * C, n, n, seed=5)
    dev = torch.device("cuda", 0)
    tf, tub = torch.from_numpy(f).to(dev), torch.from_numpy(ub).to(dev)
    s = TVSolver(n, n, B * C, device=0)
    s.set_data_device(tub.data_ptr(), tf.data_ptr())
    return torch, dev, s, tf, tub


def time_solve(K, reps, B=10, C=3, n=128, alpha=0.08):
    torch, dev, s, tf, tub = _setup(B, C, n)
    ta = torch.tensor([alpha], dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    rows = {"tv_pdhg_ms": [], "color_pdhg_ms": []}
    plans = {}
    for r in range(reps + 1):          # round 0 is the warm-up
        s.denoise_device(ta.data_ptr(), 1, 1, maxiter=K)
        st = s.stats()
        t = [st["pdhg_ms"]]
        plans["tv"] = {k: st[k] for k in PLAN + ("pdhg_variant", "region_i", "region_j")}
        s.color_denoise_device(C, ta.data_ptr(), 1, 1, maxiter=K)
        st = s.stats()
        t.append(st["pdhg_ms"])
        plans["color"] = {k: st[k] for k in PLAN}
        if r:
            for k, v in zip(rows, t):
                rows[k].append(v)
    out = {"case": "%dx%dx%dx%d scalar" % (B, C, n, n), "maxiter": K, "plans": plans}
    out.update({k: _stats(v) for k, v in rows.items()})
    out["ratios"] = {"colour solve / channel-wise solve": out["color_pdhg_ms"]["median"] / out["tv_pdhg_ms"]["median"]}
    s.close()
    return out


def time_unrolled(K, reps, B=10, C=3, n=128, alpha=0.08):
    torch, dev, s, tf, tub = _setup(B, C, n)
    ta = torch.tensor([alpha], dtype=torch.float64, device=dev)
    tape = torch.empty(s.unrolled_tape_doubles(maxiter=K), dtype=torch.float64, device=dev)
    u, gf = torch.empty_like(tf), torch.empty_like(tf)
    ga = torch.empty(1, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    rows = {k: [] for k in ("tv_unrolled_pdhg_ms", "tv_unrolled_vjp_ms", "color_unrolled_pdhg_ms", "color_unrolled_vjp_ms")}
    plans = {}
    for r in range(reps + 1):
        t = []
        s.unrolled_denoise_device(ta.data_ptr(), 1, 1, tape_ptr=tape.data_ptr(), maxiter=K)
        st = s.stats()
        t.append(st["pdhg_ms"])
        plans["tv"] = {k: st[k] for k in PLAN}
        s.copy_u_device(u.data_ptr())
        gu = u - tub
        torch.cuda.synchronize()
        s.unrolled_vjp_device(tape.data_ptr(), ta.data_ptr(), 1, 1, gu.data_ptr(), gf.data_ptr(), ga.data_ptr(), maxiter=K)
        t.append(s.stats()["adjoint_ms"])
        s.color_unrolled_denoise_device(C, ta.data_ptr(), 1, 1, tape_ptr=tape.data_ptr(), maxiter=K)
        st = s.stats()
        t.append(st["pdhg_ms"])
        plans["color"] = {k: st[k] for k in PLAN}
        s.copy_u_device(u.data_ptr())
        gu = u - tub
        torch.cuda.synchronize()
        s.color_unrolled_vjp_device(C, tape.data_ptr(), ta.data_ptr(), 1, 1, gu.data_ptr(), gf.data_ptr(), ga.data_ptr(), maxiter=K)
        t.append(s.stats()["adjoint_ms"])
        if r:
            for k, v in zip(rows, t):
                rows[k].append(v)
    out = {"case": "%dx%dx%dx%d scalar" % (B, C, n, n), "maxiter": K, "tape_MB": tape.numel() * 8 / 1e6, "plans": plans}
    out.update({k: _stats(v) for k, v in rows.items()})
    med = lambda k: out[k]["median"]
    out["ratios"] = {"colour taped solve / channel-wise taped solve": med("color_unrolled_pdhg_ms") / med("tv_unrolled_pdhg_ms"),
                     "colour sweep / channel-wise sweep": med("color_unrolled_vjp_ms") / med("tv_unrolled_vjp_ms"),
                     "colour solve + sweep / channel-wise solve + sweep":
                         (med("color_unrolled_pdhg_ms") + med("color_unrolled_vjp_ms")) / (med("tv_unrolled_pdhg_ms") + med("tv_unrolled_vjp_ms"))}
    s.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "results"))
    a = ap.parse_args()
    res = [time_solve(5000, a.reps)]
    print(json.dumps(res[-1]), flush=True)
    res.append(time_unrolled(50, a.reps))
    print(json.dumps(res[-1]), flush=True)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "color_time.json"), "w") as fh:
        json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
