#!/usr/bin/env python3
"""Developer probe: what the fidelity weight costs the channel-coupled model, and what the coupling costs the weighted one.

    python tools/gpu_color_weighted_time.py [--reps 7] [--out DIR]

10 x 3 x 128^2 (30 planes), alpha = 0.08, w in [0.25, 4] with one plane per channel (wo = O), one MI355X, ONE handle.  After a
warm-up of every call (graphs built, workspaces allocated), `reps` rounds in which the calls of a triple alternate:
    K = 5000:  bpltv_color_denoise_device  |  bpltv_color_weighted_denoise_device, channels = 3  |  bpltv_weighted_denoise_device
               (channel-wise, the same w on the 30 planes)                                                  -> stats.pdhg_ms
    K = 50:    the bpltv_color_unrolled_* pair  |  the bpltv_color_weighted_unrolled_* pair (with grad_w)  |  the
               bpltv_weighted_unrolled_* pair (with grad_w), each on a caller's tape           -> stats.pdhg_ms, stats.adjoint_ms
HIP-event medians with min / max and the ratios weighted colour / colour and weighted colour / channel-wise weighted; one
JSON line per triple, both collected in DIR/color_weighted_time.json."""
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
    import numpy as np
    import torch
    from conftest import synth_batch
    from bpldenoising_amd import TVSolver
    ub, f = synth_batch(B * C, n, n, seed=5)
    w = 0.25 + 3.75 * np.random.default_rng(11).random((B * C, n, n))
    dev = torch.device("cuda", 0)
    tf, tub, tw = torch.from_numpy(f).to(dev), torch.from_numpy(ub).to(dev), torch.from_numpy(w).to(dev)
    s = TVSolver(n, n, B * C, device=0)
    s.set_data_device(tub.data_ptr(), tf.data_ptr())
    return torch, dev, s, tf, tub, tw


def time_solve(K, reps, B=10, C=3, n=128, alpha=0.08):
    torch, dev, s, tf, tub, tw = _setup(B, C, n)
    O = B * C
    ta = torch.tensor([alpha], dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    calls = {"color": lambda: s.color_denoise_device(C, ta.data_ptr(), 1, 1, maxiter=K),
             "color_weighted": lambda: s.color_weighted_denoise_device(C, tw.data_ptr(), O, ta.data_ptr(), 1, 1, maxiter=K),
             "weighted": lambda: s.weighted_denoise_device(tw.data_ptr(), O, ta.data_ptr(), 1, 1, maxiter=K)}
    rows = {k + "_pdhg_ms": [] for k in calls}
    plans = {}
    for r in range(reps + 1):          # round 0 is the warm-up
        for k, call in calls.items():
            call()
            st = s.stats()
            plans[k] = {p: st[p] for p in PLAN}
            if r:
                rows[k + "_pdhg_ms"].append(st["pdhg_ms"])
    out = {"case": "%dx%dx%dx%d scalar, w per plane" % (B, C, n, n), "maxiter": K, "plans": plans}
    out.update({k: _stats(v) for k, v in rows.items()})
    med = lambda k: out[k + "_pdhg_ms"]["median"]
    out["ratios"] = {"weighted colour solve / colour solve": med("color_weighted") / med("color"),
                     "weighted colour solve / channel-wise weighted solve": med("color_weighted") / med("weighted")}
    s.close()
    return out


def time_unrolled(K, reps, B=10, C=3, n=128, alpha=0.08):
    torch, dev, s, tf, tub, tw = _setup(B, C, n)
    O = B * C
    ta = torch.tensor([alpha], dtype=torch.float64, device=dev)
    tape = torch.empty(s.weighted_unrolled_tape_doubles(maxiter=K), dtype=torch.float64, device=dev)   # (the colour tape is 2/3 of it)
    u, gf, gw = torch.empty_like(tf), torch.empty_like(tf), torch.empty_like(tf)
    ga = torch.empty(1, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    tp, ap, wp = tape.data_ptr(), ta.data_ptr(), tw.data_ptr()
    pairs = {"color": (lambda: s.color_unrolled_denoise_device(C, ap, 1, 1, tape_ptr=tp, maxiter=K),
                       lambda g: s.color_unrolled_vjp_device(C, tp, ap, 1, 1, g, gf.data_ptr(), ga.data_ptr(), maxiter=K)),
             "color_weighted": (lambda: s.color_weighted_unrolled_denoise_device(C, wp, O, ap, 1, 1, tape_ptr=tp, maxiter=K),
                                lambda g: s.color_weighted_unrolled_vjp_device(C, tp, wp, O, ap, 1, 1, g, gf.data_ptr(), ga.data_ptr(),
                                                                               gw.data_ptr(), maxiter=K)),
             "weighted": (lambda: s.weighted_unrolled_denoise_device(wp, O, ap, 1, 1, tape_ptr=tp, maxiter=K),
                          lambda g: s.weighted_unrolled_vjp_device(tp, wp, O, ap, 1, 1, g, gf.data_ptr(), ga.data_ptr(), gw.data_ptr(),
                                                                   maxiter=K))}
    rows = {k + e: [] for k in pairs for e in ("_unrolled_pdhg_ms", "_unrolled_vjp_ms")}
    plans = {}
    for r in range(reps + 1):
        for k, (solve, sweep) in pairs.items():
            solve()
            st = s.stats()
            plans[k] = {p: st[p] for p in PLAN}
            s.copy_u_device(u.data_ptr())
            gu = u - tub
            torch.cuda.synchronize()
            sweep(gu.data_ptr())
            st2 = s.stats()
            if r:
                rows[k + "_unrolled_pdhg_ms"].append(st["pdhg_ms"])
                rows[k + "_unrolled_vjp_ms"].append(st2["adjoint_ms"])
    out = {"case": "%dx%dx%dx%d scalar, w per plane" % (B, C, n, n), "maxiter": K, "tape_MB": tape.numel() * 8 / 1e6, "plans": plans}
    out.update({k: _stats(v) for k, v in rows.items()})
    sol = lambda k: out[k + "_unrolled_pdhg_ms"]["median"]
    swp = lambda k: out[k + "_unrolled_vjp_ms"]["median"]
    both = lambda k: sol(k) + swp(k)
    out["ratios"] = {}
    for other, label in (("color", "colour"), ("weighted", "channel-wise weighted")):
        out["ratios"]["weighted colour taped solve / %s taped solve" % label] = sol("color_weighted") / sol(other)
        out["ratios"]["weighted colour sweep / %s sweep" % label] = swp("color_weighted") / swp(other)
        out["ratios"]["weighted colour solve + sweep / %s solve + sweep" % label] = both("color_weighted") / both(other)
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
    with open(os.path.join(a.out, "color_weighted_time.json"), "w") as fh:
        json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
