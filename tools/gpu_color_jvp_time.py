#!/usr/bin/env python3
"""Developer probe: what the tangent sweep through the channel-coupled iterations costs, against the channel-wise tangent
sweep on the same planes and against reverse mode (taped colour solve + reverse sweep).

    python tools/gpu_color_jvp_time.py [--reps 7] [--channels 3,4,2] [--out DIR]

10 x C x 128^2 for C = 3 (30 planes), C = 4 (40 planes) and C = 2 (20 planes), scalar alpha = 0.08, one direction (dalpha),
K = 50 and K = 5000, one MI355X, ONE handle per case.  After a warm-up round (graphs built, workspaces allocated), `reps`
rounds in which the calls alternate:
    bpltv_color_unrolled_jvp_device, channels = C                                  -> stats.adjoint_ms
    bpltv_unrolled_jvp_device on the same planes                                   -> stats.adjoint_ms
    bpltv_color_unrolled_denoise_device + bpltv_color_unrolled_vjp_device          -> stats.pdhg_ms + stats.adjoint_ms
(K = 50: on a caller's full tape; K = 5000: checkpoint_every = -1, the tape of 2*K*planes*128^2 doubles being 39 / 52 / 26 GB).
HIP-event medians with min / max and the ratios; one JSON line per case, all collected in DIR/color_jvp_time.json."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def _stats(xs):
    import numpy as np
    xs = np.asarray(xs, dtype=float)
    return {"median": float(np.median(xs)), "min": float(xs.min()), "max": float(xs.max()), "n": int(xs.size)}


def time_case(K, reps, C, B=10, n=128, alpha=0.08):
    import torch
    from conftest import synth_batch
    from bpldenoising_amd import TVSolver
    ub, f = synth_batch(B * C, n, n, seed=5)
    dev = torch.device("cuda", 0)
    tf, tub = torch.from_numpy(f).to(dev), torch.from_numpy(ub).to(dev)
    s = TVSolver(n, n, B * C, device=0)
    s.set_data_device(tub.data_ptr(), tf.data_ptr())
    ta = torch.tensor([alpha], dtype=torch.float64, device=dev)
    tda = torch.ones(1, dtype=torch.float64, device=dev)
    du, u, gf = torch.empty_like(tf), torch.empty_like(tf), torch.empty_like(tf)
    ga = torch.empty(1, dtype=torch.float64, device=dev)
    ck = dict(checkpoint_every=-1) if K > 500 else {}
    tape = torch.empty(s.unrolled_tape_doubles(maxiter=K, **ck), dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    rows = {k: [] for k in ("color_jvp_ms", "tv_jvp_ms", "color_taped_pdhg_ms", "color_vjp_ms")}
    for r in range(reps + 1):          # round 0 is the warm-up
        t = []
        s.color_unrolled_jvp_device(C, ta.data_ptr(), 1, 1, None, tda.data_ptr(), du.data_ptr(), None, ndir=1, maxiter=K)
        t.append(s.stats()["adjoint_ms"])
        s.unrolled_jvp_device(ta.data_ptr(), 1, 1, None, tda.data_ptr(), du.data_ptr(), None, ndir=1, maxiter=K)
        t.append(s.stats()["adjoint_ms"])
        s.color_unrolled_denoise_device(C, ta.data_ptr(), 1, 1, tape_ptr=tape.data_ptr(), maxiter=K, **ck)
        t.append(s.stats()["pdhg_ms"])
        s.copy_u_device(u.data_ptr())
        gu = u - tub
        torch.cuda.synchronize()
        s.color_unrolled_vjp_device(C, tape.data_ptr(), ta.data_ptr(), 1, 1, gu.data_ptr(), gf.data_ptr(), ga.data_ptr(), maxiter=K, **ck)
        t.append(s.stats()["adjoint_ms"])
        if r:
            for k, v in zip(rows, t):
                rows[k].append(v)
    out = {"case": "%dx%dx%dx%d scalar" % (B, C, n, n), "maxiter": K,
           "reverse_mode": "checkpoint_every=-1" if ck else "full tape", "tape_MB": tape.numel() * 8 / 1e6}
    out.update({k: _stats(v) for k, v in rows.items()})
    med = lambda k: out[k]["median"]
    out["ns_per_plane_iteration"] = {"colour tangent sweep": 1e6 * med("color_jvp_ms") / (K * B * C),
                                     "channel-wise tangent sweep": 1e6 * med("tv_jvp_ms") / (K * B * C)}
    out["ratios"] = {"colour tangent sweep / channel-wise tangent sweep": med("color_jvp_ms") / med("tv_jvp_ms"),
                     "colour tangent sweep / colour taped solve + reverse sweep":
                         med("color_jvp_ms") / (med("color_taped_pdhg_ms") + med("color_vjp_ms"))}
    s.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--channels", default="3,4,2")
    ap.add_argument("--out", default=os.path.join(ROOT, "results"))
    a = ap.parse_args()
    res = []
    for C in (int(c) for c in a.channels.split(",")):
        for K in (50, 5000):
            res.append(time_case(K, a.reps, C))
            print(json.dumps(res[-1]), flush=True)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "color_jvp_time.json"), "w") as fh:
        json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
