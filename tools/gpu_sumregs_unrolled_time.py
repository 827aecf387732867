#!/usr/bin/env python3
"""Developer probe: what the tape costs the sum-of-regularisers solve, and what the reverse sweep over it costs.

    python tools/gpu_sumregs_unrolled_time.py [--reps 7] [--iters 50 1000 5000] [--out DIR]

10 x 128^2, alpha = (0.03, 0.02, 0.04), one MI355X.  Per iteration count, after a warm-up of every call (graphs built,
workspaces allocated), `reps` rounds in which ONE handle runs in alternation:
    bpltv_sumregs_denoise_device, reserved[0] = 1 (the 32 x 32 kernel)    -> stats.pdhg_ms
    bpltv_sumregs_unrolled_denoise_device (a caller's tape)                -> stats.pdhg_ms
    bpltv_sumregs_unrolled_vjp_device on that tape, both gradients         -> stats.adjoint_ms (HIP events around the sweep)
HIP-event medians with min / max, the ratio taped / untaped beside the ratio by bytes (168 / 120 = 1.4), the tape size, and
whether u is bitwise the plain solve's; one JSON line per count, all of them collected in DIR/sumregs_unrolled_time.json.  A
count whose tape (6 * maxiter * M*N*O doubles: 39 GB at 5000 iterations) does not fit beside what else runs on the device is
skipped."""
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


def time_case(K, reps, O=10, n=128, alpha=(0.03, 0.02, 0.04)):
    import torch
    from conftest import synth_batch
    from bpldenoising_amd import TVSolver
    ub, f = synth_batch(O, n, n, seed=5)
    dev = torch.device("cuda", 0)
    tf, tub = torch.from_numpy(f).to(dev), torch.from_numpy(ub).to(dev)
    ta = torch.tensor(alpha, dtype=torch.float64, device=dev)
    s = TVSolver(n, n, O, device=0)
    s.set_data_device(tub.data_ptr(), tf.data_ptr())
    free = torch.cuda.mem_get_info(dev)[0]
    need = 8 * s.sumregs_unrolled_tape_doubles(maxiter=K)
    if need > 0.8 * free:
        s.close()
        return {"case": "%dx%dx%d vector" % (O, n, n), "maxiter": K, "skipped": "a tape of %.1f GB does not fit" % (need / 1e9)}
    tape = torch.empty(s.sumregs_unrolled_tape_doubles(maxiter=K), dtype=torch.float64, device=dev)
    u0, u1, gf = torch.empty_like(tf), torch.empty_like(tf), torch.empty_like(tf)
    ga = torch.empty(3, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    rows = {k: [] for k in ("sumregs_pdhg_ms", "sumregs_unrolled_pdhg_ms", "sumregs_unrolled_vjp_ms")}
    plan = rplan = None
    for r in range(reps + 1):          # round 0 is the warm-up
        t = []
        s.sumregs_denoise_device(ta.data_ptr(), 1, 1, maxiter=K, variant=1)
        st = s.stats()
        t.append(st["pdhg_ms"])
        rplan = {k: st[k] for k in ("tile_iters", "tiles", "launches", "launch_chains", "graph_used", "bytes_per_px_iter")}
        s.copy_u_device(u0.data_ptr())
        s.sumregs_unrolled_denoise_device(ta.data_ptr(), 1, 1, tape_ptr=tape.data_ptr(), maxiter=K)
        st = s.stats()
        t.append(st["pdhg_ms"])
        plan = {k: st[k] for k in ("tile_iters", "tiles", "launches", "launch_chains", "graph_used", "bytes_per_px_iter")}
        s.copy_u_device(u1.data_ptr())
        gu = u1 - tub
        torch.cuda.synchronize()
        s.sumregs_unrolled_vjp_device(tape.data_ptr(), ta.data_ptr(), 1, 1, gu.data_ptr(), gf.data_ptr(), ga.data_ptr(), maxiter=K)
        t.append(s.stats()["adjoint_ms"])
        if r:
            for k, v in zip(rows, t):
                rows[k].append(v)
    out = {"case": "%dx%dx%d vector" % (O, n, n), "maxiter": K, "tape_MB": tape.numel() * 8 / 1e6,
           "u_bitwise_equal": bool(torch.equal(u0, u1)), "plan": plan, "plain_plan": rplan, "grad_alpha": ga.cpu().tolist()}
    out.update({k: _stats(v) for k, v in rows.items()})
    med = lambda k: out[k]["median"]
    out["ratios"] = {"taped solve / plain solve (by bytes 168/120 = 1.4)": med("sumregs_unrolled_pdhg_ms") / med("sumregs_pdhg_ms"),
                     "reverse sweep / taped solve": med("sumregs_unrolled_vjp_ms") / med("sumregs_unrolled_pdhg_ms")}
    s.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, nargs="+", default=[50, 1000, 5000])
    ap.add_argument("--out", default=os.path.join(ROOT, "results"))
    a = ap.parse_args()
    res = []
    for K in a.iters:
        res.append(time_case(K, a.reps))
        print(json.dumps(res[-1]), flush=True)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "sumregs_unrolled_time.json"), "w") as fh:
        json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
