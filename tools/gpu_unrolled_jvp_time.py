#!/usr/bin/env python3
"""Developer probe: what one tangent sweep through the iterations costs against the plain solve, the taped solve plus its
reverse sweep, and the implicit adjoint.

    python tools/gpu_unrolled_jvp_time.py [--reps 7] [--iters 50 500 5000] [--large-iters 500] [--out DIR]

10 x 128^2, scalar alpha, one MI355X.  Per iteration count, after a warm-up of every call (graphs built, workspaces
allocated), `reps` rounds in which two handles alternate:
    handle A: bpltv_denoise_device                               -> stats.pdhg_ms
    handle B: bpltv_unrolled_jvp_device, dalpha = 1, one sweep   -> stats.adjoint_ms (HIP events around the sweep)
    handle B: bpltv_unrolled_denoise_device (a caller's tape)    -> stats.pdhg_ms
    handle B: bpltv_unrolled_vjp_device on that tape             -> stats.adjoint_ms
    handle A: bpltv_vjp_device on A's u, the same cotangent      -> stats.adjoint_ms (the implicit adjoint)
Medians with min / max; one JSON line per count.  Then one line for a 1 x 1024^2 scalar sweep of --large-iters iterations
beside the plain solve (no tape: at 5000 iterations it would not fit).  Everything is collected in DIR/unrolled_jvp_time.json."""
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


def time_count(K, reps, O=10, n=128, alpha=0.08, taped=True):
    import torch
    from conftest import synth_batch
    from bpldenoising_amd import TVSolver
    ub, f = synth_batch(O, n, n, seed=5)
    dev = torch.device("cuda", 0)
    tf, tub = torch.from_numpy(f).to(dev), torch.from_numpy(ub).to(dev)
    ta = torch.tensor([alpha], dtype=torch.float64, device=dev)
    one = torch.ones(1, dtype=torch.float64, device=dev)
    A, B = TVSolver(n, n, O, device=0), TVSolver(n, n, O, device=0)
    for s in (A, B):
        s.set_data_device(tub.data_ptr(), tf.data_ptr())
    tape = torch.empty(B.unrolled_tape_doubles(maxiter=K) if taped else 0, dtype=torch.float64, device=dev)
    uA, uB, du = torch.empty_like(tf), torch.empty_like(tf), torch.empty_like(tf)
    gfA, gfB = torch.empty_like(tf), torch.empty_like(tf)
    gaA, gaB = torch.empty(1, dtype=torch.float64, device=dev), torch.empty(1, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    rows = {"denoise_pdhg_ms": [], "unrolled_jvp_sweep_ms": []}
    if taped:
        rows.update({"unrolled_pdhg_ms": [], "unrolled_vjp_adjoint_ms": [], "implicit_vjp_adjoint_ms": []})
    for r in range(reps + 1):          # round 0 is the warm-up
        A.denoise_device(ta.data_ptr(), 1, 1, maxiter=K)
        ts = [A.stats()["pdhg_ms"]]
        A.copy_u_device(uA.data_ptr())
        B.unrolled_jvp_device(ta.data_ptr(), 1, 1, None, one.data_ptr(), du.data_ptr(), uB.data_ptr(), ndir=1, maxiter=K)
        ts.append(B.stats()["adjoint_ms"])
        if taped:
            B.unrolled_denoise_device(ta.data_ptr(), 1, 1, tape_ptr=tape.data_ptr(), maxiter=K)
            ts.append(B.stats()["pdhg_ms"])
            gu = uB - tub
            torch.cuda.synchronize()
            B.unrolled_vjp_device(tape.data_ptr(), ta.data_ptr(), 1, 1, gu.data_ptr(), gfB.data_ptr(), gaB.data_ptr(), maxiter=K)
            ts.append(B.stats()["adjoint_ms"])
            A.vjp_device(uA.data_ptr(), ta.data_ptr(), 1, 1, gu.data_ptr(), gfA.data_ptr(), gaA.data_ptr(), maxiter=K)
            ts.append(A.stats()["adjoint_ms"])
        if r:
            for k, t in zip(rows, ts):
                rows[k].append(t)
    out = {"case": "%dx%dx%d scalar" % (O, n, n), "maxiter": K, "tape_MB": tape.numel() * 8 / 1e6,
           "sweep_workspace_MB": 14 * tf.numel() * 8 / 1e6, "u_bitwise_equal": bool(torch.equal(uA, uB))}
    if taped:   # the transpose identity on the way: <du, gu> against dL/dalpha of the reverse sweep
        out["du_dot_gu"] = float((du * (uB - tub)).sum())
        out["grad_alpha_unrolled"] = float(gaB[0])
        out["grad_alpha_implicit"] = float(gaA[0])
    out.update({k: _stats(v) for k, v in rows.items()})
    A.close()
    B.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, nargs="*", default=[50, 500, 5000])
    ap.add_argument("--large-iters", type=int, default=500)
    ap.add_argument("--out", default=os.path.join(ROOT, "results"))
    a = ap.parse_args()
    res = []
    for K in a.iters:
        res.append(time_count(K, a.reps))
        print(json.dumps(res[-1]), flush=True)
    if a.large_iters > 0:
        res.append(time_count(a.large_iters, a.reps, O=1, n=1024, taped=False))
        print(json.dumps(res[-1]), flush=True)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "unrolled_jvp_time.json"), "w") as fh:
        json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
