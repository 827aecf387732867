#!/usr/bin/env python3
"""Developer probe: what the Kullback-Leibler data term costs against the quadratic one.

    python tools/gpu_kl_time.py [--reps 7] [--out DIR] [--log FILE]

10 x 128^2, scalar alpha, w in [0.5, 2] with one plane per image (wo = O), one MI355X, ONE handle per step.  The dataset is
Poisson counts at a peak of 30 on a background (tests/kl_ref.py's recipe on synth_batch's clean images).  After a warm-up round of
every call (graphs built, workspaces allocated), `reps` rounds in which the calls of a pair alternate:
    K = 5000:  bpltv_kl_denoise_device  |  bpltv_weighted_denoise_device                                      -> stats.pdhg_ms
    K = 50:    the bpltv_kl_unrolled_* pair  |  the bpltv_weighted_unrolled_* pair, both with grad_w, each on a caller's tape
                                                                                         -> stats.pdhg_ms, stats.adjoint_ms
alpha is 0.15 for the KL calls and 0.08 for the weighted ones: each model at a parameter at which it does its work.  HIP-event
medians with min / max and the ratios KL / weighted; one JSON line per step, both collected in DIR/kl_time.json and, with --log,
written to FILE.  Each step runs in a process of its own under a time limit; a step that fails ends the run."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

PLAN = ("tile_iters", "tiles", "launches", "launch_chains", "graph_used", "bytes_per_px_iter")
ALPHA = {"kl": 0.15, "weighted": 0.08}
STEP_LIMIT_S = 240


def _stats(xs):
    import numpy as np
    xs = np.asarray(xs, dtype=float)
    return {"median": float(np.median(xs)), "min": float(xs.min()), "max": float(xs.max()), "n": int(xs.size)}


def _setup(O, n):
    import numpy as np
    import torch
    from conftest import synth_batch
    from bpldenoising_amd import TVSolver
    ub, _ = synth_batch(O, n, n, seed=5)
    clean = np.clip(ub, 0.0, None)
    clean = clean * (30.0 / clean.max())
    f = np.random.default_rng(31).poisson(clean).astype(np.float64) / 30.0 + 0.1
    w = 0.5 + 1.5 * np.random.default_rng(11).random((O, n, n))
    dev = torch.device("cuda", 0)
    tf, tub, tw = torch.from_numpy(f).to(dev), torch.from_numpy(ub).to(dev), torch.from_numpy(w).to(dev)
    s = TVSolver(n, n, O, device=0)
    s.set_data_device(tub.data_ptr(), tf.data_ptr())
    ta = {k: torch.tensor([a], dtype=torch.float64, device=dev) for k, a in ALPHA.items()}
    return torch, dev, s, tf, tub, tw, ta


def time_solve(K, reps, O=10, n=128):
    torch, dev, s, tf, tub, tw, ta = _setup(O, n)
    torch.cuda.synchronize()
    calls = {"kl": lambda: s.kl_denoise_device(tw.data_ptr(), O, ta["kl"].data_ptr(), 1, 1, maxiter=K),
             "weighted": lambda: s.weighted_denoise_device(tw.data_ptr(), O, ta["weighted"].data_ptr(), 1, 1, maxiter=K)}
    rows = {k + "_pdhg_ms": [] for k in calls}
    plans = {}
    for r in range(reps + 1):          # round 0 is the warm-up
        for k, call in calls.items():
            call()
            st = s.stats()
            plans[k] = {p: st[p] for p in PLAN}
            if r:
                rows[k + "_pdhg_ms"].append(st["pdhg_ms"])
    out = {"case": "%dx%dx%d scalar, w per image" % (O, n, n), "maxiter": K, "alpha": ALPHA, "plans": plans}
    out.update({k: _stats(v) for k, v in rows.items()})
    out["ratios"] = {"KL solve / weighted solve": out["kl_pdhg_ms"]["median"] / out["weighted_pdhg_ms"]["median"]}
    s.close()
    return out


def time_unrolled(K, reps, O=10, n=128):
    torch, dev, s, tf, tub, tw, ta = _setup(O, n)
    tape = torch.empty(s.weighted_unrolled_tape_doubles(maxiter=K), dtype=torch.float64, device=dev)
    u, gf, gw = torch.empty_like(tf), torch.empty_like(tf), torch.empty_like(tf)
    ga = torch.empty(1, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    tp, wp = tape.data_ptr(), tw.data_ptr()
    al, aw = ta["kl"].data_ptr(), ta["weighted"].data_ptr()
    pairs = {"kl": (lambda: s.kl_unrolled_denoise_device(wp, O, al, 1, 1, tape_ptr=tp, maxiter=K),
                    lambda g: s.kl_unrolled_vjp_device(tp, wp, O, al, 1, 1, g, gf.data_ptr(), ga.data_ptr(), gw.data_ptr(), maxiter=K)),
             "weighted": (lambda: s.weighted_unrolled_denoise_device(wp, O, aw, 1, 1, tape_ptr=tp, maxiter=K),
                          lambda g: s.weighted_unrolled_vjp_device(tp, wp, O, aw, 1, 1, g, gf.data_ptr(), ga.data_ptr(), gw.data_ptr(),
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
    out = {"case": "%dx%dx%d scalar, w per image" % (O, n, n), "maxiter": K, "alpha": ALPHA, "tape_MB": tape.numel() * 8 / 1e6,
           "plans": plans}
    out.update({k: _stats(v) for k, v in rows.items()})
    sol = lambda k: out[k + "_unrolled_pdhg_ms"]["median"]
    swp = lambda k: out[k + "_unrolled_vjp_ms"]["median"]
    out["ratios"] = {"KL taped solve / weighted taped solve": sol("kl") / sol("weighted"),
                     "KL sweep / weighted sweep": swp("kl") / swp("weighted"),
                     "KL solve + sweep / weighted solve + sweep": (sol("kl") + swp("kl")) / (sol("weighted") + swp("weighted"))}
    s.close()
    return out


STEPS = {"solve": lambda reps: time_solve(5000, reps), "unrolled": lambda reps: time_unrolled(50, reps)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "results"))
    ap.add_argument("--log", default=None, help="write the JSON lines to this file (profiles/kl_time.log)")
    ap.add_argument("--step", choices=sorted(STEPS), default=None, help="run this step only, in this process")
    a = ap.parse_args()
    if a.step:
        print(json.dumps(STEPS[a.step](a.reps)), flush=True)
        return 0
    res = []
    for step in ("solve", "unrolled"):     # a fresh process per step, each under its own time limit; nothing after a failure
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", step, "--reps", str(a.reps)], capture_output=True,
                               text=True, timeout=STEP_LIMIT_S)
        except subprocess.TimeoutExpired:
            print("step %s: no answer within %d s; stopping" % (step, STEP_LIMIT_S), file=sys.stderr)
            return 124
        if r.returncode != 0:
            sys.stderr.write(r.stdout + r.stderr)
            print("step %s: exit status %d; stopping" % (step, r.returncode), file=sys.stderr)
            return r.returncode if r.returncode > 0 else 1
        line = r.stdout.strip().splitlines()[-1]
        res.append(json.loads(line))
        print(line, flush=True)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "kl_time.json"), "w") as fh:
        json.dump(res, fh, indent=1)
    if a.log:
        with open(a.log, "w") as fh:
            for r in res:
                fh.write(json.dumps(r) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
