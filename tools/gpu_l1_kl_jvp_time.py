#!/usr/bin/env python3
"""Developer probe: what a tangent sweep through the TV-L1 and the TV-KL iterations costs against the weighted model's.

    python tools/gpu_l1_kl_jvp_time.py [--reps 7] [--out DIR] [--log FILE]

10 x 128^2, scalar alpha, w in [0.5, 2] with one plane per image (wo = O), one MI355X, ONE handle per step.  The dataset is
tools/gpu_kl_time.py's: Poisson counts at a peak of 30 on a background, which all three models take.  One direction with all
three tangents (df, dalpha, dw), everything resident in HBM.  After a warm-up round of every call (graphs built, the workspace
allocated), `reps` rounds in which the three calls alternate:
    bpltv_lone_unrolled_jvp_device  |  bpltv_kl_unrolled_jvp_device  |  bpltv_weighted_unrolled_jvp_device   -> stats.adjoint_ms
at K = 50 and at K = 5000, each depth a step of its own.  alpha is 0.7 for L1, 0.15 for KL and 0.08 for the weighted model: each
model at a parameter at which it does its work.  HIP-event medians with min / max and the ratios to the weighted sweep; one JSON
line per step, both collected in DIR/l1_kl_jvp_time.json and, with --log, written to FILE.  Each step runs in a process of its own
under a time limit; a step that fails ends the run."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

ALPHA = {"l1": 0.7, "kl": 0.15, "weighted": 0.08}
STEP_LIMIT_S = 240


def _stats(xs):
    import numpy as np
    xs = np.asarray(xs, dtype=float)
    return {"median": float(np.median(xs)), "min": float(xs.min()), "max": float(xs.max()), "n": int(xs.size)}


def time_sweeps(K, reps, O=10, n=128):
    import numpy as np
    import torch
    from conftest import synth_batch
    from bpldenoising_amd import TVSolver
    ub, _ = synth_batch(O, n, n, seed=5)
    clean = np.clip(ub, 0.0, None)
    clean = clean * (30.0 / clean.max())
    f = np.random.default_rng(31).poisson(clean).astype(np.float64) / 30.0 + 0.1
    w = 0.5 + 1.5 * np.random.default_rng(11).random((O, n, n))
    rng = np.random.default_rng(305)
    dev = torch.device("cuda", 0)
    tf, tub, tw = torch.from_numpy(f).to(dev), torch.from_numpy(ub).to(dev), torch.from_numpy(w).to(dev)
    tdf, tdw = torch.from_numpy(rng.standard_normal(f.shape)).to(dev), torch.from_numpy(rng.standard_normal(w.shape)).to(dev)
    tda = torch.ones(1, dtype=torch.float64, device=dev)
    du = torch.empty_like(tf)
    s = TVSolver(n, n, O, device=0)
    s.set_data_device(tub.data_ptr(), tf.data_ptr())
    ta = {k: torch.tensor([a], dtype=torch.float64, device=dev) for k, a in ALPHA.items()}
    torch.cuda.synchronize()
    calls = {k: (lambda k=k: getattr(s, k + "_unrolled_jvp_device")(tw.data_ptr(), O, ta[k].data_ptr(), 1, 1, tdf.data_ptr(), tda.data_ptr(),
                                                                    tdw.data_ptr(), du.data_ptr(), None, ndir=1, maxiter=K))
             for k in ("l1", "kl", "weighted")}
    rows = {k + "_jvp_ms": [] for k in calls}
    norms = {}
    for r in range(reps + 1):          # round 0 is the warm-up
        for k, call in calls.items():
            call()
            st = s.stats()
            if r:
                rows[k + "_jvp_ms"].append(st["adjoint_ms"])
            else:
                norms[k] = float(du.abs().max())
    out = {"case": "%dx%dx%d scalar, w per image, df + dalpha + dw" % (O, n, n), "maxiter": K, "alpha": ALPHA, "max_abs_du": norms}
    out.update({k: _stats(v) for k, v in rows.items()})
    wj = out["weighted_jvp_ms"]["median"]
    out["ratios"] = {"L1 sweep / weighted sweep": out["l1_jvp_ms"]["median"] / wj, "KL sweep / weighted sweep": out["kl_jvp_ms"]["median"] / wj}
    s.close()
    return out


STEPS = {"k50": lambda reps: time_sweeps(50, reps), "k5000": lambda reps: time_sweeps(5000, reps)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "results"))
    ap.add_argument("--log", default=None, help="write the JSON lines to this file (profiles/l1_kl_jvp_time.log)")
    ap.add_argument("--step", choices=sorted(STEPS), default=None, help="run this step only, in this process")
    a = ap.parse_args()
    if a.step:
        print(json.dumps(STEPS[a.step](a.reps)), flush=True)
        return 0
    res = []
    for step in ("k50", "k5000"):     # a fresh process per step, each under its own time limit; nothing after a failure
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
    with open(os.path.join(a.out, "l1_kl_jvp_time.json"), "w") as fh:
        json.dump(res, fh, indent=1)
    if a.log:
        with open(a.log, "w") as fh:
            for r in res:
                fh.write(json.dumps(r) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
