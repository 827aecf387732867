#!/usr/bin/env python3
"""Developer probe: the batched sum-of-regularisers sweep (bpltv_sumregs_sweep) against a loop of sumregs_denoise calls,
and the 10 x 128^2 sumregs_denoise of two builds, alternated.

    python tools/gpu_sumregs_sweep_time.py [--base ROOT] [--rounds 3] [--out DIR]

1. Sweep vs loop (this tree's library), 5000 iterations: cameraman_128_10 (1 x 128^2) with K = 100 triples and
   faces_train (10 x 128^2) with K = 20.  The loop is what a caller does without the sweep: per parameter one
   sumregs_denoise, the result fetched and its loss taken on the host.  The sweep's u must equal the loop's bit for bit.
2. --base ROOT: a checkout of another commit with its library built.  Fresh child processes time the 10 x 128^2
   sumregs_denoise (5000 iterations, 20 calls after 3 warm-up calls) with ROOT's package and with this tree's,
   alternated for --rounds rounds.
Every number is printed as one JSON line and collected in DIR/sumregs_sweep_time.json."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NPZ = os.path.join(ROOT, "tests", "golden", "datasets.npz")


def _triples(K, seed=0):
    import numpy as np
    rng = np.random.default_rng(seed)
    return np.array([0.03, 0.02, 0.05])[None] * (0.25 + 1.5 * rng.random((K, 3)))


def child_denoise(root, calls, warmup):
    """10 x 128^2 sumregs_denoise with the package under `root` (run in a fresh process)."""
    sys.path.insert(0, root)
    import numpy as np
    from bpldenoising_amd import TVSolver, testdataset
    ub, f = testdataset("faces_train", npz=NPZ)
    s = TVSolver(128, 128, 10)
    s.set_data(ub[:10], f[:10])
    a3 = np.array([0.03, 0.02, 0.05])
    for _ in range(warmup):
        s.sumregs_denoise(a3, fetch=False)
    wall, pdhg = [], []
    for _ in range(calls):
        t = time.perf_counter()
        s.sumregs_denoise(a3, fetch=False)   # returns after a device synchronise
        wall.append(1e3 * (time.perf_counter() - t))
        pdhg.append(s.stats()["pdhg_ms"])
    u = s.sumregs_denoise(a3)
    s.close()
    return {"wall_ms_median": float(np.median(wall)), "wall_ms_min": float(np.min(wall)),
            "pdhg_ms_median": float(np.median(pdhg)), "pdhg_ms_min": float(np.min(pdhg)),
            "u_sum": float(u.sum()), "u_bytes_sha": __import__("hashlib").sha256(u.tobytes()).hexdigest()[:16]}


def sweep_vs_loop(ds, O, K, maxiter=5000, reps=3):
    import numpy as np
    sys.path.insert(0, ROOT)
    from bpldenoising_amd import TVSolver, testdataset
    ub, f = testdataset(ds, npz=NPZ)
    ub, f = ub[:O], f[:O]
    P = _triples(K, seed=K)
    s = TVSolver(128, 128, O)
    s.set_data(ub, f)
    res = {"what": "sweep_vs_loop", "dataset": ds, "O": O, "K": K, "maxiter": maxiter}
    # warm-up of every shape the timed windows use
    s.sumregs_sweep(P, maxiter=maxiter)
    s.sumregs_denoise(P[0], maxiter=maxiter)
    t_sweep, pd = [], []
    for _ in range(reps):
        t = time.perf_counter()
        costs = s.sumregs_sweep(P, maxiter=maxiter)
        t_sweep.append(1e3 * (time.perf_counter() - t))
        pd.append(s.stats()["pdhg_ms"])
    st = s.stats()
    res.update(sweep_ms=t_sweep, sweep_pdhg_ms=pd, sweep_region=st["region_i"], sweep_chains=st["launch_chains"],
               sweep_groups=st["sweep_groups"])
    costs_u, us = s.sumregs_sweep(P, fetch_u=True, maxiter=maxiter)
    t = time.perf_counter()
    loop_costs, same_u = [], True
    for k in range(K):
        u = s.sumregs_denoise(P[k], maxiter=maxiter)
        d = u - ub
        loop_costs.append(0.5 * float(np.sum(d * d)))
    loop_ms = 1e3 * (time.perf_counter() - t)
    for k in range(K):   # outside the timed loop: the sweep's u of every parameter against a denoise call
        same_u &= bool(np.array_equal(s.sumregs_denoise(P[k], maxiter=maxiter), us[k]))
    res.update(loop_ms=loop_ms, loop_ms_per_call=loop_ms / K, speedup_median=loop_ms / float(np.median(t_sweep)),
               same_u=same_u, costs_equal=bool(np.array_equal(costs, costs_u)),
               max_rel_cost_diff_vs_host=float(np.max(np.abs(costs - np.array(loop_costs)) / np.array(loop_costs))))
    # both kernels forced on the sweep, for the record
    for var in (1, 2):
        s.sumregs_sweep(P, maxiter=maxiter, variant=var)
        t = time.perf_counter()
        s.sumregs_sweep(P, maxiter=maxiter, variant=var)
        res["sweep_ms_variant%d" % var] = 1e3 * (time.perf_counter() - t)
    s.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--base", default=None, help="root of a checkout of another commit, its library built")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default=".", help="directory of sumregs_sweep_time.json")
    ap.add_argument("--child-denoise", default=None, metavar="ROOT", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child_denoise:
        print(json.dumps(child_denoise(a.child_denoise, a.calls, 3)))
        return 0
    out = []

    def emit(d):
        print(json.dumps(d), flush=True)
        out.append(d)

    for ds, O, K in (("cameraman_128_10", 1, 100), ("faces_train", 10, 20)):
        emit(sweep_vs_loop(ds, O, K))
    if a.base:
        for r in range(a.rounds):
            for name, root in (("base", os.path.abspath(a.base)), ("new", ROOT)):
                p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child-denoise", root, "--calls", str(a.calls)],
                                   capture_output=True, text=True, timeout=600)
                if p.returncode != 0:
                    emit({"what": "denoise_10x128", "build": name, "round": r, "rc": p.returncode, "stderr": p.stderr[-2000:]})
                    return 1
                d = json.loads(p.stdout.strip().splitlines()[-1])
                d.update(what="denoise_10x128", build=name, round=r)
                emit(d)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "sumregs_sweep_time.json"), "w") as fh:
        json.dump(out, fh, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
