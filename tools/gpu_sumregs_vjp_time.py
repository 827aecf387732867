#!/usr/bin/env python3
"""Developer probe: the cost of the sum-of-regularisers vector-Jacobian product (bpltv_sumregs_vjp) and of its PyTorch
layer.

    python tools/gpu_sumregs_vjp_time.py [--reps 10] [--base ROOT] [--rounds 3] [--out DIR]

1. Adjoint device time (stats.adjoint_ms) of bpltv_sumregs_vjp against the adjoint inside bpltv_sumregs_evaluate on the
   same u, alternated after a warm-up: 10 x 128^2 vector (nested-dissection Cholesky), 10 x 128^2 2 x 2 patch with
   reg = 1 (nested-dissection LU) and 4 x 256^2 vector; u of a 5000-iteration solve (the model's default count).
2. Wall time of the host VJP (grad_f copied back) and of one torch forward + backward (sumregs_denoise, L2 loss) against
   one bpltv_sumregs_evaluate of the same solve, alternated.
3. --base ROOT: a checkout of another commit with its library built.  Fresh child processes time the 10 x 128^2
   sumregs_evaluate (20 calls after 3 warm-up calls) with ROOT's package and with this tree's, alternated for --rounds
   rounds, and report whether cost and gradient are bitwise the same.
Every number is printed as one JSON line and collected in DIR/sumregs_vjp_time.json."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

A3 = [0.03, 0.02, 0.05]
P22 = [[[0.03, 0.05], [0.02, 0.04]], [[0.02, 0.03], [0.05, 0.02]], [[0.04, 0.02], [0.03, 0.06]]]
CASES = {"10x128_vector_reg0": (10, 128, A3, 0), "10x128_patch22_reg1": (10, 128, P22, 1),
         "4x256_vector_reg0": (4, 256, A3, 0)}
MAXITER = 5000


def _stats(xs):
    import numpy as np
    xs = np.asarray(xs, dtype=float)
    return {"median": float(np.median(xs)), "min": float(xs.min()), "max": float(xs.max()), "n": int(xs.size)}


def time_case(name, reps):
    import numpy as np
    import torch
    from conftest import synth_batch
    from bpldenoising_amd import TVSolver
    from bpldenoising_amd.torch_layer import sumregs_denoise
    O, n, x, reg = CASES[name]
    x = np.asarray(x, dtype=np.float64)
    delta = 1e-4 if reg else 0.1
    ub, f = synth_batch(O, n, n, seed=5)
    s = TVSolver(n, n, O, device=0)
    s.set_data(ub, f)
    u, _, g = s.sumregs_evaluate(x, delta, maxiter=MAXITER)
    gu = u - ub
    s.sumregs_vjp(u, x, gu, reg=reg)   # warm-up
    ev_adj, vjp_adj, ev_wall, vjp_wall = [], [], [], []
    for _ in range(reps):
        t = time.perf_counter()
        _, _, g = s.sumregs_evaluate(x, delta, maxiter=MAXITER, fetch_u=False)
        ev_wall.append(1e3 * (time.perf_counter() - t))
        ev_adj.append(s.stats()["adjoint_ms"])
        t = time.perf_counter()
        gf, ga = s.sumregs_vjp(u, x, gu, reg=reg)
        vjp_wall.append(1e3 * (time.perf_counter() - t))
        vjp_adj.append(s.stats()["adjoint_ms"])
    method = s.stats()["adjoint_method"]
    same = bool(np.array_equal(np.asarray(g), np.asarray(ga)))
    dev = torch.device("cuda", 0)
    tf, tub = torch.from_numpy(f).to(dev), torch.from_numpy(ub).to(dev)
    ta = torch.tensor(x, dtype=torch.float64, device=dev, requires_grad=True)

    def torch_step():
        ta.grad = None
        loss = 0.5 * ((sumregs_denoise(tf, ta, reg=bool(reg), maxiter=MAXITER) - tub) ** 2).sum()
        loss.backward()
        torch.cuda.synchronize()

    torch_step()
    t_torch, t_eval = [], []
    for _ in range(reps):
        t = time.perf_counter()
        torch_step()
        t_torch.append(1e3 * (time.perf_counter() - t))
        t = time.perf_counter()
        _, _, ge = s.sumregs_evaluate(x, delta, maxiter=MAXITER, fetch_u=False)
        t_eval.append(1e3 * (time.perf_counter() - t))
    same_torch = bool(np.array_equal(ta.grad.cpu().numpy(), np.asarray(ge)))
    s.close()
    return {"what": "sumregs_vjp_vs_evaluate", "case": name, "maxiter": MAXITER, "adjoint_method": method,
            "evaluate_adjoint_ms": _stats(ev_adj), "vjp_adjoint_ms": _stats(vjp_adj),
            "evaluate_wall_ms": _stats(ev_wall), "vjp_host_wall_ms": _stats(vjp_wall), "vjp_equals_evaluate": same,
            "torch_fwd_bwd_wall_ms": _stats(t_torch), "evaluate_wall_ms_2": _stats(t_eval),
            "torch_grad_equals_evaluate": same_torch}


def child_evaluate(root, reps):
    """10 x 128^2 sumregs_evaluate (vector parameter) with the package under `root` (run in a fresh process)."""
    sys.path.insert(0, root)
    import numpy as np
    from conftest import synth_batch
    from bpldenoising_amd import TVSolver
    ub, f = synth_batch(10, 128, 128, seed=5)
    s = TVSolver(128, 128, 10, device=0)
    s.set_data(ub, f)
    x = np.asarray(A3)
    for _ in range(3):
        s.sumregs_evaluate(x, 0.1, fetch_u=False)
    wall, adj, pdhg = [], [], []
    for _ in range(reps):
        t = time.perf_counter()
        _, c, g = s.sumregs_evaluate(x, 0.1, fetch_u=False)
        wall.append(1e3 * (time.perf_counter() - t))
        adj.append(s.stats()["adjoint_ms"])
        pdhg.append(s.stats()["pdhg_ms"])
    s.close()
    return {"evaluate_wall_ms": _stats(wall), "pdhg_ms": _stats(pdhg), "adjoint_ms": _stats(adj), "cost": c,
            "grad": [float(v) for v in np.ravel(g)]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--base", default=None)
    ap.add_argument("--child-root", default=None)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=".", help="directory of sumregs_vjp_time.json")
    ap.add_argument("--cases", default=",".join(CASES))
    a = ap.parse_args()
    if a.child_root:
        print(json.dumps(child_evaluate(a.child_root, a.reps)))
        return
    res = []
    for name in a.cases.split(","):
        r = time_case(name, a.reps)
        print(json.dumps(r), flush=True)
        res.append(r)
    if a.base:
        roots = {"base": os.path.abspath(a.base), "this": ROOT}
        outs = {}
        for rnd in range(a.rounds):
            for tag in (("base", "this") if rnd % 2 == 0 else ("this", "base")):
                out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child-root", roots[tag], "--reps", "20"],
                                     capture_output=True, text=True, timeout=600)
                if out.returncode != 0:
                    raise SystemExit("child (%s) failed rc=%d: %s" % (tag, out.returncode, out.stderr[-2000:]))
                r = dict(json.loads(out.stdout.strip().splitlines()[-1]), what="sumregs_evaluate_ab", lib=tag, round=rnd)
                outs.setdefault(tag, []).append((r["cost"], r["grad"]))
                r.pop("grad")
                print(json.dumps(r), flush=True)
                res.append(r)
        same = all(o == outs["base"][0] for o in outs["base"] + outs["this"])
        print(json.dumps({"what": "sumregs_evaluate_ab_identical", "identical": same}), flush=True)
        res.append({"what": "sumregs_evaluate_ab_identical", "identical": same})
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "sumregs_vjp_time.json"), "w") as fh:
        json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
