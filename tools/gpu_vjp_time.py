#!/usr/bin/env python3
"""Developer probe: the cost of the vector-Jacobian product (bpltv_vjp) and of the PyTorch layer.

    python tools/gpu_vjp_time.py [--reps 10] [--base ROOT] [--rounds 3] [--out DIR]

1. Adjoint device time (stats.adjoint_ms) of bpltv_vjp against bpltv_gradient on the same u, alternated after a
   warm-up: 10 x 128^2 (faces_train, scalar alpha, u of a 5000-iteration solve) and 8 x 1024^2 (pixel map).
2. Wall time of one torch forward + backward (tv_denoise, L2 loss) against one bpltv_evaluate of the same solve,
   alternated, on the same two shapes.
3. --base ROOT: a checkout of another commit with its library built.  Fresh child processes time the 10 x 128^2
   evaluate (5000 iterations, 20 calls after 3 warm-up calls) with ROOT's package and with this tree's, alternated for
   --rounds rounds, so that a change of the existing path shows against its spread.
Every number is printed as one JSON line and collected in DIR/vjp_time.json."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
NPZ = os.path.join(ROOT, "tests", "golden", "datasets.npz")


def _stats(xs):
    import numpy as np
    xs = np.asarray(xs, dtype=float)
    return {"median": float(np.median(xs)), "min": float(xs.min()), "max": float(xs.max()), "n": int(xs.size)}


def _shape_case(name):
    import numpy as np
    if name == "10x128_scalar":
        from bpldenoising_amd import testdataset
        ub, f = testdataset("faces_train", npz=NPZ)
        return ub[:10], f[:10], 0.1, 5000
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from conftest import synth_batch
    ub, f = synth_batch(8, 1024, 1024, seed=52)
    return ub, f, 0.05 + 0.1 * np.random.default_rng(12).random((1024, 1024)), 1000


def time_case(name, reps):
    import numpy as np
    import torch
    from bpldenoising_amd import TVSolver
    from bpldenoising_amd.torch_layer import tv_denoise
    ub, f, alpha, maxiter = _shape_case(name)
    O, N, M = f.shape
    s = TVSolver(M, N, O, device=0)
    s.set_data(ub, f)
    u, _, _ = s.evaluate(alpha, 0.1, maxiter=maxiter)
    gu = u - ub
    s.gradient(u, ub, alpha)
    s.vjp(u, alpha, gu)   # warm-up of both
    grad_ms, vjp_ms, grad_wall, vjp_wall = [], [], [], []
    for _ in range(reps):
        t = time.perf_counter()
        g0 = s.gradient(u, ub, alpha)
        grad_wall.append(1e3 * (time.perf_counter() - t))
        grad_ms.append(s.stats()["adjoint_ms"])
        t = time.perf_counter()
        gf, ga = s.vjp(u, alpha, gu)
        vjp_wall.append(1e3 * (time.perf_counter() - t))
        vjp_ms.append(s.stats()["adjoint_ms"])
    same = bool(np.array_equal(np.asarray(g0), np.asarray(ga)))
    # torch forward + backward against one evaluate (same solve, same adjoint)
    dev = torch.device("cuda", 0)
    tf, tub = torch.from_numpy(f).to(dev), torch.from_numpy(ub).to(dev)
    ta = torch.tensor(alpha, dtype=torch.float64, device=dev, requires_grad=True)

    def torch_step():
        ta.grad = None
        loss = 0.5 * ((tv_denoise(tf, ta, maxiter=maxiter) - tub) ** 2).sum()
        loss.backward()
        torch.cuda.synchronize()

    torch_step()
    s.evaluate(alpha, 0.1, maxiter=maxiter, fetch_u=False)
    t_torch, t_eval = [], []
    for _ in range(reps):
        t = time.perf_counter()
        torch_step()
        t_torch.append(1e3 * (time.perf_counter() - t))
        t = time.perf_counter()
        _, _, ge = s.evaluate(alpha, 0.1, maxiter=maxiter, fetch_u=False)
        t_eval.append(1e3 * (time.perf_counter() - t))
    same_torch = bool(np.array_equal(ta.grad.cpu().numpy(), np.asarray(ge)))
    st = s.stats()
    s.close()
    return {"what": "vjp_vs_gradient", "case": name, "maxiter": maxiter, "adjoint_method": st["adjoint_method"],
            "gradient_adjoint_ms": _stats(grad_ms), "vjp_adjoint_ms": _stats(vjp_ms),
            "gradient_wall_ms": _stats(grad_wall), "vjp_wall_ms": _stats(vjp_wall), "vjp_equals_gradient": same,
            "torch_fwd_bwd_wall_ms": _stats(t_torch), "evaluate_wall_ms": _stats(t_eval),
            "torch_grad_equals_evaluate": same_torch}


def child_evaluate(root, reps):
    """10 x 128^2 evaluate with the package under `root` (run in a fresh process)."""
    sys.path.insert(0, root)
    from bpldenoising_amd import TVSolver, testdataset
    ub, f = testdataset("faces_train", npz=NPZ)
    s = TVSolver(128, 128, 10, device=0)
    s.set_data(ub[:10], f[:10])
    for _ in range(3):
        s.evaluate(0.1, 0.1, fetch_u=False)
    wall, adj, pdhg = [], [], []
    for _ in range(reps):
        t = time.perf_counter()
        _, c, g = s.evaluate(0.1, 0.1, fetch_u=False)
        wall.append(1e3 * (time.perf_counter() - t))
        adj.append(s.stats()["adjoint_ms"])
        pdhg.append(s.stats()["pdhg_ms"])
    s.close()
    return {"evaluate_wall_ms": _stats(wall), "pdhg_ms": _stats(pdhg), "adjoint_ms": _stats(adj), "cost": c, "grad": g}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--base", default=None)
    ap.add_argument("--child-root", default=None)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=".", help="directory of vjp_time.json")
    ap.add_argument("--cases", default="10x128_scalar,8x1024_map")
    a = ap.parse_args()
    if a.child_root:
        print(json.dumps(child_evaluate(a.child_root, a.reps)))
        return
    res = []
    for name in a.cases.split(","):
        r = time_case(name, a.reps if name.startswith("10x") else max(3, a.reps // 2))
        print(json.dumps(r), flush=True)
        res.append(r)
    if a.base:
        roots = {"base": os.path.abspath(a.base), "this": ROOT}
        for rnd in range(a.rounds):
            for tag in (("base", "this") if rnd % 2 == 0 else ("this", "base")):
                out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child-root", roots[tag], "--reps", "20"],
                                     capture_output=True, text=True, timeout=600)
                if out.returncode != 0:
                    raise SystemExit("child (%s) failed rc=%d: %s" % (tag, out.returncode, out.stderr[-2000:]))
                r = dict(json.loads(out.stdout.strip().splitlines()[-1]), what="evaluate_ab", lib=tag, round=rnd)
                print(json.dumps(r), flush=True)
                res.append(r)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "vjp_time.json"), "w") as fh:
        json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
