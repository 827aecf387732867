#!/usr/bin/env python3
"""Developer probe: the cost of per-image sum-of-regularisers weights (bpltv_sumregs_denoise_each,
bpltv_sumregs_vjp_each) and what the shared path pays for them.

    python tools/gpu_sumregs_each_time.py [--reps 10] [--base ROOT] [--rounds 3] [--out DIR]

1. PDHG device time (stats.pdhg_ms) of sumregs_denoise_each with a different block per image against sumregs_denoise
   with one shared block of the same kind on the same handle, alternated after a warm-up: 10 x 128^2 at 5000 iterations,
   (3,) vectors and three 128^2 maps per image.
2. Adjoint device time (stats.adjoint_ms) of sumregs_vjp_each against sumregs_vjp on the same u and cotangent,
   alternated, same cases.
3. Wall time of one batched forward + backward through torch_layer.sumregs_denoise_each (L2 loss) against a loop of
   one-image torch_layer.sumregs_denoise calls doing the same, 10 x 128^2 vectors, 5000 iterations.
4. --base ROOT: a checkout of another commit with its library built.  Fresh child processes time the shared
   sumregs_denoise of 10 x 128^2 at 5000 iterations (20 solves after 3 warm-up solves, stats.pdhg_ms) with ROOT's
   package and with this tree's, alternated for --rounds rounds, and report whether u is bitwise the same.
Every number is printed as one JSON line and collected in DIR/sumregs_each_time.json."""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

A3 = [0.03, 0.02, 0.05]
O, N, M, MAXITER = 10, 128, 128, 5000


def _stats(xs):
    import numpy as np
    xs = np.asarray(xs, dtype=float)
    return {"median": float(np.median(xs)), "min": float(xs.min()), "max": float(xs.max()), "n": int(xs.size)}


def _case(kind):
    """(ubar, f, shared block, O blocks)"""
    import numpy as np
    from conftest import synth_batch
    rng = np.random.default_rng(5)
    ub, f = synth_batch(O, N, M, seed=5)
    if kind == "vector":
        return ub, f, np.asarray(A3), 0.02 + 0.04 * rng.random((O, 3))
    return ub, f, 0.02 + 0.04 * rng.random((3, N, M)), 0.02 + 0.04 * rng.random((O, 3, N, M))


def time_case(kind, reps, out):
    from bpldenoising_amd import TVSolver
    ub, f, shared, each = _case(kind)
    s = TVSolver(M, N, O, device=0)
    s.set_data(ub, f)
    s.sumregs_denoise(shared, maxiter=MAXITER, fetch=False)
    s.sumregs_denoise_each(each, maxiter=MAXITER, fetch=False)   # warm-up: graphs of both
    sh_ms, ea_ms = [], []
    for _ in range(reps):
        s.sumregs_denoise(shared, maxiter=MAXITER, fetch=False)
        sh_ms.append(s.stats()["pdhg_ms"])
        s.sumregs_denoise_each(each, maxiter=MAXITER, fetch=False)
        ea_ms.append(s.stats()["pdhg_ms"])
    rec = {"case": "10x128_" + kind, "what": "pdhg", "maxiter": MAXITER, "shared_ms": _stats(sh_ms), "each_ms": _stats(ea_ms),
           "variant": s.stats()["pdhg_variant"], "launch_chains": s.stats()["launch_chains"]}
    print(json.dumps(rec), flush=True)
    out.append(rec)
    u = s.sumregs_denoise_each(each, maxiter=MAXITER)
    gu = u - ub
    s.sumregs_vjp(u, shared, gu)
    s.sumregs_vjp_each(u, each, gu)   # warm-up of both
    vj, ve = [], []
    for _ in range(reps):
        s.sumregs_vjp(u, shared, gu)
        vj.append(s.stats()["adjoint_ms"])
        s.sumregs_vjp_each(u, each, gu)
        ve.append(s.stats()["adjoint_ms"])
    rec = {"case": "10x128_" + kind, "what": "adjoint", "vjp_ms": _stats(vj), "vjp_each_ms": _stats(ve),
           "adjoint_method": s.stats()["adjoint_method"]}
    print(json.dumps(rec), flush=True)
    out.append(rec)
    s.close()


def time_layer(reps, out):
    """One batched forward + backward of sumregs_denoise_each against a loop of one-image sumregs_denoise calls."""
    import torch
    from bpldenoising_amd.torch_layer import sumregs_denoise, sumregs_denoise_each
    ub, f, _, each = _case("vector")
    dev = torch.device("cuda", 0)
    tf, tub = torch.from_numpy(f).to(dev), torch.from_numpy(ub).to(dev)
    ta = torch.tensor(each, dtype=torch.float64, device=dev, requires_grad=True)
    tas = [torch.tensor(each[k], dtype=torch.float64, device=dev, requires_grad=True) for k in range(O)]

    def batched():
        ta.grad = None
        loss = 0.5 * ((sumregs_denoise_each(tf, ta, maxiter=MAXITER) - tub) ** 2).sum()
        loss.backward()
        torch.cuda.synchronize()

    def loop():
        for k in range(O):
            tas[k].grad = None
            loss = 0.5 * ((sumregs_denoise(tf[k:k + 1], tas[k], maxiter=MAXITER) - tub[k:k + 1]) ** 2).sum()
            loss.backward()
        torch.cuda.synchronize()

    batched(); loop()   # warm-up
    tb, tl = [], []
    for _ in range(reps):
        t = time.perf_counter(); batched(); tb.append(1e3 * (time.perf_counter() - t))
        t = time.perf_counter(); loop(); tl.append(1e3 * (time.perf_counter() - t))
    worst = max(float((ta.grad[k] - tas[k].grad).abs().max() / tas[k].grad.abs().max()) for k in range(O))
    rec = {"case": "10x128_vector", "what": "layer forward+backward wall", "maxiter": MAXITER, "batched_ms": _stats(tb),
           "loop_of_one_image_calls_ms": _stats(tl), "grad_worst_rel_diff": worst}
    print(json.dumps(rec), flush=True)
    out.append(rec)


def child_shared(root, reps):
    """The shared sumregs_denoise of 10 x 128^2 (vector parameter) with the package under `root` (a fresh process)."""
    sys.path.insert(0, root)
    import numpy as np
    from bpldenoising_amd import TVSolver
    ub, f, shared, _ = _case("vector")
    s = TVSolver(M, N, O, device=0)
    s.set_data(ub, f)
    for _ in range(3):
        s.sumregs_denoise(shared, maxiter=MAXITER, fetch=False)
    pdhg = []
    for _ in range(reps):
        s.sumregs_denoise(shared, maxiter=MAXITER, fetch=False)
        pdhg.append(s.stats()["pdhg_ms"])
    u = s.sumregs_denoise(shared, maxiter=MAXITER)
    st = s.stats()
    s.close()
    return {"pdhg_ms": _stats(pdhg), "variant": st["pdhg_variant"], "launch_chains": st["launch_chains"],
            "u_sha256": hashlib.sha256(np.ascontiguousarray(u).tobytes()).hexdigest()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--base", default=None)
    ap.add_argument("--child-root", default=None)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=".", help="directory of sumregs_each_time.json")
    ap.add_argument("--skip", default="", help="comma-separated parts to leave out: cases, layer")
    a = ap.parse_args()
    if a.child_root:
        print(json.dumps(child_shared(a.child_root, a.reps)))
        return
    res = []
    skip = set(a.skip.split(","))
    if "cases" not in skip:
        for kind in ("vector", "map"):
            time_case(kind, a.reps, res)
    if "layer" not in skip:
        time_layer(a.reps, res)
    if a.base:
        roots = {"base": os.path.abspath(a.base), "this": ROOT}
        medians, lo, hi, shas = {"base": [], "this": []}, {"base": [], "this": []}, {"base": [], "this": []}, set()
        for rnd in range(a.rounds):
            for tag in (("base", "this") if rnd % 2 == 0 else ("this", "base")):
                out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child-root", roots[tag], "--reps", "20"],
                                     capture_output=True, text=True, timeout=600)
                if out.returncode != 0:
                    raise SystemExit("child (%s) failed rc=%d: %s" % (tag, out.returncode, out.stderr[-2000:]))
                r = dict(json.loads(out.stdout.strip().splitlines()[-1]), what="shared_sumregs_denoise_ab", lib=tag, round=rnd)
                medians[tag].append(r["pdhg_ms"]["median"])
                lo[tag].append(r["pdhg_ms"]["min"])
                hi[tag].append(r["pdhg_ms"]["max"])
                shas.add(r.pop("u_sha256"))
                print(json.dumps(r), flush=True)
                res.append(r)
        summary = {"what": "shared_sumregs_denoise_ab_summary", "u_identical": len(shas) == 1,
                   "base_medians_ms": medians["base"], "this_medians_ms": medians["this"],
                   "base_median_of_medians_ms": _stats(medians["base"])["median"],
                   "this_median_of_medians_ms": _stats(medians["this"])["median"],
                   "base_all_solves_ms": [min(lo["base"]), max(hi["base"])], "this_all_solves_ms": [min(lo["this"]), max(hi["this"])],
                   "this_median_inside_base_medians": bool(min(medians["base"]) <= _stats(medians["this"])["median"] <= max(medians["base"])),
                   "this_median_inside_base_solves": bool(min(lo["base"]) <= _stats(medians["this"])["median"] <= max(hi["base"]))}
        print(json.dumps(summary), flush=True)
        res.append(summary)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "sumregs_each_time.json"), "w") as fh:
        json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
