#!/usr/bin/env python3
"""Developer probe: the cost of one parameter per image (bpltv_denoise_each, bpltv_vjp_each).

    python tools/gpu_each_time.py [--reps 10] [--out DIR]

1. PDHG device time (stats.pdhg_ms) of denoise_each with a different parameter per image against denoise with one
   shared parameter of the same kind, alternated after a warm-up: 10 x 128^2 scalars (5000 iterations), 8 x 1024^2
   scalars and 8 x 1024^2 maps (480 iterations, reported as iterations per second too).  On the maps also denoise_each
   with O copies of the shared map: equal values, O distinct planes to read.
2. Adjoint device time (stats.adjoint_ms) of vjp_each against vjp on the same u and cotangent, alternated, on the same
   two shapes.
3. Wall time of one batched forward + backward (denoise_each + vjp_each) against a loop of O one-image handles doing the
   same (denoise + vjp per image) on 10 x 128^2 scalars, 5000 iterations.
Every number is printed as one JSON line and collected in DIR/each_time.json."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def _stats(xs):
    import numpy as np
    xs = np.asarray(xs, dtype=float)
    return {"median": float(np.median(xs)), "min": float(xs.min()), "max": float(xs.max()), "n": int(xs.size)}


def _case(name):
    import numpy as np
    from conftest import synth_batch
    rng = np.random.default_rng(5)
    if name == "10x128_scalar":
        ub, f = synth_batch(10, 128, 128, seed=1)
        return ub, f, 0.1, 0.05 + 0.1 * rng.random(10), 5000
    ub, f = synth_batch(8, 1024, 1024, seed=52)
    if name == "8x1024_scalar":
        return ub, f, 0.1, 0.05 + 0.1 * rng.random(8), 480
    return ub, f, 0.05 + 0.1 * rng.random((1024, 1024)), 0.05 + 0.1 * rng.random((8, 1024, 1024)), 480


def time_case(name, reps, out):
    from bpldenoising_amd import TVSolver
    ub, f, shared, each, maxiter = _case(name)
    O, N, M = f.shape
    s = TVSolver(M, N, O, device=0)
    s.set_data(ub, f)
    s.denoise(shared, maxiter=maxiter, fetch=False)
    s.denoise_each(each, maxiter=maxiter, fetch=False)   # warm-up: graphs of both
    sh_ms, ea_ms = [], []
    for _ in range(reps):
        s.denoise(shared, maxiter=maxiter, fetch=False)
        sh_ms.append(s.stats()["pdhg_ms"])
        s.denoise_each(each, maxiter=maxiter, fetch=False)
        ea_ms.append(s.stats()["pdhg_ms"])
    rec = {"case": name, "what": "pdhg", "maxiter": maxiter, "shared_ms": _stats(sh_ms), "each_ms": _stats(ea_ms),
           "shared_it_per_s": maxiter / (_stats(sh_ms)["median"] / 1e3), "each_it_per_s": maxiter / (_stats(ea_ms)["median"] / 1e3),
           "variant": s.stats()["pdhg_variant"]}
    if name.endswith("_map"):   # O copies of the shared map: the cost of O planes to read, whatever their values
        import numpy as np
        copies = np.stack([shared] * O)
        s.denoise_each(copies, maxiter=maxiter, fetch=False)
        cp = []
        for _ in range(reps):
            s.denoise_each(copies, maxiter=maxiter, fetch=False)
            cp.append(s.stats()["pdhg_ms"])
        rec["each_copies_ms"] = _stats(cp)
        rec["each_copies_it_per_s"] = maxiter / (_stats(cp)["median"] / 1e3)
    print(json.dumps(rec), flush=True)
    out.append(rec)
    u = s.denoise_each(each, maxiter=maxiter)
    gu = u - ub
    s.vjp(u, shared, gu)
    s.vjp_each(u, each, gu)   # warm-up of both
    vj, ve = [], []
    for _ in range(reps):
        s.vjp(u, shared, gu)
        vj.append(s.stats()["adjoint_ms"])
        s.vjp_each(u, each, gu)
        ve.append(s.stats()["adjoint_ms"])
    rec = {"case": name, "what": "adjoint", "vjp_ms": _stats(vj), "vjp_each_ms": _stats(ve)}
    print(json.dumps(rec), flush=True)
    out.append(rec)
    s.close()


def time_loop(reps, out):
    """O one-image handles (denoise + vjp each) against one batched handle (denoise_each + vjp_each)."""
    from bpldenoising_amd import TVSolver
    ub, f, _, each, maxiter = _case("10x128_scalar")
    O, N, M = f.shape
    s = TVSolver(M, N, O, device=0)
    s.set_data(ub, f)
    ones = []
    for k in range(O):
        h = TVSolver(M, N, 1, device=0)
        h.set_data(ub[k:k + 1], f[k:k + 1])
        ones.append(h)

    def batched():
        u = s.denoise_each(each, maxiter=maxiter)
        s.vjp_each(u, each, u - ub)

    def loop():
        for k, h in enumerate(ones):
            u = h.denoise(float(each[k]), maxiter=maxiter)
            h.vjp(u, float(each[k]), u - ub[k:k + 1])

    batched(); loop()   # warm-up
    tb, tl = [], []
    for _ in range(reps):
        t = time.perf_counter(); batched(); tb.append(1e3 * (time.perf_counter() - t))
        t = time.perf_counter(); loop(); tl.append(1e3 * (time.perf_counter() - t))
    rec = {"case": "10x128_scalar", "what": "forward+backward wall", "maxiter": maxiter, "batched_ms": _stats(tb),
           "loop_of_one_image_handles_ms": _stats(tl)}
    print(json.dumps(rec), flush=True)
    out.append(rec)
    for h in ones:
        h.close()
    s.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=".", help="directory of each_time.json")
    a = ap.parse_args()
    out = []
    for name in ("10x128_scalar", "8x1024_scalar", "8x1024_map"):
        time_case(name, a.reps, out)
    time_loop(a.reps, out)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "each_time.json"), "w") as fh:
        json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
