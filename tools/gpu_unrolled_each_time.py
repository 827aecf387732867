#!/usr/bin/env python3
"""Developer probe: the cost of one parameter per image through the PDHG iterations (bpltv_unrolled_denoise_each,
bpltv_unrolled_vjp_each).

    python tools/gpu_unrolled_each_time.py [--reps 10] [--repeats 5] [--shared-only] [--out DIR]

On 10 x 128^2 with ten different scalars at maxiter = 50:
1. Wall time of forward + backward by one per-image call pair (unrolled_denoise_each + unrolled_vjp_each on one handle)
   against a loop over ten one-image handles doing the same (unrolled_denoise + unrolled_vjp per image), alternated after a
   warm-up.
2. Wall time of the shared unrolled_denoise + unrolled_vjp on the same batch (one scalar) -- the path that must not get
   slower.  --shared-only runs this part alone and uses no per-image entry point, so the same script times an older
   checkout of the library.
Each measurement is the median of --reps calls, repeated --repeats times; the spread of a number is the min - max of its
repeats.  Every number is printed as one JSON line and collected in DIR/unrolled_each_time.json."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

MAXITER = 50


def _stats(xs):
    import numpy as np
    xs = np.asarray(xs, dtype=float)
    return {"median": float(np.median(xs)), "min": float(xs.min()), "max": float(xs.max()), "n": int(xs.size)}


def _case():
    import numpy as np
    from conftest import synth_batch
    ub, f = synth_batch(10, 128, 128, seed=1)
    return ub, f, 0.1, 0.05 + 0.1 * np.random.default_rng(5).random(10)


def _median_ms(call, reps):
    import numpy as np
    ts = []
    for _ in range(reps):
        t = time.perf_counter(); call(); ts.append(1e3 * (time.perf_counter() - t))
    return float(np.median(ts))


def time_shared(reps, repeats, out):
    from bpldenoising_amd import TVSolver
    ub, f, shared, _ = _case()
    O, N, M = f.shape
    s = TVSolver(M, N, O, device=0)
    s.set_data(ub, f)

    def call():
        u = s.unrolled_denoise(shared, maxiter=MAXITER)
        s.unrolled_vjp(shared, u - ub, maxiter=MAXITER)
    call(); call()   # warm-up: graphs of both
    rec = {"case": "10x128_scalar", "what": "shared forward+backward wall", "maxiter": MAXITER,
           "shared_ms": _stats([_median_ms(call, reps) for _ in range(repeats)])}
    call()
    st = s.stats()
    rec["pdhg_ms"], rec["adjoint_ms"] = st["pdhg_ms"], st["adjoint_ms"]
    print(json.dumps(rec), flush=True)
    out.append(rec)
    s.close()


def time_each(reps, repeats, out):
    """One per-image call pair against a loop of O one-image handles."""
    from bpldenoising_amd import TVSolver
    ub, f, _, each = _case()
    O, N, M = f.shape
    s = TVSolver(M, N, O, device=0)
    s.set_data(ub, f)
    ones = []
    for k in range(O):
        h = TVSolver(M, N, 1, device=0)
        h.set_data(ub[k:k + 1], f[k:k + 1])
        ones.append(h)

    def batched():
        u = s.unrolled_denoise_each(each, maxiter=MAXITER)
        s.unrolled_vjp_each(each, u - ub, maxiter=MAXITER)

    def loop():
        for k, h in enumerate(ones):
            u = h.unrolled_denoise(float(each[k]), maxiter=MAXITER)
            h.unrolled_vjp(float(each[k]), u - ub[k:k + 1], maxiter=MAXITER)

    for _ in range(2):
        batched(); loop()   # warm-up
    tb, tl = [], []
    for _ in range(repeats):
        tb.append(_median_ms(batched, reps))
        tl.append(_median_ms(loop, reps))
    rec = {"case": "10x128_scalar", "what": "per-image forward+backward wall", "maxiter": MAXITER, "each_ms": _stats(tb),
           "loop_of_one_image_handles_ms": _stats(tl), "loop_over_each": _stats(tl)["median"] / _stats(tb)["median"]}
    print(json.dumps(rec), flush=True)
    out.append(rec)
    for h in ones:
        h.close()
    s.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10, help="calls per measurement (their median is one repeat)")
    ap.add_argument("--repeats", type=int, default=5, help="repeats of every measurement (min - max = the spread)")
    ap.add_argument("--shared-only", action="store_true", help="only the shared path (also runs on an older library)")
    ap.add_argument("--out", default=".", help="directory of unrolled_each_time.json")
    a = ap.parse_args()
    out = []
    time_shared(a.reps, a.repeats, out)
    if not a.shared_only:
        time_each(a.reps, a.repeats, out)
        time_shared(a.reps, a.repeats, out)   # once more after the per-image calls: the same handle type, a warm device
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "unrolled_each_time.json"), "w") as fh:
        json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
