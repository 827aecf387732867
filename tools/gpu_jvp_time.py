#!/usr/bin/env python3
"""Developer probe: the cost of the Jacobian-vector product (bpltv_jvp) and of bpltv_gauss_newton.

    python tools/gpu_jvp_time.py [--reps 10] [--out DIR] [--cases 10x128_scalar,8x1024_map,10x128_patch22]

One process, candidates alternated after a warm-up, median with min - max of stats.adjoint_ms (device time):
1. bpltv_jvp with one direction against bpltv_vjp on the same u: 10 x 128^2 (faces_train, scalar alpha, u of a
   5000-iteration solve) and 8 x 1024^2 (pixel map).  The factorisation and the substitutions are the same; the
   JVP adds one pass that writes the tangent right-hand side.
2. The shared factorisation, 10 x 128^2 with a 2 x 2 patch: one bpltv_jvp call with four directions against four calls
   with one direction each, and bpltv_gauss_newton (four columns + the Gram reduction) against bpltv_gradient.
Every result is printed as one JSON line and collected in DIR/jvp_time.json."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
NPZ = os.path.join(ROOT, "tests", "golden", "datasets.npz")
P22 = [[0.08, 0.12], [0.1, 0.05]]


def _stats(xs):
    import numpy as np
    xs = np.asarray(xs, dtype=float)
    return {"median": float(np.median(xs)), "min": float(xs.min()), "max": float(xs.max()), "n": int(xs.size)}


def _shape_case(name):
    import numpy as np
    if name.startswith("10x128"):
        from bpldenoising_amd import testdataset
        ub, f = testdataset("faces_train", npz=NPZ)
        return ub[:10], f[:10], (0.1 if name.endswith("scalar") else np.array(P22)), 5000
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from conftest import synth_batch
    ub, f = synth_batch(8, 1024, 1024, seed=52)
    return ub, f, 0.05 + 0.1 * np.random.default_rng(12).random((1024, 1024)), 1000


def _timed(fn, s):
    t = time.perf_counter()
    fn()
    return 1e3 * (time.perf_counter() - t), s.stats()["adjoint_ms"]


def time_jvp_vs_vjp(name, reps):
    import numpy as np
    from bpldenoising_amd import TVSolver
    ub, f, alpha, maxiter = _shape_case(name)
    O, N, M = f.shape
    s = TVSolver(M, N, O, device=0)
    s.set_data(ub, f)
    u = s.denoise(alpha, maxiter=maxiter)
    rng = np.random.default_rng(1)
    gu, df = u - ub, rng.standard_normal(u.shape)
    da = rng.standard_normal(np.shape(alpha)) if np.ndim(alpha) else 1.0
    cands = {"vjp": lambda: s.vjp(u, alpha, gu), "jvp_df": lambda: s.jvp(u, alpha, df=df),
             "jvp_dalpha": lambda: s.jvp(u, alpha, dalpha=da), "jvp_both": lambda: s.jvp(u, alpha, df=df, dalpha=da)}
    for fn in cands.values():
        fn()   # warm-up
    dev, wall = {k: [] for k in cands}, {k: [] for k in cands}
    for _ in range(reps):
        for k, fn in cands.items():
            w, d = _timed(fn, s)
            wall[k].append(w)
            dev[k].append(d)
    st = s.stats()
    s.close()
    r = {"what": "jvp_vs_vjp", "case": name, "maxiter": maxiter, "adjoint_method": st["adjoint_method"]}
    for k in cands:
        r[k + "_adjoint_ms"] = _stats(dev[k])
        r[k + "_wall_ms"] = _stats(wall[k])
    r["jvp_both_over_vjp"] = r["jvp_both_adjoint_ms"]["median"] / r["vjp_adjoint_ms"]["median"]
    return r


def time_shared_factorisation(name, reps):
    import numpy as np
    from bpldenoising_amd import TVSolver
    ub, f, alpha, maxiter = _shape_case(name)
    O, N, M = f.shape
    s = TVSolver(M, N, O, device=0)
    s.set_data(ub, f)
    u = s.denoise(alpha, maxiter=maxiter)
    P = int(np.size(alpha))
    eye = np.eye(P).reshape((P,) + np.shape(alpha))

    def four_calls():
        ts = [_timed(lambda j=j: s.jvp(u, alpha, dalpha=eye[j]), s) for j in range(P)]
        return sum(t[0] for t in ts), sum(t[1] for t in ts)
    cands = {"jvp_ndir4": lambda: _timed(lambda: s.jvp(u, alpha, dalpha=eye), s), "jvp_4x_ndir1": four_calls,
             "gauss_newton": lambda: _timed(lambda: s.gauss_newton(u, ub, alpha), s),
             "gradient": lambda: _timed(lambda: s.gradient(u, ub, alpha), s)}
    for fn in cands.values():
        fn()
    dev, wall = {k: [] for k in cands}, {k: [] for k in cands}
    for _ in range(reps):
        for k, fn in cands.items():
            w, d = fn()
            wall[k].append(w)
            dev[k].append(d)
    s.close()
    r = {"what": "shared_factorisation", "case": name, "ndir": P,
         "note": "adjoint_ms of gauss_newton excludes its Gram reduction; the wall times include it and the host copies"}
    for k in cands:
        r[k + "_adjoint_ms"] = _stats(dev[k])
        r[k + "_wall_ms"] = _stats(wall[k])
    r["ndir4_over_4x_ndir1"] = r["jvp_ndir4_adjoint_ms"]["median"] / r["jvp_4x_ndir1_adjoint_ms"]["median"]
    r["gauss_newton_over_gradient"] = r["gauss_newton_adjoint_ms"]["median"] / r["gradient_adjoint_ms"]["median"]
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=".", help="directory of jvp_time.json")
    ap.add_argument("--cases", default="10x128_scalar,8x1024_map,10x128_patch22")
    a = ap.parse_args()
    res = []
    for name in a.cases.split(","):
        if name.endswith("patch22"):
            r = time_shared_factorisation(name, a.reps)
        else:
            r = time_jvp_vs_vjp(name, a.reps if name.startswith("10x") else max(3, a.reps // 2))
        print(json.dumps(r), flush=True)
        res.append(r)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "jvp_time.json"), "w") as fh:
        json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
