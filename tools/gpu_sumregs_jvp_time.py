#!/usr/bin/env python3
"""Developer probe: the cost of the sum-of-regularisers Jacobian-vector product (bpltv_sumregs_jvp) and of
bpltv_sumregs_gauss_newton.

    python tools/gpu_sumregs_jvp_time.py [--reps 10] [--out DIR] [--vjp-lib PATH]

One process, candidates alternated after a warm-up, median with min - max of stats.adjoint_ms (device time between two
events around the adjoint) and of the wall time.  10 x 128^2 (faces_train), u of a 5000-iteration sumregs_denoise:
1. sumregs_jvp with one direction against sumregs_vjp on the same u: the vector [a1; a2; a3] with reg = 0 (nested
   dissection, Cholesky) and a 2 x 2 x 3 patch with reg = 1 (the row-scaled system, LU; the JVP factors its transpose).
   One factorisation and one solve each.  --vjp-lib PATH times sumregs_vjp of another build of the library (the commit
   before forward mode) on the same data in a fresh child process (BPLTV_LIB_PATH) and adds it to the record.
2. One call with eight directions against eight calls with one direction each.
3. sumregs_gauss_newton with P = 3 (vector) and P = 12 (2 x 2 patch) against P single-direction calls.
Every result is printed as one JSON line and collected in DIR/sumregs_jvp_time.json."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
NPZ = os.path.join(ROOT, "tests", "golden", "datasets.npz")
A3 = [0.03, 0.02, 0.05]
P22 = [[[0.03, 0.05], [0.02, 0.04]], [[0.02, 0.03], [0.05, 0.02]], [[0.04, 0.02], [0.03, 0.06]]]
CASES = {"vector_reg0": (A3, 0), "patch22_reg1": (P22, 1)}
MAXITER = 5000


def _stats(xs):
    import numpy as np
    xs = np.asarray(xs, dtype=float)
    return {"median": float(np.median(xs)), "min": float(xs.min()), "max": float(xs.max()), "n": int(xs.size)}


def _setup(case):
    import numpy as np
    from bpldenoising_amd import TVSolver, testdataset
    x, reg = CASES[case]
    x = np.array(x)
    ub, f = testdataset("faces_train", npz=NPZ)
    ub, f = ub[:10], f[:10]
    O, N, M = f.shape
    s = TVSolver(M, N, O, device=0)
    s.set_data(ub, f)
    u = s.sumregs_denoise(x, maxiter=MAXITER)
    return s, ub, u, x, reg


def _timed(fn, s):
    t = time.perf_counter()
    fn()
    return 1e3 * (time.perf_counter() - t), s.stats()["adjoint_ms"]


def _alternate(cands, reps):
    for fn in cands.values():
        fn()   # warm-up
    dev, wall = {k: [] for k in cands}, {k: [] for k in cands}
    for _ in range(reps):
        for k, fn in cands.items():
            w, d = fn()
            wall[k].append(w)
            dev[k].append(d)
    r = {}
    for k in cands:
        r[k + "_adjoint_ms"] = _stats(dev[k])
        r[k + "_wall_ms"] = _stats(wall[k])
    return r


def time_vjp_only(case, reps):
    """sumregs_vjp alone: what a child process with another build of the library runs."""
    import ctypes
    from bpldenoising_amd import _lib
    other = ctypes.CDLL(_lib.LIB_PATH)   # an older build lacks the newer entry points: bind what it exports
    for name in [n for n in _lib.SYMBOLS if not hasattr(other, n)]:
        del _lib.SYMBOLS[name]
    s, ub, u, x, reg = _setup(case)
    gu = u - ub
    r = {"what": "vjp_only", "case": case, "lib": os.environ.get("BPLTV_LIB_PATH", "")}
    r.update(_alternate({"vjp": lambda: _timed(lambda: s.sumregs_vjp(u, x, gu, reg=reg), s)}, reps))
    r["adjoint_method"] = s.stats()["adjoint_method"]
    s.close()
    return r


def time_case(case, reps, vjp_lib):
    import numpy as np
    s, ub, u, x, reg = _setup(case)
    rng = np.random.default_rng(1)
    gu, df, dx = u - ub, rng.standard_normal(u.shape), rng.standard_normal(x.shape)
    K = 8
    df8, dx8 = rng.standard_normal((K,) + u.shape), rng.standard_normal((K,) + x.shape)
    P = int(x.size)
    eye = np.eye(P).reshape((P,) + x.shape)

    def calls(n, fn):
        def run():
            ts = [_timed(lambda j=j: fn(j), s) for j in range(n)]
            return sum(t[0] for t in ts), sum(t[1] for t in ts)
        return run
    cands = {"vjp": lambda: _timed(lambda: s.sumregs_vjp(u, x, gu, reg=reg), s),
             "jvp_df": lambda: _timed(lambda: s.sumregs_jvp(u, x, df=df, reg=reg), s),
             "jvp_both": lambda: _timed(lambda: s.sumregs_jvp(u, x, df=df, dalpha=dx, reg=reg), s),
             "jvp_ndir8": lambda: _timed(lambda: s.sumregs_jvp(u, x, df=df8, dalpha=dx8, reg=reg), s),
             "jvp_8x_ndir1": calls(K, lambda j: s.sumregs_jvp(u, x, df=df8[j], dalpha=dx8[j], reg=reg)),
             "gauss_newton": lambda: _timed(lambda: s.sumregs_gauss_newton(u, ub, x, reg=reg), s),
             "jvp_Px_ndir1": calls(P, lambda j: s.sumregs_jvp(u, x, dalpha=eye[j], reg=reg))}
    r = {"what": "sumregs_jvp", "case": case, "reg": reg, "P": P, "maxiter": MAXITER,
         "note": "adjoint_ms of gauss_newton excludes its Gram reduction; the wall times include it and the host copies"}
    r.update(_alternate(cands, reps))
    r["adjoint_method"] = s.stats()["adjoint_method"]
    s.close()
    med = lambda k: r[k + "_adjoint_ms"]["median"]
    r["jvp_both_over_vjp"] = med("jvp_both") / med("vjp")
    r["ndir8_over_8x_ndir1"] = med("jvp_ndir8") / med("jvp_8x_ndir1")
    r["gauss_newton_over_Px_ndir1"] = med("gauss_newton") / med("jvp_Px_ndir1")
    if vjp_lib:   # a fresh process: the library is chosen when bpldenoising_amd._lib is imported
        env = dict(os.environ, BPLTV_LIB_PATH=os.path.abspath(vjp_lib))
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--vjp-only", case, "--reps", str(reps)], env=env,
                             capture_output=True, text=True, timeout=600, check=True).stdout
        other = json.loads([ln for ln in out.splitlines() if ln.startswith("{")][-1])
        r["other_build_vjp_adjoint_ms"] = other["vjp_adjoint_ms"]
        r["other_build_vjp_wall_ms"] = other["vjp_wall_ms"]
        r["jvp_both_over_other_build_vjp"] = med("jvp_both") / other["vjp_adjoint_ms"]["median"]
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=".", help="directory of sumregs_jvp_time.json")
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--vjp-lib", default="", help="another build of libbpltv.so whose sumregs_vjp is timed on the same data")
    ap.add_argument("--vjp-only", default="", help="(child process) time sumregs_vjp of this case alone")
    a = ap.parse_args()
    if a.vjp_only:
        print(json.dumps(time_vjp_only(a.vjp_only, a.reps)), flush=True)
        return
    res = []
    for case in a.cases.split(","):
        r = time_case(case, a.reps, a.vjp_lib)
        print(json.dumps(r), flush=True)
        res.append(r)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "sumregs_jvp_time.json"), "w") as fh:
        json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
