#!/usr/bin/env python3
"""Developer probe: do two (or more) builds of libbpltv run the adjoint solves to the same bits, statistics, refusals and
speed?  Written for the fold of the two adjoint host drivers into run_adjoint, where the answer has
to be "yes".

Every build runs in fresh child processes of its own (BPLTV_LIB_PATH), each under a time limit; nothing more is started after
a child fails.

bits: a child runs one part of the matrix and prints, per call, the SHA-256 of every output array and the statistics
    adjoint_method, adjoint_chunks, adjoint_attempts, kappa_used, reg_gradient_used, hb_sync, adjoint_residual(_raw) -- or, for
    a refused call, the return code and bpltv_last_error's text.  The parent compares every entry between the builds.
    Inputs: tests/tv_active_ref.py / tests/sumregs_active_ref.py, layout "flat" (a constant image, two flat blocks, an untouched
    image) on 3 x 24 x 40 (LDS band, block cyclic reduction, nested dissection) and 3 x 12 x 140 (M > 138: the band in HBM), each
    with the whole batch at once and with adjoint_budget_mb forcing groups of 2 + 1 images.
      tv-*        scalar / 2 x 2 patch / map, reg 0 / 1, adjoint_method nd / bcr / band: evaluate, gradient, vjp (both outputs,
                  grad_f alone, grad_alpha alone), vjp_each, jvp (1 and 3 directions), jvp_each, gauss_newton
      weighted-*  weighted_vjp with one weight plane and one per image, with and without grad_w, the three methods and kinds
      sr-*        vector / 2 x 2 patch / map, reg 0 / 1 (reg with an array parameter: the row-scaled LU), nd / band, sr_force_lu
                  0 / 1: the sumregs_ forms of the same entry points
      fixed       the kappa retry (kappa_cap = 1e300 on the 10 x 128^2 batch of test_breakdown_retry_is_visible_...) and one
                  refused call per model (reg with a patch that holds a zero)
time: a child times, after a warm-up, `per` calls each on faces_train_128_10 (10 x 128^2): stats()["adjoint_ms"] of a scalar
    evaluate and of a sumregs_vjp, stats()["total_ms"] and wall time of a vjp_device (host-bound).  The builds alternate in
    rounds; list the same build twice (a copy of the file under another name) for the spread between two loads of one build.
usage: python tools/adjoint_driver_ab.py bits name=path/to/libbpltv.so name=path [...]
       python tools/adjoint_driver_ab.py time rounds per name=path name=path [...]                         (GPU box)"""
import ctypes as C
import hashlib, json, os, re, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np

STATS = ("adjoint_method", "adjoint_chunks", "adjoint_attempts", "kappa_used", "reg_gradient_used", "hb_sync", "adjoint_residual",
         "adjoint_residual_raw")
SHAPES = {"small": (3, 24, 40), "wide": (3, 12, 140)}
PARTS = ["%s-%s" % (m, s) for m in ("tv", "weighted", "sr") for s in SHAPES] + ["fixed"]


def record(out, name, s, call):
    from bpldenoising_amd._lib import BpltvError
    try:
        res = call()
    except BpltvError as e:
        out[name] = {"rc": e.code, "err": str(e)}
        return
    res = res if isinstance(res, tuple) else (res,)
    st = s.stats()
    out[name] = {"sha": [None if a is None else hashlib.sha256(np.ascontiguousarray(a, dtype=np.float64).tobytes()).hexdigest() for a in res],
                 "stats": {k: repr(st[k]) for k in STATS}}


def workspace_bytes(M, N):
    """Per image: the nested-dissection workspaces (the host check tool runs the library's symbolic code) and the block arrays
    of the cyclic reduction."""
    o = subprocess.run([os.path.join(ROOT, "tools", "_bin", "nd_host_check"), "bytes", str(M), str(N)], capture_output=True, text=True, timeout=120).stdout
    MP = (M + 15) // 16 * 16
    return {"nd": float(re.search(r"bytes_per_image tv (\d+)", o).group(1)), "sr": float(re.search(r"bytes_per_image sr (\d+)", o).group(1)),
            "bcr": 8.0 * (7 * N * MP * MP + 3 * N * M)}


def groupings(s, per_image, factor=2.5):
    """The whole batch at once, then groups of 2 + 1 images (factor: 2.5 workspaces fit; the LU trees take two each: 4.5)."""
    for name, mb in (("whole", 0.0), ("2+1", factor * per_image / 1e6)):
        s.set_option("adjoint_budget_mb", mb)
        yield name


def part_tv(shape, weighted):
    import tv_active_ref as ta
    from bpldenoising_amd import TVSolver
    O, N, M = shape
    ws, out, rng = workspace_bytes(M, N), {}, np.random.default_rng(5)
    s = TVSolver(M, N, O)
    for kind in ta.KINDS:
        alpha, f, u, gu, df, da = ta.case(shape, kind, "flat")
        alphas = np.stack([np.asarray(alpha) * (1.0 + 0.1 * k) for k in range(O)])
        df3, da3, das = rng.standard_normal((3,) + u.shape), rng.standard_normal((3,) + np.shape(alpha)), rng.standard_normal(alphas.shape)
        w = 0.25 + 3.75 * rng.random(u.shape)
        s.set_data(u, f)
        for method in ("nd", "bcr", "band"):
            for grp in groupings(s, ws["bcr" if method == "bcr" else "nd"]):
                if weighted:
                    for wname, wa in (("w1", w[0]), ("wO", w)):
                        for want_w in (True, False):
                            record(out, "weighted_vjp %s %s %s %s grad_w=%d" % (kind, method, grp, wname, want_w), s,
                                   lambda: s.weighted_vjp(u, f, alpha, wa, gu, want_w=want_w, adjoint_method=method))
                    continue
                for reg in (0, 1):
                    kw = dict(reg=reg, adjoint_method=method)
                    calls = {"evaluate": lambda: s.evaluate(alpha, 0.0 if reg else 0.1, maxiter=60, adjoint_method=method),
                             "gradient": lambda: s.gradient(u, f, alpha, **kw),
                             "vjp": lambda: s.vjp(u, alpha, gu, **kw),
                             "vjp grad_f": lambda: s.vjp(u, alpha, gu, want_alpha=False, **kw),
                             "vjp grad_alpha": lambda: s.vjp(u, alpha, gu, want_f=False, **kw),
                             "vjp_each": lambda: s.vjp_each(u, alphas, gu, **kw),
                             "jvp": lambda: s.jvp(u, alpha, df, da, **kw),
                             "jvp ndir=3": lambda: s.jvp(u, alpha, df3, da3, **kw),
                             "jvp_each": lambda: s.jvp_each(u, alphas, df, das, **kw)}
                    if kind != "map":   # at most 16 parameter entries
                        calls["gauss_newton"] = lambda: s.gauss_newton(u, f, alpha, **kw)
                    for name, call in calls.items():
                        record(out, "%s %s reg=%d %s %s" % (name, kind, reg, method, grp), s, call)
    s.close()
    return out


def part_sr(shape):
    import sumregs_active_ref as sa
    from bpldenoising_amd import TVSolver
    O, N, M = shape
    ws, out, rng = workspace_bytes(M, N), {}, np.random.default_rng(6)
    s = TVSolver(M, N, O)
    for kind in ("vector", "patch22", "map"):
        x, f, u, gu, df, dx = sa.case(shape, kind, "flat")
        xs = np.stack([x * (1.0 + 0.1 * k) for k in range(O)])
        df3, dx3, dxs = rng.standard_normal((3,) + u.shape), rng.standard_normal((3,) + x.shape), rng.standard_normal(xs.shape)
        s.set_data(u, f)
        for method in ("nd", "band"):
            for flu in (0, 1):
                s.set_option("sr_force_lu", flu)
                for reg in (0, 1):
                    lu = flu or (reg and kind != "vector")
                    for grp in groupings(s, ws["sr"], 4.5 if lu else 2.5):
                        kw = dict(reg=reg, adjoint_method=method)
                        calls = {"evaluate": lambda: s.sumregs_evaluate(x, 0.0 if reg else 0.1, maxiter=60, adjoint_method=method),
                                 "vjp": lambda: s.sumregs_vjp(u, x, gu, **kw),
                                 "vjp grad_f": lambda: s.sumregs_vjp(u, x, gu, want_alpha=False, **kw),
                                 "vjp grad_alpha": lambda: s.sumregs_vjp(u, x, gu, want_f=False, **kw),
                                 "vjp_each": lambda: s.sumregs_vjp_each(u, xs, gu, **kw),
                                 "jvp": lambda: s.sumregs_jvp(u, x, df, dx, **kw),
                                 "jvp ndir=3": lambda: s.sumregs_jvp(u, x, df3, dx3, **kw),
                                 "jvp_each": lambda: s.sumregs_jvp_each(u, xs, df, dxs, **kw)}
                        if kind != "map":
                            calls["gauss_newton"] = lambda: s.sumregs_gauss_newton(u, f, x, **kw)
                        for name, call in calls.items():
                            record(out, "sumregs %s %s reg=%d %s force_lu=%d %s" % (name, kind, reg, method, flu, grp), s, call)
    s.close()
    return out


def part_fixed():
    from bpldenoising_amd import TVSolver
    from conftest import DATASETS_NPZ
    from oracle import np_twin as tw
    out = {}
    ub, f = tw.load_dataset(DATASETS_NPZ, "faces_train_128_10")
    s = TVSolver(128, 128, 10)
    s.set_data(ub, f)
    record(out, "evaluate 10x128^2", s, lambda: s.evaluate(0.1, 0.1))
    record(out, "evaluate 10x128^2 kappa_cap=1e300 (retry)", s, lambda: s.evaluate(0.1, 0.1, kappa_cap=1e300))
    u = s.denoise(0.1, maxiter=50)
    zero = np.array([[0.1, 0.0], [0.1, 0.1]])
    record(out, "refused: vjp reg=1, patch with a zero", s, lambda: s.vjp(u, zero, u - ub, reg=1))
    record(out, "refused: gradient reg=1, patch with a zero", s, lambda: s.gradient(u, ub, zero, reg=1))
    record(out, "refused: sumregs_vjp reg=1, patch with a zero", s, lambda: s.sumregs_vjp(u, np.stack([zero, zero + 0.1, zero + 0.1]), u - ub, reg=1))
    s.close()
    return out


def child_bits(part):
    if part == "fixed":
        out = part_fixed()
    else:
        model, shape = part.split("-")
        out = part_sr(SHAPES[shape]) if model == "sr" else part_tv(SHAPES[shape], model == "weighted")
    print("ABJSON " + json.dumps(out), flush=True)


def child_time(per):
    import bench
    from bpldenoising_amd import TVSolver
    hip = C.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]

    def dev(a):
        p = C.c_void_p()
        assert hip.hipMalloc(C.byref(p), a.nbytes) == 0
        assert hip.hipMemcpy(p, a.ctypes.data_as(C.c_void_p), a.nbytes, 1) == 0
        return p.value

    ub, f, _ = bench.load_batch("faces_train_128_10", 10, 128, 128, 20211004)
    s = TVSolver(128, 128, 10)
    s.set_data(ub, f)
    a3 = np.array([0.03, 0.02, 0.05])
    u, u3 = s.denoise(0.1, maxiter=5000), s.sumregs_denoise(a3, maxiter=2000)
    d_u, d_a, d_gu = dev(u), dev(np.array([0.1])), dev(u - ub)
    d_gf, d_ga = dev(np.zeros_like(u)), dev(np.zeros(1))
    cases = {"evaluate": (lambda: s.evaluate(0.1, 0.1, fetch_u=False, maxiter=500), "adjoint_ms"),
             "sumregs_vjp": (lambda: s.sumregs_vjp(u3, a3, u3 - ub), "adjoint_ms"),
             "vjp_device": (lambda: s.vjp_device(d_u, d_a, 1, 1, d_gu, d_gf, d_ga), "total_ms")}
    out = {}
    for name, (call, key) in cases.items():
        for _ in range(3):
            call()
        ev, wall = [], []
        for _ in range(per):
            t0 = time.perf_counter()
            call()
            wall.append((time.perf_counter() - t0) * 1e3)
            ev.append(s.stats()[key])
        out[name] = {"ev": ev, "wall": wall}
    s.close()
    print("ABJSON " + json.dumps(out), flush=True)


def run_child(build, path, args, limit):
    pr = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, cwd=ROOT, capture_output=True, text=True, timeout=limit,
                        env=dict(os.environ, BPLTV_LIB_PATH=os.path.abspath(path)))
    if pr.returncode != 0:   # nothing more is started on the GPU after a failure
        sys.exit("child %s of build %s failed (%d):\n%s\n%s" % (args, build, pr.returncode, pr.stdout[-2000:], pr.stderr[-2000:]))
    return json.loads([l for l in pr.stdout.splitlines() if l.startswith("ABJSON ")][-1][7:])


def main_bits(builds):
    first, bad, total = builds[0][0], 0, 0
    for part in PARTS:
        res, secs = {}, {}
        for b, path in builds:
            t0 = time.perf_counter()
            res[b] = run_child(b, path, ["--child-bits", part], 120)
            secs[b] = time.perf_counter() - t0
        ref = res[first]
        refused = sum("rc" in v for v in ref.values())
        methods = sorted({v["stats"]["adjoint_method"] for v in ref.values() if "stats" in v})
        chunks = sorted({v["stats"]["adjoint_chunks"] for v in ref.values() if "stats" in v})
        diff = [(b, k) for b, _ in builds[1:] for k in sorted(set(ref) | set(res[b])) if ref.get(k) != res[b].get(k)]
        total += len(ref)
        bad += len(diff)
        print("%-15s %4d calls (%d refused; adjoint_method %s, adjoint_chunks %s), child %s s: %s" % (
            part, len(ref), refused, ",".join(methods), ",".join(chunks), " / ".join("%.1f" % secs[b] for b, _ in builds),
            "every entry equal" if not diff else "%d entries DIFFER" % len(diff)))
        for b, k in diff[:20]:
            print("    %s: %s\n      %s: %s\n      %s: %s" % (k, b, first, json.dumps(ref.get(k)), b, json.dumps(res[b].get(k))))
        if part == "fixed":
            for k, v in ref.items():
                print("    %s: %s" % (k, json.dumps(v.get("stats", v))))
    print("%d calls per build, builds %s: %s" % (total, ", ".join(b for b, _ in builds), "ALL EQUAL" if bad == 0 else "%d DIFFERENCES" % bad), flush=True)
    sys.exit(1 if bad else 0)


def main_time(rounds, per, builds):
    acc = {b: {} for b, _ in builds}
    for r in range(rounds):
        for b, path in builds:
            for name, v in run_child(b, path, ["--child-time", str(per)], 150).items():
                a = acc[b].setdefault(name, {"ev": [], "wall": []})
                a["ev"] += v["ev"]
                a["wall"] += v["wall"]
    print("faces_train_128_10, 10 x 128^2; %d rounds x %d calls per build, a fresh process per build and round" % (rounds, per))
    print("event ms = stats()['adjoint_ms'] (vjp_device: stats()['total_ms']), wall ms = the call; median [min .. max]")
    print("%-12s %-8s %-31s %s" % ("case", "build", "event ms", "wall ms"))
    first = builds[0][0]
    for name in acc[first]:
        med = {}
        for b, _ in builds:
            e, w = np.array(acc[b][name]["ev"]), np.array(acc[b][name]["wall"])
            med[b] = (np.median(e), np.median(w))
            print("%-12s %-8s %8.3f [%8.3f .. %8.3f]  %8.3f [%8.3f .. %8.3f]" % (name, b, med[b][0], e.min(), e.max(), med[b][1], w.min(), w.max()))
        print("%-12s medians against %s: %s" % (name, first, ", ".join("%s event %+.3f wall %+.3f ms" % (b, med[b][0] - med[first][0], med[b][1] - med[first][1]) for b, _ in builds[1:])), flush=True)


if __name__ == "__main__":
    if sys.argv[1] == "--child-bits":
        child_bits(sys.argv[2])
    elif sys.argv[1] == "--child-time":
        child_time(int(sys.argv[2]))
    elif sys.argv[1] == "bits":
        main_bits([a.split("=", 1) for a in sys.argv[2:]])
    else:
        main_time(int(sys.argv[2]), int(sys.argv[3]), [a.split("=", 1) for a in sys.argv[4:]])
