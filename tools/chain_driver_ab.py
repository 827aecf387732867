#!/usr/bin/env python3
"""Developer probe: do two (or more) builds of libbpltv run the solves at the same speed?  Written for the fold of the
three launch drivers into run_chains, where the answer has to be "yes".

Every build runs in a fresh child process of its own (BPLTV_LIB_PATH), the builds alternating in rounds; a child times,
after a warm-up, `per` calls of each case on the faces_train_128_10 batch (10 x 128^2), 5000 iterations:
    denoise, sumregs_denoise, weighted_denoise   HIP-event time of the launch sequence (stats()["pdhg_ms"]) and wall time
    vjp_device                                   a short call, host overhead dominates (stats()["total_ms"] and wall time)
List the same build twice (a copy of the file under another name) to get the spread between two loads of one build: the
yardstick for the difference between two builds.  Results of the builds are compared by a checksum of u and grad_alpha.
usage: python tools/chain_driver_ab.py rounds per name=path/to/libbpltv.so [name=path ...]   (GPU box)"""
import ctypes as C
import json, os, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np


def child(per):
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
    w = 0.25 + 3.75 * np.random.default_rng(3).random((128, 128))
    a3 = np.array([0.03, 0.02, 0.05])
    u = s.denoise(0.1, maxiter=5000)
    d_u, d_a, d_gu = dev(u), dev(np.array([0.1])), dev(u - ub)
    d_gf, d_ga = dev(np.zeros_like(u)), dev(np.zeros(1))
    cases = {
        "denoise": lambda: s.denoise(0.1, fetch=False, maxiter=5000),
        "sumregs_denoise": lambda: s.sumregs_denoise(a3, fetch=False, maxiter=5000),
        "weighted_denoise": lambda: s.weighted_denoise(0.1, w, fetch=False, maxiter=5000),
        "vjp_device": lambda: s.vjp_device(d_u, d_a, 1, 1, d_gu, d_gf, d_ga),
    }
    out = {}
    for name, call in cases.items():
        for _ in range(3):
            call()
        ev, wall = [], []
        for _ in range(per):
            t0 = time.perf_counter()
            call()
            wall.append((time.perf_counter() - t0) * 1e3)
            st = s.stats()
            ev.append(st["total_ms"] if name == "vjp_device" else st["pdhg_ms"])
        out[name] = {"ev": ev, "wall": wall, "info": [st["launches"], st["launch_chains"], st["graph_used"]]}
    ga = np.empty(1)
    hip.hipMemcpy(ga.ctypes.data_as(C.c_void_p), C.c_void_p(d_ga), 8, 2)
    out["check"] = {"u_sum64": int(np.frombuffer(u.tobytes(), dtype=np.uint64).sum() & 0xFFFFFFFF), "grad_alpha": float(ga[0])}
    s.close()
    print("ABJSON " + json.dumps(out), flush=True)


def main():
    rounds, per = int(sys.argv[1]), int(sys.argv[2])
    builds = [a.split("=", 1) for a in sys.argv[3:]]
    acc, checks = {b: {} for b, _ in builds}, {}
    for r in range(rounds):
        for b, path in builds:
            pr = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(per)], cwd=ROOT, capture_output=True, text=True,
                                timeout=150, env=dict(os.environ, BPLTV_LIB_PATH=os.path.abspath(path)))
            if pr.returncode != 0:   # nothing more is started on the GPU after a failure
                sys.exit("child of build %s failed (%d):\n%s\n%s" % (b, pr.returncode, pr.stdout[-2000:], pr.stderr[-2000:]))
            d = json.loads([l for l in pr.stdout.splitlines() if l.startswith("ABJSON ")][-1][7:])
            checks.setdefault(b, d.pop("check"))
            for name, v in d.items():
                a = acc[b].setdefault(name, {"ev": [], "wall": [], "info": v["info"]})
                a["ev"] += v["ev"]
                a["wall"] += v["wall"]
    print("faces_train_128_10, 10 x 128^2, 5000 iterations; %d rounds x %d calls per build, a fresh process per build and round" % (rounds, per))
    print("event ms = stats()['pdhg_ms'] (vjp_device: stats()['total_ms']), wall ms = the call; median [min .. max]")
    print("%-17s %-8s %-31s %-31s %s" % ("case", "build", "event ms", "wall ms", "launches, chains, graph"))
    first = builds[0][0]
    for name in acc[first]:
        med = {}
        for b, _ in builds:
            e, w = np.array(acc[b][name]["ev"]), np.array(acc[b][name]["wall"])
            med[b] = (np.median(e), np.median(w))
            print("%-17s %-8s %8.3f [%8.3f .. %8.3f]  %8.3f [%8.3f .. %8.3f]  %s" % (name, b, med[b][0], e.min(), e.max(), med[b][1], w.min(), w.max(), acc[b][name]["info"]))
        print("%-17s medians against %s: %s" % (name, first, ", ".join("%s event %+.3f wall %+.3f ms" % (b, med[b][0] - med[first][0], med[b][1] - med[first][1]) for b, _ in builds[1:])))
    print("results per build (checksum of u, grad_alpha): %s; all equal: %s" % (json.dumps(checks), all(c == checks[first] for c in checks.values())), flush=True)


if __name__ == "__main__":
    child(int(sys.argv[2])) if sys.argv[1] == "--child" else main()
