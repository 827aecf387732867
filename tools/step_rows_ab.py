#!/usr/bin/env python3
"""Developer probe: what do the scalar-memory waits of the 32x32 / 1 px PDHG kernel cost, and what does taking the
launch's step rows from LDS get back?

The headline solve (10 x 128^2 faces, scalar alpha, 5000 iterations) timed by the HIP events of the launch sequences,
with one and with two launch chains, the forms alternating in rounds inside one process (params.reserved[3]):
    lds      the launch's rows copied to LDS with the state loads, every iteration reads its row there (the product, 0)
    sload    rows by scalar loads: first row behind the first barrier, next row inside the loop (8192: the kernel as it was)
    noloop   as sload, but the loop keeps the first row and fetches nothing (8192 + 16384; WRONG results)
    const    as sload, but the first row comes from the kernel arguments (8192 + 32768; WRONG results)
    none     both (WRONG results): sload - none bounds what the two fetches can cost
lds and sload give the same bits (checked here).  Needs the EXPERIMENTS build of the library:
    python -c "import __graft_entry__ as g; g.build_experiments()"     # -> tools/_bin/libbpltv_exp.so
usage: python tools/step_rows_ab.py [rounds [steps_per_round]] [tile_iters=T] [images=O]   (GPU box)"""
import ctypes as C
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
os.environ.setdefault("BPLTV_LIB_PATH", os.path.join(ROOT, "tools", "_bin", "libbpltv_exp.so"))
sys.path.insert(0, ROOT)
import numpy as np
import bench
from bpldenoising_amd import TVSolver

pos = [a for a in sys.argv[1:] if "=" not in a]
opt = dict(a.split("=") for a in sys.argv[1:] if "=" in a)
rounds = int(pos[0]) if len(pos) > 0 else 10
per = int(pos[1]) if len(pos) > 1 else 10
images = int(opt.get("images", 10))
kw = {"maxiter": 5000}
if "tile_iters" in opt:
    kw["tile_iters"] = int(opt["tile_iters"])
ub, f, _ = bench.load_batch("faces_train_128_10", images, 128, 128, 20211004)
s = TVSolver(128, 128, images)
s.set_data(ub, f)
a = np.array([0.1])
FORMS = (("lds", 0), ("sload", 8192), ("noloop", 8192 + 16384), ("const", 8192 + 32768), ("none", 8192 + 16384 + 32768))


def run(dbg, chains, out=None):
    p = s.params(chains=chains, **kw)
    p.reserved[3] = dbg
    s._check(s._lib.bpltv_denoise(s._h, a.ctypes.data_as(C.POINTER(C.c_double)), 1, 1, C.byref(p),
                                  out.ctypes.data_as(C.POINTER(C.c_double)) if out is not None else None))
    return s.stats()


for chains in (1, 2) if images > 1 else (1,):
    us = {}
    for name, dbg in FORMS:
        u = np.empty((images, 128, 128))
        st = run(dbg, chains, u)
        us[name] = u
        for _ in range(3):
            run(dbg, chains)
    assert np.array_equal(us["lds"], us["sload"]), "rows from LDS and rows by scalar loads differ"
    ev = {name: [] for name, _ in FORMS}
    for r in range(rounds):
        for name, dbg in FORMS:
            for _ in range(per):
                ev[name].append(run(dbg, chains)["pdhg_ms"])
    for name, _ in FORMS:
        e = np.array(ev[name])
        print("chains %d T %d launches %d %-6s: event ms min %.3f median %.3f mean %.3f max %.3f; slow steps (> 1.1 x min) %d of %d; %.3e it/s at the median"
              % (chains, st["tile_iters"], st["launches"], name, e.min(), np.median(e), e.mean(), e.max(), (e > 1.1 * e.min()).sum(), e.size,
                 kw["maxiter"] / np.median(e) * 1e3), flush=True)
