#!/usr/bin/env python3
"""Developer probe: what do the branch-free 32-bit prologue (the FAST instantiation of pdhg_tile_kernel) and the peeled
last iteration of a launch buy on the headline solve ("One argument round trip")?

The headline solve (10 x 128^2 faces, scalar alpha, 5000 iterations) timed by the HIP events of the launch sequences,
with one and with two launch chains, the forms alternating in rounds inside one process (params.reserved[3]):
    product  FAST instantiation, last iteration peeled (0)
    general  the general instantiation where FAST would run: sweep / rho / patch branches, 64-bit indices (262144)
    tail     FAST, but the last iteration of a launch writes y to LDS and passes barrier #2 as before (524288)
    both     general and the old tail
All four give the same bits (checked here).  The one argument round trip and the host's launch-invariant words are in
every form: what they buy shows only against the parent commit's library (the A/B of the product libraries).  Needs the
EXPERIMENTS build of the library.  It misstates effects: its switches cost registers and branches, and the run-time
switch of the tail keeps both forms of the tail in one kernel -- this probe saw nothing of the peeled tail (0.00-0.01 ms)
where product libraries built with and without it differ by 0.3 ms.
    python -c "import __graft_entry__ as g; g.build_experiments()"     # -> tools/_bin/libbpltv_exp.so
usage: python tools/prologue_ab.py [rounds [steps_per_round]] [tile_iters=T] [images=O]   (GPU box)"""
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
FORMS = (("product", 0), ("general", 262144), ("tail", 524288), ("both", 262144 + 524288))


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
    for name, _ in FORMS:
        assert np.array_equal(us["product"], us[name]), "the forms differ: product / " + name
    ev = {name: [] for name, _ in FORMS}
    for r in range(rounds):
        for name, dbg in FORMS:
            for _ in range(per):
                ev[name].append(run(dbg, chains)["pdhg_ms"])
    for name, _ in FORMS:
        e = np.array(ev[name])
        print("chains %d T %d launches %d %-7s: event ms min %.3f median %.3f mean %.3f max %.3f; slow steps (> 1.1 x min) %d of %d; %.3e it/s at the median"
              % (chains, st["tile_iters"], st["launches"], name, e.min(), np.median(e), e.mean(), e.max(), (e > 1.1 * e.min()).sum(), e.size,
                 kw["maxiter"] / np.median(e) * 1e3), flush=True)
