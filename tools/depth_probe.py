#!/usr/bin/env python3
"""Developer probe: is the planner's fusion depth (plan_pdhg, csrc/tiling.hpp) still the fastest one?

For each batch the 5000-iteration denoise is timed (HIP events of the launch sequences, median of `reps` solves after
3 warm-ups) with the planner's own depth and with the depths around it; one line per batch.
usage: python tools/depth_probe.py [reps] [size=128] [images=1,2,5,6,7,8,9,10,12,16,32] [span=2]   (GPU box)"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from bpldenoising_amd import TVSolver
sys.path.insert(0, os.path.join(ROOT, "tests"))
from conftest import synth_batch

pos = [a for a in sys.argv[1:] if "=" not in a]
opt = dict(a.split("=") for a in sys.argv[1:] if "=" in a)
reps = int(pos[0]) if pos else 12
size = int(opt.get("size", 128))
span = int(opt.get("span", 2))
images = [int(v) for v in opt.get("images", "1,2,5,6,7,8,9,10,12,16,32").split(",")]


def timed(s, **kw):
    for _ in range(3):
        s.denoise(0.1, fetch=False, maxiter=5000, **kw)
    t = [0.0] * reps
    for k in range(reps):
        s.denoise(0.1, fetch=False, maxiter=5000, **kw)
        t[k] = s.stats()["pdhg_ms"]
    return float(np.median(t)), s.stats()


for O in images:
    ub, f = synth_batch(O, size, size, seed=1)
    s = TVSolver(size, size, O)
    s.set_data(ub, f)
    t0, st = timed(s)
    T0, v0 = st["tile_iters"], st["pdhg_variant"]
    line = "%2d x %d^2: plan variant %d T %d chains %d tiles %d: %.3f ms |" % (O, size, v0, T0, st["launch_chains"], st["tiles"], t0)
    for T in range(max(2, T0 - span), T0 + span + 1):
        if T == T0:
            continue
        t, st = timed(s, variant=v0, tile_iters=T)
        if st["tile_iters"] == T:
            line += " T %d: %.3f (%+.1f %%)" % (T, t, 100 * (t / t0 - 1))
    print(line, flush=True)
    s.close()
