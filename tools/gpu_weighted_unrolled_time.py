#!/usr/bin/env python3
"""Developer probe: what the weighted tape costs the solve, and the weighted reverse sweep against the unweighted one.

    python tools/gpu_weighted_unrolled_time.py [--reps 7] [--iters 50 5000] [--out DIR]

10 x 128^2, scalar alpha, one MI355X.  Per iteration count and per weight (a real weight in [0.25, 4], one plane per image;
a mask, one plane with about 30 % zeros), after a warm-up of every call (graphs built, workspaces allocated), `reps` rounds
in which ONE handle runs in alternation:
    bpltv_weighted_denoise_device                                  -> stats.pdhg_ms
    bpltv_unrolled_denoise_device (a caller's tape)                -> stats.pdhg_ms
    bpltv_weighted_unrolled_denoise_device (a caller's tape)       -> stats.pdhg_ms
    bpltv_unrolled_vjp_device on its tape                          -> stats.adjoint_ms (HIP events around the sweep)
    bpltv_weighted_unrolled_vjp_device, grad_f and grad_alpha      -> stats.adjoint_ms
    bpltv_weighted_unrolled_vjp_device, grad_w as well             -> stats.adjoint_ms
HIP-event medians with min / max, the ratios, the tape sizes, and whether u is bitwise the weighted solve's; one JSON line
per case, all of them collected in DIR/weighted_unrolled_time.json.  A count whose tapes do not fit is skipped."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def _stats(xs):
    import numpy as np
    xs = np.asarray(xs, dtype=float)
    return {"median": float(np.median(xs)), "min": float(xs.min()), "max": float(xs.max()), "n": int(xs.size)}


def time_case(K, wkind, reps, O=10, n=128, alpha=0.08):
    import numpy as np
    import torch
    from conftest import synth_batch
    from bpldenoising_amd import TVSolver
    ub, f = synth_batch(O, n, n, seed=5)
    if wkind == "real":
        w, wo = 0.25 + 3.75 * np.random.default_rng(11).random((O, n, n)), O
    else:
        w, wo = (np.random.default_rng(12).random((n, n)) > 0.3).astype(np.float64), 1
    dev = torch.device("cuda", 0)
    tf, tub, tw_ = torch.from_numpy(f).to(dev), torch.from_numpy(ub).to(dev), torch.from_numpy(w).to(dev)
    ta = torch.tensor([alpha], dtype=torch.float64, device=dev)
    s = TVSolver(n, n, O, device=0)
    s.set_data_device(tub.data_ptr(), tf.data_ptr())
    free = torch.cuda.mem_get_info(dev)[0]
    need = 8 * (s.unrolled_tape_doubles(maxiter=K) + s.weighted_unrolled_tape_doubles(maxiter=K))
    if need > 0.8 * free:
        s.close()
        return {"case": "%dx%dx%d scalar, %s" % (O, n, n, wkind), "maxiter": K, "skipped": "tapes of %.1f GB do not fit" % (need / 1e9)}
    tape = torch.empty(s.unrolled_tape_doubles(maxiter=K), dtype=torch.float64, device=dev)
    wtape = torch.empty(s.weighted_unrolled_tape_doubles(maxiter=K), dtype=torch.float64, device=dev)
    u0, u1 = torch.empty_like(tf), torch.empty_like(tf)
    gf, gw = torch.empty_like(tf), torch.empty_like(tw_)
    ga = torch.empty(1, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    rows = {k: [] for k in ("weighted_pdhg_ms", "unrolled_pdhg_ms", "weighted_unrolled_pdhg_ms", "unrolled_vjp_ms",
                            "weighted_unrolled_vjp_ms", "weighted_unrolled_vjp_with_grad_w_ms")}
    plan = None
    for r in range(reps + 1):          # round 0 is the warm-up
        t = []
        s.weighted_denoise_device(tw_.data_ptr(), wo, ta.data_ptr(), 1, 1, maxiter=K)
        t.append(s.stats()["pdhg_ms"])
        s.copy_u_device(u0.data_ptr())
        s.unrolled_denoise_device(ta.data_ptr(), 1, 1, tape_ptr=tape.data_ptr(), maxiter=K)
        t.append(s.stats()["pdhg_ms"])
        s.weighted_unrolled_denoise_device(tw_.data_ptr(), wo, ta.data_ptr(), 1, 1, tape_ptr=wtape.data_ptr(), maxiter=K)
        st = s.stats()
        t.append(st["pdhg_ms"])
        plan = {k: st[k] for k in ("tile_iters", "tiles", "launches", "launch_chains", "graph_used", "bytes_per_px_iter")}
        s.copy_u_device(u1.data_ptr())
        gu = u1 - tub
        torch.cuda.synchronize()
        s.unrolled_vjp_device(tape.data_ptr(), ta.data_ptr(), 1, 1, gu.data_ptr(), gf.data_ptr(), ga.data_ptr(), maxiter=K)
        t.append(s.stats()["adjoint_ms"])
        s.weighted_unrolled_vjp_device(wtape.data_ptr(), tw_.data_ptr(), wo, ta.data_ptr(), 1, 1, gu.data_ptr(), gf.data_ptr(),
                                       ga.data_ptr(), None, maxiter=K)
        t.append(s.stats()["adjoint_ms"])
        s.weighted_unrolled_vjp_device(wtape.data_ptr(), tw_.data_ptr(), wo, ta.data_ptr(), 1, 1, gu.data_ptr(), gf.data_ptr(),
                                       ga.data_ptr(), gw.data_ptr(), maxiter=K)
        t.append(s.stats()["adjoint_ms"])
        if r:
            for k, v in zip(rows, t):
                rows[k].append(v)
    out = {"case": "%dx%dx%d scalar, %s" % (O, n, n, wkind), "maxiter": K, "tape_MB": tape.numel() * 8 / 1e6,
           "weighted_tape_MB": wtape.numel() * 8 / 1e6, "u_bitwise_equal": bool(torch.equal(u0, u1)), "plan": plan,
           "grad_alpha": float(ga[0]), "grad_w_finite": bool(torch.isfinite(gw).all())}
    out.update({k: _stats(v) for k, v in rows.items()})
    med = lambda k: out[k]["median"]
    out["ratios"] = {"solve / weighted solve (traffic 88/64 = 1.375)": med("weighted_unrolled_pdhg_ms") / med("weighted_pdhg_ms"),
                     "solve / unrolled solve (traffic 88/72 = 1.222)": med("weighted_unrolled_pdhg_ms") / med("unrolled_pdhg_ms"),
                     "vjp with grad_w / unrolled vjp (tape 24/16 = 1.5)": med("weighted_unrolled_vjp_with_grad_w_ms") / med("unrolled_vjp_ms"),
                     "vjp without grad_w / unrolled vjp (tape 16/16)": med("weighted_unrolled_vjp_ms") / med("unrolled_vjp_ms")}
    s.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, nargs="+", default=[50, 5000])
    ap.add_argument("--out", default=os.path.join(ROOT, "results"))
    a = ap.parse_args()
    res = []
    for K in a.iters:
        for wkind in ("real", "mask"):
            res.append(time_case(K, wkind, a.reps))
            print(json.dumps(res[-1]), flush=True)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "weighted_unrolled_time.json"), "w") as fh:
        json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
