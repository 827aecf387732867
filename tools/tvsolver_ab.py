#!/usr/bin/env python3
"""Developer probe: does another revision of bpldenoising_amd/learning_function.py give the same bits at the same host cost as the
one in the tree?  Written for the fold of TVSolver's method bodies into cores over one row per model, where
the answer has to be "yes": the library is the same binary and gets the same calls (tests/test_tvsolver_calls.py holds those).

The other revision is a file, e.g. `git show <commit>:bpldenoising_amd/learning_function.py > /tmp/learning_function_parent.py`; it
is loaded next to the tree's as a second module of the package (tools/torch_layer_ab.py's way), over the same libbpltv.so.

bits: one handle per revision on the same 2 x 32 x 40 batch, maxiter = 5; every model's solve, every vjp (implicit and over the tape,
    one of them checkpointed), every jvp, every gauss_newton, the two evaluates, the tape sizes and a device-pointer solve and
    sweep; every returned array and number compared between the two revisions with np.array_equal.  Any difference is a failure.
time: wall time around one denoise_device and one weighted_unrolled_vjp_device call on that batch (the cheapest calls: an extra
    Python frame shows most), median of 300 calls after 30, in three child processes per file, alternating.  The tree's medians are
    set against the min ... max of the other revision's three; one above that range is reported with its size.  No threshold.
usage: python tools/tvsolver_ab.py bits path/to/other_learning_function.py
       python tools/tvsolver_ab.py time path/to/other_learning_function.py                                (GPU box)"""
import importlib.util
import json
import os
import subprocess
import sys
import time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

O, N, M, KW = 2, 32, 40, {"maxiter": 5}


def load(path):
    """The file at `path` as the module bpldenoising_amd.learning_function_other: its relative imports resolve inside the package."""
    spec = importlib.util.spec_from_file_location("bpldenoising_amd.learning_function_other", path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = mod
    spec.loader.exec_module(mod)
    return mod


def data():
    rng = np.random.default_rng(5)
    d = {"f": rng.random((O, N, M)), "gu": rng.standard_normal((O, N, M)), "ubar": rng.random((O, N, M)),
         "df": rng.standard_normal((O, N, M)), "w": 0.5 + rng.random((N, M)), "w3": 0.5 + rng.random((O, N, M)),
         "tv": 0.1, "patch": 0.05 + 0.05 * rng.random((2, 3)), "sr": 0.03 + 0.02 * rng.random(3),
         "each": 0.05 + 0.05 * rng.random(O), "sr_each": 0.03 + 0.02 * rng.random((O, 3, 2, 3))}
    d["dw"] = rng.standard_normal((N, M))
    return d


def results(lf):
    """name -> what the method returned, for one representative call per core and model."""
    import torch
    d = data()
    s = lf.TVSolver(M, N, O)
    s.set_data(d["ubar"], d["f"])
    out = {}
    x = {"": d["patch"], "each": d["each"], "sumregs": d["sr"], "sumregs_each": d["sr_each"]}
    # solves: every row
    for name, args in (("denoise", (x[""],)), ("denoise_each", (x["each"],)), ("sumregs_denoise", (x["sumregs"],)),
                       ("sumregs_denoise_each", (x["sumregs_each"],)), ("weighted_denoise", (d["tv"], d["w3"])),
                       ("l1_denoise", (4.0 * x[""], d["w"])), ("kl_denoise", (x[""], d["w"])), ("color_denoise", (x[""], 2)),
                       ("color_weighted_denoise", (d["tv"], 2, d["w3"]))):
        out[name] = getattr(s, name)(*args, **KW)
    out["evaluate"] = s.evaluate(x[""], 1e-4, **KW)
    out["sumregs_evaluate"] = s.sumregs_evaluate(x["sumregs"], 1e-4, **KW)
    # implicit reverse and forward mode
    for pre, key in (("", ""), ("sumregs_", "sumregs")):
        for e in ("", "_each"):
            p = x[(key + e).lstrip("_")]
            u = out[pre + "denoise" + e]
            out[pre + "vjp" + e] = getattr(s, pre + "vjp" + e)(u, p, d["gu"], **KW)
            out[pre + "jvp" + e] = getattr(s, pre + "jvp" + e)(u, p, df=d["df"], **({"dalpha": 0.5 * p} if not e else {"dalphas": 0.5 * p}), **KW)
        out[pre + "gauss_newton"] = getattr(s, pre + "gauss_newton")(out[pre + "denoise"], d["ubar"], x[key] if key else d["tv"], **KW)
    out["weighted_vjp"] = s.weighted_vjp(out["weighted_denoise"], d["f"], d["tv"], d["w3"], d["gu"], **KW)
    # through the iterations: solve, sweep over the tape, tangent sweep, Gauss-Newton
    for pre, first, w, ck in (("", (x[""],), (), {}), ("weighted_", (x[""], d["w"]), (), {"checkpoint_every": 2}), ("l1_", (4.0 * x[""], d["w3"]), (), {}),
                              ("kl_", (d["tv"], d["w"]), (), {}), ("color_", (x[""], 2), (), {}), ("color_weighted_", (x[""], 2, d["w"]), (), {}),
                              ("sumregs_", (x["sumregs"],), (), {"checkpoint_every": -1})):
        out[pre + "unrolled_denoise"] = getattr(s, pre + "unrolled_denoise")(*first, **KW, **ck)
        out[pre + "unrolled_vjp"] = getattr(s, pre + "unrolled_vjp")(*first, d["gu"], **KW, **ck)
        if pre not in ("sumregs_", "color_weighted_"):
            dw = {"dw": d["dw"]} if pre in ("weighted_", "kl_") else {}
            out[pre + "unrolled_jvp"] = getattr(s, pre + "unrolled_jvp")(*first, df=d["df"], dalpha=0.5 * np.asarray(first[0]), want_u=True, **dw, **KW)
            out[pre + "unrolled_gauss_newton"] = getattr(s, pre + "unrolled_gauss_newton")(*first, **KW)
    for pre, p in (("", x["each"]), ("sumregs_", x["sumregs_each"])):
        out[pre + "unrolled_denoise_each"] = getattr(s, pre + "unrolled_denoise_each")(p, **KW)
        out[pre + "unrolled_vjp_each"] = getattr(s, pre + "unrolled_vjp_each")(p, d["gu"], **KW)
    out["unrolled_jvp_each"] = s.unrolled_jvp_each(x["each"], dalphas=x["each"], **KW)
    for name in ("unrolled_tape_doubles", "weighted_unrolled_tape_doubles", "sumregs_unrolled_tape_doubles"):
        out[name] = (getattr(s, name)(**KW), getattr(s, name)(checkpoint_every=2, **KW))
    # device pointers
    t = {k: torch.tensor(np.asarray(v, dtype=np.float64), device="cuda") for k, v in d.items()}
    gf, ga, gw, u = torch.zeros_like(t["f"]), torch.zeros(6, dtype=torch.float64, device="cuda"), torch.zeros_like(t["w"]), torch.zeros_like(t["f"])
    torch.cuda.synchronize()
    s.denoise_device(t["patch"].data_ptr(), 3, 2, **KW)
    s.copy_u_device(u.data_ptr())
    torch.cuda.synchronize()
    out["denoise_device"] = u.cpu().numpy()
    s.weighted_unrolled_denoise_device(t["w"].data_ptr(), 1, t["patch"].data_ptr(), 3, 2, **KW)
    s.weighted_unrolled_vjp_device(None, t["w"].data_ptr(), 1, t["patch"].data_ptr(), 3, 2, t["gu"].data_ptr(), gf.data_ptr(), ga.data_ptr(),
                                   gw.data_ptr(), **KW)
    torch.cuda.synchronize()
    out["weighted_unrolled_vjp_device"] = (gf.cpu().numpy(), ga.cpu().numpy(), gw.cpu().numpy())
    s.close()
    return out


def flat(v):
    if isinstance(v, (tuple, list)):
        return [a for x in v for a in flat(x)]
    return [np.asarray(v)]


def main_bits(path):
    from bpldenoising_amd import learning_function as new
    a, b = results(load(path)), results(new)
    assert a.keys() == b.keys()
    bad = total = 0
    for k in a:
        fa, fb = flat(a[k]), flat(b[k])
        same = len(fa) == len(fb) and all(x.shape == y.shape and x.dtype == y.dtype and np.array_equal(x, y) for x, y in zip(fa, fb))
        live = all(np.isfinite(y).all() and y.any() for y in fb)
        total += len(fb)
        bad += not same
        print("%-36s %2d arrays %s%s" % (k, len(fb), "bitwise equal" if same else "DIFFER", "" if live else " (all zero or not finite: look)"))
    print("%d arrays of %d calls compared between %s and the tree: %s" % (total, len(a), os.path.basename(path),
                                                                       "ALL BITWISE EQUAL" if bad == 0 else "%d CALLS DIFFER" % bad), flush=True)
    sys.exit(1 if bad else 0)


def child(path, calls=300, warm=30):
    """One process: {name: median wall microseconds of one call} with the module at `path` ("tree": the package's own)."""
    import torch
    if path == "tree":
        from bpldenoising_amd import learning_function as lf
    else:
        lf = load(path)
    d = data()
    s = lf.TVSolver(M, N, O)
    s.set_data(d["ubar"], d["f"])
    t = {k: torch.tensor(np.asarray(v, dtype=np.float64), device="cuda") for k, v in d.items()}
    gf, ga, gw = torch.zeros_like(t["f"]), torch.zeros(1, dtype=torch.float64, device="cuda"), torch.zeros_like(t["w"])
    a = torch.tensor([0.1], dtype=torch.float64, device="cuda")
    ptr = {k: v.data_ptr() for k, v in t.items()}
    s.weighted_unrolled_denoise_device(ptr["w"], 1, a.data_ptr(), 1, 1, **KW)
    runs = {"weighted_unrolled_vjp_device": lambda: s.weighted_unrolled_vjp_device(None, ptr["w"], 1, a.data_ptr(), 1, 1, ptr["gu"], gf.data_ptr(),
                                                                                     ga.data_ptr(), gw.data_ptr(), **KW),
            "denoise_device": lambda: s.denoise_device(a.data_ptr(), 1, 1, **KW)}
    out = {}
    for name, fn in runs.items():
        us = []
        for k in range(warm + calls):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            t1 = time.perf_counter()
            if k >= warm:
                us.append((t1 - t0) * 1e6)
        out[name] = float(np.median(us))
    s.close()
    print(json.dumps(out), flush=True)


def main_time(path):
    runs = {"other": [], "tree": []}
    for k in range(3):
        for who, arg in (("other", path), ("tree", "tree")):
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "child", arg], capture_output=True, text=True, timeout=240)
            if r.returncode != 0:
                print(r.stdout, r.stderr)
                sys.exit("the %s child failed with status %d: stopping" % (who, r.returncode))
            runs[who].append(json.loads(r.stdout.strip().splitlines()[-1]))
            print("process %d %-5s %s" % (k, who, r.stdout.strip().splitlines()[-1]), flush=True)
    print("wall microseconds of one call, 2 x 32 x 40, maxiter = 5: median of 300 calls per process, three processes per file")
    for name in runs["tree"][0]:
        other, tree = [r[name] for r in runs["other"]], [r[name] for r in runs["tree"]]
        print("%-30s other %s   tree %s" % (name, " ".join("%8.2f" % v for v in other), " ".join("%8.2f" % v for v in tree)))
        for v in tree:
            where = "inside" if min(other) <= v <= max(other) else ("BELOW by %.2f us" % (min(other) - v) if v < min(other) else
                                                                     "ABOVE by %.2f us (%.1f %%)" % (v - max(other), 100 * (v - max(other)) / max(other)))
            print("%-30s the tree's median %8.2f is %s the other revision's %.2f .. %.2f" % (name, v, where, min(other), max(other)), flush=True)


if __name__ == "__main__":
    {"bits": main_bits, "time": main_time, "child": child}[sys.argv[1]](sys.argv[2])
