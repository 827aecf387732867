#!/usr/bin/env python3
"""Developer probe: does another revision of bpldenoising_amd/torch_layer.py give the same bits at the same host cost as the one
in the tree?  Written for the fold of the sixteen autograd Functions into _forward / _backward / _jvp over one row per model
(DESIGN.md section 4.14), where the answer has to be "yes": the library is the same binary and gets the same calls
(tests/test_gpu_torch_layer_calls.py holds those).

The other revision is a file, e.g. `git show <commit>:bpldenoising_amd/torch_layer.py > /tmp/torch_layer_parent.py`; it is loaded
next to the tree's as a second module of the package, with library handles of its own.

bits: every model row of tests/test_gpu_torch_layer_calls.py (the two checkpointed ones included) at maxiter = 5 on 2 x 9 x 12 and
    2 x 17 x 33 (colour: 2 x 3 x ...), alpha once a scalar / vector and once a (2, 3) patch, w > 0: u, f.grad, alpha.grad, w.grad of
    a random linear loss and, where the model has one, the forward-mode tangent with a tangent on every input, compared between
    the two revisions with np.array_equal.  Any difference is a failure.
time: wall time of forward + backward (both gradients, synchronised) of tv_denoise and tv_denoise_unrolled, maxiter = 50, on
    10 x 128 x 128: 20 calls after 5 warm-up calls, for the other revision, a second load of the other revision (the yardstick:
    what two loads of one file differ by) and the tree's.  The tree's median has to lie inside the min ... max of the other
    revision's two runs.
usage: python tools/torch_layer_ab.py bits path/to/other_torch_layer.py
       python tools/torch_layer_ab.py time path/to/other_torch_layer.py                                    (GPU box)"""
import importlib.util
import os
import sys
import time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np
import torch
import torch.autograd.forward_ad as fwAD
from conftest import synth_batch

KW, CK = {"maxiter": 5}, {"maxiter": 5, "checkpoint_every": 2}
# row -> (function, alpha's leading shape with B = 2, solver keywords, the keyword that selects the forward-mode function or None: no jvp)
FM = {"forward_mode": True}
ROWS = {"tv": ("tv_denoise", (), KW, {}), "tv-each": ("tv_denoise_each", (2,), KW, {}),
        "sumregs": ("sumregs_denoise", (3,), KW, FM), "sumregs-each": ("sumregs_denoise_each", (2, 3), KW, FM),
        "weighted": ("tv_denoise_weighted", (), KW, None),
        "unrolled": ("tv_denoise_unrolled", (), KW, FM), "unrolled-ck": ("tv_denoise_unrolled", (), CK, FM),
        "unrolled-each": ("tv_denoise_unrolled_each", (2,), KW, FM),
        "weighted-unrolled": ("tv_denoise_weighted_unrolled", (), KW, FM),
        "weighted-unrolled-ck": ("tv_denoise_weighted_unrolled", (), CK, FM),
        "sumregs-unrolled": ("sumregs_denoise_unrolled", (3,), KW, None),
        "sumregs-unrolled-each": ("sumregs_denoise_unrolled_each", (2, 3), KW, None),
        "color-unrolled": ("tv_denoise_color_unrolled", (), KW, FM)}


def load(path, name):
    """The file at `path` as the module bpldenoising_amd.<name>: its relative imports resolve inside the package."""
    spec = importlib.util.spec_from_file_location("bpldenoising_amd." + name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = mod
    spec.loader.exec_module(mod)
    return mod


def inputs(row, lead, H, W, patch, seed):
    rng = np.random.default_rng(seed)
    shape = (2, 3, H, W) if row.startswith("color") else (2, H, W)
    arrays = [rng.random(shape), 0.05 + 0.05 * rng.random(lead + ((2, 3) if patch else ()))]
    if row.startswith("weighted"):
        arrays.append(0.5 + rng.random((2, H, W) if patch else (H, W)))
    return arrays + [rng.standard_normal(shape)] + [rng.standard_normal(a.shape) for a in arrays]   # gu, then the tangents


def outputs(layer, row, H, W, patch):
    """name -> array: u, the gradients of <gu, u> and the tangent of u."""
    fn_name, lead, kw, fm = ROWS[row]
    fn = getattr(layer, fn_name)
    arrays = [torch.tensor(a, dtype=torch.float64, device="cuda") for a in inputs(row, lead, H, W, patch, 31)]
    n = (len(arrays) - 1) // 2
    x, gu, dx = arrays[:n], arrays[n], arrays[n + 1:]
    leaves = [t.clone().requires_grad_(True) for t in x]
    u = fn(*leaves, **kw)
    (u * gu).sum().backward()
    out = {"u": u.detach()}
    out.update({"grad_" + k: t.grad for k, t in zip(("f", "alpha", "w"), leaves)})
    if fm is not None:
        with fwAD.dual_level():
            dual = fwAD.unpack_dual(fn(*[fwAD.make_dual(t, d) for t, d in zip(x, dx)], **fm, **kw))
            assert torch.equal(dual.primal, out["u"])
            out["tangent"] = dual.tangent.clone()
    return {k: v.cpu().numpy() for k, v in out.items()}


def main_bits(path):
    from bpldenoising_amd import torch_layer as new
    old = load(path, "torch_layer_other")
    bad = total = 0
    for H, W in ((9, 12), (17, 33)):
        for row in ROWS:
            for patch in (False, True):
                a, b = outputs(old, row, H, W, patch), outputs(new, row, H, W, patch)
                assert a.keys() == b.keys() and all(np.isfinite(v).all() and v.any() for v in b.values()), (row, list(b))
                diff = [k for k in a if not np.array_equal(a[k], b[k])]
                total += len(a)
                bad += len(diff)
                print("%-22s 2 x %2d x %2d %-6s %-44s %s" % (row, H, W, "patch" if patch else "scalar", " ".join(a),
                                                            "bitwise equal" if not diff else "DIFFER: " + " ".join(diff)))
    print("%d arrays compared between %s and the tree: %s" % (total, os.path.basename(path), "ALL BITWISE EQUAL" if bad == 0 else "%d DIFFER" % bad),
          flush=True)
    sys.exit(1 if bad else 0)


def timed(layer, calls=20, warm=5):
    """name -> wall ms per forward + backward, 10 x 128 x 128, maxiter = 50."""
    _, f = synth_batch(10, 128, 128, seed=3)
    ft = torch.tensor(f, device="cuda")
    out = {}
    for name in ("tv_denoise", "tv_denoise_unrolled"):
        fn, ms = getattr(layer, name), []
        for k in range(warm + calls):
            x, a = ft.clone().requires_grad_(True), torch.tensor(0.1, dtype=torch.float64, device="cuda", requires_grad=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn(x, a, maxiter=50).sum().backward()
            torch.cuda.synchronize()
            if k >= warm:
                ms.append((time.perf_counter() - t0) * 1e3)
        out[name] = np.array(ms)
    return out


def main_time(path):
    from bpldenoising_amd import torch_layer as new
    runs = [("other", timed(load(path, "torch_layer_other"))), ("other again", timed(load(path, "torch_layer_other2"))),
            ("tree", timed(new))]
    print("forward + backward, 10 x 128 x 128, maxiter = 50, 20 calls after 5 warm-up calls; wall ms: median [min .. max]")
    ok = True
    for name in runs[0][1]:
        for who, r in runs:
            print("%-20s %-12s %8.3f [%8.3f .. %8.3f]" % (name, who, np.median(r[name]), r[name].min(), r[name].max()))
        both = np.concatenate([runs[0][1][name], runs[1][1][name]])
        med, gap = np.median(runs[2][1][name]), abs(np.median(runs[0][1][name]) - np.median(runs[1][1][name]))
        inside = both.min() <= med <= both.max()
        ok &= bool(inside)
        print("%-20s the tree's median %.3f is %s the other revision's %.3f .. %.3f (its two medians differ by %.3f)"
              % (name, med, "inside" if inside else "OUTSIDE", both.min(), both.max(), gap), flush=True)
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    (main_bits if sys.argv[1] == "bits" else main_time)(sys.argv[2])
