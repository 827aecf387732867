"""TV-L1 denoising on a machine without a GPU: the library exports the six bpltv_lone_* functions with
the header's argument lists, the binding covers them, TVSolver and the torch layer have the entries, the layer rejects wrong
inputs before it touches the library, and the numpy twin the GPU tests compare against (tests/l1_ref.py) is pinned: its reverse
sweep agrees with torch autograd and with central differences of its forward, it removes isolated spikes exactly, and every GPU
case keeps its decisions -- the projection's and the threshold's -- away from a tie while taking both branches."""
import ctypes as C
import os
import re

import numpy as np
import pytest
from conftest import ROOT

import l1_ref as lr
from oracle import np_twin as tw

NAMES = {"bpltv_lone_denoise": 8, "bpltv_lone_denoise_device": 7, "bpltv_lone_unrolled_denoise": 8, "bpltv_lone_unrolled_denoise_device": 8,
         "bpltv_lone_unrolled_vjp": 11, "bpltv_lone_unrolled_vjp_device": 12}


def _header_text():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bpltv.h")).read(), flags=re.S)


def _header_args(name):
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name, _header_text())
    assert m, name
    return [" ".join(a.split()) for a in m.group(1).split(",")]


@pytest.mark.parametrize("name", sorted(NAMES))
def test_library_exports_and_binds_the_l1_functions(name):
    from bpldenoising_amd import _lib
    lib = _lib.load()
    assert hasattr(lib, name)
    res, args = _lib.SYMBOLS[name]
    assert res is C.c_int
    hdr = _header_args(name)
    assert len(args) == len(hdr) == NAMES[name]
    assert getattr(lib, name).argtypes == args
    for a, decl in zip(args, hdr):
        if decl.startswith("bpltv_t *"):
            assert a is C.c_void_p
        elif decl.startswith("const bpltv_params *"):
            assert a is _lib._PP
        elif decl.startswith("int "):
            assert a is C.c_int
        else:   # arrays: host forms take POINTER(c_double), device forms raw addresses
            assert "double *" in decl, decl
            assert a is (C.c_void_p if name.endswith("_device") else C.POINTER(C.c_double)), (decl, a)


def test_signatures_are_the_weighted_twins():
    """Argument for argument bpltv_weighted_*'s, in the header and in the binding."""
    from bpldenoising_amd import _lib
    for name in NAMES:
        twin = name.replace("bpltv_lone_", "bpltv_weighted_")
        assert _header_args(name) == _header_args(twin), name
        assert _lib.SYMBOLS[name] == _lib.SYMBOLS[twin], name


def test_binding_covers_the_header_and_names_the_sweep():
    from bpldenoising_amd import _lib
    declared = set(re.findall(r"\b(bpltv_\w+)\s*\(", _header_text()))
    assert set(NAMES) <= declared
    assert declared == set(_lib.SYMBOLS), declared ^ set(_lib.SYMBOLS)
    hdr = open(os.path.join(ROOT, "include", "bpltv.h")).read()
    assert "15 reverse sweep over the taped TV-L1 iterations" in hdr
    st = _lib.BpltvStats()
    st.adjoint_method = 15
    assert st.as_dict()["adjoint_method"] == "l1-unrolled"


def test_solver_and_layer_have_the_entries():
    pytest.importorskip("torch")
    from bpldenoising_amd import TVSolver, torch_layer
    for m in ("l1_denoise", "l1_denoise_device", "l1_unrolled_denoise", "l1_unrolled_denoise_device", "l1_unrolled_vjp",
              "l1_unrolled_vjp_device"):
        assert callable(getattr(TVSolver, m))
    assert callable(torch_layer.tv_l1_denoise_unrolled)
    import torch
    assert issubclass(torch_layer.TVL1DenoiseUnrolledFunction, torch.autograd.Function)
    row = torch_layer._L1_UNROLLED
    assert row.w and row.w_zeros and row.reads_f and row.jvp is None and not row.channels
    assert row.tape == "weighted_unrolled_tape_doubles"
    m = torch_layer.TVL1DenoiseUnrolled(0.7, np.ones((4, 5)), maxiter=7)
    assert [n for n, _ in m.named_parameters()] == ["alpha"] and [n for n, _ in m.named_buffers()] == ["w"]
    m = torch_layer.TVL1DenoiseUnrolled(0.7, np.ones((4, 5)), maxiter=7, learn_w=True)
    assert sorted(n for n, _ in m.named_parameters()) == ["alpha", "w"] and m.w.dtype == torch.float64 and m.maxiter == 7


@pytest.fixture
def layer(monkeypatch):
    """torch_layer with every library entry refused: a rejection must come before any library call."""
    pytest.importorskip("torch")
    from bpldenoising_amd import torch_layer

    def no_library(*a, **k):
        raise AssertionError("the library was called")
    monkeypatch.setattr(torch_layer, "_solver", no_library)
    monkeypatch.setattr(torch_layer, "_sync", no_library)
    return torch_layer


def test_the_layer_rejects_before_any_library_call(layer):
    """tests/test_weighted_unrolled_abi.py's rejections of tv_denoise_weighted_unrolled, for tv_l1_denoise_unrolled."""
    import torch
    f = torch.zeros(2, 8, 6, dtype=torch.float64)
    a = torch.tensor(0.7, dtype=torch.float64)
    w = torch.ones(8, 6, dtype=torch.float64)
    fn = layer.tv_l1_denoise_unrolled
    with pytest.raises(TypeError, match="torch tensors"):
        fn(np.zeros((2, 8, 6)), a, w, maxiter=5)
    with pytest.raises(TypeError, match="float64"):
        fn(f.float(), a, w, maxiter=5)
    with pytest.raises(TypeError, match="float64"):
        fn(f, a.float(), w, maxiter=5)
    with pytest.raises(TypeError, match="tv_l1_denoise_unrolled: w must be a torch tensor"):
        fn(f, a, np.ones((8, 6)), maxiter=5)
    with pytest.raises(TypeError, match="tv_l1_denoise_unrolled: w must be float64"):
        fn(f, a, w.float(), maxiter=5)
    with pytest.raises(ValueError, match="f must have shape"):   # a colour batch
        fn(torch.zeros(2, 3, 8, 6, dtype=torch.float64), a, w, maxiter=5)
    for bad in (torch.ones(6, 8, dtype=torch.float64), torch.ones(3, 8, 6, dtype=torch.float64),
                torch.ones(1, 8, 6, dtype=torch.float64), torch.ones(2, 1, 8, 6, dtype=torch.float64)):
        with pytest.raises(ValueError, match="tv_l1_denoise_unrolled: w must have shape"):
            fn(f, a, bad, maxiter=5)
    neg, nan, inf = w.clone(), w.clone(), torch.ones(2, 8, 6, dtype=torch.float64)
    neg[3, 2] = -1e-300
    nan[0, 0] = float("nan")
    inf[1, 7, 5] = -float("inf")
    for bad in (neg, nan, inf):
        with pytest.raises(ValueError, match="tv_l1_denoise_unrolled: w must be finite and >= 0"):
            fn(f, a, bad, maxiter=5)
    for bad in (torch.zeros(2, dtype=torch.float64), torch.zeros(9, 6, dtype=torch.float64), torch.zeros(2, 8, 6, dtype=torch.float64)):
        with pytest.raises(ValueError, match="alpha must be"):
            fn(f, bad, w, maxiter=5)
    with pytest.raises(ValueError, match="w is on"):
        fn(f, a, w.to("meta"), maxiter=5)
    with pytest.raises(ValueError, match="tv_l1_denoise_unrolled: forward mode through the TV-L1 iterations does not exist"):
        fn(f, a, w, maxiter=5, forward_mode=True)
    for good in (w, torch.zeros(8, 6, dtype=torch.float64), torch.ones(2, 8, 6, dtype=torch.float64)):   # everything valid, on the CPU
        with pytest.raises(ValueError, match="ROCm device"):
            fn(f, a, good, maxiter=5, checkpoint_every=2)
    with pytest.raises(ValueError, match="ROCm device"):
        fn(f[0], a, w)
    with pytest.raises(ValueError, match="ROCm device"):
        layer.TVL1DenoiseUnrolled(0.7, np.ones((8, 6)), maxiter=5, learn_w=True)(f)


# ---- the twin -------------------------------------------------------------------------------------------------------
def _case(name, kind, wkind):
    O, N, M = lr.GPU_SHAPES[name]
    f, gu = lr.gpu_data(name)
    return f, gu, tw.alpha_to_map(lr.alpha_of(kind, N, M), M, N), lr.weight_of(wkind, O, N, M)


def test_the_step_table_has_no_acceleration_in_it():
    """gamma = 0: omega = 1, constant steps, and accel 0 and 1 give the same table and the same bits."""
    for K in (1, 7, 50):
        a, b = lr.step_table(K, accel=True), lr.step_table(K, accel=False)
        assert np.array_equal(a, b) and (a[:, 2] == 1.0).all() and (a == a[0]).all()
    f, gu, amap, w = _case("2x17x33", "map", "real")
    assert np.array_equal(lr.fwd_tape(f, amap, w, 20, accel=True)[1], lr.fwd_tape(f, amap, w, 20, accel=False)[1])


@pytest.mark.parametrize("K", lr.GRADIENT_K)
@pytest.mark.parametrize("wkind", lr.WEIGHTS)
@pytest.mark.parametrize("name", lr.GRADIENT_SHAPES)
def test_twin_reverse_agrees_with_torch_autograd(name, wkind, K):
    """1e-11 * max|ref| on grad_f, on the per-pixel parameter terms summed over the images and on grad_w, for a scalar, a patch
    and a map (measured: at most 5.8e-13 relative)."""
    pytest.importorskip("torch")
    O, N, M = lr.GPU_SHAPES[name]
    for kind in lr.KINDS:
        f, gu, amap, w = _case(name, kind, wkind)
        _, gf, ga, gw, _ = lr.twin_case(name, kind, wkind, K)
        gf0, ga0, gw0 = lr.torch_reference(f, amap, w, K, gu)
        gas = np.zeros((N, M))
        for k in range(O):
            gas = gas + ga[k]
        for what, g, g0 in (("grad_f", gf, gf0), ("ga", gas, ga0), ("grad_w", lr.reduce_w(gw, w), gw0)):
            d, ref = float(np.abs(g - g0).max()), float(np.abs(g0).max())
            print("%s %s %s K %d: %s %.2e (max|ref| %.2e, rel %.2e)" % (name, kind, wkind, K, what, d, ref, d / ref if ref else 0.0))
            assert g.shape == g0.shape and d <= 1e-11 * ref


def test_twin_gradient_against_central_differences():
    """0.5 |u_K - ubar|^2 on 1 x 24 x 28, K = 30, alpha = 0.7: the reverse sweep against central differences of the twin forward,
    h = 1e-6, relative 1e-5, along alpha, along a random direction of f and along a random direction of w on the kept pixels."""
    ub, f, w, df, dw = lr.central_difference_case()
    N, M, K, alpha, h = 24, 28, lr.CD_K, lr.CD_ALPHA, lr.CD_H
    assert w.min() == 0.0 and 0.2 < 1.0 - w.mean() < 0.4
    amap = tw.alpha_to_map(alpha, M, N)
    u, tape, tab = lr.fwd_tape(f, amap, w, K)
    gf, ga, gw = lr.reverse(u - ub, tape, tab, amap, w, f)
    cost = lambda f_, a_, w_: tw.l2_cost(lr.fwd_tape(f_, tw.alpha_to_map(a_, M, N), w_, K)[0], ub)
    for what, g, fd in (("alpha", float(ga.sum()), (cost(f, alpha + h, w) - cost(f, alpha - h, w)) / (2 * h)),
                        ("f", float((gf * df).sum()), (cost(f + h * df, alpha, w) - cost(f - h * df, alpha, w)) / (2 * h)),
                        ("w", float((lr.reduce_w(gw, w) * dw).sum()), (cost(f, alpha, w + h * dw) - cost(f, alpha, w - h * dw)) / (2 * h))):
        print("%s: reverse sweep %.10g central difference %.10g rel %.2e" % (what, g, fd, abs(g - fd) / abs(fd)))
        assert fd != 0.0 and abs(g - fd) <= 1e-5 * abs(fd)


@pytest.mark.parametrize("wkind", lr.WEIGHTS)
@pytest.mark.parametrize("name", sorted(lr.GPU_SHAPES))
def test_gpu_cases_keep_their_decisions_clear_of_a_tie_and_take_both_branches(name, wkind):
    """Of every case tests/test_gpu_l1.py holds against the twin, on every iteration: min |n2 - alpha^2| / alpha^2 >= 1e-9 (measured:
    at least 1.1e-8) and min |m| / max(tau w, |d|) >= 1e-9 over the pixels with w > 0 (at least 1.2e-8), so a decision that
    differs between the kernel's fma and the twin's plain arithmetic would need an error orders of magnitude above rounding; the
    threshold lets the step through in 10 % ... 90 % of the pixel-iterations (measured 14 % ... 66 %) and u differs from f on at
    least 10 % of the pixels (at least 22 %), so no case tests one branch only.  One more, which the data (l1_ref.gpu_data) are
    made for: at a pixel with w = 0, where grad_w is -tau sign(d) h, |d| >= 1e-9 in every iteration whose div is not exactly
    zero (at least 1.2e-7) -- the data are O(1), so no rounding decides that sign."""
    O, N, M = lr.GPU_SHAPES[name]
    f, _ = lr.gpu_data(name)
    for kind in lr.KINDS:
        for K in lr.GRADIENT_K:
            u0, _, _, _, st = lr.twin_case(name, kind, wkind, K)
            moved = float((u0 != f).mean())
            print("%s %s %s K %d: projection margin %.2e threshold margin %.2e |d| at w = 0 %.2e active %.2f u != f %.2f"
                  % (name, kind, wkind, K, st["decision_margin"], st["threshold_margin"], st["nodata_margin"], st["active_share"], moved))
            assert st["nodata_margin"] >= 1e-9
            assert st["decision_margin"] >= 1e-9
            assert st["threshold_margin"] >= 1e-9
            assert 0.1 <= st["active_share"] <= 0.9
            assert moved >= 0.1


@pytest.mark.parametrize("alpha", [0.35, 0.5])
def test_twin_removes_isolated_spikes_exactly(alpha):
    """A constant plane with four isolated spikes, w = 1: removing a spike of height h costs w h and saves (2 + sqrt 2) alpha h,
    so for alpha = 0.35 and 0.5 the answer is the constant.  max|u - 0.5| <= 1e-13 at K = 203 (measured 1.2e-16; 3.3e-8 at
    K = 50)."""
    f, heights = lr.spikes()
    assert len(heights) == 4 and float(np.abs(f - 0.5).max()) == 0.45
    amap = tw.alpha_to_map(alpha, 33, 17)
    d50 = float(np.abs(lr.fwd_tape(f, amap, np.ones((17, 33)), 50)[0] - 0.5).max())
    d203 = float(np.abs(lr.fwd_tape(f, amap, np.ones((17, 33)), 203)[0] - 0.5).max())
    print("alpha %g: max|u - 0.5| %.2e at K = 50, %.2e at K = 203" % (alpha, d50, d203))
    assert d203 <= 1e-13


def test_twin_keeps_spikes_below_the_threshold_exactly():
    """alpha = 0.2: (2 + sqrt 2) alpha < w, and u_K = f bit for bit."""
    f, _ = lr.spikes()
    for K in (50, 203):
        assert np.array_equal(lr.fwd_tape(f, tw.alpha_to_map(0.2, 33, 17), np.ones((17, 33)), K)[0], f)
