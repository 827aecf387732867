"""Forward mode through the TV-L1 and the TV-KL iterations on a machine without a GPU: the library
exports the six functions with the weighted twins' argument lists, the binding covers them, TVSolver and the torch layer have the
entries, the new layer functions reject wrong inputs before they touch the library, and the numpy twin the GPU tests compare
against (tests/l1_kl_jvp_ref.py) is pinned: its primal is the committed twins' bit for bit, its tangent is the transpose of their
reverse sweeps, agrees with torch's forward-mode AD and with central differences, keeps the two models' conventions, and is not
trivially zero in any case the GPU tests count as a tangent check."""
import ctypes as C
import os
import re

import numpy as np
import pytest
from conftest import ROOT

import kl_ref as kr
import l1_kl_jvp_ref as j
import l1_ref as lr
from oracle import np_twin as tw

TWINS = {"bpltv_%s_unrolled_%s" % (m, s): "bpltv_weighted_unrolled_%s" % s
         for m in ("lone", "kl") for s in ("jvp", "jvp_device", "gauss_newton")}
CASES = [(name, kind, wkind) for name in j.GRADIENT_SHAPES for kind in j.KINDS for wkind in j.WEIGHTS]


def _header_text():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bpltv.h")).read(), flags=re.S)


def _header_args(name):
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name, _header_text())
    assert m, name
    return [" ".join(a.split()) for a in m.group(1).split(",")]


@pytest.mark.parametrize("name", sorted(TWINS))
def test_library_exports_and_binds_the_function_with_its_weighted_twin_s_arguments(name):
    from bpldenoising_amd import _lib
    lib = _lib.load()
    assert re.fullmatch(r"bpltv_[a-z_]+", name)
    assert hasattr(lib, name)
    assert _header_args(name) == _header_args(TWINS[name])
    assert _lib.SYMBOLS[name] == _lib.SYMBOLS[TWINS[name]]
    assert getattr(lib, name).argtypes == _lib.SYMBOLS[name][1] and _lib.SYMBOLS[name][0] is C.c_int


def test_binding_covers_the_header_and_names_the_sweeps():
    from bpldenoising_amd import _lib
    declared = set(re.findall(r"\b(bpltv_\w+)\s*\(", _header_text()))
    assert set(TWINS) <= declared
    assert declared == set(_lib.SYMBOLS), declared ^ set(_lib.SYMBOLS)
    hdr = open(os.path.join(ROOT, "include", "bpltv.h")).read()
    assert "17 tangent sweep through the TV-L1 iterations" in hdr and "18 tangent sweep through the TV-KL iterations" in hdr
    st = _lib.BpltvStats()
    for code, name in ((17, "l1-unrolled-jvp"), (18, "kl-unrolled-jvp"), (15, "l1-unrolled"), (16, "kl-unrolled"), (11, "weighted-unrolled-jvp")):
        st.adjoint_method = code
        assert st.as_dict()["adjoint_method"] == name


def test_solver_and_layer_have_the_entries():
    pytest.importorskip("torch")
    import inspect
    import torch
    from bpldenoising_amd import TVSolver, torch_layer
    for m in ("l1", "kl"):
        for s in ("jvp", "jvp_device", "gauss_newton"):
            fn, twin = getattr(TVSolver, "%s_unrolled_%s" % (m, s)), getattr(TVSolver, "weighted_unrolled_%s" % s)
            assert str(inspect.signature(fn)) == str(inspect.signature(twin)), (m, s)
    for M, old, new, fwd, base in (("L1", torch_layer._L1_UNROLLED, torch_layer._L1_UNROLLED_FWD, torch_layer.TVL1DenoiseUnrolledForwardFunction,
                                    torch_layer.TVL1DenoiseUnrolledFunction),
                                   ("KL", torch_layer._KL_UNROLLED, torch_layer._KL_UNROLLED_FWD, torch_layer.TVKLDenoiseUnrolledForwardFunction,
                                    torch_layer.TVKLDenoiseUnrolledFunction)):
        assert old.jvp is None                                         # the old rows still carry none
        assert new.jvp == "%s_unrolled_jvp_device" % M.lower() and callable(getattr(TVSolver, new.jvp))
        assert new._replace(jvp=None, w=old.w) == old                  # the same model otherwise
        assert issubclass(fwd, base) and issubclass(fwd, torch.autograd.Function)
        assert fwd.backward is base.backward and fwd.forward is not base.forward and "jvp" in vars(fwd)
        assert "jvp" not in vars(base)
    for fn in (torch_layer.tv_l1_denoise_unrolled_fwd, torch_layer.tv_kl_denoise_unrolled_fwd):
        p = inspect.signature(fn).parameters
        assert list(p) == ["f", "alpha", "w", "maxiter", "checkpoint_every", "solver_kw"]
        assert p["maxiter"].default == 50 and p["checkpoint_every"].default is None
    for cls in (torch_layer.TVL1DenoiseUnrolled, torch_layer.TVKLDenoiseUnrolled):
        m = cls(0.7, np.ones((4, 5)), maxiter=7)
        assert m.forward_mode is False
        m = cls(0.7, np.ones((4, 5)), maxiter=7, learn_w=True, forward_mode=True)
        assert m.forward_mode is True and sorted(n for n, _ in m.named_parameters()) == ["alpha", "w"]
        assert "forward_mode" not in m.solver_kw


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


@pytest.mark.parametrize("model", j.MODELS)
def test_the_fwd_function_rejects_before_any_library_call(layer, model):
    """tests/test_l1_abi.py's rejections of tv_l1_denoise_unrolled, for the two _fwd functions; the old flag still raises."""
    import torch
    name = "tv_%s_denoise_unrolled_fwd" % model
    fn, old = getattr(layer, name), getattr(layer, "tv_%s_denoise_unrolled" % model)
    f = torch.zeros(2, 8, 6, dtype=torch.float64)
    a = torch.tensor(0.7, dtype=torch.float64)
    w = torch.ones(8, 6, dtype=torch.float64)
    with pytest.raises(TypeError, match="torch tensors"):
        fn(np.zeros((2, 8, 6)), a, w, maxiter=5)
    with pytest.raises(TypeError, match="float64"):
        fn(f.float(), a, w, maxiter=5)
    with pytest.raises(TypeError, match="float64"):
        fn(f, a.float(), w, maxiter=5)
    with pytest.raises(TypeError, match=name + ": w must be a torch tensor"):
        fn(f, a, np.ones((8, 6)), maxiter=5)
    with pytest.raises(TypeError, match=name + ": w must be float64"):
        fn(f, a, w.float(), maxiter=5)
    with pytest.raises(ValueError, match="f must have shape"):   # a colour batch
        fn(torch.zeros(2, 3, 8, 6, dtype=torch.float64), a, w, maxiter=5)
    for bad in (torch.ones(6, 8, dtype=torch.float64), torch.ones(3, 8, 6, dtype=torch.float64),
                torch.ones(1, 8, 6, dtype=torch.float64), torch.ones(2, 1, 8, 6, dtype=torch.float64)):
        with pytest.raises(ValueError, match=name + ": w must have shape"):
            fn(f, a, bad, maxiter=5)
    neg, nan, inf = w.clone(), w.clone(), torch.ones(2, 8, 6, dtype=torch.float64)
    neg[3, 2] = -1e-300
    nan[0, 0] = float("nan")
    inf[1, 7, 5] = -float("inf")
    for bad in (neg, nan, inf):
        with pytest.raises(ValueError, match=name + ": w must be finite and >= 0"):
            fn(f, a, bad, maxiter=5)
    for bad in (torch.zeros(2, dtype=torch.float64), torch.zeros(9, 6, dtype=torch.float64), torch.zeros(2, 8, 6, dtype=torch.float64)):
        with pytest.raises(ValueError, match="alpha must be"):
            fn(f, bad, w, maxiter=5)
    with pytest.raises(ValueError, match="w is on"):
        fn(f, a, w.to("meta"), maxiter=5)
    if model == "kl":   # the layer's own f >= 0 check
        for v in (-1e-300, float("nan"), float("inf")):
            bad = f.clone()
            bad[1, 2, 3] = v
            with pytest.raises(ValueError, match=name + ": f must be finite and >= 0"):
                fn(bad, a, w, maxiter=5)
    with pytest.raises(TypeError):   # the _fwd function has no flag: it is the forward mode
        fn(f, a, w, 5, None, True)
    with pytest.raises(ValueError, match="forward mode through the TV-%s iterations does not exist; tv_%s_denoise_unrolled_fwd" % (model.upper(), model)):
        old(f, a, w, maxiter=5, forward_mode=True)
    for good in (w, torch.zeros(8, 6, dtype=torch.float64), torch.ones(2, 8, 6, dtype=torch.float64)):   # everything valid, on the CPU
        with pytest.raises(ValueError, match="ROCm device"):
            fn(f, a, good, maxiter=5, checkpoint_every=2)
    cls = layer.TVL1DenoiseUnrolled if model == "l1" else layer.TVKLDenoiseUnrolled
    with pytest.raises(ValueError, match="ROCm device"):
        cls(0.7, np.ones((8, 6)), maxiter=5, learn_w=True, forward_mode=True)(f)


# ---- the twin -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", j.GRADIENT_SHAPES)
@pytest.mark.parametrize("model", j.MODELS)
def test_twin_primal_transpose_identity_and_non_triviality(model, name):
    """For every parameter form, weight and depth of the shape: u is fwd_tape's bit for bit; <du, gu> = <df, grad_f> + <dalpha,
    grad_alpha> + <dw, grad_w> against the committed reverse to 1e-12 * sum|du * gu| (all three tangents together; the sums differ
    in rounding only: measured at most 2.9e-15 for L1, 1.6e-14 for KL); and each single direction gives a du that is non-zero on
    at least 5 % of the pixels -- but for the listed dalpha-alone cases of L1 on a single row or column at K = 50, whose nine
    pixels end held at f or flat: those are identically zero."""
    ref = j.REF[model]
    worst, listed = 0.0, 0
    for kind in j.KINDS:
        for wkind in j.WEIGHTS:
            f, gu, _, amap, w = j.case(model, name, kind, wkind)
            df, _, dam, dw = j.tangents_of(name, wkind, kind)
            for K in j.GRADIENT_K:
                u0, tape, tab = ref.fwd_tape(f, amap, w, K)
                gf, ga, gw = ref.reverse(gu, tape, tab, amap, w, f)
                u, du = j.twin_tangent(model, name, kind, wkind, K, "all")
                assert np.array_equal(u, u0), (kind, wkind, K)
                lhs = float((du * gu).sum())
                rhs = float((df * gf).sum()) + float((dam * ga).sum()) + float((dw * ref.reduce_w(gw, w)).sum())
                scale = float(np.abs(du * gu).sum())
                worst = max(worst, abs(lhs - rhs) / scale)
                assert abs(lhs - rhs) <= 1e-12 * scale, (kind, wkind, K, abs(lhs - rhs) / scale)
                for direction in ("f", "alpha", "w"):
                    u1, d1 = j.twin_tangent(model, name, kind, wkind, K, direction)
                    assert np.array_equal(u1, u0)
                    share = float((d1 != 0).mean())
                    if j.is_zero_case(model, name, kind, wkind, K, direction):
                        listed += 1
                        assert share == 0.0, (kind, wkind, K, direction, share)
                    else:
                        assert share >= 0.05, (kind, wkind, K, direction, share)
    print("%s %s: transpose identity, worst relative %.2e; %d identically zero (listed)" % (model, name, worst, listed))
    expect = sum(1 for n, _, _ in j.L1_ZERO_DALPHA if n == name) if model == "l1" else 0
    assert listed == expect


def test_the_listed_zero_cases_are_the_single_row_and_column_only():
    assert len(j.L1_ZERO_DALPHA) == 13 and {n for n, _, _ in j.L1_ZERO_DALPHA} == {"1x1x9", "1x9x1"}
    assert j.L1_ZERO_DALPHA_K == 50 and 203 in j.GRADIENT_K
    assert j.L1_ZERO_DALPHA <= set(CASES)


@pytest.mark.parametrize("wkind", ["real", "mask"])
@pytest.mark.parametrize("model", j.MODELS)
def test_twin_agrees_with_torch_forward_mode(model, wkind):
    """1e-11 * max|ref|, the bound the reverse twins are held to against torch autograd: each tangent alone and all together, on
    the odd shape and on the single row, K = 50."""
    pytest.importorskip("torch")
    for name, kind in (("2x17x33", "map"), ("2x17x33", "patch"), ("1x1x9", "scalar")):
        f, _, _, amap, w = j.case(model, name, kind, wkind)
        tangents = j.tangents_of(name, wkind, kind)
        for direction in j.DIRECTIONS:
            tf, _, tam, tw_ = j.select(direction, *tangents)
            u0, du0 = j.torch_forward_reference(model, f, amap, w, 50, tf, tam, tw_)
            u, du = j.twin_tangent(model, name, kind, wkind, 50, direction)
            d, m = float(np.abs(du - du0).max()), float(np.abs(du0).max())
            print("%s %s %s %s d%s: max|du - torch| %.2e  max|torch| %.2e" % (model, name, kind, wkind, direction, d, m))
            assert d <= 1e-11 * m
            assert float(np.abs(u - u0).max()) <= 1e-11 * float(np.abs(u0).max())


@pytest.mark.parametrize("model", j.MODELS)
def test_twin_against_central_differences(model):
    """central_difference_case() of the model with its CD_ALPHA, CD_K and CD_H: one direction each in alpha, f and w; 1e-5 relative
    in the maximum norm."""
    ref = j.REF[model]
    _, f, w, df, dw = ref.central_difference_case()
    N, M = f.shape[-2:]
    a, K, h = ref.CD_ALPHA, ref.CD_K, ref.CD_H
    amap = np.full((N, M), a)
    one = np.ones((N, M))

    def u_of(ff, aa, ww):
        return ref.fwd_tape(ff, aa, ww, K)[0]
    for what, tf, ta, tw_ in (("alpha", None, one, None), ("f", df, None, None), ("w", None, None, dw)):
        _, du = j.forward_tangent(model, f, amap, w, K, tf, ta, tw_)
        fp, fm = (f + h * tf, f - h * tf) if tf is not None else (f, f)
        ap, am = (amap + h * ta, amap - h * ta) if ta is not None else (amap, amap)
        wp, wm = (w + h * tw_, w - h * tw_) if tw_ is not None else (w, w)
        fd = (u_of(fp, ap, wp) - u_of(fm, am, wm)) / (2 * h)
        d, m = float(np.abs(du - fd).max()), float(np.abs(fd).max())
        print("%s d/d%s: max|du - fd| %.3e  max|fd| %.3e  rel %.2e" % (model, what, d, m, d / m))
        assert d <= 1e-5 * m, what


# ---- the conventions, each on a plane of a few pixels --------------------------------------------------------------------
def test_l1_a_held_pixel_passes_df_and_nothing_else():
    """alpha = 0: the duals stay zero and every pixel with w > 0 stays held at f (|d| = 0 <= tau w): du = df there, whatever
    dalpha and dw are."""
    rng = np.random.default_rng(1)
    f = rng.random((1, 3, 4))
    w = 0.5 + rng.random((3, 4))
    df, dam, dw = rng.standard_normal(f.shape), rng.standard_normal((3, 4)), rng.standard_normal((3, 4))
    for K in (1, 5):
        u, du = j.forward_tangent("l1", f, np.zeros((3, 4)), w, K, df, dam, dw)
        assert np.array_equal(u, f) and np.array_equal(du, df)
    # with a regulariser, one step: the pixels that stay at f pass df exactly, the others do not
    amap = np.full((3, 4), 0.7)
    u, du = j.forward_tangent("l1", f, amap, w, 2, df, dam, dw)
    held = u == f
    assert held.any() and np.array_equal(du[held], df[held])
    _, du_no_f = j.forward_tangent("l1", f, amap, w, 2, None, dam, dw)
    assert not du_no_f[held].any()


def test_l1_a_pixel_without_data_passes_dv():
    """w == 0 everywhere: the threshold is the identity, x+ = v and dx+ = dv (with dw, the one-sided -tau sign(d) dw beside it) --
    never df, which a pixel held at f would pass: a tangent in alpha alone reaches every pixel, and a tangent in f alone is not
    handed through unchanged."""
    rng = np.random.default_rng(2)
    f = rng.random((1, 3, 4))
    w = np.zeros((3, 4))
    amap = np.full((3, 4), 0.05)
    df, dam, dw = rng.standard_normal(f.shape), rng.standard_normal((3, 4)), rng.standard_normal((3, 4))
    # one step from x = f, y = 0: div = 0, v = f, dv = df -- what a held pixel answers too; the later steps tell them apart
    _, du1 = j.forward_tangent("l1", f, amap, w, 1, df, dam, None)
    assert np.array_equal(du1, df)
    u, du_a = j.forward_tangent("l1", f, amap, w, 6, None, dam, None)
    assert du_a.all()                                   # (held pixels would pass df = 0)
    _, du_f = j.forward_tangent("l1", f, amap, w, 6, df, None, None)
    assert (du_f != df).all()
    # dv is the tangent of the iteration without a data term: the twin with a tiny threshold that every pixel clears agrees
    pytest.importorskip("torch")
    for tf, ta, tw_ in ((df, None, None), (None, dam, None), (df, dam, dw)):
        _, du = j.forward_tangent("l1", f, amap, w, 6, tf, ta, tw_)
        ut, dut = j.torch_forward_reference("l1", f, amap, w, 6, tf, ta, tw_)
        assert float(np.abs(du - dut).max()) <= 1e-11 * float(np.abs(dut).max())
        assert float(np.abs(u - ut).max()) <= 1e-11 * float(np.abs(ut).max())


def test_kl_a_clamped_pixel_passes_exactly_zero_and_its_neighbours_do_not():
    """f = 0 at one pixel (w f = 0) next to bright neighbours: c = -tau w < 0 and g = 0, so the prox clamps it at x+ = 0 exactly, and
    the tangent there is exactly zero -- df, dalpha and dw alike -- while its neighbours' is not."""
    f = np.full((1, 3, 5), 2.0)
    f[0, 1, 2] = 0.0
    w = np.ones((3, 5))
    amap = np.full((3, 5), 0.1)   # (tau |div| <= 5 * 4 * 0.1 < tau w: the pixel's c stays below zero)
    rng = np.random.default_rng(3)
    df, dam, dw = rng.standard_normal(f.shape), rng.standard_normal((3, 5)), rng.standard_normal((3, 5))
    u, du = j.forward_tangent("kl", f, amap, w, 1, df, dam, dw)
    assert np.array_equal(u, kr.fwd_tape(f, amap, w, 1)[0])
    assert u[0, 1, 2] == 0.0 and du[0, 1, 2] == 0.0
    others = np.ones(f.shape, dtype=bool)
    others[0, 1, 2] = False
    assert (u[others] > 0).all() and du[others].all()
    # ... and stays so while the duals move: c = v - tau w stays below zero (v = tau |div| <= 2 would have to exceed 5), every step passes nothing
    for K in (2, 3, 8):
        u, du = j.forward_tangent("kl", f, amap, w, K, df, dam, dw)
        assert np.array_equal(u, kr.fwd_tape(f, amap, w, K)[0])
        assert u[0, 1, 2] == 0.0 and du[0, 1, 2] == 0.0 and (u[others] > 0).all() and du[others].all()


def test_the_three_models_tangents_differ():
    """The same w, alpha and K: the weighted, the L1 and the KL sweep give tangents that differ pairwise by more than
    1e-3 * max|du| (tests/test_gpu_l1_kl_jvp.py runs the three on one handle and relies on it)."""
    import weighted_unrolled_jvp_ref as wuj
    f, alpha, w, K, df, dam, dw = j.cross_model_case()
    N, M = f.shape[-2:]
    amap = tw.alpha_to_map(alpha, M, N)
    du = {"weighted": wuj.forward_tangent(f, amap, w, K, df, dam, dw)[1],
          "l1": j.forward_tangent("l1", f, amap, w, K, df, dam, dw)[1],
          "kl": j.forward_tangent("kl", f, amap, w, K, df, dam, dw)[1]}
    for a, b in (("weighted", "l1"), ("weighted", "kl"), ("l1", "kl")):
        d = float(np.abs(du[a] - du[b]).max())
        m = max(float(np.abs(du[a]).max()), float(np.abs(du[b]).max()))
        print("%s vs %s: max|diff| %.2e  max|du| %.2e" % (a, b, d, m))
        assert d > 1e-3 * m
