"""GPU checks of the vector-Jacobian product of u = denoise(f, alpha) (bpltv_vjp / bpltv_vjp_device).

The VJP solves the adjoint system of bpltv_gradient with the cotangent gu in place of u - ubar (-gu for gradient_reg,
/ sqrt(alpha) with an array parameter).  So gu = u - ubar gives bpltv_gradient's result bit for bit, grad_f is the
oracle's adjoint state p (-p for gradient_reg) for ubar' = u - gu, and the VJP never touches the last solve."""
import functools

import numpy as np
import pytest
from conftest import synth_batch

pytestmark = pytest.mark.gpu

P22 = np.array([[0.08, 0.12], [0.1, 0.05]])
E_ARG, E_UNSUPPORTED = 1, 6

# (O, N, M, parameter kind): 10 x 128^2 scalar, and a non-square batch (N != M catches a transposed layout)
CASES = [(10, 128, 128, "scalar"), (3, 48, 40, "scalar"), (3, 48, 40, "patch22"), (3, 48, 40, "map")]
IDS = ["10x128_scalar", "3x48x40_scalar", "3x48x40_patch22", "3x48x40_map"]


def _alpha(kind, N, M, scale=1.0):
    if kind == "scalar":
        return 0.1 * scale
    if kind == "patch22":
        return P22 * scale
    return (0.05 + 0.1 * np.random.default_rng(8).random((N, M))) * scale


@functools.lru_cache(maxsize=None)
def _case(O, N, M, kind):
    """(ubar, f, alpha, u): u from a 300-iteration solve of the library (the VJP takes any u)."""
    from bpldenoising_amd import TVSolver
    ub, f = synth_batch(O, N, M, seed=40 + M)
    alpha = _alpha(kind, N, M)
    s = TVSolver(M, N, O)
    s.set_data(ub, f)
    u = s.denoise(alpha, maxiter=300)
    s.close()
    return ub, f, alpha, u


def _cotangent(u, seed=3):
    return np.random.default_rng(seed).standard_normal(u.shape)


def _nd_bytes_per_image(M, N):
    """Workspace of the nested-dissection solver per image, from the host check tool (the same symbolic code)."""
    import os, re, subprocess
    from conftest import ROOT
    exe = os.path.join(ROOT, "tools", "_bin", "nd_host_check")
    out = subprocess.run([exe, "bytes", str(M), str(N)], capture_output=True, text=True, timeout=120).stdout
    return float(re.search(r"bytes_per_image tv (\d+)", out).group(1))


def _same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b))


@pytest.mark.parametrize("reg", [0, 1])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_vjp_of_u_minus_ubar_is_the_gradient_bitwise(gpu_solver_cls, case, reg):
    O, N, M, kind = case
    ub, f, alpha, u = _case(*case)
    s = gpu_solver_cls(M, N, O)
    g0 = s.gradient(u, ub, alpha, reg=reg)
    gf, ga = s.vjp(u, alpha, u - ub, reg=reg)
    assert np.shape(ga) == np.shape(g0) and _same(ga, g0)
    assert gf.shape == u.shape and np.all(np.isfinite(gf))
    st = s.stats()
    assert st["reg_gradient_used"] == reg and st["adjoint_residual"] <= 1e-6 and st["adjoint_ms"] > 0, st
    # u from evaluate: the evaluate gradient (delta = 0.1: gradient, delta = 0: gradient_reg)
    s.set_data(ub, f)
    ue, _, ge = s.evaluate(alpha, 0.0 if reg else 0.1, maxiter=300)
    _, ga2 = s.vjp(ue, alpha, ue - ub, reg=reg, want_f=False)
    assert _same(ga2, ge)
    s.close()


@pytest.mark.parametrize("reg", [0, 1])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_vjp_matches_the_oracle_adjoint_state(gpu_solver_cls, oracle, case, reg):
    """grad_f == +-p of oracle.gradient_image(u_k, u_k - gu_k, ...) image by image; grad_alpha == oracle.gradient."""
    O, N, M, kind = case
    ub, f, alpha, u = _case(*case)
    gu = _cotangent(u)
    s = gpu_solver_cls(M, N, O)
    gf, ga = s.vjp(u, alpha, gu, reg=reg)
    s.close()
    amap = oracle.patch_upsample(alpha, M, N)
    patch = np.ndim(alpha) != 0
    for k in range(O):
        _, p, _ = oracle.gradient_image(u[k], u[k] - gu[k], amap, patch=patch, reg=bool(reg))
        want = -p if reg else p
        assert np.allclose(gf[k], want, rtol=1e-6, atol=1e-8 * np.abs(p).max()), k
    g0 = oracle.gradient(alpha, u, u - gu, reg=bool(reg))
    assert np.allclose(ga, g0, rtol=1e-6, atol=1e-8 * np.abs(g0).max())


@pytest.mark.parametrize("reg", [0, 1])
@pytest.mark.parametrize("case", CASES[1:], ids=IDS[1:])
def test_vjp_is_linear_in_the_cotangent_and_zero_at_zero(gpu_solver_cls, case, reg):
    O, N, M, kind = case
    _, _, alpha, u = _case(*case)
    g1, g2 = _cotangent(u, 5), _cotangent(u, 6)
    s = gpu_solver_cls(M, N, O)
    f1, a1 = s.vjp(u, alpha, g1, reg=reg)
    f2, a2 = s.vjp(u, alpha, g2, reg=reg)
    f3, a3 = s.vjp(u, alpha, 2.0 * g1 - 0.5 * g2, reg=reg)
    rel = lambda x, y: np.linalg.norm(np.ravel(x) - np.ravel(y)) / np.linalg.norm(np.ravel(y))
    assert rel(f3, 2.0 * f1 - 0.5 * f2) <= 1e-8
    assert rel(a3, 2.0 * np.asarray(a1) - 0.5 * np.asarray(a2)) <= 1e-8
    f0, a0 = s.vjp(u, alpha, np.zeros_like(u), reg=reg)
    assert not np.any(f0) and not np.any(a0)
    s.close()


@pytest.mark.parametrize("reg", [0, 1])
@pytest.mark.parametrize("case", CASES[1:], ids=IDS[1:])
def test_vjp_variants_agree_bitwise(gpu_solver_cls, case, reg):
    """Host and device forms, each output alone and both, image groups (adjoint_budget_mb) and a dtype-32 handle."""
    import torch
    O, N, M, kind = case
    _, _, alpha, u = _case(*case)
    gu = _cotangent(u, 7)
    s = gpu_solver_cls(M, N, O)
    gf, ga = s.vjp(u, alpha, gu, reg=reg)
    assert s.stats()["adjoint_chunks"] == 1
    assert _same(s.vjp(u, alpha, gu, reg=reg, want_alpha=False)[0], gf)
    assert _same(s.vjp(u, alpha, gu, reg=reg, want_f=False)[1], ga)
    dev = torch.device("cuda", 0)
    tu, tg = torch.from_numpy(u).to(dev), torch.from_numpy(gu).to(dev)
    a = np.asarray(alpha, dtype=np.float64)
    ta = torch.from_numpy(a.reshape(-1).copy()).to(dev)
    am, an = (1, 1) if a.ndim == 0 else (a.shape[1], a.shape[0])
    tf, tga = torch.empty_like(tu), torch.empty(am * an, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    s.vjp_device(tu.data_ptr(), ta.data_ptr(), am, an, tg.data_ptr(), tf.data_ptr(), tga.data_ptr(), reg=reg)
    assert _same(tf.cpu().numpy(), gf) and _same(tga.cpu().numpy(), np.ravel(ga))
    tf2 = torch.zeros_like(tu)
    s.vjp_device(tu.data_ptr(), ta.data_ptr(), am, an, tg.data_ptr(), tf2.data_ptr(), None, reg=reg)
    tga2 = torch.zeros_like(tga)
    s.vjp_device(tu.data_ptr(), ta.data_ptr(), am, an, tg.data_ptr(), None, tga2.data_ptr(), reg=reg)
    assert _same(tf2.cpu().numpy(), gf) and _same(tga2.cpu().numpy(), np.ravel(ga))
    s.close()
    # image groups: a budget of two images' nested-dissection workspace
    sg = gpu_solver_cls(M, N, O)
    sg.vjp(u, alpha, gu, reg=reg)
    sg.set_option("adjoint_budget_mb", 2.5 * _nd_bytes_per_image(M, N) / 1e6)
    gfg, gag = sg.vjp(u, alpha, gu, reg=reg)
    assert sg.stats()["adjoint_chunks"] > 1
    assert _same(gfg, gf) and _same(gag, ga)
    sg.close()
    s32 = gpu_solver_cls(M, N, O, dtype=32)
    g32f, g32a = s32.vjp(u, alpha, gu, reg=reg)
    assert _same(g32f, gf) and _same(g32a, ga)
    s32.close()


def _snapshot(s):
    import torch
    n = s.O * s.N * s.M
    buf = torch.empty(n, dtype=torch.float64, device="cuda")
    s.copy_u_device(buf.data_ptr())
    return buf.cpu().numpy(), s.duality_gap()


@pytest.mark.parametrize("kind", ["scalar", "patch22", "map"])
def test_vjp_leaves_the_last_solve_untouched(gpu_solver_cls, kind):
    """After a denoise, VJPs at another alpha (host and device forms) leave u_device, the duality gap and the next
    graph-replayed denoise of the old alpha bit for bit as they were."""
    import torch
    O, N, M = 3, 48, 40
    ub, f = synth_batch(O, N, M, seed=50)
    alpha, other = _alpha(kind, N, M), _alpha(kind, N, M, scale=3.0)
    s = gpu_solver_cls(M, N, O)
    s.set_data(ub, f)
    u0 = s.denoise(alpha, maxiter=200)
    assert s.stats()["graph_used"] == 1
    snap_u, snap_gap = _snapshot(s)
    gu = _cotangent(u0, 9)
    for reg in (0, 1):
        s.vjp(u0, other, gu, reg=reg)
    a = np.asarray(other, dtype=np.float64)
    am, an = (1, 1) if a.ndim == 0 else (a.shape[1], a.shape[0])
    ta = torch.from_numpy(a.reshape(-1).copy()).cuda()
    tu, tg = torch.from_numpy(u0).cuda(), torch.from_numpy(gu).cuda()
    tf = torch.empty_like(tu)
    torch.cuda.synchronize()
    s.vjp_device(tu.data_ptr(), ta.data_ptr(), am, an, tg.data_ptr(), tf.data_ptr(), None)
    u_now, gap_now = _snapshot(s)
    assert _same(u_now, snap_u) and _same(gap_now, snap_gap)
    u1 = s.denoise(alpha, maxiter=200)
    assert s.stats()["graph_used"] == 1 and _same(u1, u0)
    s.close()


def test_vjp_rejects_bad_input_and_changes_nothing(gpu_solver_cls):
    import torch
    from bpldenoising_amd._lib import BpltvError
    O, N, M = 3, 48, 40
    ub, f = synth_batch(O, N, M, seed=51)
    s = gpu_solver_cls(M, N, O)
    s.set_data(ub, f)
    u0 = s.denoise(P22, maxiter=200)
    gu = _cotangent(u0, 10)
    ref = s.vjp(u0, P22, gu)
    snap = _snapshot(s)
    bad_gu = gu.copy()
    bad_gu[1, 7, 5] = np.nan
    inf_gu = gu.copy()
    inf_gu[2, 0, 0] = -np.inf
    zero_patch = P22.copy()
    zero_patch[0, 1] = 0.0
    calls = [(P22 * np.nan, gu, 0), (-P22, gu, 0), (P22, bad_gu, 0), (P22, inf_gu, 1), (zero_patch, gu, 1),
             (-0.1, gu, 0), (float("nan"), gu, 1)]
    for alpha, g, reg in calls:
        with pytest.raises(BpltvError) as e:
            s.vjp(u0, alpha, g, reg=reg)
        assert e.value.code == E_ARG, (alpha, reg, str(e.value))
    # device form: parameter and cotangent checked on the device
    tu, tg, tbad = (torch.from_numpy(x).cuda() for x in (u0, gu, bad_gu))
    tf = torch.empty_like(tu)
    for a, g in ((-P22, tg), (P22 * np.nan, tg), (P22, tbad)):
        ta = torch.from_numpy(np.ascontiguousarray(a).reshape(-1)).cuda()
        torch.cuda.synchronize()
        with pytest.raises(BpltvError) as e:
            s.vjp_device(tu.data_ptr(), ta.data_ptr(), 2, 2, g.data_ptr(), tf.data_ptr(), None)
        assert e.value.code == E_ARG
    # both outputs NULL
    from bpldenoising_amd.learning_function import _ptr
    a = np.ascontiguousarray(P22)
    assert s._lib.bpltv_vjp(s._h, _ptr(u0), _ptr(a), 2, 2, 0, None, _ptr(gu), None, None) == E_ARG
    with pytest.raises(ValueError):
        s.vjp(u0, P22, gu, want_f=False, want_alpha=False)
    now = _snapshot(s)
    assert _same(now[0], snap[0]) and _same(now[1], snap[1])
    again = s.vjp(u0, P22, gu)
    assert _same(again[0], ref[0]) and _same(again[1], ref[1])
    assert _same(s.denoise(P22, maxiter=200), u0)
    s.close()


@pytest.mark.parametrize("kind", ["scalar", "patch22", "map"])
def test_vjp_on_shards_of_one_device(gpu_solver_cls, kind):
    """bpltv_create_sharded with a repeated device: grad_f bitwise a single handle's, grad_alpha the shards' sum."""
    import torch
    from bpldenoising_amd._lib import BpltvError
    case = (3, 48, 40, kind)
    O, N, M, _ = case
    _, _, alpha, u = _case(*case)
    gu = _cotangent(u, 11)
    s = gpu_solver_cls(M, N, O)
    for reg in (0, 1):
        gf, ga = s.vjp(u, alpha, gu, reg=reg)
        m = gpu_solver_cls(M, N, O, devices=[0, 0])
        mf, ma = m.vjp(u, alpha, gu, reg=reg)
        assert _same(mf, gf)
        assert np.allclose(ma, ga, rtol=1e-13, atol=0)
        assert m.stats()["shards"] == 2
        assert _same(m.vjp(u, alpha, gu, reg=reg, want_alpha=False)[0], gf)
        tu = torch.from_numpy(u).cuda()
        tf = torch.empty_like(tu)
        ta = torch.from_numpy(np.asarray(alpha, dtype=np.float64).reshape(-1).copy()).cuda()
        am, an = (1, 1) if np.ndim(alpha) == 0 else (np.shape(alpha)[1], np.shape(alpha)[0])
        torch.cuda.synchronize()
        with pytest.raises(BpltvError) as e:
            m.vjp_device(tu.data_ptr(), ta.data_ptr(), am, an, tu.data_ptr(), tf.data_ptr(), None, reg=reg)
        assert e.value.code == E_UNSUPPORTED
        m.close()
    s.close()


def test_vjp_config5_share_8x1024_pixel_map(gpu_solver_cls):
    """BASELINE config 5's share of one GPU: 8 x 1024^2 with a pixel-map parameter, bitwise bpltv_gradient on
    u - ubar."""
    O, N, M = 8, 1024, 1024
    ub, f = synth_batch(O, N, M, seed=52)
    amap = 0.05 + 0.1 * np.random.default_rng(12).random((N, M))
    s = gpu_solver_cls(M, N, O)
    s.set_data(ub, f)
    u = s.denoise(amap, maxiter=200)
    g0 = s.gradient(u, ub, amap)
    gf, ga = s.vjp(u, amap, u - ub)
    st = s.stats()
    assert _same(ga, g0) and ga.shape == (N, M)
    assert np.all(np.isfinite(gf)) and st["adjoint_residual"] <= 1e-6, st
    s.close()
