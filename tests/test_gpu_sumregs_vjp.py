"""GPU checks of the vector-Jacobian product of u = sumregs_denoise(f, x) (bpltv_sumregs_vjp / _device) and of
bpltv_sumregs_denoise_device.

The VJP solves the adjoint system of bpltv_sumregs_evaluate's gradient with the cotangent gu in place of u - ubar (-gu
for sumregs_gradient_reg, whose row-scaled system takes ubar - u as it is).  So gu = u - ubar gives the evaluate's
gradient bit for bit, grad_f is the literal system's adjoint state p (-p for sumregs_gradient_reg) for ubar' = u - gu,
and the VJP never touches the last solve."""
import functools

import numpy as np
import pytest
from conftest import synth_batch

pytestmark = pytest.mark.gpu

E_ARG, E_UNSUPPORTED = 1, 6
A3 = np.array([0.03, 0.02, 0.05])
P22 = np.stack([np.array([[0.03, 0.05], [0.02, 0.04]]), np.array([[0.02, 0.03], [0.05, 0.02]]),
                np.array([[0.04, 0.02], [0.03, 0.06]])])

# (O, N, M, parameter kind).  numpy (3, n, m) == Julia m x n x 3: "patch35" is Julia's 3 x 5 patch, numpy (3, 5, 3),
# which divides neither side of the 48 x 40 images.
CASES = [(10, 128, 128, "vector"), (3, 48, 40, "vector"), (3, 48, 40, "patch22"), (3, 48, 40, "patch35"),
         (3, 48, 40, "map")]
IDS = ["10x128_vector", "3x48x40_vector", "3x48x40_patch22", "3x48x40_patch35", "3x48x40_map"]
SMALL, SMALL_IDS = CASES[1:], IDS[1:]
# delta of the evaluate each branch corresponds to (delta_t = 1e-3)
DELTA = {0: 0.1, 1: 1e-4}
# grad_f against the literal system's adjoint state, relative to max|p|: the literal-system goldens' 5e-6 (kappa 1e14
# against 1/eps).  Measured on MI355X: worst 5.4e-8 (3 x 48 x 40, 2 x 2 patch, reg = 0); reg = 1 at most 1.7e-9 (map).
GRADF_TOL = 5e-6


def _alpha(kind, N, M, scale=1.0):
    if kind == "vector":
        return A3 * scale
    if kind == "patch22":
        return P22 * scale
    if kind == "patch35":
        return (0.02 + 0.04 * np.random.default_rng(31).random((3, 5, 3))) * scale
    return (0.02 + 0.04 * np.random.default_rng(32).random((3, N, M))) * scale


@functools.lru_cache(maxsize=None)
def _case(O, N, M, kind):
    """(ubar, f, x, u): u from a 300-iteration sumregs_denoise of the library (the VJP takes any u)."""
    from bpldenoising_amd import TVSolver
    ub, f = synth_batch(O, N, M, seed=60 + M + O)
    x = _alpha(kind, N, M)
    s = TVSolver(M, N, O)
    s.set_data(ub, f)
    u = s.sumregs_denoise(x, maxiter=300)
    s.close()
    return ub, f, x, u


def _cotangent(u, seed=3):
    return np.random.default_rng(seed).standard_normal(u.shape)


def _same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b))


def _amn(x):
    x = np.asarray(x)
    return (1, 1) if x.ndim == 1 else (x.shape[2], x.shape[1])


@pytest.mark.parametrize("reg", [0, 1])
@pytest.mark.parametrize("case", CASES + [(2, 256, 256, "vector")], ids=IDS + ["2x256_vector"])
def test_sumregs_vjp_of_u_minus_ubar_is_the_evaluate_gradient_bitwise(gpu_solver_cls, case, reg):
    O, N, M, kind = case
    ub, f = synth_batch(O, N, M, seed=70 + M)
    x = _alpha(kind, N, M)
    s = gpu_solver_cls(M, N, O)
    s.set_data(ub, f)
    u, _, g = s.sumregs_evaluate(x, DELTA[reg], maxiter=300)
    assert s.stats()["reg_gradient_used"] == reg
    gf, ga = s.sumregs_vjp(u, x, u - ub, reg=reg)
    assert np.shape(ga) == np.shape(g) == np.shape(x) and _same(ga, g)
    assert gf.shape == u.shape and np.all(np.isfinite(gf))
    st = s.stats()
    assert st["reg_gradient_used"] == reg and st["adjoint_residual"] <= 1e-6 and st["adjoint_ms"] > 0, st
    assert st["adjoint_attempts"] >= 1 and st["adjoint_chunks"] >= 1
    s.close()


@pytest.mark.parametrize("reg", [0, 1])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_sumregs_vjp_matches_the_oracle(gpu_solver_cls, oracle, case, reg):
    """grad_x == oracle.sumregs_gradient(x, u, u - gu); grad_f == +-p of the literal system image by image (the
    10 x 128^2 case: its first two images, the scipy system is large)."""
    from oracle import np_twin_sumregs as TS
    O, N, M, kind = case
    ub, f, x, u = _case(*case)
    gu = _cotangent(u)
    s = gpu_solver_cls(M, N, O)
    gf, ga = s.sumregs_vjp(u, x, gu, reg=reg)
    s.close()
    g0 = oracle.sumregs_gradient(x, u, u - gu, reg=bool(reg))
    scale = np.abs(g0).max()
    assert np.shape(ga) == np.shape(g0)
    assert np.abs(ga - g0).max() <= (1e-7 if reg else 1e-6) * scale, np.abs(ga - g0).max() / scale
    worst = 0.0
    for k in range(O if O <= 3 else 2):
        if reg:
            p = -TS.gradient_reg_image(x, u[k], u[k] - gu[k])[1]
        else:
            p = TS.gradient_image(x, u[k], u[k] - gu[k])[1]
        p = p.reshape(N, M)
        err = np.abs(gf[k] - p).max() / np.abs(p).max()
        worst = max(worst, err)
        assert err <= GRADF_TOL, (k, err)
    print("grad_f vs literal system %s reg=%d: %.3e of max|p|" % ("x".join(map(str, case[:3])) + "_" + kind, reg, worst))


@pytest.mark.parametrize("reg", [0, 1])
@pytest.mark.parametrize("case", SMALL, ids=SMALL_IDS)
def test_sumregs_vjp_is_linear_in_the_cotangent_and_zero_at_zero(gpu_solver_cls, case, reg):
    O, N, M, kind = case
    _, _, x, u = _case(*case)
    g1, g2 = _cotangent(u, 5), _cotangent(u, 6)
    s = gpu_solver_cls(M, N, O)
    f1, a1 = s.sumregs_vjp(u, x, g1, reg=reg)
    f2, a2 = s.sumregs_vjp(u, x, g2, reg=reg)
    f3, a3 = s.sumregs_vjp(u, x, 2.0 * g1 - 0.5 * g2, reg=reg)
    rel = lambda a, b: np.linalg.norm(np.ravel(a) - np.ravel(b)) / np.linalg.norm(np.ravel(b))
    assert rel(f3, 2.0 * f1 - 0.5 * f2) <= 1e-8
    assert rel(a3, 2.0 * np.asarray(a1) - 0.5 * np.asarray(a2)) <= 1e-8
    f0, a0 = s.sumregs_vjp(u, x, np.zeros_like(u), reg=reg)
    assert not np.any(f0) and not np.any(a0)
    s.close()


def _methods(reg, x):
    """(name, adjoint_method, sr_force_lu, refine) of every factorisation that applies (sumregs_gradient_reg with an
    array parameter is row-scaled: only the two LU factorisations take it).  Refinement counts pinned as in
    test_gpu_sumregs_edges (forced LU on the symmetric system gains about one digit per sweep)."""
    if reg and np.ndim(x) == 3:
        return [("nd-lu", "nd", 0, 3), ("band-lu", "band", 0, 3)]
    return [("nd", "nd", 0, 3), ("nd-lu", "nd", 1, 3 if reg else 10), ("band-hbm", "band", 0, 3),
            ("band-lu", "band", 1, 3 if reg else 10)]


@pytest.mark.parametrize("reg", [0, 1])
@pytest.mark.parametrize("case", SMALL, ids=SMALL_IDS)
def test_sumregs_vjp_factorisations_agree(gpu_solver_cls, case, reg):
    """nd, nd-lu (forced), band-hbm and band-lu within 1e-9 of max|.| of each other; nd_staged = 0 and image groups
    (adjoint_budget_mb) bitwise; host and device forms, each output alone and a dtype-32 handle bitwise."""
    import os, re, subprocess
    import torch
    from conftest import ROOT
    O, N, M, kind = case
    _, _, x, u = _case(*case)
    gu = _cotangent(u, 7)
    s = gpu_solver_cls(M, N, O)
    res = {}
    for name, adj, flu, nref in _methods(reg, x):
        s.set_option("sr_force_lu", flu)
        res[name] = s.sumregs_vjp(u, x, gu, reg=reg, adjoint_method=adj, refine=nref)
        st = s.stats()
        assert st["adjoint_method"] == name and st["reg_gradient_used"] == reg, (name, st)
    s.set_option("sr_force_lu", 0)
    ref = next(iter(res.values()))
    tol = 1e-9   # measured on MI355X: at most 1.5e-15 (reg = 0) and 3.3e-12 (band-lu, reg = 1, map)
    for name, (gf, ga) in res.items():
        ef = np.abs(gf - ref[0]).max() / np.abs(ref[0]).max()
        ea = np.abs(np.asarray(ga) - ref[1]).max() / np.abs(ref[1]).max()
        print("factorisation %s vs nd, %s reg=%d: grad_f %.2e, grad_x %.2e" % (name, kind, reg, ef, ea))
        assert ef <= tol and ea <= tol, (name, ef, ea)
    gf, ga = s.sumregs_vjp(u, x, gu, reg=reg)
    assert s.stats()["adjoint_chunks"] == 1
    s.set_option("nd_staged", 0)
    assert all(_same(a, b) for a, b in zip(s.sumregs_vjp(u, x, gu, reg=reg), (gf, ga)))
    s.set_option("nd_staged", 1)
    assert _same(s.sumregs_vjp(u, x, gu, reg=reg, want_alpha=False)[0], gf)
    assert _same(s.sumregs_vjp(u, x, gu, reg=reg, want_f=False)[1], ga)
    dev = torch.device("cuda", 0)
    tu, tg = torch.from_numpy(u).to(dev), torch.from_numpy(gu).to(dev)
    ta = torch.from_numpy(np.ascontiguousarray(x).reshape(-1).copy()).to(dev)
    am, an = _amn(x)
    tf, tga = torch.empty_like(tu), torch.empty(3 * am * an, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    s.sumregs_vjp_device(tu.data_ptr(), ta.data_ptr(), am, an, tg.data_ptr(), tf.data_ptr(), tga.data_ptr(), reg=reg)
    assert _same(tf.cpu().numpy(), gf) and _same(tga.cpu().numpy(), np.ravel(ga))
    tf2, tga2 = torch.zeros_like(tu), torch.zeros_like(tga)
    s.sumregs_vjp_device(tu.data_ptr(), ta.data_ptr(), am, an, tg.data_ptr(), tf2.data_ptr(), None, reg=reg)
    s.sumregs_vjp_device(tu.data_ptr(), ta.data_ptr(), am, an, tg.data_ptr(), None, tga2.data_ptr(), reg=reg)
    assert _same(tf2.cpu().numpy(), gf) and _same(tga2.cpu().numpy(), np.ravel(ga))
    s.close()
    # image groups: a budget of 2.5 images' nested-dissection workspace (the LU variant's is larger: more groups)
    out = subprocess.run([os.path.join(ROOT, "tools", "_bin", "nd_host_check"), "bytes", str(M), str(N)],
                         capture_output=True, text=True, timeout=120).stdout
    per_image = float(re.search(r"bytes_per_image sr (\d+)", out).group(1))
    sg = gpu_solver_cls(M, N, O)
    sg.set_option("adjoint_budget_mb", 2.5 * per_image / 1e6)
    gfg, gag = sg.sumregs_vjp(u, x, gu, reg=reg)
    assert sg.stats()["adjoint_chunks"] > 1
    assert _same(gfg, gf) and _same(gag, ga)
    sg.close()
    s32 = gpu_solver_cls(M, N, O, dtype=32)
    g32f, g32a = s32.sumregs_vjp(u, x, gu, reg=reg)
    assert _same(g32f, gf) and _same(g32a, ga)
    s32.close()


def _snapshot(s):
    import torch
    buf = torch.empty(s.O * s.N * s.M, dtype=torch.float64, device="cuda")
    s.copy_u_device(buf.data_ptr())
    return buf.cpu().numpy(), s.duality_gap()


@pytest.mark.parametrize("kind", ["vector", "patch22", "map"])
def test_sumregs_vjp_leaves_the_last_solve_untouched(gpu_solver_cls, kind):
    """After a graph-replayed sumregs_denoise, VJPs at another parameter (host and device) leave u_device, the duality
    gap and the next sumregs_denoise of the old parameter bit for bit; a TV denoise on the same handle too."""
    import torch
    O, N, M = 3, 48, 40
    ub, f = synth_batch(O, N, M, seed=80)
    x, other = _alpha(kind, N, M), _alpha(kind, N, M, scale=3.0)
    s = gpu_solver_cls(M, N, O)
    s.set_data(ub, f)
    u0 = s.sumregs_denoise(x, maxiter=200)
    st0 = s.stats()
    assert st0["graph_used"] == 1
    snap = _snapshot(s)
    gu = _cotangent(u0, 9)
    for reg in (0, 1):
        s.sumregs_vjp(u0, other, gu, reg=reg)
    am, an = _amn(other)
    ta = torch.from_numpy(np.ascontiguousarray(other).reshape(-1).copy()).cuda()
    tu, tg = torch.from_numpy(u0).cuda(), torch.from_numpy(gu).cuda()
    tf = torch.empty_like(tu)
    torch.cuda.synchronize()
    for reg in (0, 1):
        s.sumregs_vjp_device(tu.data_ptr(), ta.data_ptr(), am, an, tg.data_ptr(), tf.data_ptr(), None, reg=reg)
    assert s.stats()["iterations"] == st0["iterations"]
    now = _snapshot(s)
    assert _same(now[0], snap[0]) and _same(now[1], snap[1])
    u1 = s.sumregs_denoise(x, maxiter=200)
    assert s.stats()["graph_used"] == 1 and _same(u1, u0)
    # the TV model on the same handle
    t0 = s.denoise(0.1, maxiter=200)
    tsnap = _snapshot(s)
    s.sumregs_vjp(u0, other, gu, reg=0)
    tnow = _snapshot(s)
    assert _same(tnow[0], tsnap[0]) and _same(tnow[1], tsnap[1])
    assert _same(s.denoise(0.1, maxiter=200), t0)
    s.close()


def test_sumregs_vjp_rejects_bad_input_and_changes_nothing(gpu_solver_cls):
    import torch
    from bpldenoising_amd._lib import BpltvError
    from bpldenoising_amd.learning_function import _ptr
    O, N, M = 3, 48, 40
    ub, f = synth_batch(O, N, M, seed=81)
    s = gpu_solver_cls(M, N, O)
    s.set_data(ub, f)
    u0 = s.sumregs_denoise(P22, maxiter=200)
    gu = _cotangent(u0, 10)
    ref = s.sumregs_vjp(u0, P22, gu, reg=1)
    snap = _snapshot(s)
    bad_gu, inf_gu = gu.copy(), gu.copy()
    bad_gu[1, 7, 5] = np.nan
    inf_gu[2, 0, 0] = -np.inf
    zero_patch = P22.copy()
    zero_patch[1, 0, 1] = 0.0
    big = np.full((3, N + 1, M), 0.03)
    calls = [(P22 * np.nan, gu, 0, E_ARG), (-P22, gu, 0, E_ARG), (P22 + np.inf, gu, 1, E_ARG), (P22, bad_gu, 0, E_ARG),
             (P22, inf_gu, 1, E_ARG), (zero_patch, gu, 1, E_ARG), (big, gu, 0, E_ARG),
             (A3 * np.nan, gu, 0, E_ARG), (-A3, gu, 1, E_ARG)]
    for x, g, reg, code in calls:
        with pytest.raises(BpltvError) as e:
            s.sumregs_vjp(u0, x, g, reg=reg)
        assert e.value.code == code, (reg, str(e.value))
    with pytest.raises(BpltvError) as e:
        s.sumregs_vjp(u0, P22, gu, adjoint_method="bcr")
    assert e.value.code == E_UNSUPPORTED
    # a zero entry is fine for sumregs_gradient (reg = 0) and for a vector parameter
    s.sumregs_vjp(u0, zero_patch, gu, reg=0)
    # device form: parameter and cotangent checked on the device
    tu, tg, tbad, tinf = (torch.from_numpy(a).cuda() for a in (u0, gu, bad_gu, inf_gu))
    tf = torch.empty_like(tu)
    for x, g, reg, code in ((-P22, tg, 0, E_ARG), (P22 * np.nan, tg, 1, E_ARG), (P22 + np.inf, tg, 0, E_ARG),
                            (P22, tbad, 0, E_ARG), (P22, tinf, 1, E_ARG), (zero_patch, tg, 1, E_ARG)):
        ta = torch.from_numpy(np.ascontiguousarray(x).reshape(-1).copy()).cuda()
        torch.cuda.synchronize()
        with pytest.raises(BpltvError) as e:
            s.sumregs_vjp_device(tu.data_ptr(), ta.data_ptr(), 2, 2, g.data_ptr(), tf.data_ptr(), None, reg=reg)
        assert e.value.code == code
    a = np.ascontiguousarray(P22)
    assert s._lib.bpltv_sumregs_vjp(s._h, _ptr(u0), _ptr(a), 2, 2, 0, None, _ptr(gu), None, None) == E_ARG
    ta = torch.from_numpy(a.reshape(-1).copy()).cuda()
    assert s._lib.bpltv_sumregs_vjp_device(s._h, tu.data_ptr(), ta.data_ptr(), 2, 2, 0, None, tg.data_ptr(), None,
                                           None) == E_ARG
    with pytest.raises(ValueError):
        s.sumregs_vjp(u0, P22, gu, want_f=False, want_alpha=False)
    now = _snapshot(s)
    assert _same(now[0], snap[0]) and _same(now[1], snap[1])
    again = s.sumregs_vjp(u0, P22, gu, reg=1)
    assert _same(again[0], ref[0]) and _same(again[1], ref[1])
    assert _same(s.sumregs_denoise(P22, maxiter=200), u0)
    s.close()


@pytest.mark.parametrize("kind", ["vector", "patch22", "map"])
def test_sumregs_vjp_on_shards_of_one_device(gpu_solver_cls, kind):
    """devices = [0, 0]: grad_f bitwise a single handle's, grad_x the shards' sum; the device form is refused."""
    import torch
    from bpldenoising_amd._lib import BpltvError
    case = (3, 48, 40, kind)
    O, N, M, _ = case
    _, _, x, u = _case(*case)
    gu = _cotangent(u, 11)
    s = gpu_solver_cls(M, N, O)
    m = gpu_solver_cls(M, N, O, devices=[0, 0])
    rtol = 1e-12 if kind == "map" else 1e-13
    for reg in (0, 1):
        gf, ga = s.sumregs_vjp(u, x, gu, reg=reg)
        mf, ma = m.sumregs_vjp(u, x, gu, reg=reg)
        assert _same(mf, gf)
        assert np.shape(ma) == np.shape(ga) and np.allclose(ma, ga, rtol=rtol, atol=0)
        assert m.stats()["shards"] == 2
        assert _same(m.sumregs_vjp(u, x, gu, reg=reg, want_alpha=False)[0], gf)
        tu = torch.from_numpy(u).cuda()
        tf = torch.empty_like(tu)
        ta = torch.from_numpy(np.ascontiguousarray(x).reshape(-1).copy()).cuda()
        am, an = _amn(x)
        torch.cuda.synchronize()
        with pytest.raises(BpltvError) as e:
            m.sumregs_vjp_device(tu.data_ptr(), ta.data_ptr(), am, an, tu.data_ptr(), tf.data_ptr(), None, reg=reg)
        assert e.value.code == E_UNSUPPORTED
        with pytest.raises(BpltvError) as e:
            m.sumregs_denoise_device(ta.data_ptr(), am, an, maxiter=50)
        assert e.value.code == E_UNSUPPORTED
    m.close()
    s.close()


@pytest.mark.parametrize("kind", ["vector", "patch22", "map"])
def test_sumregs_denoise_device(gpu_solver_cls, kind):
    """bitwise sumregs_denoise with the parameter in HBM, the graph replayed; a rejected device parameter (NaN,
    negative, rho != 0 with a zero entry) leaves u, the gap and the next solve as they were."""
    import torch
    from bpldenoising_amd._lib import BpltvError
    O, N, M = 3, 48, 40
    ub, f = synth_batch(O, N, M, seed=82)
    x = _alpha(kind, N, M)
    am, an = _amn(x)
    s = gpu_solver_cls(M, N, O)
    s.set_data(ub, f)
    u0 = s.sumregs_denoise(x, maxiter=200)
    ta = torch.from_numpy(np.ascontiguousarray(x).reshape(-1).copy()).cuda()
    torch.cuda.synchronize()
    s.sumregs_denoise_device(ta.data_ptr(), am, an, maxiter=200)
    assert s.stats()["graph_used"] == 1
    u1, gap1 = _snapshot(s)
    assert _same(u1, u0.ravel())
    s.sumregs_denoise_device(ta.data_ptr(), am, an, maxiter=200)
    assert s.stats()["graph_used"] == 1 and _same(_snapshot(s)[0], u1)
    bad = [x * np.nan, -x]
    z = np.ascontiguousarray(x).copy()
    z.reshape(-1)[1] = 0.0
    for b, kw in [(bad[0], {}), (bad[1], {}), (z, {"rho": 0.5})]:
        tb = torch.from_numpy(np.ascontiguousarray(b).reshape(-1).copy()).cuda()
        torch.cuda.synchronize()
        with pytest.raises(BpltvError) as e:
            s.sumregs_denoise_device(tb.data_ptr(), am, an, maxiter=200, **kw)
        assert e.value.code == E_ARG
        now = _snapshot(s)
        assert _same(now[0], u1) and _same(now[1], gap1)
    assert _same(s.sumregs_denoise(x, maxiter=200), u0)
    s.close()
