"""GPU checks of the Jacobian-vector product of u = denoise(f, alpha) (bpltv_jvp / bpltv_jvp_device).

The JVP is the linear map whose transpose bpltv_vjp computes: <gu, jvp(df, dalpha)> = <grad_f(gu), df> +
<grad_alpha(gu), dalpha>.  It is checked against the library's own VJP by that identity, against the CPU reference of
tests/jvp_ref.py (numpy right-hand side + the oracle's solve; pinned by tests/test_jvp_abi.py), for linearity, for the
bitwise agreement of its forms, and against central differences of long solves.  Cases: those of test_gpu_vjp.py."""
import numpy as np
import pytest
from conftest import synth_batch

import jvp_ref
from test_gpu_vjp import CASES, IDS, P22, _alpha, _case, _nd_bytes_per_image, _same, _snapshot

pytestmark = pytest.mark.gpu

E_ARG, E_UNSUPPORTED = 1, 6


def _tangents(u, alpha, seed, K=None):
    """(df, dalpha): random directions; with K a leading direction axis."""
    rng = np.random.default_rng(seed)
    lead = () if K is None else (K,)
    df = rng.standard_normal(lead + u.shape)
    da = rng.standard_normal(lead + np.shape(alpha))
    return df, (float(da) if da.ndim == 0 else da)


def _dot(a, b):
    return float(np.sum(np.asarray(a) * np.asarray(b)))


def _dev_shape(alpha):
    a = np.asarray(alpha, dtype=np.float64)
    return (1, 1) if a.ndim == 0 else (a.shape[1], a.shape[0])


@pytest.mark.parametrize("reg", [0, 1])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_jvp_is_the_transpose_of_the_vjp(gpu_solver_cls, case, reg):
    """|lhs - rhs| <= 1e-6 (|<gf,df>| + |<ga,dalpha>|): 1e-6 is the rtol between the library's adjoint and the oracle."""
    O, N, M, kind = case
    _, _, alpha, u = _case(*case)
    df, da = _tangents(u, alpha, 21)
    gu = np.random.default_rng(22).standard_normal(u.shape)
    s = gpu_solver_cls(M, N, O)
    du = s.jvp(u, alpha, df=df, dalpha=da, reg=reg)
    st = s.stats()
    assert du.shape == u.shape and np.all(np.isfinite(du))
    assert st["reg_gradient_used"] == reg and st["adjoint_residual"] <= 1e-6 and st["adjoint_ms"] > 0, st
    gf, ga = s.vjp(u, alpha, gu, reg=reg)
    s.close()
    lhs, t1, t2 = _dot(gu, du), _dot(gf, df), _dot(ga, da)
    print("%s reg %d: lhs %.15g rhs %.15g rel %.3e" % (kind, reg, lhs, t1 + t2, abs(lhs - t1 - t2) / (abs(t1) + abs(t2))))
    assert abs(lhs - (t1 + t2)) <= 1e-6 * (abs(t1) + abs(t2))


@pytest.mark.parametrize("reg", [0, 1])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_jvp_matches_the_cpu_reference(gpu_solver_cls, oracle, case, reg):
    """du image by image against tests/jvp_ref.py: both tangents, and each alone."""
    O, N, M, kind = case
    _, _, alpha, u = _case(*case)
    df, da = _tangents(u, alpha, 23)
    s = gpu_solver_cls(M, N, O)
    got = {"both": s.jvp(u, alpha, df=df, dalpha=da, reg=reg), "df": s.jvp(u, alpha, df=df, reg=reg),
           "dalpha": s.jvp(u, alpha, dalpha=da, reg=reg)}
    s.close()
    for k in range(O):
        want = {"both": jvp_ref.jvp_image(oracle, u[k], alpha, df[k], da, reg),
                "df": jvp_ref.jvp_image(oracle, u[k], alpha, df[k], None, reg),
                "dalpha": jvp_ref.jvp_image(oracle, u[k], alpha, None, da, reg)}
        for name, w in want.items():
            err = np.abs(got[name][k] - w).max() / np.abs(w).max()
            if k == 0:
                print("%s reg %d %s: max err / max|du| %.3e" % (kind, reg, name, err))
            assert np.allclose(got[name][k], w, rtol=1e-6, atol=1e-8 * np.abs(w).max()), (k, name, err)


@pytest.mark.parametrize("reg", [0, 1])
@pytest.mark.parametrize("case", CASES[1:], ids=IDS[1:])
def test_jvp_is_linear_and_zero_at_zero(gpu_solver_cls, case, reg):
    O, N, M, kind = case
    _, _, alpha, u = _case(*case)
    (f1, a1), (f2, a2) = _tangents(u, alpha, 25), _tangents(u, alpha, 26)
    s = gpu_solver_cls(M, N, O)
    rel = lambda x, y: np.linalg.norm(np.ravel(x) - np.ravel(y)) / np.linalg.norm(np.ravel(y))
    d1 = s.jvp(u, alpha, df=f1, dalpha=a1, reg=reg)
    d2 = s.jvp(u, alpha, df=f2, dalpha=a2, reg=reg)
    assert rel(d1, s.jvp(u, alpha, df=f1, reg=reg) + s.jvp(u, alpha, dalpha=a1, reg=reg)) <= 1e-8
    d3 = s.jvp(u, alpha, df=2.0 * f1 - 0.5 * f2, dalpha=2.0 * np.asarray(a1) - 0.5 * np.asarray(a2), reg=reg)
    assert rel(d3, 2.0 * d1 - 0.5 * d2) <= 1e-8
    z, za = np.zeros_like(u), np.zeros(np.shape(alpha))
    assert not np.any(s.jvp(u, alpha, df=z, dalpha=za if za.ndim else 0.0, reg=reg))
    assert not np.any(s.jvp(u, alpha, df=z, reg=reg))
    assert not np.any(s.jvp(u, alpha, dalpha=za if za.ndim else 0.0, reg=reg))
    s.close()


@pytest.mark.parametrize("reg", [0, 1])
@pytest.mark.parametrize("case", CASES[1:], ids=IDS[1:])
def test_jvp_variants_agree_bitwise(gpu_solver_cls, case, reg):
    """Direction d of an ndir = K call against the ndir = 1 call, host against device form, one image group against
    several, a dtype-32 handle against a dtype-64 one."""
    import torch
    O, N, M, kind = case
    _, _, alpha, u = _case(*case)
    K = 3
    df, da = _tangents(u, alpha, 27, K=K)
    s = gpu_solver_cls(M, N, O)
    du = s.jvp(u, alpha, df=df, dalpha=da, reg=reg)
    assert du.shape == (K,) + u.shape and s.stats()["adjoint_chunks"] == 1
    for d in range(K):
        one = s.jvp(u, alpha, df=df[d], dalpha=da[d], reg=reg)
        assert one.shape == u.shape and _same(one, du[d]), d
    assert _same(s.jvp(u, alpha, df=df, reg=reg)[1], s.jvp(u, alpha, df=df[1], reg=reg))
    assert _same(s.jvp(u, alpha, dalpha=da, reg=reg)[2], s.jvp(u, alpha, dalpha=da[2], reg=reg))
    # device form
    dev = torch.device("cuda", 0)
    am, an = _dev_shape(alpha)
    tu = torch.from_numpy(u).to(dev)
    ta = torch.from_numpy(np.asarray(alpha, dtype=np.float64).reshape(-1).copy()).to(dev)
    tdf, tda = torch.from_numpy(df).to(dev), torch.from_numpy(np.ascontiguousarray(da)).to(dev)
    tdu = torch.zeros(K, *u.shape, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    s.jvp_device(tu.data_ptr(), ta.data_ptr(), am, an, tdf.data_ptr(), tda.data_ptr(), tdu.data_ptr(), ndir=K, reg=reg)
    assert _same(tdu.cpu().numpy(), du)
    tdu1 = torch.zeros_like(tu)
    s.jvp_device(tu.data_ptr(), ta.data_ptr(), am, an, tdf[1].data_ptr(), None, tdu1.data_ptr(), reg=reg)
    assert _same(tdu1.cpu().numpy(), s.jvp(u, alpha, df=df[1], reg=reg))
    s.jvp_device(tu.data_ptr(), ta.data_ptr(), am, an, None, tda[2].data_ptr(), tdu1.data_ptr(), reg=reg)
    assert _same(tdu1.cpu().numpy(), s.jvp(u, alpha, dalpha=da[2], reg=reg))
    s.close()
    # image groups: a budget of two images' nested-dissection workspace
    sg = gpu_solver_cls(M, N, O)
    sg.jvp(u, alpha, df=df[0], reg=reg)
    sg.set_option("adjoint_budget_mb", 2.5 * _nd_bytes_per_image(M, N) / 1e6)
    dug = sg.jvp(u, alpha, df=df, dalpha=da, reg=reg)
    assert sg.stats()["adjoint_chunks"] > 1 and _same(dug, du)
    sg.close()
    s32 = gpu_solver_cls(M, N, O, dtype=32)
    assert _same(s32.jvp(u, alpha, df=df, dalpha=da, reg=reg), du)
    s32.close()


@pytest.mark.parametrize("kind", ["scalar", "patch22", "map"])
def test_jvp_on_shards_of_one_device(gpu_solver_cls, kind):
    """bpltv_create_sharded with a repeated device: du bitwise a single handle's; the device form is refused."""
    import torch
    from bpldenoising_amd._lib import BpltvError
    case = (3, 48, 40, kind)
    O, N, M, _ = case
    _, _, alpha, u = _case(*case)
    df, da = _tangents(u, alpha, 29, K=2)
    s = gpu_solver_cls(M, N, O)
    am, an = _dev_shape(alpha)
    for reg in (0, 1):
        du = s.jvp(u, alpha, df=df, dalpha=da, reg=reg)
        m = gpu_solver_cls(M, N, O, devices=[0, 0])
        assert _same(m.jvp(u, alpha, df=df, dalpha=da, reg=reg), du)
        assert m.stats()["shards"] == 2
        assert _same(m.jvp(u, alpha, dalpha=da[1], reg=reg), s.jvp(u, alpha, dalpha=da[1], reg=reg))
        tu = torch.from_numpy(u).cuda()
        ta = torch.from_numpy(np.asarray(alpha, dtype=np.float64).reshape(-1).copy()).cuda()
        tdu = torch.empty_like(tu)
        torch.cuda.synchronize()
        with pytest.raises(BpltvError) as e:
            m.jvp_device(tu.data_ptr(), ta.data_ptr(), am, an, tu.data_ptr(), None, tdu.data_ptr(), reg=reg)
        assert e.value.code == E_UNSUPPORTED
        m.close()
    s.close()


@pytest.mark.parametrize("kind", ["scalar", "patch22", "map"])
def test_jvp_leaves_the_last_solve_untouched(gpu_solver_cls, kind):
    import torch
    O, N, M = 3, 48, 40
    ub, f = synth_batch(O, N, M, seed=50)
    alpha, other = _alpha(kind, N, M), _alpha(kind, N, M, scale=3.0)
    s = gpu_solver_cls(M, N, O)
    s.set_data(ub, f)
    u0 = s.denoise(alpha, maxiter=200)
    assert s.stats()["graph_used"] == 1
    snap_u, snap_gap = _snapshot(s)
    df, da = _tangents(u0, other, 31, K=2)
    for reg in (0, 1):
        s.jvp(u0, other, df=df, dalpha=da, reg=reg)
    am, an = _dev_shape(other)
    ta = torch.from_numpy(np.asarray(other, dtype=np.float64).reshape(-1).copy()).cuda()
    tu, tdf = torch.from_numpy(u0).cuda(), torch.from_numpy(df[0]).cuda()
    tdu = torch.empty_like(tu)
    torch.cuda.synchronize()
    s.jvp_device(tu.data_ptr(), ta.data_ptr(), am, an, tdf.data_ptr(), None, tdu.data_ptr())
    u_now, gap_now = _snapshot(s)
    assert _same(u_now, snap_u) and _same(gap_now, snap_gap)
    u1 = s.denoise(alpha, maxiter=200)
    assert s.stats()["graph_used"] == 1 and _same(u1, u0)
    s.close()


def test_jvp_rejects_bad_input_and_changes_nothing(gpu_solver_cls):
    import torch
    from bpldenoising_amd._lib import BpltvError
    from bpldenoising_amd.learning_function import _ptr
    O, N, M = 3, 48, 40
    ub, f = synth_batch(O, N, M, seed=51)
    s = gpu_solver_cls(M, N, O)
    s.set_data(ub, f)
    u0 = s.denoise(P22, maxiter=200)
    df, da = _tangents(u0, P22, 33)
    ref = s.jvp(u0, P22, df=df, dalpha=da)
    snap = _snapshot(s)
    bad_df = df.copy()
    bad_df[1, 7, 5] = np.nan
    bad_da = da.copy()
    bad_da[1, 0] = np.inf
    zero_patch = P22.copy()
    zero_patch[0, 1] = 0.0
    calls = [(P22 * np.nan, df, da, 0), (-P22, df, da, 0), (P22, bad_df, da, 0), (P22, bad_df, None, 1),
             (P22, df, bad_da, 1), (P22, None, bad_da, 0), (zero_patch, df, da, 1), (-0.1, df, None, 0),
             (float("nan"), df, None, 1)]
    for alpha, tf, tda, reg in calls:
        with pytest.raises(BpltvError) as e:
            s.jvp(u0, alpha, df=tf, dalpha=tda, reg=reg)
        assert e.value.code == E_ARG, (alpha, reg, str(e.value))
    # ndir = 0, and both tangents NULL
    a = np.ascontiguousarray(P22)
    du = np.empty_like(u0)
    assert s._lib.bpltv_jvp(s._h, _ptr(u0), _ptr(a), 2, 2, 0, None, 0, _ptr(df), _ptr(da), _ptr(du)) == E_ARG
    assert s._lib.bpltv_jvp(s._h, _ptr(u0), _ptr(a), 2, 2, 0, None, 1, None, None, _ptr(du)) == E_ARG
    with pytest.raises(ValueError):
        s.jvp(u0, P22)
    # device form: parameter and tangents checked on the device
    tu, tdf, tbad = (torch.from_numpy(x).cuda() for x in (u0, df, bad_df))
    tda, tbad_da = torch.from_numpy(da).cuda(), torch.from_numpy(bad_da).cuda()
    tdu = torch.empty_like(tu)
    for al, tf_, ta_ in ((-P22, tdf, tda), (P22 * np.nan, tdf, tda), (P22, tbad, tda), (P22, tdf, tbad_da)):
        tal = torch.from_numpy(np.ascontiguousarray(al).reshape(-1)).cuda()
        torch.cuda.synchronize()
        with pytest.raises(BpltvError) as e:
            s.jvp_device(tu.data_ptr(), tal.data_ptr(), 2, 2, tf_.data_ptr(), ta_.data_ptr(), tdu.data_ptr())
        assert e.value.code == E_ARG
    tal = torch.from_numpy(a.reshape(-1)).cuda()
    torch.cuda.synchronize()
    for ndir, p1, p2 in ((0, tdf.data_ptr(), tda.data_ptr()), (1, None, None)):
        with pytest.raises(BpltvError) as e:
            s.jvp_device(tu.data_ptr(), tal.data_ptr(), 2, 2, p1, p2, tdu.data_ptr(), ndir=ndir)
        assert e.value.code == E_ARG
    now = _snapshot(s)
    assert _same(now[0], snap[0]) and _same(now[1], snap[1])
    assert _same(s.jvp(u0, P22, df=df, dalpha=da), ref)
    assert _same(s.denoise(P22, maxiter=200), u0)
    s.close()


def test_jvp_against_central_differences(gpu_solver_cls):
    """One 24 x 24 image, scalar alpha = 0.08, 20000-iteration solves, eps = 1e-4.

    On this very input the CPU reference (tests/jvp_ref.py on the oracle's solves) is 1.71e-4 (dalpha, reg 0 and 1) and
    1.18e-4 (df) in relative L2 from the same central differences of the oracle's 20000-iteration solves; the bound
    is 10 times that, because the active set (225 of 576 pixels here) moves with eps -- test_finite_difference's note."""
    O, N, M = 1, 24, 24
    ub, f = synth_batch(O, N, M, seed=63)
    a, eps, it = 0.08, 1e-4, 20000
    df = np.random.default_rng(64).standard_normal((O, N, M))
    s = gpu_solver_cls(M, N, O)
    s.set_data(ub, f)
    u = s.denoise(a, maxiter=it)
    fd_a = (s.denoise(a + eps, maxiter=it) - s.denoise(a - eps, maxiter=it)) / (2 * eps)
    s.set_data(ub, f + eps * df)
    up = s.denoise(a, maxiter=it)
    s.set_data(ub, f - eps * df)
    fd_f = (up - s.denoise(a, maxiter=it)) / (2 * eps)
    rel = lambda x, y: np.linalg.norm(x - y) / np.linalg.norm(y)
    for reg in (0, 1):
        ea, ef = rel(s.jvp(u, a, dalpha=1.0, reg=reg), fd_a), rel(s.jvp(u, a, df=df, reg=reg), fd_f)
        print("reg %d: dalpha %.3e (bound 1.71e-3), df %.3e (bound 1.18e-3)" % (reg, ea, ef))
        assert ea <= 10 * 1.71e-4 and ef <= 10 * 1.18e-4
    s.close()


def test_jvp_config5_share_8x1024_pixel_map(gpu_solver_cls):
    """8 x 1024^2 with a pixel-map parameter: the transpose identity against bpltv_vjp at the largest shape."""
    O, N, M = 8, 1024, 1024
    ub, f = synth_batch(O, N, M, seed=52)
    amap = 0.05 + 0.1 * np.random.default_rng(12).random((N, M))
    s = gpu_solver_cls(M, N, O)
    s.set_data(ub, f)
    u = s.denoise(amap, maxiter=200)
    df, da = _tangents(u, amap, 35)
    du = s.jvp(u, amap, df=df, dalpha=da)
    st = s.stats()
    assert np.all(np.isfinite(du)) and st["adjoint_residual"] <= 1e-6, st
    gu = np.random.default_rng(36).standard_normal(u.shape)
    gf, ga = s.vjp(u, amap, gu)
    s.close()
    lhs, t1, t2 = _dot(gu, du), _dot(gf, df), _dot(ga, da)
    assert abs(lhs - (t1 + t2)) <= 1e-6 * (abs(t1) + abs(t2))
