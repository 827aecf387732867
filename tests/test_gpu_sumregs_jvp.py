"""GPU checks of the Jacobian-vector product of u = sumregs_denoise(f, x) (bpltv_sumregs_jvp / _device).

The JVP is the linear map whose transpose bpltv_sumregs_vjp computes: <gu, jvp(df, dx)> = <grad_f(gu), df> +
<grad_x(gu), dx>.  It is checked against the library's own VJP by that identity, against the CPU reference of
tests/sumregs_jvp_ref.py (numpy right-hand side, scipy's LU of the transposed reduced system; pinned by
tests/test_sumregs_jvp_abi.py), through every factorisation -- sumregs_gradient_reg with an array parameter has a
row-scaled, non-symmetric system, and the test tells A^-T from A^-1 there --, at the edge shapes, for linearity, and for
the bitwise agreement of its forms.  Cases: those of test_gpu_sumregs_vjp.py."""
import os
import re
import subprocess

import numpy as np
import pytest
from conftest import ROOT, synth_batch

import sumregs_jvp_ref as ref
from test_gpu_sumregs_edges import REFINE, REFINE_FORCED_LU
from test_gpu_sumregs_edges import _methods as _edge_methods
from test_gpu_sumregs_vjp import A3, CASES, IDS, P22, SMALL, SMALL_IDS, _alpha, _amn, _case, _methods, _same, _snapshot
from test_oracle_sumregs import EDGE_LITERAL_SINGULAR, EDGE_MAXITER, EDGE_SHAPES, edge_case

pytestmark = pytest.mark.gpu

E_ARG, E_UNSUPPORTED = 1, 6
# a 2 x 2 patch whose three slices differ strongly: on the row-scaled system A^-1 r and A^-T r are then far apart
P22_SKEW = P22 * np.array([1.0, 1.0, 5.0])[:, None, None]


def _tangents(u, x, seed, K=None):
    rng = np.random.default_rng(seed)
    lead = () if K is None else (K,)
    return rng.standard_normal(lead + u.shape), rng.standard_normal(lead + np.shape(x))


def _dot(a, b):
    return float(np.sum(np.asarray(a) * np.asarray(b)))


def _close_to_reference(got, want, reg):
    """The project's library-to-oracle bounds: rtol 1e-6 with atol 1e-8 max|du| (reg = 0), 1e-7 of max|du| (reg = 1)."""
    scale = np.abs(want).max()
    err = np.abs(got - want).max() / scale if scale > 0 else np.abs(got).max()
    ok = np.abs(got - want).max() <= 1e-7 * scale if reg else np.allclose(got, want, rtol=1e-6, atol=1e-8 * scale)
    return ok, err


@pytest.mark.parametrize("reg", [0, 1])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_sumregs_jvp_is_the_transpose_of_the_vjp(gpu_solver_cls, case, reg):
    """|lhs - rhs| <= 1e-6 (|<gf,df>| + |<ga,dx>|): 1e-6 is the rtol between the library's adjoint and the oracle.
    Measured on MI355X: at most 2.7e-15 on the symmetric systems, 7.7e-12 on the row-scaled one (map, reg = 1)."""
    O, N, M, kind = case
    _, _, x, u = _case(*case)
    df, dx = _tangents(u, x, 21)
    gu = np.random.default_rng(22).standard_normal(u.shape)
    s = gpu_solver_cls(M, N, O)
    du = s.sumregs_jvp(u, x, df=df, dalpha=dx, reg=reg)
    st = s.stats()
    assert du.shape == u.shape and np.all(np.isfinite(du))
    assert st["reg_gradient_used"] == reg and st["adjoint_residual"] <= 1e-6 and st["adjoint_ms"] > 0, st
    gf, ga = s.sumregs_vjp(u, x, gu, reg=reg)
    assert s.stats()["adjoint_method"] == st["adjoint_method"]
    s.close()
    lhs, t1, t2 = _dot(gu, du), _dot(gf, df), _dot(ga, dx)
    print("%s reg %d: lhs %.15g rhs %.15g rel %.3e" % (kind, reg, lhs, t1 + t2, abs(lhs - t1 - t2) / (abs(t1) + abs(t2))))
    assert abs(lhs - (t1 + t2)) <= 1e-6 * (abs(t1) + abs(t2))


@pytest.mark.parametrize("reg", [0, 1])
@pytest.mark.parametrize("case", SMALL, ids=SMALL_IDS)
def test_sumregs_jvp_matches_the_cpu_reference(gpu_solver_cls, case, reg):
    """du image by image against tests/sumregs_jvp_ref.py: both tangents, and each alone.  Measured on MI355X, of max|du|:
    at most 2.8e-8 for reg = 0 (2 x 2 patch) and 3.5e-9 for reg = 1 (3 x 5 patch)."""
    O, N, M, kind = case
    _, _, x, u = _case(*case)
    df, dx = _tangents(u, x, 23)
    s = gpu_solver_cls(M, N, O)
    got = {"both": s.sumregs_jvp(u, x, df=df, dalpha=dx, reg=reg), "df": s.sumregs_jvp(u, x, df=df, reg=reg),
           "dx": s.sumregs_jvp(u, x, dalpha=dx, reg=reg)}
    s.close()
    for k in range(O):
        lu = ref.factor(u[k], x, reg)
        want = {"both": ref.jvp_image(u[k], x, df[k], dx, reg, lu=lu), "df": ref.jvp_image(u[k], x, df[k], None, reg, lu=lu),
                "dx": ref.jvp_image(u[k], x, None, dx, reg, lu=lu)}
        for name, w in want.items():
            ok, err = _close_to_reference(got[name][k], w, reg)
            print("%s reg %d image %d %s: max err / max|du| %.3e" % (kind, reg, k, name, err))
            assert ok, (k, name, err)


@pytest.mark.parametrize("reg", [0, 1])
@pytest.mark.parametrize("case", SMALL, ids=SMALL_IDS)
def test_sumregs_jvp_every_factorisation_on_one_handle(gpu_solver_cls, case, reg):
    """nd, nd-lu (forced on the symmetric systems, genuine on the row-scaled one), band-hbm and band-lu on one handle:
    within 1e-9 (reg = 1) / 1e-6 (reg = 0) of max|du| of each other.  In forward mode the LU paths factor the transposed
    planes, so the forced-LU results on the symmetric systems cross-check the plane swap against Cholesky, and the
    row-scaled case (2 x 2 patch with its third slice scaled by 5) is told apart from an untransposed factor: A^-1 r,
    from the reference, is far from the result, and A^-T r is at it."""
    O, N, M, kind = case
    _, _, x, u = _case(*case)
    if kind == "patch22":
        x = P22_SKEW
    df, dx = _tangents(u, x, 24)
    s = gpu_solver_cls(M, N, O)
    res = {}
    for name, adj, flu, nref in _methods(reg, x):
        s.set_option("sr_force_lu", flu)
        res[name] = s.sumregs_jvp(u, x, df=df, dalpha=dx, reg=reg, adjoint_method=adj, refine=nref)
        st = s.stats()
        assert st["adjoint_method"] == name and st["reg_gradient_used"] == reg, (name, st)
        assert st["adjoint_residual"] <= 1e-6, (name, st["adjoint_residual"])
    s.set_option("sr_force_lu", 0)
    s.close()
    first = next(iter(res.values()))
    scale = np.abs(first).max()
    tol = 1e-9 if reg else 1e-6
    for name, du in res.items():
        e = np.abs(du - first).max() / scale
        print("factorisation %s, %s reg=%d: %.2e of max|du| from %s" % (name, kind, reg, e, next(iter(res))))
        assert e <= tol, (name, e)
    if reg and np.ndim(x) == 3:   # row-scaled: the transposed solve, not the VJP's
        for k in range(O):
            right = ref.jvp_image(u[k], x, df[k], dx, reg)
            wrong = ref.jvp_image(u[k], x, df[k], dx, reg, transposed=False)
            gap = np.abs(right - wrong).max() / np.abs(right).max()
            print("%s image %d: |A^-T r - A^-1 r| = %.2e of max|du|" % (kind, k, gap))
            assert gap > 1e3 * 1e-7
            for name, du in res.items():
                assert np.abs(du[k] - wrong).max() > 0.5 * gap * np.abs(right).max(), name
                assert np.abs(du[k] - right).max() <= 1e-7 * np.abs(right).max(), name


@pytest.mark.parametrize("shape", EDGE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_sumregs_jvp_at_edge_shapes(gpu_solver_cls, shape):
    """1 x 9 ... 3 x 3: the boundary branches of the three stencils and the coinciding band offsets for M <= 3, every
    factorisation that applies, refine = 3 (10 for LU forced on the symmetric kappa system), against the CPU reference.
    The case whose literal system is singular must match or fail with a clean BpltvError; on 1 x 1, du == df.

    The reference here is sumregs_jvp_ref.jvp_image_small: scipy's LU where cond(A) eps <= 1e-8, the same system in
    rational arithmetic where not.  On (2, 1, 9) map, (1, 2, 2) map and (2, 5, 3) vector with reg = 0 the active elements
    (kappa = 1e14) connect most of the image, cond(A) is 2e14 to 6e14 and scipy's LU of the assembled double matrix is
    5.8e-3, 2.7e-3 and 6.5e-3 of max|du| away from the exact solution; the library is within 5.6e-8, 1.2e-7 and 1.7e-10
    of it there (MI355X, nested dissection), its four factorisations agreeing among themselves as everywhere else."""
    from bpldenoising_amd._lib import BpltvError
    O, N, M = shape
    for kind in ("vector", "patch", "map"):
        ub, f, x = edge_case(shape, kind)
        s = gpu_solver_cls(M, N, O)
        s.set_data(ub, f)
        u = s.sumregs_denoise(x, maxiter=EDGE_MAXITER)
        df, dx = _tangents(u, x, 40 + N + M)
        for reg in (0, 1):
            want = None
            for name, adj, flu in _edge_methods(bool(reg), x, N * M):
                s.set_option("sr_force_lu", flu)
                nref = REFINE_FORCED_LU if (flu and not reg) else REFINE
                try:
                    du = s.sumregs_jvp(u, x, df=df, dalpha=dx, reg=reg, adjoint_method=adj, refine=nref)
                except BpltvError as e:
                    assert (shape, kind, bool(reg)) in EDGE_LITERAL_SINGULAR and e.code != 0 and str(e), (name, str(e))
                    continue
                assert s.stats()["adjoint_method"] == name and np.all(np.isfinite(du)), name
                if N * M == 1:
                    assert _same(du, df), (kind, reg)
                    continue
                if want is None:
                    want = np.stack([ref.jvp_image_small(u[k], x, df[k], dx, reg) for k in range(O)])
                ok, err = _close_to_reference(du, want, reg)
                print("%s %s reg %d %s: %.3e of max|du|" % ("x".join(map(str, shape)), kind, reg, name, err))
                assert ok, (kind, reg, name, err)
            s.set_option("sr_force_lu", 0)
        s.close()


@pytest.mark.parametrize("reg", [0, 1])
@pytest.mark.parametrize("case", SMALL, ids=SMALL_IDS)
def test_sumregs_jvp_is_linear_and_zero_at_zero(gpu_solver_cls, case, reg):
    O, N, M, kind = case
    _, _, x, u = _case(*case)
    (f1, a1), (f2, a2) = _tangents(u, x, 25), _tangents(u, x, 26)
    s = gpu_solver_cls(M, N, O)
    rel = lambda p, q: np.linalg.norm(np.ravel(p) - np.ravel(q)) / np.linalg.norm(np.ravel(q))
    d1 = s.sumregs_jvp(u, x, df=f1, dalpha=a1, reg=reg)
    d2 = s.sumregs_jvp(u, x, df=f2, dalpha=a2, reg=reg)
    only_f, only_a = s.sumregs_jvp(u, x, df=f1, reg=reg), s.sumregs_jvp(u, x, dalpha=a1, reg=reg)
    assert rel(d1, only_f + only_a) <= 1e-8
    assert rel(s.sumregs_jvp(u, x, df=2.0 * f1 - 0.5 * f2, dalpha=2.0 * a1 - 0.5 * a2, reg=reg), 2.0 * d1 - 0.5 * d2) <= 1e-8
    z, za = np.zeros_like(u), np.zeros(np.shape(x))
    assert not np.any(s.sumregs_jvp(u, x, df=z, dalpha=za, reg=reg))
    assert not np.any(s.sumregs_jvp(u, x, df=z, reg=reg)) and not np.any(s.sumregs_jvp(u, x, dalpha=za, reg=reg))
    # a NULL tangent is a zero tangent
    assert _same(s.sumregs_jvp(u, x, df=f1, dalpha=za, reg=reg), only_f)
    assert _same(s.sumregs_jvp(u, x, df=z, dalpha=a1, reg=reg), only_a)
    s.close()


def _sr_bytes_per_image(M, N):
    out = subprocess.run([os.path.join(ROOT, "tools", "_bin", "nd_host_check"), "bytes", str(M), str(N)],
                         capture_output=True, text=True, timeout=120).stdout
    return float(re.search(r"bytes_per_image sr (\d+)", out).group(1))


@pytest.mark.parametrize("reg", [0, 1])
@pytest.mark.parametrize("case", SMALL, ids=SMALL_IDS)
def test_sumregs_jvp_variants_agree_bitwise(gpu_solver_cls, case, reg):
    """Direction d of an ndir = 4 call against the ndir = 1 call, host against device form, one image group against
    several, a dtype-32 handle against a dtype-64 one."""
    import torch
    O, N, M, kind = case
    _, _, x, u = _case(*case)
    K = 4
    df, dx = _tangents(u, x, 27, K=K)
    s = gpu_solver_cls(M, N, O)
    du = s.sumregs_jvp(u, x, df=df, dalpha=dx, reg=reg)
    assert du.shape == (K,) + u.shape and s.stats()["adjoint_chunks"] == 1
    for d in range(K):
        one = s.sumregs_jvp(u, x, df=df[d], dalpha=dx[d], reg=reg)
        assert one.shape == u.shape and _same(one, du[d]), d
    assert _same(s.sumregs_jvp(u, x, df=df, reg=reg)[1], s.sumregs_jvp(u, x, df=df[1], reg=reg))
    assert _same(s.sumregs_jvp(u, x, dalpha=dx, reg=reg)[2], s.sumregs_jvp(u, x, dalpha=dx[2], reg=reg))
    dev = torch.device("cuda", 0)
    am, an = _amn(x)
    tu = torch.from_numpy(u).to(dev)
    ta = torch.from_numpy(np.ascontiguousarray(x).reshape(-1).copy()).to(dev)
    tdf, tdx = torch.from_numpy(df).to(dev), torch.from_numpy(np.ascontiguousarray(dx)).to(dev)
    tdu = torch.zeros(K, *u.shape, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    s.sumregs_jvp_device(tu.data_ptr(), ta.data_ptr(), am, an, tdf.data_ptr(), tdx.data_ptr(), tdu.data_ptr(), ndir=K, reg=reg)
    assert _same(tdu.cpu().numpy(), du)
    tdu1 = torch.zeros_like(tu)
    s.sumregs_jvp_device(tu.data_ptr(), ta.data_ptr(), am, an, tdf[1].data_ptr(), None, tdu1.data_ptr(), reg=reg)
    assert _same(tdu1.cpu().numpy(), s.sumregs_jvp(u, x, df=df[1], reg=reg))
    s.sumregs_jvp_device(tu.data_ptr(), ta.data_ptr(), am, an, None, tdx[2].data_ptr(), tdu1.data_ptr(), reg=reg)
    assert _same(tdu1.cpu().numpy(), s.sumregs_jvp(u, x, dalpha=dx[2], reg=reg))
    s.close()
    # image groups: a budget of 2.5 images' nested-dissection workspace splits the 3 images (the LU variant's workspace
    # is larger: more groups)
    sg = gpu_solver_cls(M, N, O)
    sg.set_option("adjoint_budget_mb", 2.5 * _sr_bytes_per_image(M, N) / 1e6)
    dug = sg.sumregs_jvp(u, x, df=df, dalpha=dx, reg=reg)
    assert sg.stats()["adjoint_chunks"] > 1 and _same(dug, du)
    sg.close()
    s32 = gpu_solver_cls(M, N, O, dtype=32)
    assert _same(s32.sumregs_jvp(u, x, df=df, dalpha=dx, reg=reg), du)
    s32.close()


@pytest.mark.parametrize("kind", ["vector", "patch22", "map"])
def test_sumregs_jvp_on_shards_of_one_device(gpu_solver_cls, kind):
    """devices = [0, 0]: du bitwise a single handle's; the device form is refused."""
    import torch
    from bpldenoising_amd._lib import BpltvError
    case = (3, 48, 40, kind)
    O, N, M, _ = case
    _, _, x, u = _case(*case)
    df, dx = _tangents(u, x, 29, K=2)
    am, an = _amn(x)
    s = gpu_solver_cls(M, N, O)
    m = gpu_solver_cls(M, N, O, devices=[0, 0])
    for reg in (0, 1):
        du = s.sumregs_jvp(u, x, df=df, dalpha=dx, reg=reg)
        assert _same(m.sumregs_jvp(u, x, df=df, dalpha=dx, reg=reg), du)
        assert m.stats()["shards"] == 2
        assert _same(m.sumregs_jvp(u, x, dalpha=dx[1], reg=reg), s.sumregs_jvp(u, x, dalpha=dx[1], reg=reg))
        tu = torch.from_numpy(u).cuda()
        ta = torch.from_numpy(np.ascontiguousarray(x).reshape(-1).copy()).cuda()
        tdu = torch.empty_like(tu)
        torch.cuda.synchronize()
        with pytest.raises(BpltvError) as e:
            m.sumregs_jvp_device(tu.data_ptr(), ta.data_ptr(), am, an, tu.data_ptr(), None, tdu.data_ptr(), reg=reg)
        assert e.value.code == E_UNSUPPORTED
    m.close()
    s.close()


def test_sumregs_jvp_rejects_bad_input_and_changes_nothing(gpu_solver_cls):
    """Every rejection, host and device, and an accepted JVP leave the last solve as it was: u_device, the duality gap and
    the next sumregs_denoise bit for bit."""
    import torch
    from bpldenoising_amd._lib import BpltvError
    from bpldenoising_amd.learning_function import _ptr
    O, N, M = 3, 48, 40
    ub, f = synth_batch(O, N, M, seed=81)
    s = gpu_solver_cls(M, N, O)
    s.set_data(ub, f)
    u0 = s.sumregs_denoise(P22, maxiter=200)
    assert s.stats()["graph_used"] == 1
    snap = _snapshot(s)
    df, dx = _tangents(u0, P22, 33)
    ref_du = s.sumregs_jvp(u0, P22, df=df, dalpha=dx, reg=1)
    s.sumregs_jvp(u0, 3.0 * P22, df=df, dalpha=dx, reg=0)
    now = _snapshot(s)
    assert _same(now[0], snap[0]) and _same(now[1], snap[1])          # an accepted JVP at another parameter
    bad_df, bad_dx = df.copy(), dx.copy()
    bad_df[1, 7, 5] = np.nan
    bad_dx[2, 1, 0] = np.inf
    zero_patch = P22.copy()
    zero_patch[1, 0, 1] = 0.0
    calls = [(P22 * np.nan, df, dx, 0), (-P22, df, dx, 0), (P22, bad_df, dx, 0), (P22, bad_df, None, 1), (P22, df, bad_dx, 1),
             (P22, None, bad_dx, 0), (zero_patch, df, dx, 1), (A3 * np.nan, df, None, 0), (-A3, df, None, 1)]
    for x, tf, tx, reg in calls:
        with pytest.raises(BpltvError) as e:
            s.sumregs_jvp(u0, x, df=tf, dalpha=(tx if tx is None or np.ndim(x) == 3 else None), reg=reg)
        assert e.value.code == E_ARG, (reg, str(e.value))
    s.sumregs_jvp(u0, zero_patch, df=df, dalpha=dx, reg=0)          # a zero entry is fine for sumregs_gradient
    with pytest.raises(BpltvError) as e:
        s.sumregs_jvp(u0, P22, df=df, adjoint_method="bcr")         # reserved[4] = 2
    assert e.value.code == E_UNSUPPORTED
    a = np.ascontiguousarray(P22)
    du = np.empty_like(u0)
    assert s._lib.bpltv_sumregs_jvp(s._h, _ptr(u0), _ptr(a), 2, 2, 0, None, 0, _ptr(df), _ptr(dx), _ptr(du)) == E_ARG
    assert s._lib.bpltv_sumregs_jvp(s._h, _ptr(u0), _ptr(a), 2, 2, 0, None, 1, None, None, _ptr(du)) == E_ARG
    with pytest.raises(ValueError):
        s.sumregs_jvp(u0, P22)
    # device form: parameter and tangents checked on the device
    tu, tdf, tbad = (torch.from_numpy(v).cuda() for v in (u0, df, bad_df))
    tdx, tbad_dx = torch.from_numpy(dx).cuda(), torch.from_numpy(bad_dx).cuda()
    tdu = torch.empty_like(tu)
    for x, tf_, tx_, reg in ((-P22, tdf, tdx, 0), (P22 * np.nan, tdf, tdx, 1), (P22, tbad, tdx, 0), (P22, tdf, tbad_dx, 1),
                             (zero_patch, tdf, tdx, 1)):
        tal = torch.from_numpy(np.ascontiguousarray(x).reshape(-1).copy()).cuda()
        torch.cuda.synchronize()
        with pytest.raises(BpltvError) as e:
            s.sumregs_jvp_device(tu.data_ptr(), tal.data_ptr(), 2, 2, tf_.data_ptr(), tx_.data_ptr(), tdu.data_ptr(), reg=reg)
        assert e.value.code == E_ARG
    tal = torch.from_numpy(a.reshape(-1).copy()).cuda()
    torch.cuda.synchronize()
    for ndir, p1, p2 in ((0, tdf.data_ptr(), tdx.data_ptr()), (1, None, None)):
        with pytest.raises(BpltvError) as e:
            s.sumregs_jvp_device(tu.data_ptr(), tal.data_ptr(), 2, 2, p1, p2, tdu.data_ptr(), ndir=ndir)
        assert e.value.code == E_ARG
    with pytest.raises(BpltvError) as e:
        s.sumregs_jvp_device(tu.data_ptr(), tal.data_ptr(), 2, 2, tdf.data_ptr(), None, tdu.data_ptr(), adjoint_method="bcr")
    assert e.value.code == E_UNSUPPORTED
    now = _snapshot(s)
    assert _same(now[0], snap[0]) and _same(now[1], snap[1])
    assert _same(s.sumregs_jvp(u0, P22, df=df, dalpha=dx, reg=1), ref_du)
    assert _same(s.sumregs_denoise(P22, maxiter=200), u0) and s.stats()["graph_used"] == 1
    s.close()
