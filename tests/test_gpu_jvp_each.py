"""GPU checks of the Jacobian-vector product with one parameter per image (bpltv_jvp_each / bpltv_jvp_each_device).

Image k reads its own parameter block and its own tangent block: equal blocks give bitwise the shared form, image k is
bitwise a one-image handle's result, and the map is the transpose of bpltv_vjp_each.  Every case uses a different
parameter per image, so a block index taken from the wrong image fails."""
import numpy as np
import pytest
from conftest import synth_batch

from test_gpu_each import KINDS, _blocks, _same, _shared_alpha, _snapshot

pytestmark = pytest.mark.gpu

E_ARG, E_UNSUPPORTED = 1, 6
O, N, M = 4, 48, 40


def _setup(cls, kind, seed, equal=False):
    """(u, blocks): u from a 200-iteration per-image solve of the library (the JVP takes any u)."""
    ub, f = synth_batch(O, N, M, seed=seed)
    if equal:
        a = np.stack([np.asarray(_shared_alpha(kind, N, M), dtype=np.float64)] * O)
    else:
        a = _blocks(kind, O, N, M, seed=seed + 1)
    s = cls(M, N, O)
    s.set_data(ub, f)
    u = s.denoise_each(a, maxiter=200)
    s.close()
    return u, a


def _tangents(u, a, seed, K=None):
    rng = np.random.default_rng(seed)
    lead = () if K is None else (K,)
    return rng.standard_normal(lead + u.shape), rng.standard_normal(lead + a.shape)


@pytest.mark.parametrize("reg", [0, 1])
@pytest.mark.parametrize("kind", KINDS)
def test_equal_blocks_give_the_shared_jvp_bitwise(gpu_solver_cls, kind, reg):
    u, a = _setup(gpu_solver_cls, kind, 71, equal=True)
    df, da = _tangents(u, a, 72, K=2)
    da[:] = da[:, :1]   # the same tangent block for every image, as the shared form applies it
    s = gpu_solver_cls(M, N, O)
    each = s.jvp_each(u, a, df=df, dalphas=da, reg=reg)
    shared = s.jvp(u, a[0] if a.ndim > 1 else float(a[0]), df=df, dalpha=da[:, 0], reg=reg)
    assert each.shape == (2,) + u.shape and _same(each, shared)
    s.close()


@pytest.mark.parametrize("reg", [0, 1])
@pytest.mark.parametrize("kind", KINDS)
def test_image_k_is_a_one_image_handles_result_bitwise(gpu_solver_cls, kind, reg):
    u, a = _setup(gpu_solver_cls, kind, 73)
    df, da = _tangents(u, a, 74, K=2)
    s = gpu_solver_cls(M, N, O)
    du = s.jvp_each(u, a, df=df, dalphas=da, reg=reg)
    du_f = s.jvp_each(u, a, df=df[1], reg=reg)
    du_a = s.jvp_each(u, a, dalphas=da[0], reg=reg)
    s.close()
    one = gpu_solver_cls(M, N, 1)
    for k in range(O):
        ak = a[k] if a.ndim > 1 else float(a[k])
        dk = da[:, k]
        assert _same(one.jvp(u[k:k + 1], ak, df=df[:, k:k + 1], dalpha=dk, reg=reg), du[:, k:k + 1]), k
        assert _same(one.jvp(u[k:k + 1], ak, df=df[1, k:k + 1], reg=reg), du_f[k:k + 1]), k
        assert _same(one.jvp(u[k:k + 1], ak, dalpha=dk[0] if a.ndim > 1 else float(dk[0]), reg=reg), du_a[k:k + 1]), k
    one.close()


@pytest.mark.parametrize("reg", [0, 1])
@pytest.mark.parametrize("kind", KINDS)
def test_jvp_each_is_the_transpose_of_vjp_each(gpu_solver_cls, kind, reg):
    """The bound of tests/test_gpu_jvp.py: 1e-6 of the terms' magnitude."""
    u, a = _setup(gpu_solver_cls, kind, 75)
    df, da = _tangents(u, a, 76)
    gu = np.random.default_rng(77).standard_normal(u.shape)
    s = gpu_solver_cls(M, N, O)
    du = s.jvp_each(u, a, df=df, dalphas=da, reg=reg)
    gf, ga = s.vjp_each(u, a, gu, reg=reg)
    s.close()
    lhs, t1, t2 = float(np.sum(gu * du)), float(np.sum(gf * df)), float(np.sum(ga * da))
    print("%s reg %d: lhs %.15g rhs %.15g" % (kind, reg, lhs, t1 + t2))
    assert abs(lhs - (t1 + t2)) <= 1e-6 * (abs(t1) + abs(t2))
    # ... and per image: image k's du pairs with image k's blocks alone
    for k in range(O):
        l, r1, r2 = float(np.sum(gu[k] * du[k])), float(np.sum(gf[k] * df[k])), float(np.sum(ga[k] * da[k]))
        assert abs(l - (r1 + r2)) <= 1e-6 * (abs(r1) + abs(r2)), k


@pytest.mark.parametrize("kind", KINDS)
def test_jvp_each_device_form_groups_and_float_handle(gpu_solver_cls, kind):
    import torch
    from test_gpu_vjp import _nd_bytes_per_image
    u, a = _setup(gpu_solver_cls, kind, 78)
    K = 2
    df, da = _tangents(u, a, 79, K=K)
    am, an = (1, 1) if a.ndim == 1 else (a.shape[2], a.shape[1])
    s = gpu_solver_cls(M, N, O)
    for reg in (0, 1):
        du = s.jvp_each(u, a, df=df, dalphas=da, reg=reg)
        tu, ta, tdf, tda = (torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (u, a, df, da))
        tdu = torch.zeros(K, *u.shape, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        s.jvp_each_device(tu.data_ptr(), ta.data_ptr(), am, an, tdf.data_ptr(), tda.data_ptr(), tdu.data_ptr(), ndir=K, reg=reg)
        assert _same(tdu.cpu().numpy(), du)
        s.jvp_each_device(tu.data_ptr(), ta.data_ptr(), am, an, None, tda[1].data_ptr(), tdu[0].data_ptr(), reg=reg)
        assert _same(tdu[0].cpu().numpy(), s.jvp_each(u, a, dalphas=da[1], reg=reg))
        sg = gpu_solver_cls(M, N, O)
        sg.set_option("adjoint_budget_mb", 1.5 * _nd_bytes_per_image(M, N) / 1e6)
        assert _same(sg.jvp_each(u, a, df=df, dalphas=da, reg=reg), du) and sg.stats()["adjoint_chunks"] == O
        sg.close()
        s32 = gpu_solver_cls(M, N, O, dtype=32)
        assert _same(s32.jvp_each(u, a, df=df, dalphas=da, reg=reg), du)
        s32.close()
    s.close()


@pytest.mark.parametrize("kind", KINDS)
def test_jvp_each_on_shards_of_one_device(gpu_solver_cls, kind):
    """Shards [0, 2) and [2, 4) of one device: every shard reads its own parameter and tangent blocks."""
    import torch
    from bpldenoising_amd._lib import BpltvError
    u, a = _setup(gpu_solver_cls, kind, 80)
    df, da = _tangents(u, a, 81, K=2)
    am, an = (1, 1) if a.ndim == 1 else (a.shape[2], a.shape[1])
    s = gpu_solver_cls(M, N, O)
    m = gpu_solver_cls(M, N, O, devices=[0, 0])
    for reg in (0, 1):
        assert _same(m.jvp_each(u, a, df=df, dalphas=da, reg=reg), s.jvp_each(u, a, df=df, dalphas=da, reg=reg))
        assert m.stats()["shards"] == 2
        assert _same(m.jvp_each(u, a, dalphas=da[1], reg=reg), s.jvp_each(u, a, dalphas=da[1], reg=reg))
    tu, ta = torch.from_numpy(u).cuda(), torch.from_numpy(a).cuda()
    tdu = torch.empty_like(tu)
    torch.cuda.synchronize()
    with pytest.raises(BpltvError) as e:
        m.jvp_each_device(tu.data_ptr(), ta.data_ptr(), am, an, tu.data_ptr(), None, tdu.data_ptr())
    assert e.value.code == E_UNSUPPORTED
    m.close()
    s.close()


def test_jvp_each_rejects_bad_input_and_changes_nothing(gpu_solver_cls):
    from bpldenoising_amd._lib import BpltvError
    from bpldenoising_amd.learning_function import _ptr
    ub, f = synth_batch(O, N, M, seed=82)
    a = _blocks("patch23", O, N, M, seed=83)
    s = gpu_solver_cls(M, N, O)
    s.set_data(ub, f)
    u0 = s.denoise_each(a, maxiter=200)
    df, da = _tangents(u0, a, 84)
    ref = s.jvp_each(u0, a, df=df, dalphas=da)
    snap = _snapshot(s)
    bad_df, bad_da, neg, zero = df.copy(), da.copy(), a.copy(), a.copy()
    bad_df[3, 2, 1] = np.nan
    bad_da[2, 1, 2] = -np.inf
    neg[3, 0, 0] = -0.01
    zero[1, 1, 1] = 0.0
    for al, tf, tda, reg in [(neg, df, da, 0), (a * np.nan, df, None, 0), (a, bad_df, da, 1), (a, None, bad_da, 0),
                             (zero, df, da, 1)]:
        with pytest.raises(BpltvError) as e:
            s.jvp_each(u0, al, df=tf, dalphas=tda, reg=reg)
        assert e.value.code == E_ARG, str(e.value)
    du = np.empty_like(u0)
    assert s._lib.bpltv_jvp_each(s._h, _ptr(u0), _ptr(a), 3, 2, 0, None, 0, _ptr(df), _ptr(da), _ptr(du)) == E_ARG
    assert s._lib.bpltv_jvp_each(s._h, _ptr(u0), _ptr(a), 3, 2, 0, None, 1, None, None, _ptr(du)) == E_ARG
    with pytest.raises(ValueError):
        s.jvp_each(u0, a[:2], df=df)
    now = _snapshot(s)
    assert _same(now[0], snap[0]) and _same(now[1], snap[1])
    assert _same(s.jvp_each(u0, a, df=df, dalphas=da), ref)
    assert _same(s.denoise_each(a, maxiter=200), u0)
    s.close()
