"""GPU checks of the sum-of-regularisers Jacobian-vector product with one block of three weights per image
(bpltv_sumregs_jvp_each / bpltv_sumregs_jvp_each_device).

Image k reads its own parameter block and its own tangent block: equal blocks give bitwise the shared form, image k is
bitwise a one-image handle's result, and the map is the transpose of bpltv_sumregs_vjp_each.  Every case uses a
different block per image, so a block index taken from the wrong image fails."""
import numpy as np
import pytest
from conftest import synth_batch

from test_gpu_sumregs_vjp import _alpha, _same, _snapshot

pytestmark = pytest.mark.gpu

E_ARG, E_UNSUPPORTED = 1, 6
O, N, M = 3, 48, 40
KINDS = ["vector", "patch22", "map"]


def _blocks(kind, seed, equal=False):
    """(O, 3) / (O, 3, n, m): image k's own block, scaled and perturbed per image (all entries > 0)."""
    base = np.asarray(_alpha(kind, N, M), dtype=np.float64)
    if equal:
        return np.stack([base] * O)
    rng = np.random.default_rng(seed)
    return np.stack([base * (0.6 + 0.5 * k) * (0.8 + 0.4 * rng.random(base.shape)) for k in range(O)])


def _setup(cls, kind, seed, equal=False):
    """(u, blocks): u from a 200-iteration per-image solve of the library (the JVP takes any u)."""
    ub, f = synth_batch(O, N, M, seed=seed)
    a = _blocks(kind, seed + 1, equal)
    s = cls(M, N, O)
    s.set_data(ub, f)
    u = s.sumregs_denoise_each(a, maxiter=200)
    s.close()
    return u, a


def _tangents(u, a, seed, K=None):
    rng = np.random.default_rng(seed)
    lead = () if K is None else (K,)
    return rng.standard_normal(lead + u.shape), rng.standard_normal(lead + a.shape)


def _amn(a):
    return (1, 1) if a.ndim == 2 else (a.shape[3], a.shape[2])


@pytest.mark.parametrize("reg", [0, 1])
@pytest.mark.parametrize("kind", KINDS)
def test_equal_blocks_give_the_shared_sumregs_jvp_bitwise(gpu_solver_cls, kind, reg):
    u, a = _setup(gpu_solver_cls, kind, 71, equal=True)
    df, da = _tangents(u, a, 72, K=2)
    da[:] = da[:, :1]   # the same tangent block for every image, as the shared form applies it
    s = gpu_solver_cls(M, N, O)
    each = s.sumregs_jvp_each(u, a, df=df, dalphas=da, reg=reg)
    shared = s.sumregs_jvp(u, a[0], df=df, dalpha=da[:, 0], reg=reg)
    assert each.shape == (2,) + u.shape and _same(each, shared)
    s.close()


@pytest.mark.parametrize("reg", [0, 1])
@pytest.mark.parametrize("kind", KINDS)
def test_image_k_is_a_one_image_handles_result_bitwise(gpu_solver_cls, kind, reg):
    u, a = _setup(gpu_solver_cls, kind, 73)
    df, da = _tangents(u, a, 74, K=2)
    s = gpu_solver_cls(M, N, O)
    du = s.sumregs_jvp_each(u, a, df=df, dalphas=da, reg=reg)
    du_f = s.sumregs_jvp_each(u, a, df=df[1], reg=reg)
    du_a = s.sumregs_jvp_each(u, a, dalphas=da[0], reg=reg)
    s.close()
    one = gpu_solver_cls(M, N, 1)
    for k in range(O):
        assert _same(one.sumregs_jvp(u[k:k + 1], a[k], df=df[:, k:k + 1], dalpha=da[:, k], reg=reg), du[:, k:k + 1]), k
        assert _same(one.sumregs_jvp(u[k:k + 1], a[k], df=df[1, k:k + 1], reg=reg), du_f[k:k + 1]), k
        assert _same(one.sumregs_jvp(u[k:k + 1], a[k], dalpha=da[0, k], reg=reg), du_a[k:k + 1]), k
    one.close()


@pytest.mark.parametrize("reg", [0, 1])
@pytest.mark.parametrize("kind", KINDS)
def test_sumregs_jvp_each_is_the_transpose_of_vjp_each(gpu_solver_cls, kind, reg):
    """The bound of tests/test_gpu_jvp.py, 1e-6 of the terms' magnitude, over the batch and per image."""
    u, a = _setup(gpu_solver_cls, kind, 75)
    df, da = _tangents(u, a, 76)
    gu = np.random.default_rng(77).standard_normal(u.shape)
    s = gpu_solver_cls(M, N, O)
    du = s.sumregs_jvp_each(u, a, df=df, dalphas=da, reg=reg)
    gf, ga = s.sumregs_vjp_each(u, a, gu, reg=reg)
    s.close()
    for k in [slice(None)] + list(range(O)):
        l, r1, r2 = float(np.sum(gu[k] * du[k])), float(np.sum(gf[k] * df[k])), float(np.sum(ga[k] * da[k]))
        print("%s reg %d %s: lhs %.15g rhs %.15g" % (kind, reg, k, l, r1 + r2))
        assert abs(l - (r1 + r2)) <= 1e-6 * (abs(r1) + abs(r2)), k


@pytest.mark.parametrize("kind", KINDS)
def test_sumregs_jvp_each_device_form_and_shards(gpu_solver_cls, kind):
    """The device form bitwise the host form; shards [0, 2) and [2, 3) of one device read their own parameter and tangent
    blocks; the device form is refused beyond one shard."""
    import torch
    from bpldenoising_amd._lib import BpltvError
    u, a = _setup(gpu_solver_cls, kind, 78)
    K = 2
    df, da = _tangents(u, a, 79, K=K)
    am, an = _amn(a)
    s = gpu_solver_cls(M, N, O)
    m = gpu_solver_cls(M, N, O, devices=[0, 0])
    tu, ta, tdf, tda = (torch.from_numpy(np.ascontiguousarray(v)).cuda() for v in (u, a, df, da))
    for reg in (0, 1):
        du = s.sumregs_jvp_each(u, a, df=df, dalphas=da, reg=reg)
        tdu = torch.zeros(K, *u.shape, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        s.sumregs_jvp_each_device(tu.data_ptr(), ta.data_ptr(), am, an, tdf.data_ptr(), tda.data_ptr(), tdu.data_ptr(),
                                  ndir=K, reg=reg)
        assert _same(tdu.cpu().numpy(), du)
        s.sumregs_jvp_each_device(tu.data_ptr(), ta.data_ptr(), am, an, None, tda[1].data_ptr(), tdu[0].data_ptr(), reg=reg)
        assert _same(tdu[0].cpu().numpy(), s.sumregs_jvp_each(u, a, dalphas=da[1], reg=reg))
        assert _same(m.sumregs_jvp_each(u, a, df=df, dalphas=da, reg=reg), du)
        assert m.stats()["shards"] == 2
        assert _same(m.sumregs_jvp_each(u, a, dalphas=da[1], reg=reg), s.sumregs_jvp_each(u, a, dalphas=da[1], reg=reg))
        with pytest.raises(BpltvError) as e:
            m.sumregs_jvp_each_device(tu.data_ptr(), ta.data_ptr(), am, an, tu.data_ptr(), None, tdu.data_ptr(), reg=reg)
        assert e.value.code == E_UNSUPPORTED
    m.close()
    s.close()


def test_sumregs_jvp_each_rejects_bad_input_and_changes_nothing(gpu_solver_cls):
    import torch
    from bpldenoising_amd._lib import BpltvError
    from bpldenoising_amd.learning_function import _ptr
    ub, f = synth_batch(O, N, M, seed=82)
    a = _blocks("patch22", 83)
    s = gpu_solver_cls(M, N, O)
    s.set_data(ub, f)
    u0 = s.sumregs_denoise_each(a, maxiter=200)
    df, da = _tangents(u0, a, 84)
    ref = s.sumregs_jvp_each(u0, a, df=df, dalphas=da, reg=1)
    snap = _snapshot(s)
    bad_df, bad_da, neg, zero = df.copy(), da.copy(), a.copy(), a.copy()
    bad_df[2, 2, 1] = np.nan
    bad_da[2, 1, 1, 0] = -np.inf
    neg[2, 0, 0, 0] = -0.01
    zero[1, 2, 1, 1] = 0.0
    for al, tf, tda, reg in [(neg, df, da, 0), (a * np.nan, df, None, 0), (a, bad_df, da, 1), (a, None, bad_da, 0),
                             (zero, df, da, 1)]:
        with pytest.raises(BpltvError) as e:
            s.sumregs_jvp_each(u0, al, df=tf, dalphas=tda, reg=reg)
        assert e.value.code == E_ARG, str(e.value)
    with pytest.raises(BpltvError) as e:
        s.sumregs_jvp_each(u0, a, df=df, adjoint_method="bcr")
    assert e.value.code == E_UNSUPPORTED
    du = np.empty_like(u0)
    assert s._lib.bpltv_sumregs_jvp_each(s._h, _ptr(u0), _ptr(a), 2, 2, 0, None, 0, _ptr(df), _ptr(da), _ptr(du)) == E_ARG
    assert s._lib.bpltv_sumregs_jvp_each(s._h, _ptr(u0), _ptr(a), 2, 2, 0, None, 1, None, None, _ptr(du)) == E_ARG
    with pytest.raises(ValueError):
        s.sumregs_jvp_each(u0, a[:2], df=df)
    # device form: parameter and tangents checked on the device
    tu, tdf, tbad, tda, tdu = (torch.from_numpy(v).cuda() for v in (u0, df, bad_df, da, du))
    for al, tf_, reg in ((neg, tdf, 0), (zero, tdf, 1), (a, tbad, 0)):
        tal = torch.from_numpy(al).cuda()
        torch.cuda.synchronize()
        with pytest.raises(BpltvError) as e:
            s.sumregs_jvp_each_device(tu.data_ptr(), tal.data_ptr(), 2, 2, tf_.data_ptr(), tda.data_ptr(), tdu.data_ptr(), reg=reg)
        assert e.value.code == E_ARG
    now = _snapshot(s)
    assert _same(now[0], snap[0]) and _same(now[1], snap[1])
    assert _same(s.sumregs_jvp_each(u0, a, df=df, dalphas=da, reg=1), ref)
    assert _same(s.sumregs_denoise_each(a, maxiter=200), u0)
    s.close()
