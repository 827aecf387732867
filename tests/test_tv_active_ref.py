"""CPU pins of tests/tv_active_ref.py: the literal unweighted adjoint system on images with a planted active set, at every
case tests/test_gpu_tv_active_set.py holds the library to.  The reference must be better than the bound it is used with (rtol
1e-6, atol 1e-8 max|p|) by a wide margin, its planted layouts must be what they say, its jvp must be the transpose of its vjp
and agree with the older tests/jvp_ref.py, and the regularised gradient of the C oracle must agree with the literal numpy
restatement on a u with exactly zero gradients."""
import numpy as np
import pytest

import jvp_ref
import tv_active_ref as ta
import weighted_ref as wr
from oracle import np_twin as tw

ALL = [(shape, kind, layout) for shape, layout in ta.CASES for kind in ta.KINDS]
IDS = [ta.case_id(sh, lay, k) for sh, k, lay in ALL]


@pytest.mark.parametrize("shape,kind,layout", ALL, ids=IDS)
def test_reference_is_stable_under_refinement(shape, kind, layout):
    """Plain sparse LU against ten extended-precision sweeps, vjp and jvp: rtol 1e-9 / atol 1e-10 max|p| (max|du| for the jvp),
    a hundredth of what the GPU tests allow the library.  Measured: grad_f <= 7.8e-12, grad_alpha <= 1.1e-11, du <= 1.2e-11
    absolute with max|p| 1.7 ... 2.9, the fully flat image included."""
    alpha, f, u, gu, df, da = ta.case(shape, kind, layout)
    kap = wr.kappa_default(alpha)
    r0 = ta.vjp(u, alpha, gu, kap, refine=0)
    gf, ga, pmax = ta.vjp_ref(shape, kind, layout, kap)
    for name, a, b in (("grad_f", r0[0], gf), ("grad_alpha", r0[1], ga)):
        a, b = np.asarray(a), np.asarray(b)
        print("%s %s: max|d| = %.3e (max|p| %.3e)" % (ta.case_id(shape, layout, kind), name, float(np.abs(a - b).max()), pmax))
        assert np.allclose(a, b, rtol=1e-9, atol=1e-10 * pmax), name
    d0, d1 = ta.jvp(u, alpha, df, da, kap, refine=0), ta.jvp_ref(shape, kind, layout, kap)
    print("%s du: max|d| = %.3e (max|du| %.3e)" % (ta.case_id(shape, layout, kind), float(np.abs(d0 - d1).max()), float(np.abs(d1).max())))
    assert np.allclose(d0, d1, rtol=1e-9, atol=1e-10 * np.abs(d1).max())


@pytest.mark.parametrize("shape,layout", ta.CASES, ids=[ta.case_id(sh, lay) for sh, lay in ta.CASES])
def test_active_counts_are_what_the_layout_says(shape, layout):
    """blocks: 2 x 3 elements of the 3 x 4 block and the M - 15 of one row of the block at the right border (an element is active
    when BOTH its forward differences vanish); strips: 3 full rows and 3 full columns of the two strips; flat: all of
    image 0, both blocks in image 1, nothing in the last image.  The smallest inactive |G u| stays above 1e-9."""
    O, N, M = shape
    for kind in ta.KINDS:
        alpha, f, u, gu, df, da = ta.case(shape, kind, layout)
        n = ta.active_counts(u)
        # (with N = 12 the border block's second row is the image's last: active too, less the last pixel)
        border = M - 15 if N > 12 else 2 * (M - 15) - 1
        blocks = 6 + border
        if layout == "blocks":
            want = [blocks] if O == 1 else [6] + [0] * (O - 2) + [border]
        elif layout == "strips":
            # rows 18:21 and columns 30:33, their 3 x 3 crossing counted once, and the crossing's corner (21, 33), whose
            # two neighbours lie one in each strip
            want = [3 * M + 3 * N - 9 + 1] + [0] * (O - 1)
        else:
            want = [N * M - 1, blocks] + [0] * (O - 2)
        assert list(n) == want, (kind, list(n), want)
        assert 1 <= n.sum() <= O * (N * M - 1)
        ng = ta.grad_norm(u)
        assert ng[ng >= 1e-12].min() > 1e-9
        # the same set through the sparse operator the system is built from
        for k in range(O):
            nk = tw.xi(tw.grad_matrix(M, N) @ u[k].reshape(-1))[:N * M]
            assert int((nk < 1e-12).sum()) - 1 == n[k]


@pytest.mark.parametrize("shape,kind,layout", ALL, ids=IDS)
def test_reference_jvp_is_the_transpose_of_the_reference_vjp(shape, kind, layout):
    """<gu, du> = <grad_f, df> + <grad_alpha, dalpha> to 1e-11 sum|gu du|: two solves of one matrix with different right-hand
    sides, ten extended-precision sweeps each.  Measured: at most 9.7e-15."""
    alpha, f, u, gu, df, da = ta.case(shape, kind, layout)
    kap = wr.kappa_default(alpha)
    gf, ga, _ = ta.vjp_ref(shape, kind, layout, kap)
    du = ta.jvp_ref(shape, kind, layout, kap)
    lhs, rhs = float(np.sum(gu * du)), float(np.sum(gf * df) + np.sum(np.asarray(ga) * np.asarray(da)))
    scale = float(np.sum(np.abs(gu * du)))
    print("%s: lhs %.15g rhs %.15g |d| / sum|gu du| = %.3e" % (ta.case_id(shape, layout, kind), lhs, rhs, abs(lhs - rhs) / scale))
    assert abs(lhs - rhs) <= 1e-11 * scale
    # each tangent alone adds up to both (the right-hand side is linear in them)
    both = ta.jvp_ref(shape, kind, layout, kap, "df") + ta.jvp_ref(shape, kind, layout, kap, "dalpha")
    assert np.allclose(both, du, rtol=1e-9, atol=1e-10 * np.abs(du).max())


@pytest.mark.parametrize("kind", ta.KINDS)
def test_reference_jvp_matches_the_oracle_based_jvp_without_planted_blocks(oracle, kind):
    """2 x 40 x 48, the twin's iterate after 60 iterations as it is (only the last pixel active): tests/jvp_ref.py (numpy
    right-hand side, the C oracle's reduced solve) at the tolerance tests/test_gpu_jvp.py holds the library to with it (rtol
    1e-6, atol 1e-8 max|du|).  Measured: at most 3.2e-11 max|du|."""
    O, N, M = 2, 40, 48
    alpha = ta.alpha_kind(kind, N, M)
    from conftest import synth_batch
    _, f = synth_batch(O, N, M, seed=ta.SEED)
    u = tw.pdhg_denoise(f, alpha, maxiter=60)
    assert not ta.active_counts(u).any()
    rng = np.random.default_rng(5)
    df, da = rng.standard_normal(u.shape), rng.standard_normal(np.shape(alpha))
    da = float(da) if da.ndim == 0 else da
    kap = wr.kappa_default(alpha)
    for tf, tda in ((df, da), (df, None), (None, da)):
        got = ta.jvp(u, alpha, tf, tda, kap, refine=10)
        for k in range(O):
            want = jvp_ref.jvp_image(oracle, u[k], alpha, None if tf is None else tf[k], tda, 0)
            print("%s image %d: max|d| / max|du| = %.3e" % (kind, k, float(np.abs(got[k] - want).max() / np.abs(want).max())))
            assert np.allclose(got[k], want, rtol=1e-6, atol=1e-8 * np.abs(want).max())


@pytest.mark.parametrize("shape,kind,layout", ALL, ids=IDS)
def test_regularised_gradient_on_planted_u_oracle_against_twin(oracle, shape, kind, layout):
    """reg = 1 with exactly zero gradients in the smoothed branch: the C oracle against the literal numpy restatement within
    1e-9 max|g|.  Measured: at most 3.7e-10 max|g| (3 x 33 x 17 blocks, map; scalars at most 1.9e-10)."""
    alpha, f, u, gu, df, da = ta.case(shape, kind, layout)
    g0 = np.asarray(oracle.gradient(alpha, u, u - gu, reg=True))
    g1 = np.asarray(tw.batch_gradient(alpha, u, u - gu, reg=True))
    d, gmax = float(np.abs(g0 - g1).max()), float(np.abs(g1).max())
    print("%s: max|d| = %.3e = %.3e max|g|" % (ta.case_id(shape, layout, kind), d, d / gmax))
    assert g0.shape == g1.shape and d <= 1e-9 * gmax
