"""CPU pins of tests/weighted_active_ref.py: the literal weighted adjoint system on images with a planted active set under wide
weights, at every case tests/test_gpu_weighted_active_set.py holds the library to.  Every check is a condition on the reference
alone: its planted layouts are what they say, it is better than the bound it is used with (1e-8 max|p|) by a factor of a hundred, the
node-scaled form the library factors is the same system, the solve is symmetric, and with w = 1 the module is tv_active_ref."""
import numpy as np
import pytest

import tv_active_ref as ta
import weighted_active_ref as wa
import weighted_ref as wr

# of the project's bound 1e-8 max|p|: the plain LU and ten extended-precision sweeps may differ by a hundredth of it
STABLE = 0.01 * 1e-8


def _border(N, M):
    """Active elements of the block at the right border (tests/test_tv_active_ref.py): one of its two rows, or with N = 12,
    where the second row is the image's last, both less the last pixel."""
    return M - 15 if N > 12 else 2 * (M - 15) - 1


def expected_counts(shape, layout):
    O, N, M = shape
    blocks = 6 + _border(N, M)
    if layout == "blocks":
        return [blocks] if O == 1 else [6] + [0] * (O - 2) + [_border(N, M)]
    if layout == "strips":
        return [3 * M + 3 * N - 9 + 1] + [0] * (O - 1)
    return [N * M - 1, blocks] + [0] * (O - 2)


def test_expected_counts_are_the_recorded_ones():
    """The numbers of the cases: strips 256; a constant 40 x 48 image 1919 and both blocks 39; 33 x 17: 560 and 8; 2 x 70 x 72
    blocks 6 and 57; 1 x 12 x 140 (both blocks in the one image, the second row of the border block the image's last) 255."""
    assert expected_counts((2, 40, 48), "strips") == [256, 0]
    assert expected_counts((3, 40, 48), "flat") == [1919, 39, 0]
    assert expected_counts((3, 33, 17), "flat") == [560, 8, 0]
    assert expected_counts((2, 70, 72), "blocks") == [6, 57]
    assert expected_counts((1, 12, 140), "blocks") == [255]


def test_the_weights_are_what_the_cases_need():
    for shape in ((3, 40, 48), (40, 48)):
        r, l, s = (wa.weight(n, shape) for n in wa.WEIGHTS)
        assert r.shape == l.shape == s.shape == shape and not (r.flags.writeable or l.flags.writeable or s.flags.writeable)
        assert 0.25 <= r.min() and r.max() <= 4.0
        assert 1e-3 <= l.min() < 2e-3 and 5e2 < l.max() <= 1e3
        assert np.all(s[..., :24] == 100.0) and np.all(s[..., 24:] == 0.01)
    # the jump lies inside the strips' full rows, the constant image and the block that reaches the right border
    assert 15 < 48 // 2 and 15 < 72 // 2 and 15 < 140 // 2
    assert len(wa.CASES) == len(set(wa.IDS)) == 41


@pytest.mark.parametrize("case", wa.CASES, ids=wa.IDS)
def test_active_counts_are_what_the_layout_says(case):
    """The planted regions on the weighted twin's iterate: an element is active when both its forward differences vanish.  The
    smallest inactive |G u| stays at or above 1e-9 (measured: 1.2e-9 at the smallest, 3 x 33 x 17 flat, rand, patch), so no element
    sits near the 1e-12 test."""
    shape, layout = case[:2]
    alpha, f, w, u, gu = wa.case(*case)
    n = ta.active_counts(u)
    ng = ta.grad_norm(u)
    margin = float(ng[ng >= 1e-12].min())
    print("%s: active %s smallest inactive |G u| %.3e" % (wa.case_id(*case), list(n), margin))
    assert list(n) == expected_counts(shape, layout)
    assert margin >= 1e-9
    assert w.shape == (shape if case[4] else shape[1:]) and u.shape == f.shape == gu.shape == shape
    assert not (u.flags.writeable or w.flags.writeable or gu.flags.writeable)


@pytest.mark.parametrize("case", wa.CASES, ids=wa.IDS)
def test_reference_is_stable_under_refinement(case):
    """Plain sparse LU against ten extended-precision sweeps: grad_f, grad_alpha and grad_w within a hundredth of the bound the
    library is held to, |a - b| <= 0.01 * 1e-8 max|p|.  Measured over the 41 cases: at most 0.0020 of 1e-8 max|p| (grad_f of
    3 x 40 x 48 flat, rand, patch: 5.7e-11 with max|p| 2.9); largest absolute grad_f 5.7e-11, grad_alpha 7.1e-10, grad_w 8.7e-11;
    max|p| from 1.7 to 1.6e3."""
    data = wa.case(*case)
    kap = wr.kappa_default(data[0])
    r0 = wa.vjp_of(*data, kap, refine=0)
    gf, ga, gw, pmax = wa.vjp_ref(*case, kap)
    for name, a, b in (("grad_f", r0[0], gf), ("grad_alpha", r0[1], ga), ("grad_w", r0[2], gw)):
        d = float(np.abs(np.asarray(a) - np.asarray(b)).max())
        print("%s %s: max|d| = %.3e = %.4f of 1e-8 max|p| (max|p| %.3e)" % (wa.case_id(*case), name, d, d / (1e-8 * pmax), pmax))
        assert np.shape(a) == np.shape(b) and d <= STABLE * pmax, name
    assert np.shape(ga) == np.shape(data[0]) and gw.shape == data[2].shape


@pytest.mark.parametrize("case", wa.CASES, ids=wa.IDS)
def test_scaled_form_is_the_literal_system(case):
    """p = S q of (I + S K S) q = S gu, the form the library factors, against p of the literal system, both with ten sweeps, within
    0.01 * 1e-8 max|p|.  Measured: at most 0.0069 of 1e-8 max|p| (2.0e-10 with max|p| 2.9; 3 x 40 x 48 flat, rand, patch)."""
    shape, per_image = case[0], case[4]
    alpha, f, w, u, gu = wa.case(*case)
    kap = wr.kappa_default(alpha)
    p = wa.vjp_full(*case, kap)[3]
    pmax = float(np.abs(p).max())
    for k in range(shape[0]):
        ps = wr.vjp_image_scaled(u[k], alpha, w[k] if per_image else w, gu[k], kap, refine=10)
        d = float(np.abs(ps - p[k]).max())
        print("%s image %d: max|d p| = %.3e = %.4f of 1e-8 max|p|" % (wa.case_id(*case), k, d, d / (1e-8 * pmax)))
        assert d <= STABLE * pmax, k


@pytest.mark.parametrize("case", wa.CASES, ids=wa.IDS)
def test_reference_solve_is_symmetric(case):
    """(diag(w) + K)^-1 is symmetric: |<a, p(b)> - <b, p(a)>| <= 1e-10 (|<a, p(b)>| + 1) for the case's cotangent a and a second
    one, ten sweeps each.  Measured: at most 3.2e-11 (|<a, p(b)>| + 1)."""
    alpha, f, w, u, a = wa.case(*case)
    b = np.random.default_rng(23).standard_normal(a.shape)
    kap = wr.kappa_default(alpha)
    pa = wa.vjp_full(*case, kap)[3]
    pb = wa.vjp_of(alpha, f, w, u, b, kap, refine=10)[3]
    ab, ba = float(np.sum(a * pb)), float(np.sum(b * pa))
    print("%s: <a, p(b)> %.15g <b, p(a)> %.15g |d| / (|.| + 1) = %.3e" % (wa.case_id(*case), ab, ba, abs(ab - ba) / (abs(ab) + 1)))
    assert abs(ab - ba) <= 1e-10 * (abs(ab) + 1)


UNIT = [((2, 40, 48), "blocks", "scalar"), ((2, 40, 48), "strips", "patch"), ((3, 33, 17), "flat", "map")]


@pytest.mark.parametrize("shape,layout,kind", UNIT, ids=[ta.case_id(sh, lay, k) for sh, lay, k in UNIT])
def test_unit_weight_is_the_unweighted_reference(shape, layout, kind):
    """w = 1 on the unweighted twin's u: grad_f and grad_alpha of this module's vjp_of are tv_active_ref.vjp_ref's, exactly (the
    same code on the same matrix), grad_w is -(u - f) o grad_f, with one plane its sum over the images."""
    alpha, f, u, gu, df, da = ta.case(shape, kind, layout)
    kap = wr.kappa_default(alpha)
    rf, ra, pmax = ta.vjp_ref(shape, kind, layout, kap)
    for w in (np.ones(shape), np.ones(shape[1:])):
        gf, ga, gw, p = wa.vjp_of(alpha, f, w, u, gu, kap, refine=10)
        assert np.array_equal(gf, rf) and np.array_equal(np.asarray(ga), np.asarray(ra)) and np.array_equal(p, gf)
        want = -(u - f) * rf
        assert gw.shape == w.shape and np.array_equal(gw, want if w.ndim == 3 else want.sum(axis=0))
