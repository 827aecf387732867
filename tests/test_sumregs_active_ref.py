"""CPU pins of tests/sumregs_active_ref.py: the literal sum-of-regularisers adjoint system on images with a planted active
set, at every case tests/test_gpu_sumregs_active_set.py holds the library to.  The reference must be better than the bound
it is used with (rtol 1e-6, atol 1e-8 max|p|) by a wide margin, its planted layouts must be what they say, its jvp must be
the transpose of its vjp, the C oracle's sumregs_gradient must agree with it, a rational solve must agree with it where one
is affordable, and the older reduced reference tests/sumregs_jvp_ref.py must be seen to fail on these images: that is why
this one exists."""
import functools

import numpy as np
import pytest

import sumregs_active_ref as sa
import sumregs_jvp_ref as jr

KAPPA = sa.KAPPA
ALL = ([(shape, kind, layout) for shape, layout in sa.CASES for kind in ("vector", "patch22", "map")]
       + [(shape, "vector-off", layout) for shape, layout in sa.CASES if layout in ("blocks", "stripes")])
IDS = [sa.case_id(sh, lay, k) for sh, k, lay in ALL]


@functools.lru_cache(maxsize=None)
def _oracle_gradient(shape, kind, layout):
    from oracle import c_oracle as co
    co.build()
    x, f, u, gu, df, dx = sa.case(shape, kind, layout)
    return np.asarray(co.sumregs_gradient(x, u, u - gu, reg=False))


@pytest.mark.parametrize("shape,kind,layout", ALL, ids=IDS)
def test_reference_is_stable_under_refinement(shape, kind, layout):
    """Plain sparse LU against ten extended-precision sweeps, vjp and jvp: every entry of grad_f, grad_x and du within
    1e-10 max|p| (max|du| for the jvp), a hundredth of the absolute term of the bound the GPU tests allow the library.
    Measured: grad_f <= 1.4e-12, grad_x <= 6.5e-12 (max|g| up to 76), du <= 3.3e-12 with max|p| 1.2 ... 2.5 -- the worst 0.027
    of this bound --, the constant image and the period-2 window included."""
    x, f, u, gu, df, dx = sa.case(shape, kind, layout)
    r0 = sa.vjp(u, x, gu, KAPPA, refine=0)
    gf, gx, pmax = sa.vjp_ref(shape, kind, layout, KAPPA)
    d0, d1 = sa.jvp(u, x, df, dx, KAPPA, refine=0), sa.jvp_ref(shape, kind, layout, KAPPA)
    dumax = float(np.abs(d1).max())
    dist = {"grad_f": float(np.abs(r0[0] - gf).max()), "grad_x": float(np.abs(r0[1] - gx).max()), "du": float(np.abs(d0 - d1).max())}
    print("%s: max|d| grad_f %.3e grad_x %.3e (max|p| %.3e max|g| %.3e) du %.3e (max|du| %.3e)"
          % (sa.case_id(shape, layout, kind), dist["grad_f"], dist["grad_x"], pmax, np.abs(gx).max(), dist["du"], dumax))
    assert dist["grad_f"] <= 1e-10 * pmax and dist["grad_x"] <= 1e-10 * pmax and dist["du"] <= 1e-10 * dumax, dist


@pytest.mark.parametrize("shape,layout", sa.CASES, ids=[sa.case_id(sh, lay) for sh, lay in sa.CASES])
def test_active_counts_are_what_the_layout_says(shape, layout):
    """Per image and operator, the elements with |G_k u| < 1e-12 are those the layout makes zero by construction (counted
    from the geometry alone, sumregs_active_ref.expected_counts), for every parameter kind, and the numbers of the module's
    docstring hold at 40 x 48: 25 / 23 / 11 for an image with both blocks, 1 / 1 / 532 for the period-2 window -- the centred
    operator alone is active there.  The smallest inactive |G_k u| stays above 1e-9 (measured: 9.7e-9 and up)."""
    O, N, M = shape
    want = sa.expected_counts(shape, layout)
    if (N, M) == (40, 48) and layout != "cross":
        assert list(want[0]) == {"blocks": [13, 13, 6], "stripes": [1, 1, 532], "flat": [N * M] * 3}[layout], want
        if layout == "flat":
            assert list(want[1]) == [25, 23, 11] and list(want[2]) == [1, 1, 0]
        if layout == "blocks":
            assert list(want[0] + want[1]) == [26, 24, 11]    # the two blocks of "flat" image 1, the forced rows twice
    smallest = np.inf
    for kind in sa.KINDS:
        if kind == "vector-off" and layout not in ("blocks", "stripes"):
            continue
        x, f, u, gu, df, dx = sa.case(shape, kind, layout)
        got = sa.active_counts(u)
        assert got.tolist() == want.tolist(), (kind, got.tolist(), want.tolist())
        ng = np.stack([sa.grad_norms(img) for img in u])
        smallest = min(smallest, float(ng[ng >= sa.ACT_TOL].min()))
        if layout == "stripes":
            k, rows, cols = sa._regions(shape, layout)[0]
            win = ng[k][:, rows.start + 1:rows.stop - 1, cols.start + 1:cols.stop - 1]
            assert not np.any(win[2]) and win[0].min() > 1e-9 and win[1].min() > 1e-9
            assert got[0].tolist() == [1, 1, (rows.stop - rows.start - 2) * (cols.stop - cols.start - 2)]
    print("%s: active %s, smallest inactive |G_k u| %.3e" % (sa.case_id(shape, layout), want.tolist(), smallest))
    assert smallest >= 1e-9


@pytest.mark.parametrize("shape,kind,layout", ALL, ids=IDS)
def test_reference_jvp_is_the_transpose_of_the_reference_vjp(shape, kind, layout):
    """<gu, du> = <grad_f, df> + <grad_x, dx> to 1e-12 sum|gu du|: two solves of one matrix with different right-hand sides,
    ten extended-precision sweeps each.  Measured: at most 8.4e-16.  Each tangent alone adds up to both."""
    x, f, u, gu, df, dx = sa.case(shape, kind, layout)
    gf, gx, _ = sa.vjp_ref(shape, kind, layout, KAPPA)
    du = sa.jvp_ref(shape, kind, layout, KAPPA)
    lhs, rhs = float(np.sum(gu * du)), float(np.sum(gf * df) + np.sum(gx * dx))
    scale = float(np.sum(np.abs(gu * du)))
    print("%s: lhs %.15g rhs %.15g |d| / sum|gu du| = %.3e" % (sa.case_id(shape, layout, kind), lhs, rhs, abs(lhs - rhs) / scale))
    assert abs(lhs - rhs) <= 1e-12 * scale
    both = sa.jvp_ref(shape, kind, layout, KAPPA, "df") + sa.jvp_ref(shape, kind, layout, KAPPA, "dx")
    assert np.allclose(both, du, rtol=1e-9, atol=1e-10 * np.abs(du).max())


# the worst distance measured between the C oracle's sumregs_gradient and the literal system at kappa = 1e14, as a
# fraction of max|g| (2 x 70 x 72 "cross", 2 x 2 patch: 2.9e-6 at max|g| 27); the test allows ten times as much
ORACLE_WORST = 1.1e-7


@pytest.mark.parametrize("shape,kind,layout", ALL, ids=IDS)
def test_oracle_gradient_agrees_with_the_literal_system(shape, kind, layout):
    """oracle.sumregs_gradient (reg = 0; the reduced banded system of oracle/sumregs_oracle.c with the weight 1e14) against
    grad_x of the literal system at kappa = 1e14: within ten times the worst distance measured over these cases.
    Measured: at most 1.1e-7 max|g| (the strips of 2 x 70 x 72: 2.9e-6 at max|g| 27 for the patch, 2.3e-6 at 45 for the
    vector; every other case below 8.6e-8 max|g|).  The oracle refines three times against a reduced matrix that holds 1e14
    beside 1; the library at converged refinement is closer to the literal system than the oracle is."""
    gx = sa.vjp_ref(shape, kind, layout, KAPPA)[1]
    g0 = _oracle_gradient(shape, kind, layout)
    d, gmax = float(np.abs(g0 - gx).max()), float(np.abs(gx).max())
    print("%s: oracle vs literal max|d| %.3e = %.3e max|g| (max|g| %.3e)" % (sa.case_id(shape, layout, kind), d, d / gmax, gmax))
    assert g0.shape == gx.shape and d <= 10 * ORACLE_WORST * gmax


def _tiny():
    """One 6 x 7 image with a 3 x 3 flat block: 42 pixels, 4 forward, 4 backward and 1 centred active element besides the
    forced rows."""
    from conftest import synth_batch
    from oracle import np_twin_sumregs as ts
    _, f = synth_batch(1, 6, 7, seed=sa.SEED)
    u = ts.pdhg(f[0], sa.A3, maxiter=60)
    u[1:4, 2:5] = u[1, 2]
    rng = np.random.default_rng(3)
    return u, rng.standard_normal(u.shape), rng.standard_normal(3)


@pytest.mark.parametrize("kind", ["vector", "patch22"])
def test_rational_solve_agrees_on_a_tiny_planted_image(kind):
    """sumregs_jvp_ref.jvp_image_exact (the reduced system with kap = 1e14, formed and solved in rational arithmetic) against
    the literal saddle system at kappa = 1e14 on 42 pixels: 1e-10 max|du|.  Measured: 6.7e-14 (vector), 3.8e-14 (patch) at max|du| 3.7 and 5.3."""
    u, df, dv = _tiny()
    x = sa.x_kind(kind, 6, 7)
    dx = dv if kind == "vector" else np.random.default_rng(4).standard_normal(x.shape)
    assert sa.active_counts(u[None]).tolist() == [[5, 5, 1]]
    exact = jr.jvp_image_exact(u, x, df, dx, 0)
    lit = sa.jvp_image(u, x, df, dx, jr.KAPPA)
    d, scale = float(np.abs(exact - lit).max()), float(np.abs(exact).max())
    print("tiny %s: rational vs literal max|d du| %.3e (max|du| %.3e)" % (kind, d, scale))
    assert d <= 1e-10 * scale


@pytest.mark.parametrize("kind", ["vector", "patch22", "map"])
def test_the_reduced_reference_fails_on_planted_blocks(kind):
    """tests/sumregs_jvp_ref.jvp_image -- scipy's LU of the assembled reduced matrix, where 1 + 2e14 has rounded the
    identity away -- against the literal p on 2 x 40 x 48 "blocks": worse than 1e-6 max|p|, a hundred times what the GPU
    tests allow the library.  Measured: 3.7e-4 (vector), 4.8e-4 (2 x 2 patch), 1.5e-4 (map) of max|p|.  It stays the reference where the suite uses it, on images without
    an active set."""
    shape, layout = (2, 40, 48), "blocks"
    x, f, u, gu, df, dx = sa.case(shape, kind, layout)
    p, _, pmax = sa.vjp_ref(shape, kind, layout, KAPPA)
    old = np.stack([jr.jvp_image(u[k], x, gu[k], None, 0) for k in range(shape[0])])
    d = float(np.abs(old - p).max())
    print("%s: reduced scipy LU vs literal max|d p| %.3e = %.3e max|p|" % (kind, d, d / pmax))
    assert d > 1e-6 * pmax
