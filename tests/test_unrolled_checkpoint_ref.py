"""Checkpointing the unrolled tape on the CPU, with the numpy twin tests/unrolled_ref.py: saving the
iteration state every C iterations, re-taping each segment from its saved state and reversing segment by segment -- the
cotangents carried from one segment to the one before -- reproduces unrolled_ref.reverse on the full tape BITWISE.  The
segment loops below restate the twin's loop bodies operation for operation; what is under test is the scheme itself: which
state a segment starts from, the segment-relative tape slot k - k0 against the absolute row k of the step table, and the
carry.  The automatic spacing of TVSolver.auto_checkpoint_every is held against a brute-force minimum of the memory formula."""
import numpy as np
import pytest
from conftest import synth_batch

import unrolled_ref as ur
from oracle import np_twin as tw

O, N, M, K = 2, 17, 33, 53


def _forward_segment(f, amap, state, tab, k0, k1, tape):
    """Iterations [k0, k1) of unrolled_ref.fwd_tape from state = (x, y1, y2); tape (nullable): slot k - k0 receives the
    dual before the projection of iteration k.  Returns the state after iteration k1 - 1."""
    x, y1, y2 = state
    a2 = amap * amap
    for k in range(k0, k1):
        tau, sigma, omega = tab[k]
        div = tw.grad_fwd_T(y1, y2)
        xo = x
        x = (x - tau * (div - f)) / (1.0 + tau)
        xb = (1.0 + omega) * x - omega * xo
        d1, d2 = tw.grad_fwd(xb)
        y1 = y1 + sigma * d1
        y2 = y2 + sigma * d2
        if tape is not None:
            tape[k - k0, 0] = y1
            tape[k - k0, 1] = y2
        n2 = y1 * y1 + y2 * y2
        with np.errstate(all="ignore"):
            v = np.where(n2 > a2, amap * tw.rsqrt_nr(np.where(n2 > a2, n2, 1.0)), 1.0)
        y1 = y1 * v
        y2 = y2 * v
    return x, y1, y2


def _reverse_segment(carry, tape, tab, k0, k1, amap):
    """Iterations k1 - 1 ... k0 of unrolled_ref.reverse on a segment tape (slot k - k0), from carry = (gx, gy1, gy2, gf, ga)."""
    gx, gy1, gy2, gf, ga = carry
    a2 = amap * amap
    for k in range(k1 - 1, k0 - 1, -1):
        tau, sigma, omega = tab[k]
        z1, z2 = tape[k - k0]
        n2 = z1 * z1 + z2 * z2
        out = n2 > a2
        r = tw.rsqrt_nr(np.where(out, n2, 1.0))
        e1 = z1 * r
        e2 = z2 * r
        dot = e1 * gy1 + e2 * gy2
        gz1 = np.where(out, (amap * r) * (gy1 - e1 * dot), gy1)
        gz2 = np.where(out, (amap * r) * (gy2 - e2 * dot), gy2)
        ga = ga + np.where(out, dot, 0.0)
        gxb = sigma * tw.grad_fwd_T(gz1, gz2)
        gxn = gx + (1.0 + omega) * gxb
        c = 1.0 / (1.0 + tau)
        gf = gf + tau * c * gxn
        d1, d2 = tw.grad_fwd(gxn)
        gy1 = gz1 - tau * c * d1
        gy2 = gz2 - tau * c * d2
        gx = c * gxn - omega * gxb
    return gx, gy1, gy2, gf, ga


def _case(kind):
    _, f = synth_batch(O, N, M, seed=5 + M)
    gu = np.random.default_rng(105).standard_normal(f.shape)
    amap = tw.alpha_to_map(0.08 if kind == "scalar" else 0.05 + 0.1 * np.random.default_rng(8).random((N, M)), M, N)
    return f, gu, amap


@pytest.mark.parametrize("kind", ["scalar", "map"])
@pytest.mark.parametrize("C", [1, 7, 53, 60])
def test_segment_by_segment_is_the_full_tape_bitwise(kind, C):
    f, gu, amap = _case(kind)
    u0, tape0, tab = ur.fwd_tape(f, amap, K)
    gf0, ga0 = ur.reverse(gu, tape0, tab, amap)
    ceff = min(C, K)
    nseg = -(-K // ceff)
    # the checkpoint pass: no tape, the state at the start of every segment
    state = (f.copy(), np.zeros_like(f), np.zeros_like(f))
    checkpoints = []
    for s in range(nseg):
        checkpoints.append(tuple(a.copy() for a in state))
        state = _forward_segment(f, amap, state, tab, s * ceff, min((s + 1) * ceff, K), None)
    assert np.array_equal(state[0], u0)
    # the sweep: one segment tape, reused
    seg_tape = np.full((ceff, 2) + f.shape, np.nan)
    carry = (np.array(gu), np.zeros_like(f), np.zeros_like(f), np.zeros_like(f), np.zeros_like(f))
    for s in range(nseg - 1, -1, -1):
        k0, k1 = s * ceff, min((s + 1) * ceff, K)
        _forward_segment(f, amap, checkpoints[s], tab, k0, k1, seg_tape)
        assert np.array_equal(seg_tape[:k1 - k0], tape0[k0:k1])
        carry = _reverse_segment(carry, seg_tape, tab, k0, k1, amap)
    gx, _, _, gf, ga = carry
    assert np.array_equal(gf + gx, gf0) and np.array_equal(ga, ga0)
    assert gf0.any() and ga0.any()


@pytest.mark.parametrize("model,nplanes,tape_planes", [("tv", 3, 2), ("weighted", 3, 3), ("sumregs", 7, 6)])
def test_the_automatic_spacing_is_the_least_memory_within_one_segment(model, nplanes, tape_planes):
    """planes(C) = nplanes * ceil(K / C) + tape_planes * C.  C* = sqrt(nplanes * K / tape_planes) minimises the smooth bound
    nplanes * K / C + tape_planes * C; rounding C* up costs at most tape_planes planes, and the ceiling of K / C at most
    nplanes: planes(auto) <= min planes + nplanes + tape_planes -- one segment's worth (a checkpoint and an iteration of tape)."""
    from bpldenoising_amd import TVSolver

    def planes(K, c):
        return nplanes * -(-K // c) + tape_planes * c

    for K in list(range(1, 130)) + [203, 1000, 5000, 77777]:
        c = TVSolver.auto_checkpoint_every(K, model)
        assert 1 <= c <= K
        assert c * c * tape_planes >= nplanes * K or c == K
        assert c == 1 or (c - 1) * (c - 1) * tape_planes < nplanes * K
        best = min(planes(K, q) for q in range(1, K + 1))
        assert planes(K, c) <= best + nplanes + tape_planes, (model, K, c, planes(K, c), best)
    assert TVSolver.auto_checkpoint_every(5000, "tv") == 87 and TVSolver.auto_checkpoint_every(60) == 10
    with pytest.raises(ValueError):
        TVSolver.auto_checkpoint_every(0)
