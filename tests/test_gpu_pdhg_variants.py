"""Every kernel variant of the plain TV solve against the oracle at every depth and seam.

The 36 variants of kVariants (csrc/bpltv.hip) in Float64 and Float32: one pytest case per (variant, dtype), which runs
the variant on the shapes and depths of tests/pdhg_plan_ref.py -- per depth the smallest images that hold an interior
tile, a last tile pulled back as far as it goes, a last tile that is not shifted, a single tile without halo, and an
image shorter than a region along one axis; the depths 1, 2, 8, the first halo wider than a thread's strip, and the
deepest two the halo admits (the single tile: the 32 step rows of pdhg_tile_kernel, 40 for the kernels without that
array).  Every (depth, shape) runs a scalar, a patch and a map parameter with and without the Huber term; the shapes
with a shifted tile also two launch chains out of phase, eager launches and the 1-D grid.  Every result is compared BIT
FOR BIT with the C oracle (oracle.pdhg / oracle.pdhg_f32), never with another GPU run, and every solve's plan statistics
with the restatement: variant, depth, region, tiles, launch chains, launches.  About 8600 solves of about a millisecond
per precision: the slowest case takes 0.7 s on the MI355X."""
import numpy as np
import pytest

import pdhg_plan_ref as pr
from conftest import synth_batch

pytestmark = pytest.mark.gpu

O = 2
RHO = 0.3
PATCH = np.array([[0.05, 0.12, 0.07], [0.2, 0.08, 0.1]])      # 2 blocks along j, 3 along i: divides neither axis of any shape here
_DATA, _REF = {}, {}                                          # shared by the cases: many variants have the same region


def _data(O_, N, M):
    if (O_, N, M) not in _DATA:
        _DATA[(O_, N, M)] = synth_batch(O_, N, M, seed=11 + (N * 7 + M) % 89)
    return _DATA[(O_, N, M)]


def _alpha(pname, N, M):
    if pname == "scalar":
        return 0.09
    if pname == "patch":
        return PATCH if (N >= PATCH.shape[0] and M >= PATCH.shape[1]) else np.array([[0.07]])
    return 0.03 + 0.15 * np.random.default_rng(6).random((N, M))


def _ref(oracle, dtype, O_, N, M, pname, K, rho):
    key = (O_, N, M, pname, K, rho, dtype)
    if key not in _REF:
        f = _data(O_, N, M)[1]
        fn = oracle.pdhg if dtype == 64 else oracle.pdhg_f32
        u0 = fn(f, _alpha(pname, N, M), maxiter=K, rho=rho)
        u0.setflags(write=False)
        _REF[key] = u0
    return _REF[key]


def _where(u, u0):
    bad = np.argwhere(u != u0)
    lo, hi = bad.min(axis=0), bad.max(axis=0)
    return "%d pixels differ, images %d-%d, j %d-%d, i %d-%d, max|du| = %.3g" % (
        len(bad), lo[0], hi[0], lo[1], hi[1], lo[2], hi[2], np.abs(u - u0).max())


class _Runner:
    """One handle on one shape; every solve is held to the oracle's bits and to the restated plan."""

    def __init__(self, cls, oracle, v, dtype, N, M, O_=O):
        self.oracle, self.v, self.dtype, self.N, self.M, self.O = oracle, v, dtype, N, M, O_
        self.s = cls(M, N, O_, dtype=dtype)
        self.s.set_data(*_data(O_, N, M))
        self.failed = []
        self.solves = 0

    def solve(self, T, K, pname="scalar", rho=0.0, chains=1, graph=1, xcd=0, ask=None, variant=None):
        """A solve that asks for `ask` (default T) iterations per launch and must run T."""
        v = self.v
        tag = (v, self.dtype, (self.N, self.M), "T=%d" % T, "ask=%s" % ask, "K=%d" % K, pname, "rho=%g" % rho,
               "chains=%d" % chains, "graph=%d" % graph, "xcd=%d" % xcd)
        kw = dict(variant=v) if variant is None else ({} if variant == 0 else dict(variant=variant))
        if xcd:
            kw["xcd"] = 1
        u = self.s.denoise(_alpha(pname, self.N, self.M), maxiter=K, rho=rho, tile_iters=T if ask is None else ask,
                           chains=chains, use_graph=graph, **kw)
        self.solves += 1
        st = self.s.stats()
        ri, rj, ntiles = pr.plan(v, self.N, self.M, self.O, T)
        nl, nch = pr.launches(K, T, min(chains, self.O), graph=bool(graph))
        want = dict(pdhg_variant=v, tile_iters=T, region_i=ri, region_j=rj, tiles=ntiles, launch_chains=nch, launches=nl,
                    iterations=K, graph_used=graph)
        got = {k: st[k] for k in want}
        assert got == want, (tag, got, want)           # the plan: a wrong table is a red test at the first solve
        u0 = _ref(self.oracle, self.dtype, self.O, self.N, self.M, pname, K, rho)
        if not np.array_equal(u, u0):
            self.failed.append((tag, _where(u, u0)))

    def close(self):
        self.s.close()


def _by_shape(v):
    out = {}
    for T, cls, shape in pr.cases(v):
        out.setdefault((cls, shape), []).append(T)
    return out


@pytest.mark.parametrize("dtype", [64, 32])
@pytest.mark.parametrize("v", sorted(pr.VARIANTS))
def test_variant_is_bit_identical_at_every_depth_and_seam(gpu_solver_cls, oracle, v, dtype):
    from bpldenoising_amd._lib import BpltvError
    V = pr.VARIANTS[v]
    failed, solves, handles = [], 0, 0
    for (cls, (N, M)), Ts in sorted(_by_shape(v).items()):
        cap = pr.deepest(v, N, M)
        top = cap if cap < pr.NO_CAP else max(Ts)       # a single tile of a kernel without the step-row array: no cap
        r = _Runner(gpu_solver_cls, oracle, v, dtype, N, M)
        handles += 1
        for T in Ts:
            # K = 2T + 1: two full launches and a launch of one iteration.  Every parameter form, without and with the
            # Huber division of the kernels' general path (a solve takes about a millisecond: no need to thin this)
            for rho in (0.0, RHO):
                for pname in ("scalar", "patch", "map"):
                    r.solve(T, 2 * T + 1, pname, rho=rho)
            if cls == "shift":
                # two launch chains, the second half a launch out of phase (one launch more) from T = 2 on
                assert pr.chain_out_of_phase(8 * T, T) == (T >= 2)
                r.solve(T, 8 * T, chains=2)
                r.solve(T, 8 * T, chains=2, graph=0)         # eager launches: one chain
                if T == top:
                    # the 1-D grid with the XCD-aware tile order: pdhg_tile_kernel's other instantiation, the other
                    # branch of the block decode in the rows, rows2, rowsw and stream kernels
                    for pname in ("scalar", "patch"):
                        r.solve(T, 2 * T + 1, pname, xcd=1)
                        r.solve(T, 2 * T + 1, pname, xcd=1, graph=0)
        # one request beyond the cap: clamped, the same bits -- or, the LDS-tile kernels beyond their step rows, refused
        T0 = Ts[-1]
        if cap < pr.NO_CAP:
            T1 = pr.granted(v, N, M, cap + 1)
            if T1 is None:
                assert V.lds_rows and cap == pr.MAX_T
                with pytest.raises(BpltvError) as e:
                    r.s.denoise(0.09, maxiter=2 * T0 + 1, variant=v, tile_iters=cap + 1)
                assert e.value.code == 1 and "at most 32" in str(e.value), str(e.value)
                r.solve(T0, 2 * T0 + 1)                 # the handle's next solve keeps its bits
            else:
                assert T1 == cap
                r.solve(cap, 2 * T0 + 1, ask=cap + 1)
        failed += r.failed
        solves += r.solves
        r.close()
    # a forced variant on an image below its min_image is refused; the handle's next solve keeps its bits
    if V.min_image:
        N, M = (V.RJ - 1, V.RI) if V.min_image == 1 else (V.RJ, V.RI - 1)
        assert pr.too_small(v, N, M)
        r = _Runner(gpu_solver_cls, oracle, 1, dtype, N, M)
        handles += 1
        with pytest.raises(BpltvError, match="at least %dx%d" % (V.RI, V.RJ)) as e:
            r.s.denoise(0.09, maxiter=9, variant=v, tile_iters=4)
        assert e.value.code == 1
        r.solve(4, 9)                                   # variant 1, 32 x 32 regions
        failed += r.failed
        solves += r.solves
        r.close()
    print("variant %d dtype %d: %d solves on %d handles" % (v, dtype, solves, handles))
    assert not failed, "%d of %d solves differ from the oracle: %s" % (len(failed), solves, failed[:12])


AUTO_SHAPES = [(1, 300, 60), (1, 60, 300), (2, 300, 270)]


@pytest.mark.parametrize("dtype", [64, 32])
@pytest.mark.parametrize("shape", AUTO_SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_automatic_plan_on_long_images_matches_oracle(gpu_solver_cls, oracle, shape, dtype):
    """No variant= : a narrow, long image runs the 48 x 48 tile kernel, an image of at least a rows region the 64-lane
    rows; at the planner's depth, at 12 and at the deepest halo a region of 48 admits."""
    O_, N, M = shape
    probe = _Runner(gpu_solver_cls, oracle, 1, dtype, N, M, O_)
    probe.s.denoise(0.09, maxiter=1)
    ncu = probe.s.stats()["ncu"]
    probe.close()
    v = pr.auto_variant(N, M, O_, ncu)
    assert v == (13 if min(N, M) < 64 else 20 if ncu >= 256 else v)    # (19 on a device of few compute units)
    cap = pr.depth_cap(v, N, M)
    assert cap == (31 if v == 19 else 23)
    r = _Runner(gpu_solver_cls, oracle, v, dtype, N, M, O_)
    for ask, T in ((0, 8), (12, 12), (23, 23), (cap + 1, cap)):
        for pname in ("scalar", "map"):
            r.solve(T, 2 * T + 3, pname, ask=ask, variant=0, chains=1)
    r.solve(8, 19, "patch", rho=RHO, ask=0, variant=0, chains=1)
    r.close()
    assert not r.failed, r.failed
