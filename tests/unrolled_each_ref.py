"""Per-image parameters for the numpy twins of the unrolled solve (DESIGN.md sections 4.6 and 4.7) -- TEST INFRASTRUCTURE ONLY.

unrolled_ref.fwd_tape / reverse and unrolled_jvp_ref.forward_tangent broadcast their parameter map against the (O, N, M)
batch, so a stacked (O, N, M) map is one parameter per image and the twins split image-wise bit for bit
(tests/test_unrolled_each_abi.py).  This module only stacks the maps and reduces the per-pixel terms per image."""
import numpy as np

import unrolled_ref as ur
from oracle import np_twin as tw


def stack_maps(alphas, M, N):
    """(O, N, M): np_twin.alpha_to_map of every block.  alphas: (O,) scalars or (O, n, m) blocks."""
    a = np.asarray(alphas, dtype=np.float64)
    return np.stack([tw.alpha_to_map(a[k], M, N) for k in range(a.shape[0])])


def reduce_alpha_each(ga, alphas):
    """The per-image parameter gradients in the shape of alphas: unrolled_ref.reduce_alpha's rule applied to one image."""
    a = np.asarray(alphas, dtype=np.float64)
    out = np.empty(a.shape)
    for k in range(a.shape[0]):
        out[k] = ur.reduce_alpha(ga[k:k + 1], a[k])
    return out


def alphas_of(kind, O, N, M, seed=21):
    """Per-image parameters that differ strongly between the images: the scalars 0.03, 0.08, 0.2 (cycled), 2 x 3 patches (cut
    down where the image has a single row / column) or maps drawn per image in [0.03, 0.2]."""
    rng = np.random.default_rng(seed)
    if kind == "scalar":
        return np.array([(0.03, 0.08, 0.2)[k % 3] for k in range(O)])
    if kind == "patch":
        return 0.03 + 0.17 * rng.random((O, min(2, N), min(3, M)))
    return 0.03 + 0.17 * rng.random((O, N, M))
