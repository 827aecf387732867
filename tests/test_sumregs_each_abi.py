"""Per-image sum-of-regularisers weights on a machine without a GPU: the library exports
bpltv_sumregs_denoise_each(_device) and bpltv_sumregs_vjp_each(_device) with the header's argument lists, TVSolver and
torch_layer.sumregs_denoise_each reject wrong inputs before they touch the library, and sumregs_denoise still refuses to
read a batch dimension off alpha's shape."""
import ctypes as C
import os
import re

import numpy as np
import pytest
from conftest import ROOT

EACH = {"bpltv_sumregs_denoise_each": 6, "bpltv_sumregs_denoise_each_device": 5, "bpltv_sumregs_vjp_each": 10,
        "bpltv_sumregs_vjp_each_device": 10}
TWINS = {"bpltv_sumregs_denoise_each": "bpltv_sumregs_denoise",
         "bpltv_sumregs_denoise_each_device": "bpltv_sumregs_denoise_device",
         "bpltv_sumregs_vjp_each": "bpltv_sumregs_vjp", "bpltv_sumregs_vjp_each_device": "bpltv_sumregs_vjp_device"}


def _header_args(name):
    txt = open(os.path.join(ROOT, "include", "bpltv.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name, txt)
    assert m, name
    return [" ".join(a.split()) for a in m.group(1).split(",")]


@pytest.mark.parametrize("name", sorted(EACH))
def test_library_exports_and_binds_the_per_image_entry_points(name):
    from bpldenoising_amd import _lib
    lib = _lib.load()
    assert hasattr(lib, name)
    res, args = _lib.SYMBOLS[name]
    assert res is C.c_int
    hdr = _header_args(name)
    assert len(args) == len(hdr) == EACH[name]
    assert getattr(lib, name).argtypes == args
    for a, decl in zip(args, hdr):
        if decl.startswith("bpltv_t *"):
            assert a is C.c_void_p
        elif decl.startswith("const bpltv_params *"):
            assert a is _lib._PP
        elif decl.startswith("int "):
            assert a is C.c_int, decl
        else:   # host arrays: POINTER(c_double); device arrays: raw addresses
            assert "double *" in decl
            assert a is (C.c_void_p if name.endswith("_device") else C.POINTER(C.c_double)), (decl, a)


@pytest.mark.parametrize("name", sorted(TWINS))
def test_per_image_twins_take_their_twins_arguments(name):
    """Each per-image function has the argument list of its shared-parameter twin, in the binding and in the header
    (types, in order; the names differ by the plural)."""
    from bpldenoising_amd import _lib
    assert _lib.SYMBOLS[name] == _lib.SYMBOLS[TWINS[name]]
    types = lambda n: [re.sub(r"\w+$", "", d).strip() for d in _header_args(n)]
    assert types(name) == types(TWINS[name])


def test_version_is_unchanged():
    from bpldenoising_amd import _lib
    assert _lib.load().bpltv_version() == 4


class _NoLib:
    """A TVSolver stand-in whose library refuses every call: the argument checks must come first."""
    def __getattr__(self, name):
        raise AssertionError("the library was called (%s)" % name)


def _solver_without_library(O=3, N=8, M=6):
    from bpldenoising_amd.learning_function import TVSolver
    s = TVSolver.__new__(TVSolver)
    s._lib, s._h, s.M, s.N, s.O, s.dtype = _NoLib(), None, M, N, O, 64
    return s


def test_solver_rejects_bad_block_counts_and_shapes():
    s = _solver_without_library()
    z = np.zeros((3, 8, 6))
    for bad in (np.full((2, 3), 0.1), np.full((4, 3), 0.1), np.full(3, 0.1), np.full((3, 2), 0.1), np.full((3, 3, 2), 0.1),
                np.full((2, 3, 2, 3), 0.1), np.full((3, 2, 2, 3), 0.1), np.float64(0.1), np.full((3, 3, 1, 2, 3), 0.1)):
        with pytest.raises(ValueError, match="alphas"):
            s.sumregs_denoise_each(bad)
        with pytest.raises(ValueError, match="alphas"):
            s.sumregs_vjp_each(z, bad, z)
    with pytest.raises(ValueError, match="both False"):
        s.sumregs_vjp_each(z, np.full((3, 3), 0.1), z, want_f=False, want_alpha=False)
    for bad_u in (np.zeros((2, 8, 6)), np.zeros((3, 6, 8))):
        with pytest.raises(ValueError, match="expected"):
            s.sumregs_vjp_each(bad_u, np.full((3, 3), 0.1), z)


@pytest.fixture
def layer(monkeypatch):
    """torch_layer with every library entry refused: a rejection must come before any library call."""
    pytest.importorskip("torch")
    from bpldenoising_amd import torch_layer

    def no_library(*a, **k):
        raise AssertionError("the library was called")
    monkeypatch.setattr(torch_layer, "_solver", no_library)
    monkeypatch.setattr(torch_layer, "_sync", no_library)
    return torch_layer


def test_sumregs_denoise_each_rejects_dtypes(layer):
    import torch
    f = torch.zeros(2, 8, 6, dtype=torch.float64)
    a = torch.full((2, 3), 0.1, dtype=torch.float64)
    with pytest.raises(TypeError, match="float64"):
        layer.sumregs_denoise_each(f.float(), a)
    with pytest.raises(TypeError, match="float64"):
        layer.sumregs_denoise_each(f, a.float())
    with pytest.raises(TypeError):
        layer.sumregs_denoise_each(f.numpy(), a)
    with pytest.raises(TypeError):
        layer.sumregs_denoise_each(f, a.numpy())


def test_sumregs_denoise_each_rejects_devices(layer):
    import torch
    f = torch.zeros(2, 8, 6, dtype=torch.float64)
    for shape in ((2, 3), (2, 3, 2, 3), (2, 3, 8, 6)):
        with pytest.raises(ValueError, match="ROCm device"):
            layer.sumregs_denoise_each(f, torch.full(shape, 0.1, dtype=torch.float64))
    with pytest.raises(ValueError, match="alpha is on meta"):
        layer.sumregs_denoise_each(f, torch.full((2, 3), 0.1, dtype=torch.float64, device="meta"))


def test_sumregs_denoise_each_rejects_shapes(layer):
    import torch
    f = torch.zeros(2, 8, 6, dtype=torch.float64)
    for shape in ((), (3,), (2,), (3, 3), (2, 2), (2, 4), (3, 2), (3, 8, 6), (2, 8, 6), (2, 3, 8), (3, 2, 8, 6), (2, 3, 9, 6),
                  (2, 3, 8, 7), (2, 3, 0, 2), (2, 2, 8, 6), (2, 3, 1, 8, 6), (1, 3), (1, 3, 8, 6)):
        with pytest.raises(ValueError, match="alpha must be"):
            layer.sumregs_denoise_each(f, torch.zeros(shape, dtype=torch.float64))
    for shape in ((8, 6), (1, 2, 8, 6), (0, 8, 6)):
        with pytest.raises(ValueError, match="f must have shape"):
            layer.sumregs_denoise_each(torch.zeros(shape, dtype=torch.float64), torch.full((2, 3), 0.1, dtype=torch.float64))


def test_sumregs_denoise_still_rejects_a_batch_of_parameters(layer):
    """sumregs_denoise does not infer per-image mode from alpha's shape: (B, 3, ...) stays an error there."""
    import torch
    f = torch.zeros(2, 8, 6, dtype=torch.float64)
    for shape in ((2, 3), (2, 3, 2, 2), (2, 3, 8, 6), (1, 3, 8, 6), (1, 3)):
        with pytest.raises(ValueError, match="alpha must be"):
            layer.sumregs_denoise(f, torch.zeros(shape, dtype=torch.float64))
    # and tv_denoise_each keeps its own shapes: no slice dimension
    with pytest.raises(ValueError, match="alpha must be"):
        layer.tv_denoise_each(f, torch.zeros((2, 3, 8, 6), dtype=torch.float64))
