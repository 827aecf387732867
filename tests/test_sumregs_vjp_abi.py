"""The sum-of-regularisers vector-Jacobian product and its PyTorch layer on a machine without a GPU: the library
exports bpltv_sumregs_vjp, bpltv_sumregs_vjp_device and bpltv_sumregs_denoise_device with the header's argument lists,
and the torch layer rejects wrong inputs before it touches the library."""
import ctypes as C
import os
import re

import pytest
from conftest import ROOT


def _header_args(name):
    txt = open(os.path.join(ROOT, "include", "bpltv.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name, txt)
    assert m, name
    return [a.strip() for a in m.group(1).split(",")]


def _ctype_of(decl, device):
    from bpldenoising_amd import _lib
    d = " ".join(decl.split())
    if d.startswith("bpltv_t *"):
        return C.c_void_p
    if d.startswith("const bpltv_params *"):
        return _lib._PP
    if d.startswith("int "):
        return C.c_int
    assert "double *" in d, decl
    return C.c_void_p if device else C.POINTER(C.c_double)   # device arrays: raw addresses


@pytest.mark.parametrize("name,nargs", [("bpltv_sumregs_vjp", 10), ("bpltv_sumregs_vjp_device", 10),
                                        ("bpltv_sumregs_denoise_device", 5)])
def test_library_exports_and_binds(name, nargs):
    from bpldenoising_amd import _lib
    lib = _lib.load()
    assert hasattr(lib, name)
    res, args = _lib.SYMBOLS[name]
    assert res is C.c_int
    hdr = _header_args(name)
    assert len(args) == len(hdr) == nargs
    assert getattr(lib, name).argtypes == args
    for a, decl in zip(args, hdr):
        assert a is _ctype_of(decl, name.endswith("_device")), (decl, a)


def test_the_sumregs_forms_take_the_tv_argument_lists():
    """bpltv_sumregs_vjp(_device) and bpltv_sumregs_denoise_device: bpltv_vjp(_device)'s and bpltv_denoise_device's
    argument lists (only the parameter's length differs: 3*am*an)."""
    from bpldenoising_amd import _lib
    S = _lib.SYMBOLS
    assert S["bpltv_sumregs_vjp"][1] == S["bpltv_vjp"][1]
    assert S["bpltv_sumregs_vjp_device"][1] == S["bpltv_vjp_device"][1]
    assert S["bpltv_sumregs_denoise_device"][1] == S["bpltv_denoise_device"][1]
    for a, b in (("bpltv_sumregs_vjp", "bpltv_vjp"), ("bpltv_sumregs_vjp_device", "bpltv_vjp_device"),
                 ("bpltv_sumregs_denoise_device", "bpltv_denoise_device")):
        assert [" ".join(x.split()) for x in _header_args(a)] == [" ".join(x.split()) for x in _header_args(b)]


def test_solver_methods_exist():
    from bpldenoising_amd import TVSolver
    for m in ("sumregs_vjp", "sumregs_vjp_device", "sumregs_denoise_device"):
        assert callable(getattr(TVSolver, m))


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


def test_torch_layer_rejects_float32(layer):
    import torch
    f = torch.zeros(2, 8, 6, dtype=torch.float32)
    a = torch.full((3,), 0.1, dtype=torch.float64)
    with pytest.raises(TypeError, match="sumregs_denoise: .*float64"):
        layer.sumregs_denoise(f, a)
    with pytest.raises(TypeError, match="float64"):
        layer.sumregs_denoise(f.double(), a.float())
    with pytest.raises(TypeError):
        layer.sumregs_denoise(f.double(), a.numpy())


def test_torch_layer_rejects_cpu_tensors(layer):
    import torch
    f = torch.zeros(2, 8, 6, dtype=torch.float64)
    for shape in ((3,), (3, 2, 3), (3, 8, 6)):
        with pytest.raises(ValueError, match="ROCm device"):
            layer.sumregs_denoise(f, torch.full(shape, 0.1, dtype=torch.float64))
    with pytest.raises(ValueError, match="ROCm device"):
        layer.SumRegsDenoise([0.1, 0.1, 0.1])(f)


def test_torch_layer_rejects_alpha_shapes(layer):
    import torch
    f = torch.zeros(2, 8, 6, dtype=torch.float64)
    for shape in ((2,), (3, 9, 6), (3, 8, 7), (8, 6), (), (4,), (2, 8, 6), (3, 0, 2), (3, 6), (1, 3, 8, 6)):
        with pytest.raises(ValueError, match="alpha must be \\(3,\\)"):
            layer.sumregs_denoise(f, torch.zeros(shape, dtype=torch.float64))
    for shape in ((6,), (1, 2, 8, 6), ()):
        with pytest.raises(ValueError, match="f must have shape"):
            layer.sumregs_denoise(torch.zeros(shape, dtype=torch.float64), torch.full((3,), 0.1, dtype=torch.float64))


def test_torch_layer_rejects_a_device_mismatch(layer):
    import torch
    f = torch.zeros(2, 8, 6, dtype=torch.float64)
    a = torch.full((3,), 0.1, dtype=torch.float64)
    with pytest.raises(ValueError, match="alpha is on meta"):
        layer.sumregs_denoise(f, a.to("meta"))
    with pytest.raises(ValueError, match="alpha is on cpu"):
        layer.sumregs_denoise(f.to("meta"), a)


def test_the_tv_layer_keeps_its_checks(layer):
    """The shared argument check still gives the TV layer its own shapes and messages."""
    import torch
    f = torch.zeros(2, 8, 6, dtype=torch.float64)
    with pytest.raises(ValueError, match="tv_denoise: alpha must be 0-dim"):
        layer.tv_denoise(f, torch.full((3,), 0.1, dtype=torch.float64))
    with pytest.raises(ValueError, match="tv_denoise: f must be on a ROCm device"):
        layer.tv_denoise(f, torch.full((2, 3), 0.1, dtype=torch.float64))
