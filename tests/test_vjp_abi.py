"""The vector-Jacobian product and the PyTorch layer on a machine without a GPU: the library exports bpltv_vjp and
bpltv_vjp_device with the header's argument lists, the binding covers the header, the torch layer rejects wrong
inputs before it touches the library, and `import bpldenoising_amd` does not import torch_layer (no compute calls)."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest
from conftest import ROOT


def _header_args(name):
    txt = open(os.path.join(ROOT, "include", "bpltv.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name, txt)
    assert m, name
    return [a.strip() for a in m.group(1).split(",")]


def _ctype_of(decl):
    """ctypes argument type the binding uses for one C parameter declaration of the header."""
    from bpldenoising_amd import _lib
    d = " ".join(decl.split())
    if d.startswith("bpltv_t *"):
        return C.c_void_p
    if d.startswith("const bpltv_params *"):
        return _lib._PP
    if d.startswith("int "):
        return C.c_int
    assert "double *" in d, decl
    return "double*"


@pytest.mark.parametrize("name", ["bpltv_vjp", "bpltv_vjp_device"])
def test_library_exports_and_binds_vjp(name):
    from bpldenoising_amd import _lib
    lib = _lib.load()
    assert hasattr(lib, name)
    res, args = _lib.SYMBOLS[name]
    assert res is C.c_int
    hdr = _header_args(name)
    assert len(args) == len(hdr) == 10
    assert getattr(lib, name).argtypes == args
    for a, decl in zip(args, hdr):
        want = _ctype_of(decl)
        if want == "double*":   # host arrays: POINTER(c_double); device arrays: raw addresses
            assert a is (C.c_void_p if name.endswith("_device") else C.POINTER(C.c_double)), (decl, a)
        else:
            assert a is want, (decl, a)


def test_binding_still_covers_the_header_exactly():
    from bpldenoising_amd import _lib
    txt = open(os.path.join(ROOT, "include", "bpltv.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    assert sorted(_lib.SYMBOLS) == sorted(set(re.findall(r"\b(bpltv_[a-z_]+)\s*\(", txt)))
    assert _lib.load().bpltv_version() == 4


def test_vjp_signatures_match_the_gradient_conventions():
    """Same leading (handle, u, ...) order as bpltv_gradient; the device form takes raw addresses for every array."""
    from bpldenoising_amd import _lib
    host = _lib.SYMBOLS["bpltv_vjp"][1]
    dev = _lib.SYMBOLS["bpltv_vjp_device"][1]
    assert host[3:6] == dev[3:6] == [C.c_int, C.c_int, C.c_int]
    assert [i for i, a in enumerate(dev) if a is C.c_void_p] == [0, 1, 2, 7, 8, 9]


def test_import_does_not_import_the_torch_layer():
    code = ("import sys; sys.path.insert(0, %r); import bpldenoising_amd; "
            "print('bpldenoising_amd.torch_layer' in sys.modules)" % ROOT)
    out = subprocess.check_output([sys.executable, "-c", code], cwd=ROOT).decode().strip().splitlines()[-1]
    assert out == "False"


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
    with pytest.raises(TypeError, match="float64"):
        layer.tv_denoise(f, torch.tensor(0.1, dtype=torch.float64))
    with pytest.raises(TypeError, match="float64"):
        layer.tv_denoise(f.double(), torch.tensor(0.1, dtype=torch.float32))
    with pytest.raises(TypeError):
        layer.tv_denoise(f.double().numpy(), torch.tensor(0.1, dtype=torch.float64))


def test_torch_layer_rejects_cpu_tensors(layer):
    import torch
    f = torch.zeros(2, 8, 6, dtype=torch.float64)
    for alpha in (torch.tensor(0.1, dtype=torch.float64), torch.full((2, 3), 0.1, dtype=torch.float64),
                  torch.full((8, 6), 0.1, dtype=torch.float64)):
        with pytest.raises(ValueError, match="ROCm device"):
            layer.tv_denoise(f, alpha)
    with pytest.raises(ValueError, match="ROCm device"):
        layer.TVDenoise(0.1)(f)


def test_torch_layer_rejects_alpha_shapes(layer):
    import torch
    f = torch.zeros(2, 8, 6, dtype=torch.float64)
    for shape in ((3,), (9, 6), (8, 7), (0, 2), (1, 8, 6), (2, 2, 2)):
        with pytest.raises(ValueError, match="alpha must be"):
            layer.tv_denoise(f, torch.zeros(shape, dtype=torch.float64))
    for shape in ((6,), (1, 2, 8, 6), ()):
        with pytest.raises(ValueError, match="f must have shape"):
            layer.tv_denoise(torch.zeros(shape, dtype=torch.float64), torch.tensor(0.1, dtype=torch.float64))


def test_torch_layer_rejects_a_device_mismatch(layer):
    import torch
    f = torch.zeros(2, 8, 6, dtype=torch.float64)
    alpha = torch.tensor(0.1, dtype=torch.float64, device="meta")
    with pytest.raises(ValueError, match="alpha is on meta"):
        layer.tv_denoise(f, alpha)
    with pytest.raises(ValueError, match="alpha is on cpu"):
        layer.tv_denoise(f.to("meta"), torch.tensor(0.1, dtype=torch.float64))
