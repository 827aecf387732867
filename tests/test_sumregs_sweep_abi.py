"""The batched sum-of-regularisers sweep on a machine without a GPU: the library exports it, the binding declares it,
the statistics struct reports its groups in the slot that was reserved, and generate_cost refuses a denoise function
it has no batched path for (no compute calls here)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
from conftest import ROOT


def test_library_exports_bpltv_sumregs_sweep():
    from bpldenoising_amd import _lib
    lib = _lib.load()
    assert hasattr(lib, "bpltv_sumregs_sweep")
    assert lib.bpltv_sumregs_sweep.argtypes is not None and len(lib.bpltv_sumregs_sweep.argtypes) == 8


def test_binding_declares_bpltv_sumregs_sweep():
    from bpldenoising_amd import _lib
    res, args = _lib.SYMBOLS["bpltv_sumregs_sweep"]
    assert res is C.c_int
    assert args == _lib.SYMBOLS["bpltv_sweep"][1]   # same signature as the TV sweep


def test_stats_sweep_groups_takes_the_reserved_slot(tmp_path):
    """sweep_groups sits where reserved_i was: right after sweep_shards, before launch_host_ms; the struct keeps its size."""
    from bpldenoising_amd import _lib
    src = tmp_path / "lay.c"
    src.write_text("\n".join([
        '#include <stdio.h>', '#include <stddef.h>', '#include "bpltv.h"', 'int main(void){',
        'printf("%zu %zu %zu %zu\\n", sizeof(bpltv_stats_t), offsetof(bpltv_stats_t, sweep_shards),',
        '       offsetof(bpltv_stats_t, sweep_groups), offsetof(bpltv_stats_t, launch_host_ms));',
        'return 0;}']))
    exe = tmp_path / "lay"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    size, o_shards, o_groups, o_host = (int(x) for x in subprocess.check_output([str(exe)]).decode().split())
    assert o_groups == o_shards + C.sizeof(C.c_int)
    assert o_host == 8 * ((o_groups + C.sizeof(C.c_int) + 7) // 8)
    assert size == C.sizeof(_lib.BpltvStats)
    assert _lib.BpltvStats.sweep_groups.offset == o_groups
    assert "reserved_i" not in dict(_lib.BpltvStats._fields_)
    assert "sweep_groups" in _lib.BpltvStats().as_dict()


def test_generate_cost_refuses_other_denoise_functions():
    from bpldenoising_amd.learning_function import generate_cost
    ub = np.zeros((1, 8, 8))
    with pytest.raises(TypeError, match="denoise_function"):
        generate_cost((ub, ub), np.array([0.1]), denoise_function=lambda data, x: data)
