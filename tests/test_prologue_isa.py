"""Machine code of the headline instantiation, pdhg_tile_kernel<double,1,1,32,32,true,true> ("One
argument round trip"): every kernel-argument word is requested in the entry block and waited for once, so no scalar load
follows the kernel's first s_waitcnt; nothing but index arithmetic -- no branch -- lies between that wait and the state
loads, which go out back to back; at most 64 VGPRs (two 1024-thread workgroups per CU) and no scratch.  The general
instantiations fetch their arguments in one trip as well.  Compiled to assembly with the library's own flags;
cross-compiles without a GPU."""
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

HIPCC = shutil.which(os.environ.get("HIPCC", "hipcc"))
pytestmark = pytest.mark.skipif(HIPCC is None, reason="hipcc not found")

FAST = {"f64": "double, 1, 1, 32, 32, true, true", "f32": "float, 1, 1, 32, 32, true, true"}
GENERAL = {"f64 3-D grid": "double, 1, 1, 32, 32, true", "f64 1-D grid": "double, 1, 1, 32, 32, false",
           "f32 3-D grid": "float, 1, 1, 32, 32, true", "f64 4 px": "double, 2, 2, 32, 32, true"}
SCALAR_LOADS = ("s_load", "s_buffer_load")


def _kernel_asm(tmp_path, targs):
    """The kernel's instructions (all of its blocks, up to its descriptor) and its register / scratch figures."""
    src = tmp_path / "inst.hip"
    src.write_text('#include "pdhg_kernels.hpp"\n'
                   "template __global__ void bpltv::pdhg_tile_kernel<%s>(bpltv::PdhgArgs);\n" % targs)
    out = tmp_path / "inst.s"
    flags = [f for f in ge.HIPCC_FLAGS if f not in ("-shared", "-fPIC")]
    subprocess.check_call([HIPCC] + flags + ["-Wno-unused-command-line-argument", "-S", "--cuda-device-only", "-I", ge.CSRC,
                                             str(src), "-o", str(out)])
    lines = out.read_text().splitlines()
    start = next(i for i, l in enumerate(lines) if re.match(r"_ZN5bpltv16pdhg_tile_kernel\S*:", l))
    end = next(i for i in range(start, len(lines)) if lines[i].strip().startswith(".amdhsa_kernel _ZN5bpltv16pdhg_tile_kernel"))
    desc = "\n".join(lines[end:end + 400])
    meta = {k: int(re.search(r"\.amdhsa_%s (\d+)" % k, desc).group(1)) for k in ("next_free_vgpr", "private_segment_fixed_size")}
    body = [l.split(";")[0].strip() for l in lines[start + 1:end]]
    return [l for l in body if l and not l.startswith(".")], meta


def _one_argument_round_trip(body):
    first_wait = next(i for i, l in enumerate(body) if l.startswith("s_waitcnt"))
    assert any(l.startswith(SCALAR_LOADS) for l in body[:first_wait])
    late = [l for l in body[first_wait:] if l.startswith(SCALAR_LOADS)]
    assert not late, late
    return first_wait


@pytest.mark.parametrize("name", list(FAST))
def test_headline_instantiation_one_round_trip_then_the_loads(tmp_path, name):
    body, meta = _kernel_asm(tmp_path, FAST[name])
    first_wait = _one_argument_round_trip(body)
    assert meta["next_free_vgpr"] <= 64, meta
    assert meta["private_segment_fixed_size"] == 0, meta
    assert sum(l.startswith("s_barrier") for l in body) >= 3 and any(l.startswith("v_fma_f") for l in body)   # it is the kernel
    # between the wait and the state loads: straight-line index arithmetic, far less than the ~190 instructions and ten
    # branches that stood there; then x, y1, y2, f and alpha back to back (address arithmetic of the last one between)
    loads = [i for i, l in enumerate(body) if l.startswith("global_load")]
    assert len(loads) >= 6 and loads[0] > first_wait        # five per pixel and the word of the step rows
    between = body[first_wait + 1:loads[0]]
    assert not [l for l in between if l.startswith(("s_cbranch", "s_branch", "s_waitcnt"))], between
    assert len(between) <= 64, len(between)
    assert loads[4] - loads[0] <= 6, body[loads[0]:loads[4] + 1]
    assert not [l for l in body[loads[0]:loads[4]] if l.startswith(("s_cbranch", "s_branch", "s_waitcnt"))]
    # no division by rho in this instantiation
    assert not [l for l in body if l.startswith(("v_div_", "v_rcp_"))]


@pytest.mark.parametrize("name", list(GENERAL))
def test_general_instantiations_one_round_trip(tmp_path, name):
    body, meta = _kernel_asm(tmp_path, GENERAL[name])
    _one_argument_round_trip(body)
    assert meta["private_segment_fixed_size"] == 0, meta
    if "1, 1, 32, 32" in GENERAL[name]:
        assert meta["next_free_vgpr"] <= 64, meta
