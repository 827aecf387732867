"""Structure of the headline PDHG kernel's machine code: pdhg_tile_kernel<double,1,1,32,32> takes
the step sizes of its iterations from the rows the prologue copied into LDS, so its main loop holds no scalar load, and
none stands between the first barrier and the loop.  (A scalar load there is waited for in full -- LDS and scalar memory
share one counter, and scalar loads return out of order -- in front of a barrier at which the whole workgroup waits for
its slowest wave.)  Compiled to assembly with the library's own flags; cross-compiles without a GPU."""
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

INSTANCES = {
    "f64 3-D grid": "double, 1, 1, 32, 32, true",
    "f64 1-D grid": "double, 1, 1, 32, 32, false",
    "f32 3-D grid": "float, 1, 1, 32, 32, true",
    "f64 4 px": "double, 2, 2, 32, 32, true",
}


def _kernel_asm(tmp_path, targs):
    src = tmp_path / "inst.hip"
    src.write_text('#include "pdhg_kernels.hpp"\n'
                   "template __global__ void bpltv::pdhg_tile_kernel<%s>(bpltv::PdhgArgs);\n" % targs)
    out = tmp_path / "inst.s"
    flags = [f for f in ge.HIPCC_FLAGS if f not in ("-shared", "-fPIC")]
    subprocess.check_call([HIPCC] + flags + ["-Wno-unused-command-line-argument", "-S", "--cuda-device-only", "-I", ge.CSRC,
                                             str(src), "-o", str(out)])
    lines = out.read_text().splitlines()
    start = next(i for i, l in enumerate(lines) if re.match(r"_ZN5bpltv16pdhg_tile_kernel\S*:", l))
    end = next(i for i in range(start, len(lines)) if "s_endpgm" in lines[i])
    tail = "\n".join(lines[end:end + 400])
    vgprs = int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", tail).group(1))
    return [l.split(";")[0].strip() for l in lines[start:end + 1]], vgprs


def _main_loop(body):
    """(first, last) line of the largest natural loop: from the label a backward branch goes to, to that branch."""
    labels = {m.group(1): i for i, l in enumerate(body) for m in [re.match(r"(\.LBB\d+_\d+):", l)] if m}
    loops = []
    for i, l in enumerate(body):
        m = re.match(r"s_c?branch\S*\s+(\.LBB\d+_\d+)", l)
        if m and labels.get(m.group(1), i + 1) <= i:
            loops.append((labels[m.group(1)], i))
    assert loops, "no loop found"
    # merge back edges to the same or nested headers: the loop with the most instructions is the iteration
    return max(loops, key=lambda ab: ab[1] - ab[0])


@pytest.mark.parametrize("name", list(INSTANCES))
def test_no_scalar_load_in_or_in_front_of_the_loop(tmp_path, name):
    body, vgprs = _kernel_asm(tmp_path, INSTANCES[name])
    lo, hi = _main_loop(body)
    loop = body[lo:hi + 1]
    assert sum("s_barrier" in l for l in loop) == 2 and any("v_fma_f" in l for l in loop), (lo, hi)   # it is the iteration
    assert any(l.startswith("ds_read") for l in loop)
    in_loop = [l for l in loop if l.startswith(("s_load", "s_buffer_load"))]
    assert not in_loop, in_loop
    first_barrier = next(i for i, l in enumerate(body) if l.startswith("s_barrier"))
    assert first_barrier < lo
    between = [l for l in body[first_barrier:lo] if l.startswith(("s_load", "s_buffer_load"))]
    assert not between, between
    # the kernel arguments are fetched before the state loads are issued, and only there
    first_global = next(i for i, l in enumerate(body) if l.startswith("global_load"))
    late = [l for l in body[first_global:] if l.startswith(("s_load", "s_buffer_load"))]
    assert not late, late
    if "1, 1, 32, 32" in INSTANCES[name]:
        assert vgprs <= 64, vgprs    # two 1024-thread workgroups per CU
