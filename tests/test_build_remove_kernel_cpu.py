"""What `gn_copy_ibf_spans_kernel` costs in registers, read from the metadata of the code object in libganon_hip.so (no GPU).  The kernel
streams: what hides the latency of its loads is the waves a SIMD holds, each with the loads of a whole row piece in flight, so a
compiler that pushes it into scratch, or below the occupancy stated here, shows as a failing test and not as a slower `--remove`."""
import os
import re
import shutil
import subprocess

import pytest

from ganon_amd import build as B
from test_build_update_kernel_cpu import llvm_tool

KERNELS = {1: "_Z24gn_copy_ibf_spans_kernelILj1EEv16GnSpanCopyParams", 2: "_Z24gn_copy_ibf_spans_kernelILj2EEv16GnSpanCopyParams"}


@pytest.fixture(scope="module")
def kernel_metadata(tmp_path_factory):
    """{words a thread owns: {field: int}} of the kernels' entries in the amdhsa.kernels note of the gfx950 code object that holds them"""
    assert os.path.exists(B.LIB), "libganon_hip.so is built by __graft_entry__.build()"
    d = tmp_path_factory.mktemp("code_objects")
    lib = shutil.copy(B.LIB, str(d / "lib.so"))  # (the bundles are written beside the file they come from)
    subprocess.run([llvm_tool("llvm-objdump"), "--offloading", lib], check=True, capture_output=True)
    found = {}
    for f in sorted(os.listdir(d)):
        if "gfx950" not in f:
            continue
        notes = subprocess.run([llvm_tool("llvm-readelf"), "--notes", str(d / f)], check=True, capture_output=True, text=True).stdout
        for block in re.split(r"\n  - ", notes):  # one kernel each
            for v, name in KERNELS.items():
                if re.search(r"\.name:\s+" + name + r"\s*\n", block):
                    found[v] = {k: int(x) for k, x in re.findall(r"\n\s*\.(\w+):\s+(\d+)\s*(?=\n)", "\n" + block + "\n")}
    assert sorted(found) == [1, 2], f"{sorted(KERNELS.values())} not all found in the gfx950 code objects of {B.LIB}"
    return found


@pytest.mark.parametrize("v", [1, 2])
def test_span_copy_kernel_does_not_spill(kernel_metadata, v):
    m = kernel_metadata[v]
    print(v, {k: m[k] for k in ("vgpr_count", "agpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size")})
    assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, "no scratch, no spill"
    assert m["wavefront_size"] == 64 and m["max_flat_workgroup_size"] == 256


def test_span_copy_kernel_keeps_its_waves(kernel_metadata):
    """512 registers a SIMD lane, allocated in blocks of 8.  The compiler gives the two-word kernel 86 and the one-word kernel 50 (ROCm 7.2).
    Two words a thread at up to 96 registers are five waves a SIMD, twenty a CU, each lane with at least four 8-byte loads of a row in
    flight: 20 * 64 * 32 = 40 KiB a CU, above the 32 KiB a CU that keep HBM streaming.  One word a thread (a stride of one word: IBFs of
    at most 64 bins) has half the loads a lane, so it has to keep all eight waves: at most 64 registers."""
    two, one = kernel_metadata[2], kernel_metadata[1]
    assert two["vgpr_count"] + two["agpr_count"] <= 96, two
    assert one["vgpr_count"] + one["agpr_count"] <= 64, one
