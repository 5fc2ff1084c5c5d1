"""What `gn_fold_ibf_kernel` costs in registers, read from the metadata of the code object in libganon_hip.so (no GPU).  The kernel
streams its source: what hides the latency of its loads is the waves a SIMD holds, each lane with four 8-byte loads in flight, so a
compiler that pushes it into scratch, or below the occupancy DESIGN states, shows as a failing test and not as a slower `--fold`."""
import os
import re
import shutil
import subprocess

import pytest

from ganon_amd import build as B
from test_build_update_kernel_cpu import llvm_tool

KERNEL = "_Z18gn_fold_ibf_kernel12GnFoldParams"


@pytest.fixture(scope="module")
def kernel_metadata(tmp_path_factory):
    """{field: int} of the kernel's entry in the amdhsa.kernels note of the gfx950 code object that holds it"""
    assert os.path.exists(B.LIB), "libganon_hip.so is built by __graft_entry__.build()"
    d = tmp_path_factory.mktemp("code_objects")
    lib = shutil.copy(B.LIB, str(d / "lib.so"))  # (the bundles are written beside the file they come from)
    subprocess.run([llvm_tool("llvm-objdump"), "--offloading", lib], check=True, capture_output=True)
    found = None
    for f in sorted(os.listdir(d)):
        if "gfx950" not in f:
            continue
        notes = subprocess.run([llvm_tool("llvm-readelf"), "--notes", str(d / f)], check=True, capture_output=True, text=True).stdout
        for block in re.split(r"\n  - ", notes):  # one kernel each
            if re.search(r"\.name:\s+" + KERNEL + r"\s*\n", block):
                found = {k: int(x) for k, x in re.findall(r"\n\s*\.(\w+):\s+(\d+)\s*(?=\n)", "\n" + block + "\n")}
    assert found is not None, f"{KERNEL} not found in the gfx950 code objects of {B.LIB}"
    return found


def test_fold_kernel_does_not_spill(kernel_metadata):
    m = kernel_metadata
    print({k: m[k] for k in ("vgpr_count", "agpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size", "group_segment_fixed_size")})
    assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, "no scratch, no spill"
    assert m["wavefront_size"] == 64 and m["max_flat_workgroup_size"] == 256
    assert m["group_segment_fixed_size"] == 0, "the hits are dynamic LDS, sized by the call"


def test_fold_kernel_keeps_its_waves(kernel_metadata):
    """512 registers a SIMD lane, allocated in blocks of 8: at most 64 registers are eight waves a SIMD, 32 a CU, each lane with four
    8-byte loads of its rows in flight: 32 * 64 * 32 = 64 KiB a CU, above the 32 KiB a CU that keep HBM streaming.  The compiler gives the
    kernel 38 (ROCm 7.2).  At most 80 scalar registers keep eight 256-thread blocks admitted to a CU."""
    m = kernel_metadata
    assert m["vgpr_count"] + m["agpr_count"] <= 64, m
    assert m["sgpr_count"] <= 80, m
