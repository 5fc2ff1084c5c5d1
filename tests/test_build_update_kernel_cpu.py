"""What `gn_bin_popcount_kernel` costs in registers, read from the metadata of the code object in libganon_hip.so (no GPU): the kernel
keeps 64 counters, 8 bit planes and 16 loaded words in registers, and stays at four waves a SIMD only while the compiler does not
allocate every counter as half of a register pair (the copy through `v_mov_b32` in front of the 64-bit atomicAdd).  A
compiler that changes that shows here, not as a slower index update."""
import os
import re
import shutil
import subprocess

import pytest

from ganon_amd import build as B

KERNEL = "_Z22gn_bin_popcount_kernel11GnPopParamsPy"


def llvm_tool(name):
    hipcc = os.path.realpath(B._hipcc())
    for d in (os.path.join(os.path.dirname(hipcc), "..", "llvm", "bin"), os.path.join(os.path.dirname(hipcc), "..", "lib", "llvm", "bin")):
        if os.path.exists(os.path.join(d, name)):
            return os.path.join(d, name)
    found = shutil.which(name)
    assert found, f"{name} of the ROCm LLVM not found beside {hipcc}"
    return found


@pytest.fixture(scope="module")
def kernel_metadata(tmp_path_factory):
    """{field: int} of the kernel's entry in the amdhsa.kernels note of the gfx950 code object that holds it"""
    assert os.path.exists(B.LIB), "libganon_hip.so is built by __graft_entry__.build()"
    d = tmp_path_factory.mktemp("code_objects")
    lib = shutil.copy(B.LIB, str(d / "lib.so"))  # (the bundles are written beside the file they come from)
    subprocess.run([llvm_tool("llvm-objdump"), "--offloading", lib], check=True, capture_output=True)
    for f in sorted(os.listdir(d)):
        if "gfx950" not in f:
            continue
        notes = subprocess.run([llvm_tool("llvm-readelf"), "--notes", str(d / f)], check=True, capture_output=True, text=True).stdout
        for block in re.split(r"\n  - ", notes):  # one kernel each
            if re.search(r"\.name:\s+" + KERNEL + r"\s*\n", block):
                return {k: int(v) for k, v in re.findall(r"\n\s*\.(\w+):\s+(\d+)\s*(?=\n)", "\n" + block + "\n")}
    raise AssertionError(f"{KERNEL} not found in any gfx950 code object of {B.LIB}")


def test_popcount_kernel_does_not_spill(kernel_metadata):
    m = kernel_metadata
    print({k: m[k] for k in ("vgpr_count", "agpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size")})
    assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, "no scratch, no spill"


def test_popcount_kernel_keeps_four_waves_a_simd(kernel_metadata):
    # 512 registers a SIMD lane, allocated in blocks of 8: four waves fit at up to 128 (vector + accumulation registers together)
    assert kernel_metadata["vgpr_count"] + kernel_metadata["agpr_count"] <= 128, kernel_metadata
    assert kernel_metadata["wavefront_size"] == 64 and kernel_metadata["max_flat_workgroup_size"] == 256
