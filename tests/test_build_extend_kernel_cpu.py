"""What the two kernels of gn_filter_extend_path cost in registers, read from the metadata of the code object in libganon_hip.so (no
GPU): the marking sweep keeps 8 hashes and, per word of the run, 8 * H loaded row words a lane; neither sweep may reach for scratch,
and every instantiation stays at four waves a SIMD."""
import os
import re
import shutil
import subprocess

import pytest

from ganon_amd import build as B
from test_build_update_kernel_cpu import llvm_tool

KERNELS = [r"_Z21gn_extend_mark_kernelILj%dEE\w+" % h for h in (1, 2, 3, 4, 5)] + [r"_Z23gn_extend_insert_kernel\w+"]


@pytest.fixture(scope="module")
def metadata(tmp_path_factory):
    """{kernel name: {field: int}} of the gn_extend_* entries in the amdhsa.kernels notes of the gfx950 code objects"""
    assert os.path.exists(B.LIB), "libganon_hip.so is built by __graft_entry__.build()"
    d = tmp_path_factory.mktemp("code_objects")
    lib = shutil.copy(B.LIB, str(d / "lib.so"))  # (the bundles are written beside the file they come from)
    subprocess.run([llvm_tool("llvm-objdump"), "--offloading", lib], check=True, capture_output=True)
    out = {}
    for f in sorted(os.listdir(d)):
        if "gfx950" not in f:
            continue
        notes = subprocess.run([llvm_tool("llvm-readelf"), "--notes", str(d / f)], check=True, capture_output=True, text=True).stdout
        for block in re.split(r"\n  - ", notes):  # one kernel each
            name = re.search(r"\.name:\s+(_Z\d+gn_extend_\w+)\s*\n", block)
            if name:
                out[name.group(1)] = {k: int(v) for k, v in re.findall(r"\n\s*\.(\w+):\s+(\d+)\s*(?=\n)", "\n" + block + "\n")}
    return out


@pytest.mark.parametrize("kernel", KERNELS)
def test_extend_kernels_do_not_spill_and_keep_four_waves(metadata, kernel):
    found = [m for name, m in metadata.items() if re.fullmatch(kernel, name)]
    assert len(found) == 1, f"{kernel}: {sorted(metadata)}"
    m = found[0]
    print(kernel, {k: m[k] for k in ("vgpr_count", "agpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size")})
    assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, "no scratch, no spill"
    assert m["vgpr_count"] + m["agpr_count"] <= 128 and m["wavefront_size"] == 64 and m["max_flat_workgroup_size"] == 256, m
