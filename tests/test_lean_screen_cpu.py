"""What the screen-only fast count kernel (gn_kernels.hip, gn_ibf_count_fast_kernel_lean) costs in registers, read from the code
object in libganon_hip.so as test_screen_table_cpu.py does for the screening instances: five waves a SIMD are 102 registers a
lane at most; the kernel is built for 96 with nothing in scratch.  The instances it stands beside stay in the library: the
screening one (switch `lean_screen` launches it alone) and the one without a screen, which runs the units the new kernel leaves."""
import os
import re
import shutil
import subprocess
import tempfile

from ganon_amd import build as B
from test_build_update_kernel_cpu import llvm_tool
from test_screen_table_cpu import _fast_kernels


def _lean_kernels():
    assert os.path.exists(B.LIB), "libganon_hip.so is built by __graft_entry__.build()"
    out = {}
    with tempfile.TemporaryDirectory() as d:
        lib = shutil.copy(B.LIB, os.path.join(d, "lib.so"))
        subprocess.run([llvm_tool("llvm-objdump"), "--offloading", lib], check=True, capture_output=True)
        for f in sorted(os.listdir(d)):
            if "gfx950" not in f:
                continue
            notes = subprocess.run([llvm_tool("llvm-readelf"), "--notes", os.path.join(d, f)], check=True, capture_output=True, text=True).stdout
            for block in re.split(r"\n  - ", notes):
                m = re.search(r"\.name:\s+(_Z\d+gn_ibf_count_fast_kernel\w+13GnCountParams)\s*\n", block)
                if m and "ILi" not in m.group(1):  # (the template's instances carry their arguments in the name)
                    out[m.group(1)] = {k: int(v) for k, v in re.findall(r"\n\s*\.(\w+):\s+(\d+)\s*(?=\n)", "\n" + block + "\n")}
    return out


def test_lean_kernel_fits_five_waves():
    k = _lean_kernels()
    assert list(k) == ["_Z29gn_ibf_count_fast_kernel_lean13GnCountParams"]
    m = next(iter(k.values()))
    print({f: m[f] for f in ("vgpr_count", "agpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size",
                             "group_segment_fixed_size")})
    assert m["vgpr_count"] + m["agpr_count"] <= 96
    assert m["private_segment_fixed_size"] == 0
    assert m["vgpr_spill_count"] == 0
    assert m["sgpr_spill_count"] == 0


def test_the_instances_beside_it_are_still_there():
    k = _fast_kernels()
    assert (4, 1, 1, 0, 0) in k and (4, 1, 1, 0, 1) in k
