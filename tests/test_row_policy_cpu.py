"""The stream kernels -- the fast count kernels with non-temporal row loads (gn_kernels.hip, gn_row_policy.h) -- read from the code
object in libganon_hip.so as test_lean_screen_cpu.py and test_screen_table_cpu.py do for the plain ones: they exist under their own
names, keep the register budgets of the kernels they stand beside, and the policy is in the instructions: `nt` on the row loads of
the stream kernels' loops, on no load of the plain kernels.  No result can show a policy lost in inlining; this does."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

from ganon_amd import build as B
from test_build_update_kernel_cpu import llvm_tool

LEAN, LEAN_STREAM = "_Z29gn_ibf_count_fast_kernel_lean13GnCountParams", "_Z31gn_ibf_count_stream_kernel_lean13GnCountParams"
# (hash functions, words a lane, EE, WIDE, SCRN): the screening instances, of 8-byte lanes (`lean_screen`) and of wide rows.  The
# instances without a screen, <4,1,true,false,false> and <4,2,true,true,false>, have no stream twin: they measured slower with one
# (gn_row_policy.h).
STREAM_INSTANCES = [(4, 1, 1, 0, 1), (4, 2, 1, 1, 1)]

def _instance(stem, key):
    return f"_Z{len(stem)}{stem}ILi{key[0]}ELi{key[1]}ELb{key[2]}ELb{key[3]}ELb{key[4]}EEv13GnCountParams"


@pytest.fixture(scope="module")
def kernels():
    """name -> (metadata of the code object's notes, the kernel's instructions) for every count kernel of the fast family"""
    assert os.path.exists(B.LIB), "libganon_hip.so is built by __graft_entry__.build()"
    out = {}
    with tempfile.TemporaryDirectory() as d:
        lib = shutil.copy(B.LIB, os.path.join(d, "lib.so"))
        subprocess.run([llvm_tool("llvm-objdump"), "--offloading", lib], check=True, capture_output=True)
        for f in sorted(os.listdir(d)):
            if "gfx950" not in f:
                continue
            co = os.path.join(d, f)
            notes = subprocess.run([llvm_tool("llvm-readelf"), "--notes", co], check=True, capture_output=True, text=True).stdout
            meta = {}
            for block in re.split(r"\n  - ", notes):
                m = re.search(r"\.name:\s+(_Z\d+gn_ibf_count_(?:fast|stream)_kernel\w*13GnCountParams)\s*\n", block)
                if m:
                    meta[m.group(1)] = {k: int(v) for k, v in re.findall(r"\n\s*\.(\w+):\s+(\d+)\s*(?=\n)", "\n" + block + "\n")}
            dis = subprocess.run([llvm_tool("llvm-objdump"), "-d", co], check=True, capture_output=True, text=True).stdout
            for sec in re.split(r"\n(?=[0-9a-f]+ <)", dis):
                m = re.match(r"[0-9a-f]+ <(\S+)>:", sec)
                if m and m.group(1) in meta:
                    insns = [re.sub(r"\s*//.*$", "", line).strip() for line in sec.splitlines()[1:]]
                    out[m.group(1)] = (meta[m.group(1)], [i for i in insns if i])
    return out


def _loads(insns, width):
    """(all, non-temporal) global loads of `width` of a kernel"""
    every = [i for i in insns if i.startswith(f"global_load_{width} ")]
    return len(every), len([i for i in every if re.search(r"\bnt\b", i)])


def test_stream_kernels_exist_within_their_budgets(kernels):
    assert LEAN in kernels and LEAN_STREAM in kernels
    got = sorted(k for k in kernels if "gn_ibf_count_stream_kernel" in k)
    assert got == sorted([LEAN_STREAM] + [_instance("gn_ibf_count_stream_kernel", key) for key in STREAM_INSTANCES]), "these and no other"
    for key in STREAM_INSTANCES:
        assert _instance("gn_ibf_count_fast_kernel", key) in kernels, "the plain instance stays beside it"
    budget = {LEAN_STREAM: 96}
    for key in STREAM_INSTANCES:
        budget[_instance("gn_ibf_count_stream_kernel", key)] = 128 if key[1] == 1 else 256
    for name, regs in budget.items():
        m = kernels[name][0]
        print(name, {f: m[f] for f in ("vgpr_count", "agpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size")})
        assert m["vgpr_count"] + m["agpr_count"] <= regs, name
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0, name
    # the screen-only one as its plain twin: five waves a SIMD with nothing parked anywhere
    assert kernels[LEAN_STREAM][0]["sgpr_spill_count"] == 0
    assert kernels[LEAN_STREAM][0]["group_segment_fixed_size"] == kernels[LEAN][0]["group_segment_fixed_size"]


def test_lean_stream_row_loads_are_non_temporal_and_the_plain_kernel_has_none(kernels):
    n_plain, nt_plain = _loads(kernels[LEAN][1], "dwordx2")
    n_stream, nt_stream = _loads(kernels[LEAN_STREAM][1], "dwordx2")
    print(f"lean: {n_plain} dwordx2 loads, {nt_plain} nt; lean stream: {n_stream}, {nt_stream} nt")
    assert nt_plain == 0 and not any(re.search(r"\bnt\b", i) for i in kernels[LEAN][1]), "no cache policy on any instruction of the plain kernel"
    # an iteration of the screen loop is four row loads; the loop body, its prologue and its tail each issue iterations
    assert nt_stream >= 8 and nt_stream % 4 == 0
    # the rest -- hashes, the finish's word loads -- stays plain, and the two kernels differ in nothing else
    assert n_stream == n_plain and n_stream - nt_stream >= 3
    assert len(kernels[LEAN_STREAM][1]) == len(kernels[LEAN][1])
    assert not any(re.search(r"\bnt\b", i) for i in kernels[LEAN_STREAM][1] if not i.startswith("global_load_dwordx2 ")), "no store, no other load"


@pytest.mark.parametrize("key", STREAM_INSTANCES)
def test_instances_row_loads(kernels, key):
    width = "dwordx2" if key[1] == 1 else "dwordx4"  # a lane's words of a row: 8 or 16 bytes
    plain, stream = kernels[_instance("gn_ibf_count_fast_kernel", key)][1], kernels[_instance("gn_ibf_count_stream_kernel", key)][1]
    n_plain, nt_plain = _loads(plain, width)
    n_stream, nt_stream = _loads(stream, width)
    print(f"{key}: plain {n_plain} {width} loads, {nt_plain} nt; stream {n_stream}, {nt_stream} nt")
    assert not any(re.search(r"\bnt\b", i) for i in plain)
    assert n_stream == n_plain and nt_stream >= 8 and nt_stream % 4 == 0
    if key[1] == 2:
        assert nt_stream == n_stream, "16-byte loads are row loads and nothing else"
    assert not any(re.search(r"\bnt\b", i) for i in stream if not i.startswith(f"global_load_{width} "))
