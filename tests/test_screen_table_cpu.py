"""The host-side model that gives the fast count kernel its screen lengths (ganon_amd/csrc/gn_screen_table.h), built stand-alone with
g++ (no GPU), and what the screened instances cost in registers, read from the code object in libganon_hip.so as
test_build_update_kernel_cpu.py does for its kernel."""
import os
import re
import shutil
import subprocess

import pytest

import oracle
from ganon_amd import build as B
from test_build_update_kernel_cpu import llvm_tool

MAIN = r"""
#include "gn_screen_table.h"
#include <cstdio>
#include <cstdlib>
int main(int argc, char** argv)
{
    uint8_t ds[GN_SCREEN_NMAX + 1];
    gn_screen_table(atof(argv[1]), (uint32_t)atoi(argv[2]), (uint32_t)atoi(argv[3]), ds);
    for (uint32_t n = 1; n <= GN_SCREEN_NMAX; ++n)
        printf("%u %u\n", (unsigned)ds[n], gn_screen_cutoff_count(n, atof(argv[1])));
    return 0;
}
"""


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    d = tmp_path_factory.mktemp("screen_table")
    src = d / "main.cpp"
    src.write_text(MAIN)
    exe = str(d / "screen_table")
    subprocess.run(["g++", "-O1", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", B.CSRC, str(src), "-o", exe],
                   check=True)

    def run(cutoff, h, bins):
        out = subprocess.run([exe, repr(cutoff), str(h), str(bins)], check=True, capture_output=True, text=True).stdout.split()
        vals = [int(x) for x in out]
        return [0] + vals[0::2], [0] + vals[1::2]  # ds[n], T[n] with n = 1 .. 127 at their own index

    return run


def _tail(d, p, k):
    """P[Bin(d, p) >= k]"""
    from math import comb
    return sum(comb(d, j) * p ** j * (1 - p) ** (d - j) for j in range(max(k, 0), d + 1))


@pytest.mark.parametrize("cutoff", [0.55, 0.75, 0.9, 1.0])
def test_cutoff_count_is_the_oracles(table, cutoff):
    _, T = table(cutoff, 4, 4096)
    assert T[1:] == [oracle.threshold_cutoff(n, cutoff) for n in range(1, 128)]


@pytest.mark.parametrize("cutoff", [0.0, 0.2, 0.3, 0.55, 0.75, 0.9, 1.0])
@pytest.mark.parametrize("bins", [64, 4096, 8192])
def test_screen_lengths_follow_the_model(table, cutoff, bins):
    ds, T = table(cutoff, 4, bins)
    for n in range(1, 128):
        d = ds[n]
        if T[n] < 2:
            assert d == 0  # nothing can be ruled out
            continue
        surv = [bins * _tail(x, 0.25, T[n] - (n - x)) for x in range(n + 1)]
        if surv[n] > 0.5:
            assert d == 0  # even the whole read leaves stray bins in the race
        if d:
            # a bound of at least one, the expected survivors at most a half there and more than that one hash earlier
            assert n - T[n] < d <= n and surv[d] <= 0.5 + 1e-9 and (d == n - T[n] + 1 or surv[d - 1] > 0.5 - 1e-9)


def test_screen_lengths_known_values(table):
    ds, _ = table(0.75, 4, 4096)
    assert ds[17] in (14, 15)       # 1.4 stray bins expected after 14 hashes, 0.47 after 15
    assert 21 <= ds[35] <= 25       # the paired workloads: about 46 row fetches against 72
    for cutoff in (0.3, 0.55):      # tens to hundreds of stray bins at d = n
        assert not any(table(cutoff, 4, 4096)[0][1:31])
    for h in (1, 2, 3, 5):          # fewer than four rows a hash: no screen; five: left on the unscreened flow
        assert not any(table(0.75, h, 4096)[0])


def test_screen_lengths_grow_with_the_cutoffs_room(table):
    # a higher cutoff leaves less room for misses, so a screen -- where the table gives one at both cutoffs -- is no longer
    lo, _ = table(0.75, 4, 4096)
    hi, _ = table(0.9, 4, 4096)
    both = [n for n in range(1, 128) if lo[n] and hi[n]]
    assert len(both) > 40 and all(hi[n] <= lo[n] for n in both)


# ---- the code object: the screened instances keep their register budgets ----------------------------------------------------
def _fast_kernels():
    assert os.path.exists(B.LIB), "libganon_hip.so is built by __graft_entry__.build()"
    import tempfile
    out = {}
    with tempfile.TemporaryDirectory() as d:
        lib = shutil.copy(B.LIB, os.path.join(d, "lib.so"))
        subprocess.run([llvm_tool("llvm-objdump"), "--offloading", lib], check=True, capture_output=True)
        for f in sorted(os.listdir(d)):
            if "gfx950" not in f:
                continue
            notes = subprocess.run([llvm_tool("llvm-readelf"), "--notes", os.path.join(d, f)], check=True, capture_output=True, text=True).stdout
            for block in re.split(r"\n  - ", notes):
                m = re.search(r"\.name:\s+_Z24gn_ibf_count_fast_kernelILi(\d)ELi(\d)ELb(\d)ELb(\d)ELb(\d)EEv13GnCountParams\s*\n", block)
                if m:
                    out[tuple(int(x) for x in m.groups())] = {k: int(v) for k, v in re.findall(r"\n\s*\.(\w+):\s+(\d+)\s*(?=\n)", "\n" + block + "\n")}
    return out


def test_screened_instances_keep_their_budgets():
    k = _fast_kernels()
    # (hash functions, words a lane, EE, WIDE, SCRN): the two screening instances, and beside each the one a launch without a table entry runs
    head, wide, head0, wide0 = k[(4, 1, 1, 0, 1)], k[(4, 2, 1, 1, 1)], k[(4, 1, 1, 0, 0)], k[(4, 2, 1, 1, 0)]
    print({name: {f: m[f] for f in ("vgpr_count", "agpr_count", "vgpr_spill_count", "private_segment_fixed_size")}
           for name, m in (("4,1,EE,SCRN", head), ("4,2,EE,WIDE,SCRN", wide), ("4,1,EE", head0), ("4,2,EE,WIDE", wide0), ("4,2,EE", k[(4, 2, 1, 0, 0)]))})
    # 512 registers a SIMD lane: four waves at up to 128 (8-byte lanes), two at up to 256 (the wide build); nothing in scratch
    for m in (head, head0):
        assert m["vgpr_count"] + m["agpr_count"] <= 128
    for m in (wide, wide0):
        assert m["vgpr_count"] + m["agpr_count"] <= 256
    for m in (head, wide, head0, wide0):
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0
    # only those two shapes screen: no other instance carries the screen's code (the three-wave build of 16-byte lanes keeps the
    # 8 bytes of scratch a lane it had)
    assert sorted(key for key in k if key[4]) == [(4, 1, 1, 0, 1), (4, 2, 1, 1, 1)]
    assert k[(4, 2, 1, 0, 0)]["private_segment_fixed_size"] <= 8
