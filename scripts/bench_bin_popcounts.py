"""The two kernels `ganon-build --hibf --update` adds, through the library calls alone, for a run under
`rocprofv3 --kernel-trace --stats -- python scripts/bench_bin_popcounts.py`: an IBF of --gib GiB at W = 1, 8 and 64 words a row (64,
512 and 4096 bins), filled at density 1/2, is counted by gn_filter_bin_popcounts and copied into an IBF of the same width by
gn_filter_copy_ibf, --runs times each.  The copy reads the same bytes in the same pattern and writes them too: it is the memory roof of
the count at half the bytes per second.  The counts are checked (every bin within 1% of half the rows; the copy's counts equal the
source's).  Prints one JSON object with the host-side times of the calls (launch, wait and the copy of the counts included) and the
bytes per second they amount to; the kernels' own times are in the trace.   usage: bench_bin_popcounts.py [--gib 2] [--runs 3]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ganon_amd import hip as H  # noqa: E402


def opt(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


gib, runs = opt("--gib", 2.0), opt("--runs", 3)
out = {"gib": gib, "runs": runs, "cases": []}
for W in (1, 8, 64):
    bins = 64 * W
    rows = int(gib * (1 << 30)) // (8 * W)
    one = lambda: H.HipFilter.hibf([(None, bins, rows, 3)], [np.zeros(bins, np.int64)], [np.arange(bins, dtype=np.int64)], bins)
    src, dst = one(), one()
    src.fill_random(W, 1)
    case = {"W": W, "rows": rows, "bytes": rows * W * 8, "bin_popcounts_s": [], "copy_ibf_s": []}
    for _ in range(runs):
        t = time.time()
        counts = src.bin_popcounts(bins)
        case["bin_popcounts_s"].append(round(time.time() - t, 6))
        t = time.time()
        dst.copy_ibf(0, src, 0)
        case["copy_ibf_s"].append(round(time.time() - t, 6))
    assert (np.abs(counts.astype(np.float64) / rows - 0.5) < 0.01).all(), "a bin of a matrix filled at 1/2 is about half set"
    assert np.array_equal(dst.bin_popcounts(bins), counts), "the copy holds what the source holds"
    case["popcount_read_GBps"] = round(case["bytes"] / min(case["bin_popcounts_s"]) / 1e9, 1)
    case["copy_read_GBps"] = round(case["bytes"] / min(case["copy_ibf_s"]) / 1e9, 1)
    out["cases"].append(case)
    src.free()
    dst.free()
print(json.dumps(out))
