"""The move of an IBF that `ganon-build --hibf --update --remove` makes, through the library calls alone: an IBF of about --gib GiB at a
narrow stride (64 bins, one word a row) and at a wide one (1152 bins, a stride of 32 words) is moved into an IBF of the same rows by
  plain      gn_filter_copy_ibf
  identity   gn_filter_copy_ibf_spans with the one span {0, 0, bins}
  drop16     gn_filter_copy_ibf_spans with every 16th run of 4 bins left out (the bins behind close up)
one call each to warm up, then --runs (5) rounds that alternate the three.  Host-side times of the calls (launch, the upload of the span
table and the wait included); median, spread (max - min) and the bytes per second of source plus destination at the median.  The bit
counts of every result are checked against the source's.  Prints one JSON object.   usage: bench_copy_spans.py [--gib 1] [--runs 5]"""
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


def one(bins, rows):
    return H.HipFilter.hibf([(None, bins, rows, 3)], [np.zeros(bins, np.int64)], [np.arange(bins, dtype=np.int64)], bins)


gib, runs = opt("--gib", 1.0), opt("--runs", 5)
out = {"gib": gib, "runs": runs, "cases": []}
for bins in (64, 1152):
    W = (bins + 63) >> 6
    stride = int(H.load_library().gn_hibf_row_stride_words(W))
    rows = int(gib * (1 << 30)) // (8 * stride)
    run = 4
    kept = [(s, run * 15) for s in range(run, bins, run * 16)]  # runs 1 .. 15 of every 16 stay
    drop, at = [], 0
    for s, n in kept:
        n = min(n, bins - s)
        drop.append((s, at, n))
        at += n
    src, dst = one(bins, rows), one(bins, rows)
    src.fill_random(bins, 1)
    counts = src.bin_popcounts(bins)
    calls = {"plain": lambda: dst.copy_ibf(0, src, 0), "identity": lambda: dst.copy_ibf_spans(0, src, 0, [(0, 0, bins)]),
             "drop16": lambda: dst.copy_ibf_spans(0, src, 0, drop)}
    case = {"bins": bins, "stride_words": stride, "rows": rows, "bytes_moved": 2 * rows * stride * 8, "bins_kept_drop16": at, "spans_drop16": len(drop)}
    times = {k: [] for k in calls}
    for k, call in calls.items():  # warm up, and check what each leaves
        call()
        got = dst.bin_popcounts(bins)
        exp = counts.copy()
        if k == "drop16":
            exp = np.zeros(bins, dtype=np.uint64)
            for s, d, n in drop:
                exp[d:d + n] = counts[s:s + n]
        assert np.array_equal(got, exp), k
    for _ in range(runs):
        for k, call in calls.items():
            t = time.time()
            call()
            times[k].append(round(time.time() - t, 6))
    for k, v in times.items():
        med = sorted(v)[len(v) // 2]
        case[k] = {"s": v, "median_s": med, "spread_s": round(max(v) - min(v), 6), "GBps": round(case["bytes_moved"] / med / 1e9, 1)}
    out["cases"].append(case)
    src.free()
    dst.free()
print(json.dumps(out))
