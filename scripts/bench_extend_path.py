"""gn_filter_extend_path beside the insert, through the library calls alone, for a run under
`rocprofv3 --kernel-trace --stats -- python scripts/bench_extend_path.py`: the two-level tree of bench_probe_path.py -- a root of 64
merged bins, N / 64 user bins below every one of them, here runs of 4 bins each, sized for --max-fp 0.05 at h = 4 -- takes the first
half of N sets of H random hashes along their paths (gn_filter_emplace_path); then the sets' last three quarters (a third of which the
tree holds) are added with gn_filter_extend_path, the quotas dealt evenly from gn_filter_probe_path's lost_at of the leaf entry.  A new
filter per run: a second extension would find everything present.  Prints one JSON object with the host-side times of the calls (the
staging uploads included: one for the insert, two for the extension); the kernels' own times are in the trace.
usage: bench_extend_path.py [N=512] [H=100000] [--runs 3]"""
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ganon_amd import hip as H  # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("--")]
runs = int(sys.argv[sys.argv.index("--runs") + 1]) if "--runs" in sys.argv else 3
if "--runs" in sys.argv:
    args.remove(sys.argv[sys.argv.index("--runs") + 1])
n = int(args[0]) if len(args) > 0 else 512
hashes = int(args[1]) if len(args) > 1 else 100000
assert n % 64 == 0
h, max_fp, per, split = 4, 0.05, n // 64, 4


def rows_for(count):  # the textbook size of one bin
    return int(math.ceil(-h * count / math.log(1.0 - math.exp(math.log(max_fp) / h))))


rng = np.random.default_rng(1)
sets = [np.unique(rng.integers(0, 1 << 62, size=hashes, dtype=np.uint64)) for _ in range(n)]
base = [s[:len(s) // 2] for s in sets]
more = [s[len(s) // 4:] for s in sets]
shapes = [(None, 64, rows_for(per * hashes), h)] + [(None, per * split, rows_for(hashes // split), h)] * 64
nx = [np.arange(1, 65, dtype=np.int64)] + [np.full(per * split, i, np.int64) for i in range(1, 65)]
bu = [np.full(64, -1, np.int64)] + [np.repeat(np.arange((i - 1) * per, i * per, dtype=np.int64), split) for i in range(1, 65)]
paths = np.zeros((n, 2), dtype=H.PATH_DTYPE)
for u in range(n):
    paths[u, 0] = (1 + u // per, (u % per) * split, split, 0, (len(base[u]) + split - 1) // split)
    paths[u, 1] = (0, u // per, 1, 0, 1)
out = {"user_bins": n, "bins_per_run": split, "hashes_inserted": int(sum(len(s) for s in base)), "hashes_extended": int(sum(len(s) for s in more)),
       "emplace_path_s": [], "probe_path_s": [], "extend_path_s": [], "absent": 0}
for _ in range(runs):
    flt = H.HipFilter.hibf(shapes, nx, bu, n)
    t = time.time()
    flt.emplace_path(base, paths)
    out["emplace_path_s"].append(round(time.time() - t, 5))
    t = time.time()
    _, lost, _ = flt.probe_path(more, paths)
    out["probe_path_s"].append(round(time.time() - t, 5))
    quotas = [np.full(split, int(a) // split, np.uint64) for a in lost[:, 0]]
    for q, a in zip(quotas, lost[:, 0]):
        q[:int(a) % split] += np.uint64(1)
    t = time.time()
    flt.extend_path(more, paths, quotas)
    out["extend_path_s"].append(round(time.time() - t, 5))
    out["absent"] = int(lost[:, 0].sum())
    found, lost, _ = flt.probe_path(more, paths)
    assert np.array_equal(found, [len(s) for s in more]) and not lost.any(), "every hash is found along its path after the extension"
    flt.free()
print(json.dumps(out))
