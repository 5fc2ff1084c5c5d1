"""The two probe kernels of `ganon-build --hibf --verify-index` beside the insert they read back, through the library calls alone, for
a run under `rocprofv3 --kernel-trace --stats -- python scripts/bench_probe_path.py`: a two-level tree -- a root of 64 merged bins,
N / 64 user bins of one bin each below every one of them, sized for --max-fp 0.05 at h = 4 -- takes N sets of H random hashes along
their paths (gn_filter_emplace_path), then gn_filter_probe_path looks the same sets up along the same paths and
gn_filter_probe_paths_shared asks 65 536 probes of every path, --runs times each.  Prints one JSON object with the host-side times of
the calls (staging upload included); the kernels' own times are in the trace.   usage: bench_probe_path.py [N=512] [H=100000] [--runs 3]"""
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
h, max_fp, per = 4, 0.05, n // 64


def rows_for(count):  # the textbook size of one bin
    return int(math.ceil(-h * count / math.log(1.0 - math.exp(math.log(max_fp) / h))))


rng = np.random.default_rng(1)
sets = [np.unique(rng.integers(0, 1 << 62, size=hashes, dtype=np.uint64)) for _ in range(n)]
shapes = [(None, 64, rows_for(per * hashes), h)] + [(None, per, rows_for(hashes), h)] * 64
nx = [np.arange(1, 65, dtype=np.int64)] + [np.full(per, i, np.int64) for i in range(1, 65)]
bu = [np.full(64, -1, np.int64)] + [np.arange((i - 1) * per, i * per, dtype=np.int64) for i in range(1, 65)]
flt = H.HipFilter.hibf(shapes, nx, bu, n)
paths = np.zeros((n, 2), dtype=H.PATH_DTYPE)
for u in range(n):
    paths[u, 0] = (1 + u // per, u % per, 1, 0, 1)
    paths[u, 1] = (0, u // per, 1, 0, 1)
z = np.arange(1, 65537, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)
z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
probes = (z ^ (z >> np.uint64(31))) | np.uint64(1 << 63)
out = {"user_bins": n, "hashes_per_set": hashes, "hashes": int(sum(len(s) for s in sets)), "probes": len(probes), "emplace_path_s": [], "probe_path_s": [],
       "probe_paths_shared_s": []}
for _ in range(runs):
    t = time.time()
    flt.emplace_path(sets, paths)
    out["emplace_path_s"].append(round(time.time() - t, 5))
    t = time.time()
    found, lost, first = flt.probe_path(sets, paths)
    out["probe_path_s"].append(round(time.time() - t, 5))
    t = time.time()
    hits = flt.probe_paths_shared(probes, paths)
    out["probe_paths_shared_s"].append(round(time.time() - t, 5))
assert np.array_equal(found, [len(s) for s in sets]) and not lost.any(), "every hash is found along the path it was inserted along"
out["max_observed_fp"], out["mean_observed_fp"] = round(int(hits.max()) / len(probes), 6), round(float(hits.mean()) / len(probes), 6)
flt.free()
print(json.dumps(out))
