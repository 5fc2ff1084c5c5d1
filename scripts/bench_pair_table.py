"""The two table kernels of `ganon-build --hibf --layout sketch | similarity` through the library calls alone, for a run under
`rocprofv3 --kernel-trace --stats -- python scripts/bench_pair_table.py`: N sets of H random hashes are sketched once, then
gn_sketches_pair_table over all N (N * N entries) and gn_sketches_union_table over the same N at width N (N * N entries, the rows
past the last sketch zero) run --runs times each.  Prints one JSON object with the host-side times of the calls (kernel, the copy of
the table back and its allocation); the kernels' own times are in the trace.   usage: bench_pair_table.py [N=4096] [H=2000] [--runs 3]"""
import json
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
n = int(args[0]) if len(args) > 0 else 4096
hashes = int(args[1]) if len(args) > 1 else 2000
rng = np.random.default_rng(1)
sk = H.HipSketches([rng.integers(0, 1 << 63, size=hashes, dtype=np.uint64) for _ in range(n)])
idx = rng.permutation(n).astype(np.uint32)
out = {"sketches": n, "hashes_per_set": hashes, "entries": n * n, "pair_table_s": [], "union_table_s": []}
for _ in range(runs):
    t = time.time()
    pairs = sk.pair_table(idx)
    out["pair_table_s"].append(round(time.time() - t, 5))
    t = time.time()
    unions = sk.union_table(idx, n)
    out["union_table_s"].append(round(time.time() - t, 5))
assert np.array_equal(pairs, pairs.T) and np.array_equal(pairs.diagonal(), unions[:, 0]), "E of one sketch, both ways"
assert np.array_equal(np.maximum(pairs[np.arange(n - 1), np.arange(1, n)], unions[:-1, 0]), unions[:-1, 1]), "the union table's second column"
sk.free()
print(json.dumps(out))
