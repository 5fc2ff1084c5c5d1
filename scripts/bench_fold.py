"""What `ganon-build --hibf --update --fold` costs and what it buys.  Prints one JSON object.
  kernel   gn_filter_fold_ibf through the library alone, beside the plain move of the same bytes (gn_filter_copy_ibf): an IBF of about
           --gib GiB at a narrow stride (64 bins, one word a row) and at a wide one (1152 bins, a stride of 32 words), its bins folded in
           groups of 8 into the first bins of an IBF of the same rows.  One call each to warm up, then --runs (5) rounds that alternate the
           two; host-side times of the calls (launch, the upload of the table and the wait included): median, spread (max - min), and
           the bytes per second of what the call reads and writes at the median (the fold writes ceil(groups / 64) + 1 words a row at most)
  query    [--query] --targets (1024) FASTA files of log-normal length (median --len 20000 bases, sigma 1) built with `--hibf --tmax
           <targets>` into ONE wide root, the same index held to --fold bins (the least of --fold, 1.5 x, 2.25 x ... the rule reaches),
           and --reads (2000000) reads of 150 bases cut from the files classified against both by ganon-classify, alternating, one run each
           to warm up and --runs each: the classifier's own `backend` and `classify+print wall` seconds (GANON_HOST_TIMING) and the
           process's wall time, median and spread; the .all files are compared
usage: bench_fold.py [--gib 1] [--runs 5] [--query [--targets 1024] [--len 20000] [--reads 2000000] [--fold 64] [--dir /dev/shm]]"""
import json
import os
import re
import subprocess
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


def stats(v):
    med = sorted(v)[len(v) // 2]
    return {"s": [round(x, 6) for x in v], "median_s": round(med, 6), "spread_s": round(max(v) - min(v), 6)}


gib, runs = opt("--gib", 1.0), opt("--runs", 5)
out = {"gib": gib, "runs": runs, "kernel": []}
for bins in (64, 1152):
    W = (bins + 63) >> 6
    stride = int(H.load_library().gn_hibf_row_stride_words(W))
    rows = int(gib * (1 << 30)) // (8 * stride)
    groups = bins // 8
    members = [(8 * g, 8, g) for g in range(groups)]
    src, dst = one(bins, rows), one(bins, rows)
    src.fill_random(bins, 3)
    counts = src.bin_popcounts(bins)
    dst_words = (groups + 63) // 64
    case = {"bins": bins, "stride_words": stride, "rows": rows, "groups": groups, "bytes_plain": 2 * rows * stride * 8, "bytes_fold": rows * (stride + 2 * dst_words) * 8}
    calls = {"plain": lambda: dst.copy_ibf(0, src, 0), "fold": lambda: dst.fold_ibf(0, 0, groups, src, 0, members)}
    dst.copy_ibf_spans(0, src, 0, [])  # (cleared: the fold is an OR)
    dst.fold_ibf(0, 0, groups, src, 0, members)
    got = dst.bin_popcounts(bins)
    for g in range(groups):  # an OR of 8 columns: at least the fullest of them, at most their sum
        assert counts[8 * g:8 * g + 8].max() <= got[g] <= counts[8 * g:8 * g + 8].sum(), g
    assert not got[groups:].any()
    calls["plain"]()
    times = {k: [] for k in calls}
    for _ in range(runs):
        for k, call in calls.items():
            t = time.time()
            call()
            times[k].append(time.time() - t)
    for k, v in times.items():
        case[k] = stats(v)
        case[k]["GBps"] = round(case["bytes_" + k] / case[k]["median_s"] / 1e9, 1)
    out["kernel"].append(case)
    src.free()
    dst.free()

if "--query" in sys.argv:
    n_targets, median, n_reads, bound = opt("--targets", 1024), opt("--len", 20000), opt("--reads", 2000000), opt("--fold", 64)
    d = os.path.join(opt("--dir", "/dev/shm"), "ganon_fold_bench")
    os.makedirs(d, exist_ok=True)
    rng = np.random.default_rng(7)
    lengths = np.clip(median * np.exp(rng.standard_normal(n_targets)), 2000, 20 * median).astype(np.int64)
    genome = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=int(lengths.sum()), dtype=np.uint8)]
    starts = np.concatenate([[0], np.cumsum(lengths)])
    with open(os.path.join(d, "in.tsv"), "w") as tsv:
        for t in range(n_targets):
            path = os.path.join(d, f"t{t}.fasta")
            with open(path, "wb") as o:
                o.write(b">t%d\n" % t + genome[starts[t]:starts[t + 1]].tobytes() + b"\n")
            tsv.write(f"{path}\tt{t}\n")
    # reads: 150 bases from inside one file each
    which = rng.integers(0, n_targets, size=n_reads)
    at = starts[which] + (rng.random(n_reads) * (lengths[which] - 150)).astype(np.int64)
    fq = os.path.join(d, "reads.fq")
    with open(fq, "wb") as o:  # records of one width, assembled as a byte matrix, 100 000 at a time
        for lo in range(0, n_reads, 100000):
            n = min(100000, n_reads - lo)
            rec = np.empty((n, 1 + 9 + 1 + 150 + 3 + 150 + 1), dtype=np.uint8)
            rec[:, 0] = ord("@")
            rec[:, 1:10] = np.frombuffer(b"".join(b"%09d" % i for i in range(lo, lo + n)), dtype=np.uint8).reshape(n, 9)
            rec[:, 10] = rec[:, 161] = rec[:, 163] = rec[:, -1] = ord("\n")
            rec[:, 11:161] = genome[at[lo:lo + n, None] + np.arange(150)]
            rec[:, 162] = ord("+")
            rec[:, 164:314] = ord("I")
            o.write(rec.tobytes())
    build = os.path.join(ROOT, "ganon_amd", "host", "ganon-build")
    wide, held = os.path.join(d, "wide.hibf"), os.path.join(d, "held.hibf")
    p = subprocess.run([build, "-i", os.path.join(d, "in.tsv"), "-o", wide, "--hibf", "--tmax", str(n_targets), "-p", "0.05", "-s", "4", "-t", "16", "--quiet"], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-500:]
    q = {"targets": n_targets, "bases": int(lengths.sum()), "reads": n_reads}
    while True:
        p = subprocess.run([build, "--hibf", "--update", wide, "--fold", str(bound), "-o", held, "-t", "16", "--verbose"], capture_output=True, text=True)
        if p.returncode == 0:
            break
        assert "rebuild or give a larger --fold" in p.stderr and bound < n_targets, p.stderr[-500:]
        bound = bound * 3 // 2
    q["fold"], q["index_line"], q["result_line"] = bound, p.stdout.split("\n", 1)[0], p.stdout.strip().rsplit("\n", 1)[-1]
    m = re.search(r" copy ([0-9.eE+-]+) fold ([0-9.eE+-]+) ", p.stderr)
    q["copy_s"], q["fold_s"] = (float(x) for x in m.groups()) if m else (None, None)
    q["bytes"] = {"wide": os.path.getsize(wide), "held": os.path.getsize(held)}
    classify = os.path.join(ROOT, "ganon_amd", "host", "ganon-classify")
    laps = {"wide": {"backend_s": [], "classify_wall_s": [], "process_s": []}, "held": {"backend_s": [], "classify_wall_s": [], "process_s": []}}
    for r in range(runs + 1):
        for name, index in (("wide", wide), ("held", held)):
            t = time.time()
            p = subprocess.run([classify, "--ibf", index, "--hibf", "--single-reads", fq, "-o", os.path.join(d, name), "--output-all", "--quiet"], capture_output=True, text=True,
                               env=dict(os.environ, GANON_HOST_TIMING="1"))
            wall = time.time() - t
            assert p.returncode == 0, p.stderr[-500:]
            m = re.search(r"\[host timing\] backend .*?\) ([0-9.eE+-]+) s,.* classify\+print wall ([0-9.eE+-]+) s", p.stderr)
            if r and m:
                laps[name]["backend_s"].append(float(m.group(1))), laps[name]["classify_wall_s"].append(float(m.group(2))), laps[name]["process_s"].append(wall)
    q["classify"] = {name: {k: stats(v) for k, v in lap.items() if v} for name, lap in laps.items()}
    a, b = (set(open(os.path.join(d, name + ".all")).read().splitlines()) for name in ("wide", "held"))
    q["all_lines"] = {"wide": len(a), "held": len(b), "held_not_in_wide": len(b - a), "wide_not_in_held": len(a - b)}
    out["query"] = q
print(json.dumps(out))
