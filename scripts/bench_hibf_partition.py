#!/usr/bin/env python3
"""What spreading an HIBF over several devices by subtree costs, measured with all parts on ONE GPU (the overhead of the split, not the
gain of more HBM): the skewed 65 536-user-bin tree of `bench.py --full` (workload hibf64k_skew, bench_workload.py), whole against 2, 4
and 8 subtree parts, alternating, one warm-up and `--runs` runs each.

  host clock around submit ... gather-fetch (the whole: submit ... fetch), the level kernels' own time per part (gn_stream_hibf_levels),
  and the merging gather against the concatenating gather on the same device buffers.

The plan is the test suite's Python restatement of host/hibf_partition.hpp (tests/hibf_partition_checks.py); the parts' rows are copied
out of the whole filter, the root's with word_lo.  The tree's parameters are read from bench.py's WORKLOADS["hibf64k_skew"].  Prints one
JSON line per configuration."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


class Tree:
    """what tests/hibf_partition_checks.py reads of an oracle.Hibf: shapes and tables"""

    class Shape:
        def __init__(self, bins, rows, h):
            self.bins, self.bin_size, self.hash_funs = bins, rows, h

    def __init__(self, wl):
        self.ibfs = [Tree.Shape(b, r, h) for _, b, r, h in wl.ibfs]
        self.next_ibf_id, self.bin_to_user, self.n_user_bins = wl.next_ibf_id, wl.bin_to_user, wl.n_user_bins


def med_spread(x):
    return float(np.median(x)), float(np.max(x) - np.min(x))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--user-bins", type=int, default=0, help="default: the workload's 65 536")
    ap.add_argument("--reads", type=int, default=2_000_000)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--rows-scale", type=float, default=1.0)
    ap.add_argument("--parts", default="2,4,8")
    args = ap.parse_args()
    import bench_workload as bw
    import ganon_amd as hip
    import hibf_partition_checks as hp
    L = hip.load_library()
    import bench
    spec = bench.WORKLOADS["hibf64k_skew"]
    wl, whole = bw.make_hibf_skew_device_workload(hip, "hibf64k_skew", args.user_bins or spec["user_bins"], spec["h"], args.reads, rows_scale=args.rows_scale)
    tree = Tree(wl)
    units = hp.units_of(tree)
    C = hp.cost_matrix(tree, units)
    print(json.dumps(dict(tree=wl.layout, units=len(units), whole_device_mib=round(int(C[0, len(units)]) / 2**20, 1))), flush=True)

    configs = {1: None}
    for k in [int(x) for x in args.parts.split(",")]:
        cuts = hp.even_cuts(C, k)
        cuts = [x for i, x in enumerate(cuts) if i == 0 or x != cuts[i - 1]]
        parts = []
        for a, b in zip(cuts, cuts[1:]):
            p = hp.build_part(tree, units, a, b)
            f = hip.HipFilter.hibf([(None, bins, rows, hf) for bins, rows, hf in p["shapes"]], p["next_ibf_id"], p["bin_to_user"], max(len(p["user_global"]), 1))
            for local, g in enumerate(p["ibf_global"]):
                bins, rows = tree.ibfs[g].bins, tree.ibfs[g].bin_size
                W, step = (bins + 63) >> 6, max(1, (256 << 20) // (((bins + 63) >> 6) * 8))
                for r0 in range(0, rows, step):
                    n = min(step, rows - r0)
                    f.write_rows(r0, whole.download_rows(r0, n, W, ibf_idx=g), p["word_lo"] if g == 0 else 0, ibf_idx=local)
            f.finalize()
            p["mib"] = round(int(C[a, b]) / 2**20, 1)
            parts.append((f, p))
        configs[k] = parts
        print(json.dumps(dict(parts=k, placed=len(parts), mib=[p["mib"] for _, p in parts], root_bins=[[p["bin_lo"], p["bin_hi"]] for _, p in parts])), flush=True)

    n, nb = wl.n_reads, wl.bases.size
    st_whole = hip.HipStream(whole, n, nb)
    streams = {k: [hip.HipStream(f, n, nb) for f, _ in parts] for k, parts in configs.items() if parts}
    gm = {k: hip.HipGather(0, [np.array(p["user_global"], dtype=np.uint32) for _, p in parts], merged=True) for k, parts in configs.items() if parts}
    gc = {k: hip.HipGather(0, [np.array(p["user_global"], dtype=np.uint32) for _, p in parts]) for k, parts in configs.items() if parts}
    res = {k: dict(wall=[], levels=[], merge=[]) for k in configs}
    ref = None
    for run in range(args.runs + 1):  # the first one warms up
        for k in configs:
            t0 = time.perf_counter()
            if k == 1:
                st_whole.submit(wl.bases, wl.off, None, wl.k, wl.w, wl.rel_cutoff)
                _, _, mo, m = st_whole.fetch()
                wall = time.perf_counter() - t0
                lv = sum(x["ms"] for x in st_whole.hibf_levels())
                if ref is None:
                    ref = (mo.copy(), m.copy())
                tm = 0.0
            else:
                sts = streams[k]
                sts[0].submit(wl.bases, wl.off, None, wl.k, wl.w, wl.rel_cutoff)
                for s in sts[1:]:
                    s.classify_shared(sts[0], wl.rel_cutoff)
                gm[k].run(sts)
                mo, m = gm[k].fetch()
                wall = time.perf_counter() - t0
                lv = sum(x["ms"] for s in sts for x in s.hibf_levels())
                if run == 0:
                    assert np.array_equal(mo, ref[0]) and np.array_equal(m, ref[1]), f"{k} parts: not the whole filter's result"
                # the gathers alone, on the buffers the streams hold (run + device sync, no fetch)
                t1 = time.perf_counter()
                gm[k].run(sts)
                gm[k].peer_bytes()
                tm = time.perf_counter() - t1
            if run:
                r = res[k]
                r["wall"].append(wall * 1e3)
                r["levels"].append(lv)
                r["merge"].append(tm * 1e3)
    # the concatenating gather refuses streams on an HIBF: it is timed over the same records as raw device buffers, and the merging one too
    gb = {}
    for k, sts in streams.items():
        a, b, cnt = [], [], []
        for s in sts:  # the device views of the streams' results (gn_stream_device_offsets / gn_stream_device_matches)
            po, pm, nm = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_uint64(0)
            assert L.gn_stream_device_offsets(s._h, ctypes.byref(po)) == 0 and L.gn_stream_device_matches(s._h, ctypes.byref(pm), ctypes.byref(nm)) == 0
            a.append(po.value)
            b.append(pm.value if nm.value else 0)
            cnt.append(nm.value)
        tms = {"merge_buffers": [], "concat_buffers": []}
        for run in range(args.runs + 1):
            for name, g in (("merge_buffers", gm[k]), ("concat_buffers", gc[k])):
                t1 = time.perf_counter()
                g.run_buffers(a, b, cnt, n)
                g.peer_bytes()  # (waits for the gather's stream)
                if run:
                    tms[name].append((time.perf_counter() - t1) * 1e3)
        gb[k] = tms
    whole_wall, whole_spread = med_spread(res[1]["wall"])
    for k in configs:
        r = res[k]
        out = dict(parts=k, reads=n, matches=int(len(ref[1])), wall_ms=med_spread(r["wall"]), level_kernels_ms=med_spread(r["levels"]))
        if k > 1:
            out.update(merge_on_streams_ms=med_spread(r["merge"]), merge_buffers_ms=med_spread(gb[k]["merge_buffers"]),
                       concat_buffers_ms=med_spread(gb[k]["concat_buffers"]),
                       cost_over_whole_ms=round(out["wall_ms"][0] - whole_wall, 3), whole_spread_ms=round(whole_spread, 3),
                       per_part_fixed_ms=round((out["wall_ms"][0] - whole_wall) / (k - 1), 3))
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
