"""The count step's launches over a matrix of filters, cutoffs and switches: a differential record of gn_count_plan.h.

Run under `rocprofv3 --kernel-trace` (nothing else traced, this program after `--`), the trace lists every count kernel of every cell in
order with its grid, workgroup and LDS size; two commits that launch alike give the same list (profiles/README.md:
count_launch_matrix_*).  On its own it prints one JSON line per cell -- matches, the bytes skipped, whether the launches took the
stream kernels, the units the screen-only kernel left to its list -- which must not differ between such commits either.

Filters (Bernoulli(0.5) rows): the three shapes of tests/test_gpu_row_policy.py, each with the stream threshold at its default and
at 0; one filter of three hash functions; one split-bin filter (two bins a target).  A batch of 64 reads of 150 bases, one stream a
filter (so from the second cell on the grids of the deferred lists follow the last batch's lists), cutoffs 0.2 and 0.75, nothing
switched and each of row_screen, lean_screen, stream_rows, early_exit and on_demand alone.  A few seconds.

`--trace-summary IN.csv OUT.csv` (no GPU) reduces a kernel trace to the count kernels' dispatches in order and what identifies a
launch -- kernel, LDS, workgroup, grid; no ids, no time stamps -- so that the summaries of two runs compare with `cmp`."""
import csv
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np

import ganon_amd as hip
import ganon_fixtures as gf
import gpu_util as gu

K, W = 19, 31
SHAPES = [(4096, 5003), (4160, 3001), (32768, 1201)]
SWITCHES = ("row_screen", "lean_screen", "stream_rows", "early_exit", "on_demand")


def filters():
    for bins, rows in SHAPES:
        ibf = gf.random_ibf(bins, rows, 4, 0.5, seed=bins)
        for threshold in (None, 0):
            flt = hip.HipFilter.ibf(ibf.data, bins, rows, 4)
            if threshold is not None:
                flt.set_stream_rows_min_bytes(threshold)
            yield f"h4 {bins}x{rows} threshold {'default' if threshold is None else threshold}", flt
    ibf = gf.random_ibf(4096, 1009, 3, 0.5, seed=3)
    yield "h3 4096x1009", hip.HipFilter.ibf(ibf.data, 4096, 1009, 3)
    ibf = gf.random_ibf(4096, 3001, 4, 0.5, seed=5)
    flt = hip.HipFilter.ibf(ibf.data, 4096, 3001, 4, (np.arange(4096) // 2).astype(np.uint32), 2048)
    flt.set_stream_rows_min_bytes(0)
    yield "split 4096x3001, two bins a target", flt


def main():
    hip.load_library()
    assert hip.device_count() >= 1, "no HIP device"
    rng = np.random.default_rng(64)
    bases, off1, off2 = gu.pack_reads([gu.random_seq(rng, 150) for _ in range(64)], None)
    for name, flt in filters():
        st = hip.HipStream(flt, 64, bases.size)
        for cutoff in (0.2, 0.75):
            for sw in ((),) + tuple((s,) for s in SWITCHES):
                hip.set_ablation(list(sw))
                try:
                    st.submit(bases, off1, off2, K, W, cutoff)
                    nh, status, mo, m = st.fetch()
                    tm = st.timings()
                    print(json.dumps(dict(filter=name, cutoff=cutoff, switches=sw, matches=int(len(m)), minimisers=int(nh.sum()),
                                          skipped_bytes=int(tm["algo_bytes"]) - int(tm["fetched_bytes"]), streamed=bool(st.rows_streamed()),
                                          screen_deferred=int(st.screen_deferred()))), flush=True)
                finally:
                    hip.set_ablation([])
        st.destroy()
        flt.free()


KEEP = ("Kernel_Name", "LDS_Block_Size", "Workgroup_Size_X", "Grid_Size_X")


def trace_summary(src, dst):
    with open(src, newline="") as f:
        rows = sorted((r for r in csv.DictReader(f) if "gn_ibf_count" in r["Kernel_Name"]), key=lambda r: int(r["Dispatch_Id"]))
    with open(dst, "w", newline="") as f:
        out = csv.writer(f, lineterminator="\n")
        out.writerow(KEEP)
        out.writerows([r[k].replace("void ", "").replace("(GnCountParams)", "") if k == "Kernel_Name" else r[k] for k in KEEP] for r in rows)
    print(f"{len(rows)} dispatches -> {dst}")


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--trace-summary":
        trace_summary(sys.argv[2], sys.argv[3])
    else:
        main()
