"""Throughput of the product's ganon-build on synthetic genomes: N FASTA files of L random bases each (70-column lines) are
written to a tmpfs, then `ganon-build` runs start to finish (parse -> device minimisers + sort/unique -> sizing -> device
insert -> .ibf written).  Prints one JSON object.   usage: bench_build.py [n_files=512] [len=4000000] [threads=16] [dir=/dev/shm]
  --hibf          the same FASTA built flat AND as HIBF (`ganon-build --hibf`), alternating, one run each to warm up and then the median
                  of --runs (5) each, both at --max-fp (0.05) and --hash-functions (4); the HIBF time split into hash / union / emplace /
                  write; --tmax N is passed on.  Prints one JSON object with "flat" and "hibf".
  --layout NAME   [--hibf] passed on as `--layout NAME` (rule | sketch | similarity).  A comma list (rule,sketch,similarity) builds
                  every layout in turn in each round, alternating, and prints "hibf" as one object per layout; a sketch or
                  similarity build also reports layout_s, the part of union_s that went into sketches, union tables and search,
                  a similarity build its split (layout_sketches_s, layout_tables_s, layout_pairs_s, layout_host_s) and the
                  tree it kept.
  --verify        [--hibf] after each --hibf build of a run the file is checked (`ganon-build --hibf --verify-index`): verify_hash_s,
                  verify_load_s, verify_membership_s (beside emplace_s of the same build: the same hashes along the same paths) and
                  verify_fp_s, max_observed_fp / mean_observed_fp against --max-fp, the number of WARN and of FAIL lines
  --update M      [--hibf] per layout: an index built from all but the last M files, `ganon-build --hibf --update` with those M (laps: hash,
                  load, count, plan, copy, emplace, write), the updated file checked over ALL files (--verify-index), beside one full
                  rebuild of all N checked the same way: seconds, bytes and max_observed_fp of both.  Prints "update" per layout;
                  the flat / hibf medians are not run
  --extend        [--update M] the last M files do not bring new targets: file N - M + j becomes one more file of the target of file j
                  (with --families F:D, M <= F and N - M a multiple of F, a member of the same family), and the update runs with `--extend`.  One run to warm
                  up and --runs (5) runs of the update, and as many rebuilds from all N files under the same target names: emplace_s
                  and total_s of both as min / median / max.  The files of the extended targets, old and new, are 30 % shorter than the
                  others, so that their bins have room (an index gives a bin that sets its IBF's rows none: the plan refuses,
                  which is reported as such)
  --remove N      [--update M] the update also takes the first N targets of the index out (`--remove`): its laps beside copy_s of the
                  same update without --remove (the plain move against the compacting one), the file checked over the files that are
                  left, beside a rebuild from those.  Not with --extend
  --fold N        [--update M] the update also holds every IBF to N bins (`--fold N`): its `fold` lap beside its `copy` lap, the `folded`
                  lines, the IBFs before and after, the file checked like any updated one
  --families F:D  F families in place of independent genomes: one random ancestor of `len` bases per family; file i is member
                  i // F of family i % F, the ancestor with every base substituted with probability D and a random 0 .. 10 % cut
                  from its end, so that the lengths of the families interleave
  --lognormal S   file i has len * exp(S * z_i) bases, z_i standard normal (seeded): `len` is the median, not every file's length
  --device LIST   passed on as `--device LIST` to every build; a list a,b,... only to the flat build (the hierarchical modes take one)
  --device-memory BYTES  passed on to the flat build: the filter is filled in row slabs when it is larger; the run reports "slabs",
                  "passes", "hash_bytes_uploaded" and per slab its fill and write seconds
  --hash-sets MODE  passed on to the flat build (raw | packed | spilled): the run reports "hash_sets", "hashes", "hash_set_bytes" (what the
                  sets hold, beside 8 x hashes) and "rss_anon_kb", the process's anonymous memory when hashing ends
  --hibf-memory BYTES / --hibf-devices LIST  [--hibf] passed on to the hierarchical build: the tree is filled in parts when it is larger
                  than BYTES of device rows, the parts dealt to the entries of LIST; the run reports "parts", "hash_bytes_uploaded"
                  beside "one_pass_hash_bytes", and per part its device bytes, the sets it took and its fill and write seconds
  --hibf-hash-sets MODE  [--hibf] passed on to the hierarchical build (raw | packed | spilled): the run reports "hash_sets", "hashes",
                  "hash_set_bytes" and "united" (the `hibf hash sets:` line); every hierarchical build reports "peak_rss_kb", the
                  process's largest resident set, and the median run "laps_s", the four laps of every run
  --parse MODE    passed on as `--parse MODE` to every build and check (host | device).  A comma list (host,device) builds with every
                  mode in turn in each round, alternating, one run each to warm up and then --runs (5) each, and prints "parse": per
                  mode the flat build of the median total (with --hibf the hierarchical build beside it) and "hash_lap_s" / "total_runs_s",
                  the hash lap and the total of every run as min / median / max; the device builds also report "parse_device", the
                  files tokenised on the device, those that fell back, those not eligible and the text bytes uploaded
  --gz            the synthetic genomes are written through Python's gzip (g<i>.fna.gz, level 1: the input side is measured, not
                  the compressor)"""
import gzip
import json
import math
import os
import re
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
opts = {"--runs": "5", "--max-fp": "0.05", "--hash-functions": "4", "--tmax": "", "--layout": "", "--lognormal": "", "--families": "", "--update": "", "--remove": "", "--fold": "", "--device": "", "--device-memory": "", "--hash-sets": "", "--hibf-memory": "", "--hibf-devices": "", "--hibf-hash-sets": "", "--parse": ""}
pos, hibf, check, extend, gz, argv = [], False, False, False, False, sys.argv[1:]
while argv:
    a = argv.pop(0)
    if a == "--hibf":
        hibf = True
    elif a == "--extend":
        extend = True
    elif a == "--verify":
        check = True
    elif a == "--gz":
        gz = True
    elif a in opts:
        opts[a] = argv.pop(0)
    else:
        pos.append(a)
n_files = int(pos[0]) if len(pos) > 0 else 512
L = int(pos[1]) if len(pos) > 1 else 4_000_000
threads = int(pos[2]) if len(pos) > 2 else 16
d = os.path.join(pos[3] if len(pos) > 3 else "/dev/shm", "ganon_build_bench")
os.makedirs(d, exist_ok=True)
rng = np.random.default_rng(1)
lut = np.frombuffer(b"ACGT", dtype=np.uint8)
cols = 70
lengths = [L] * n_files
if opts["--lognormal"]:
    lengths = [max(1000, int(L * math.exp(float(opts["--lognormal"]) * z))) for z in np.random.default_rng(2).standard_normal(n_files)]
if extend and opts["--update"]:  # the files of the extended targets are 30 % shorter than the others: their bins have room
    for j in range(int(opts["--update"])):
        lengths[j], lengths[n_files - int(opts["--update"]) + j] = int(0.7 * lengths[j]), int(0.7 * lengths[n_files - int(opts["--update"]) + j])
n_families, divergence, ancestors = 0, 0.0, []
if opts["--families"]:
    n_families, divergence = int(opts["--families"].split(":")[0]), float(opts["--families"].split(":")[1])
    cut = np.random.default_rng(3)
    lengths = [n - int(cut.random() * 0.1 * n) for n in lengths]
    ancestors = [rng.integers(0, 4, size=max(lengths[f::n_families]), dtype=np.uint8) for f in range(n_families)]
total_bases = sum(lengths)
with open(os.path.join(d, "in.tsv"), "w") as tsv:
    for i in range(n_files):
        L = lengths[i]
        rows = (L + cols - 1) // cols
        body = np.full((rows, cols + 1), ord("\n"), dtype=np.uint8)
        if n_families:
            ranks = ancestors[i % n_families][:L].copy()
            hit = np.nonzero(rng.random(L) < divergence)[0]
            ranks[hit] = (ranks[hit] + rng.integers(1, 4, size=len(hit), dtype=np.uint8)) & 3  # another base
            body.reshape(-1)[np.arange(L) + np.arange(L) // cols] = lut[ranks]
        else:
            body[:, :cols] = lut[rng.integers(0, 4, size=(rows, cols), dtype=np.uint8)]
        f = os.path.join(d, f"g{i}.fna" + (".gz" if gz else ""))
        with (gzip.open(f, "wb", compresslevel=1) if gz else open(f, "wb")) as o:
            o.write(f">genome{i} synthetic\n".encode())
            o.write(body.tobytes()[: L + L // cols + 1])
        tsv.write(f"{f}\tT{i}\n")
L = int(pos[1]) if len(pos) > 1 else 4_000_000
out = {"files": n_files, "bases_per_file": L, "total_gbp": round(total_bases / 1e9, 3), "threads": threads}
if n_families:
    out["families"], out["divergence"] = n_families, divergence
if opts["--lognormal"]:
    out["lognormal_sigma"], out["largest_file"], out["smallest_file"] = float(opts["--lognormal"]), max(lengths), min(lengths)
exe = os.path.join(ROOT, "ganon_amd", "host", "ganon-build")
device_flat = (["--device", opts["--device"]] if opts["--device"] else []) + (["--device-memory", opts["--device-memory"]] if opts["--device-memory"] else []) + \
              (["--hash-sets", opts["--hash-sets"]] if opts["--hash-sets"] else [])
device_hibf = ["--device", opts["--device"]] if opts["--device"] else []
parts_hibf = (["--hibf-memory", opts["--hibf-memory"]] if opts["--hibf-memory"] else []) + (["--hibf-devices", opts["--hibf-devices"]] if opts["--hibf-devices"] else [])
sets_hibf = ["--hibf-hash-sets", opts["--hibf-hash-sets"]] if opts["--hibf-hash-sets"] else []
parse_modes = [m for m in opts["--parse"].split(",") if m]
parse_mode = parse_modes[0] if len(parse_modes) == 1 else ""  # (a list: set in turn by the rounds at the end)
if gz:
    out["gz"] = True


def parse_extra():
    return ["--parse", parse_mode] if parse_mode else []


def parse_counters(stderr, res):
    m = re.search(r"^parse device: (\d+) files tokenised on the device, (\d+) fell back to the host reader, (\d+) not eligible, (\d+) text bytes uploaded", stderr, re.M)
    if m:
        res["parse_device"] = dict(zip(("device", "fell_back", "not_eligible", "text_bytes"), (int(x) for x in m.groups())))


def flat_run(max_fp="0.05", extra=()):
    res = {}
    t0 = time.time()
    p = subprocess.run([exe, "-i", os.path.join(d, "in.tsv"), "-o", os.path.join(d, "db.ibf"), "-t", str(threads), "--verbose", "-p", max_fp] + list(extra) + device_flat + parse_extra(),
                       capture_output=True, text=True)
    res["rc"], res["wall_s"] = p.returncode, round(time.time() - t0, 2)
    parse_counters(p.stderr, res)
    m = re.search(r"filled in (\d+) pass(?:es)? over the hash sets, (\d+) hash bytes uploaded", p.stderr)
    if m:
        res["passes"], res["hash_bytes_uploaded"] = int(m.group(1)), int(m.group(2))
        res["slabs"] = [ln for ln in p.stderr.splitlines() if re.match(r"slab \d+: rows ", ln)][:64]
        res["slab_fill_write_s"] = [(float(a), float(b)) for a, b in re.findall(r"^slab \d+: filled in ([0-9.eE+-]+) s, written in ([0-9.eE+-]+) s$", p.stderr, re.M)][:64]
    m = re.search(r"^hash sets: (\d+) hashes held (\w+) in (\d+) bytes", p.stderr, re.M)
    if m:
        res["hashes"], res["hash_sets"], res["hash_set_bytes"] = int(m.group(1)), m.group(2), int(m.group(3))
    m = re.search(r"^RssAnon after hashing: (\d+) kB", p.stderr, re.M)
    if m:
        res["rss_anon_kb"] = int(m.group(1))
    for key, pat in (("count_hashes_s", r"Count/save hashes start:.*\n.*\n\s*elapsed \(s\): ([0-9.eE+-]+)"),
                     ("sizing_s", r"Estimate params   start:.*\n.*\n\s*elapsed \(s\): ([0-9.eE+-]+)"),
                     ("fill_s", r"Building filter   start:.*\n.*\n\s*elapsed \(s\): ([0-9.eE+-]+)"),
                     ("write_s", r"Saving filer      start:.*\n.*\n\s*elapsed \(s\): ([0-9.eE+-]+)"),
                     ("total_s", r"ganon-build       start:.*\n.*\n\s*elapsed \(s\): ([0-9.eE+-]+)")):
        m = re.search(pat, p.stderr)
        if m:
            res[key] = float(m.group(1))
    m = re.search(r"ganon-build processed .*", p.stderr)
    res["summary"] = m.group(0) if m else p.stderr[-300:]
    for key in ("n_bins", "max_hashes_bin", "bin_size_bits", "hash_functions"):
        m = re.search(key + r"\s+(\d+)", p.stderr)
        if m:
            res[key] = int(m.group(1))
    if p.returncode == 0:
        res["ibf_bytes"] = os.path.getsize(os.path.join(d, "db.ibf"))
        res["ibf_gib"] = round(res["ibf_bytes"] / 2**30, 3)
        res["mbp_per_s"] = round(total_bases / 1e6 / res.get("total_s", res["wall_s"]), 1)
    return res


def run_with_rusage(cmd, res):
    """subprocess.run(cmd, capture_output=True, text=True) that also notes the child's largest resident set in res["peak_rss_kb"]: the
    output goes through files, so that the child can be waited for with wait4"""
    with open(os.path.join(d, "stdout.txt"), "w+") as so, open(os.path.join(d, "stderr.txt"), "w+") as se:
        child = subprocess.Popen(cmd, stdout=so, stderr=se)
        _, status, usage = os.wait4(child.pid, 0)
        child.returncode = os.waitstatus_to_exitcode(status)
        so.seek(0), se.seek(0)
        res["peak_rss_kb"] = usage.ru_maxrss
        return subprocess.CompletedProcess(cmd, child.returncode, so.read(), se.read())


def hibf_run(layout="", tsv="in.tsv", db="db.hibf"):
    res = {}
    t0 = time.time()
    cmd = [exe, "-i", os.path.join(d, tsv), "-o", os.path.join(d, db), "-t", str(threads), "--verbose", "-p", opts["--max-fp"],
           "-s", opts["--hash-functions"], "--hibf"] + (["--tmax", opts["--tmax"]] if opts["--tmax"] else []) + (["--layout", layout] if layout else []) + device_hibf + (parts_hibf if db == "db.hibf" else []) + sets_hibf + parse_extra()
    p = run_with_rusage(cmd, res)
    res["rc"], res["wall_s"] = p.returncode, round(time.time() - t0, 2)
    parse_counters(p.stderr, res)
    m = re.search(r"^hibf hash sets: (\d+) hashes held (\w+) in (\d+) bytes, (\d+) targets united$", p.stderr, re.M)
    if m:
        res["hashes"], res["hash_sets"], res["hash_set_bytes"], res["united"] = int(m.group(1)), m.group(2), int(m.group(3)), int(m.group(4))
    m = re.search(r"filled in (\d+) parts?, (\d+) hash bytes uploaded(?: \(one pass: (\d+)\))?", p.stderr)
    if m:
        res["parts"], res["hash_bytes_uploaded"], res["one_pass_hash_bytes"] = int(m.group(1)), int(m.group(2)), int(m.group(3) or m.group(2))
        res["part_bytes_sets_fill_write"] = [(int(a), int(b), float(c), float(e)) for a, b, c, e in re.findall(
            r"^part \d+ entry \d+: (\d+) device bytes, (\d+) sets taken, filled in ([0-9.eE+-]+) s, written in ([0-9.eE+-]+) s$", p.stderr, re.M)][:64]
    m = re.search(r" - seconds: hash ([0-9.eE+-]+) union ([0-9.eE+-]+) emplace ([0-9.eE+-]+) write ([0-9.eE+-]+)", p.stderr)
    if m:
        res["hash_s"], res["union_s"], res["emplace_s"], res["write_s"] = (float(x) for x in m.groups())
    m = re.search(r" write [0-9.eE+-]+ layout ([0-9.eE+-]+)", p.stderr)
    if m:
        res["layout_s"] = float(m.group(1))
    m = re.search(r" - layout seconds: sketches ([0-9.eE+-]+) tables ([0-9.eE+-]+) pairs ([0-9.eE+-]+) host ([0-9.eE+-]+)", p.stderr)
    if m:
        res["layout_sketches_s"], res["layout_tables_s"], res["layout_pairs_s"], res["layout_host_s"] = (float(x) for x in m.groups())
    m = re.search(r"layout similarity: (\d+) intervals, (\d+) of \d+ user bins moved, kept (\w+)", p.stderr)
    if m:
        res["intervals"], res["moved"], res["kept"] = int(m.group(1)), int(m.group(2)), m.group(3)
    m = re.search(r"ganon-build       start:.*\n.*\n\s*elapsed \(s\): ([0-9.eE+-]+)", p.stderr)
    if m:
        res["total_s"] = float(m.group(1))
    m = re.search(r" - hibf: .*", p.stderr)
    res["summary"] = m.group(0).strip() if m else p.stderr[-300:]
    if p.returncode == 0:
        res["hibf_bytes"] = os.path.getsize(os.path.join(d, db))
        res["mbp_per_s"] = round(total_bases / 1e6 / res.get("total_s", res["wall_s"]), 1)
        if check:
            res.update(verify_run(db))
    return res


def spread(values):
    v = sorted(values)
    return {"min": v[0], "median": v[len(v) // 2], "max": v[-1], "runs": len(v)} if v else {}


def update_run(layout, m):
    """build from all but the last m files, update with those, check the result over all; beside a rebuild of all"""
    lines = open(os.path.join(d, "in.tsv")).read().splitlines(True)
    if extend:  # the last m files under the names of the first m targets; the check and the rebuild read the same names
        assert m <= (n_families or n_files - m)
        lines = lines[:-m] + [ln.split("\t")[0] + "\t" + lines[j].split("\t")[1] for j, ln in enumerate(lines[-m:])]
        open(os.path.join(d, "in.tsv"), "w").writelines(lines)
    open(os.path.join(d, "old.tsv"), "w").writelines(lines[:-m])
    open(os.path.join(d, "new.tsv"), "w").writelines(lines[-m:])
    res = {"base": hibf_run(layout, "old.tsv", "old.hibf")}
    cmd = [exe, "-i", os.path.join(d, "new.tsv"), "--hibf", "--update", os.path.join(d, "old.hibf"), "-o", os.path.join(d, "upd.hibf"), "-t", str(threads),
           "--verbose"] + (["--extend"] if extend else []) + parse_extra()
    n_remove = int(opts["--remove"] or 0)
    lap = r" - seconds: hash ([0-9.eE+-]+) load ([0-9.eE+-]+) count ([0-9.eE+-]+) plan ([0-9.eE+-]+) copy ([0-9.eE+-]+) emplace ([0-9.eE+-]+) write ([0-9.eE+-]+)"
    lap_keys = ("hash_s", "load_s", "count_s", "plan_s", "copy_s", "emplace_s", "write_s")
    if extend:  # one warm-up, then the runs: the update's own seconds and the process's wall time
        emplace, total = [], []
        for r in range(int(opts["--runs"]) + 1):
            t0 = time.time()
            p = subprocess.run(cmd, capture_output=True, text=True)
            mm = re.search(lap, p.stderr)
            if p.returncode != 0 or not mm:
                break
            if r:
                emplace.append(float(mm.group(6))), total.append(round(time.time() - t0, 3))
        res["extend_emplace_s"], res["extend_total_s"] = spread(emplace), spread(total)
    plain_copy_s = None
    if n_remove:  # the same update without --remove first: its copy lap is the plain move of every IBF
        assert not extend and n_remove < n_files - m
        mm = re.search(lap, subprocess.run(cmd, capture_output=True, text=True).stderr)
        plain_copy_s = float(mm.group(5)) if mm else None
        open(os.path.join(d, "remove.txt"), "w").writelines(ln.rstrip("\n").split("\t")[1] + "\n" for ln in lines[:n_remove])
        open(os.path.join(d, "in.tsv"), "w").writelines(lines[n_remove:])  # what the check and the rebuild read
        cmd += ["--remove", os.path.join(d, "remove.txt")]
    if opts["--fold"]:  # (behind the runs above: their laps are those of the update without it)
        cmd += ["--fold", opts["--fold"]]
        lap, lap_keys = lap.replace(" emplace ", " fold ([0-9.eE+-]+) emplace "), lap_keys[:5] + ("fold_s",) + lap_keys[5:]
    t0 = time.time()
    p = subprocess.run(cmd, capture_output=True, text=True)
    upd = {"rc": p.returncode, "wall_s": round(time.time() - t0, 2)}
    if opts["--fold"]:
        upd["fold"], upd["index_line"] = int(opts["--fold"]), p.stdout.split("\n", 1)[0]
        upd["folded_lines"] = [ln for ln in p.stdout.splitlines() if ln.startswith("folded\t")][:12]
    if n_remove:
        upd["removed"], upd["copy_s_without_remove"] = n_remove, plain_copy_s
        upd["removed_lines"] = [ln for ln in p.stdout.splitlines() if ln.startswith(("removed\t", "dropped\t", "stale\t"))][:12]
    mm = re.search(lap, p.stderr)
    if mm:
        for key, x in zip(lap_keys, mm.groups()):
            upd[key] = float(x)
    mm = re.search(r"^result\t.*", p.stdout, re.M)
    upd["result"] = mm.group(0) if mm else (p.stderr or p.stdout)[-300:]
    upd["ibf_lines"] = [ln for ln in p.stdout.splitlines() if ln.startswith("ibf\t")][:8]
    upd["warn_fill_lines"] = sum(ln.endswith("WARN fill") for ln in p.stdout.splitlines())
    if extend:
        upd["extended_lines"] = [ln for ln in p.stdout.splitlines() if ln.startswith("extended\t")][:8]
    if p.returncode == 0:
        upd["hibf_bytes"] = os.path.getsize(os.path.join(d, "upd.hibf"))
        upd.update(verify_run("upd.hibf"))
    res["update"] = upd
    res["rebuild"] = hibf_run(layout)
    if extend and res["rebuild"]["rc"] == 0:
        again = [hibf_run(layout) for _ in range(int(opts["--runs"]))]
        res["rebuild_emplace_s"] = spread([r["emplace_s"] for r in again if "emplace_s" in r])
        res["rebuild_total_s"] = spread([r["wall_s"] for r in again])
    if not check and res["rebuild"]["rc"] == 0:
        res["rebuild"].update(verify_run())
    return res


def verify_run(db="db.hibf"):
    """an index just written against all the inputs"""
    res = {}
    t0 = time.time()
    p = subprocess.run([exe, "-i", os.path.join(d, "in.tsv"), "--hibf", "--verify-index", os.path.join(d, db), "-t", str(threads), "--verbose"] + parse_extra(),
                       capture_output=True, text=True)
    res["verify_rc"], res["verify_wall_s"] = p.returncode, round(time.time() - t0, 2)
    m = re.search(r" - seconds: hash ([0-9.eE+-]+) load ([0-9.eE+-]+) membership ([0-9.eE+-]+) fp ([0-9.eE+-]+)", p.stderr)
    if m:
        res["verify_hash_s"], res["verify_load_s"], res["verify_membership_s"], res["verify_fp_s"] = (float(x) for x in m.groups())
    m = re.search(r"max_observed_fp ([0-9.]+), mean_observed_fp ([0-9.]+)", p.stdout)
    if m:
        res["max_observed_fp"], res["mean_observed_fp"] = float(m.group(1)), float(m.group(2))
    lines = [ln for ln in p.stdout.splitlines()[2:] if not ln.startswith(("result\t", "  first false negative"))]
    res["verify_warn_lines"] = sum(ln.endswith("\tWARN fp") for ln in lines)
    res["verify_fail_lines"] = sum("\tFAIL" in ln for ln in lines)
    m = re.search(r"^result\t.*", p.stdout, re.M)
    res["verify_result"] = m.group(0) if m else (p.stderr or p.stdout)[-300:]
    return res


def median_of(runs):
    """the run with the median total time, and every run's total"""
    good = sorted((r for r in runs if r["rc"] == 0), key=lambda r: r.get("total_s", r["wall_s"]))
    if not good:
        return runs[-1]
    mid = dict(good[len(good) // 2])
    mid["totals_s"] = [r.get("total_s", r["wall_s"]) for r in runs]
    if all("emplace_s" in r for r in runs):
        mid["laps_s"] = [(r["hash_s"], r["union_s"], r["emplace_s"], r["write_s"]) for r in runs]
    return mid


if len(parse_modes) > 1:  # every mode in turn in each round; the hash lap and the total of every run
    flat_extra = ["-s", opts["--hash-functions"]]
    layout = opts["--layout"].split(",")[0]
    runs = {m: {"flat": [], "hibf": []} for m in parse_modes}
    for r in range(int(opts["--runs"]) + 1):  # (round 0 warms up)
        for parse_mode in parse_modes:
            one = {"flat": flat_run(opts["--max-fp"], flat_extra)}
            if hibf:
                one["hibf"] = hibf_run(layout)
            for kind, res in one.items():
                if r:
                    runs[parse_mode][kind].append(res)
    out["max_fp"], out["hash_functions"], out["runs"], out["parse"] = float(opts["--max-fp"]), int(opts["--hash-functions"]), int(opts["--runs"]), {}
    for m in parse_modes:
        out["parse"][m] = {}
        for kind, lap in (("flat", "count_hashes_s"), ("hibf", "hash_s")):
            if runs[m][kind]:
                mid = median_of(runs[m][kind])
                mid["hash_lap_s"] = spread([x[lap] for x in runs[m][kind] if lap in x])
                mid["total_runs_s"] = spread([x.get("total_s", x["wall_s"]) for x in runs[m][kind]])
                out["parse"][m][kind] = mid
elif not hibf:
    out.update(flat_run())
elif opts["--update"]:
    out["max_fp"], out["hash_functions"], out["updated_with"] = float(opts["--max-fp"]), int(opts["--hash-functions"]), int(opts["--update"])
    out["update"] = {name or "rule": update_run(name, int(opts["--update"])) for name in opts["--layout"].split(",")}
else:
    flat_extra = ["-s", opts["--hash-functions"]]
    layouts = opts["--layout"].split(",")
    flat_run(opts["--max-fp"], flat_extra)  # one run each to warm up
    for name in layouts:
        hibf_run(name)
    flats, hibfs = [], {name: [] for name in layouts}
    for _ in range(int(opts["--runs"])):
        flats.append(flat_run(opts["--max-fp"], flat_extra))
        for name in layouts:
            hibfs[name].append(hibf_run(name))
    out["max_fp"], out["hash_functions"], out["runs"] = float(opts["--max-fp"]), int(opts["--hash-functions"]), int(opts["--runs"])
    out["flat"] = median_of(flats)
    out["hibf"] = median_of(hibfs[layouts[0]]) if len(layouts) == 1 else {name: median_of(hibfs[name]) for name in layouts}
for f in os.listdir(d):
    os.remove(os.path.join(d, f))
os.rmdir(d)
print(json.dumps(out))
