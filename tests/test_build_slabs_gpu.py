"""A flat `ganon-build` in row slabs on the GPU: the windowed insert (gn_filter_emplace_runs_window) slab by slab against the one-pass insert
and oracle.Ibf, and the binary forced into slabs (--device-memory) or over a device list (--device a,b): the file is byte for byte the
one-pass build's, passes test_build_gpu.check_filter, and classifies the same."""
import filecmp
import os
import re
import subprocess

import numpy as np
import pytest

from test_build_cpu import BIN_BUILD, DATA, read_fasta_gz
from test_build_gpu import SEQS, SEQS2, check_filter, hip, run_build, write_inputs  # noqa: F401  (hip: a fixture)
from test_build_slabs_cpu import BINS, CUTS, TOTAL_ROWS, oracle_filter, plan_rule, window_inputs

pytestmark = pytest.mark.gpu
U64 = np.uint64


# ------------------------------------------------------------------------------------------------------------ the ABI
def slabs_of(hip, h, runs, first_bin, per_bin, chunk):
    """one windowed call per slab of CUTS, each into a storage-only filter of its own -> the downloads"""
    out = []
    for a, b in zip(CUTS, CUTS[1:]):
        f = hip.HipFilter.ibf_storage(BINS, b - a, h)
        f.emplace_runs_window(runs, first_bin, per_bin, TOTAL_ROWS, a, chunk)
        out.append(f.download_rows(0, b - a, 3))
        f.free()
    return out


@pytest.mark.parametrize("h", [1, 3, 5])
def test_windowed_insert_equals_the_one_pass_insert_and_the_oracle(hip, h):
    runs, first_bin, per_bin = window_inputs()
    whole = hip.HipFilter.ibf_storage(BINS, TOTAL_ROWS, h)
    for r, f, p in zip(runs, first_bin, per_bin):
        whole.emplace_split(r, f, p)
    one_pass = whole.download_rows(0, TOTAL_ROWS, 3)
    whole.free()
    ref = oracle_filter(runs, first_bin, per_bin, h)
    assert np.array_equal(one_pass, ref)
    for chunk in (0, 700):  # (700: the 1300-hash run is cut by staging chunks, its later pieces carry the index in the run)
        got = np.concatenate(slabs_of(hip, h, runs, first_bin, per_bin, chunk))
        assert np.array_equal(got, one_pass) and np.array_equal(got, ref), (h, chunk)
    # the whole filter as one window: what a loop of gn_filter_emplace_split sets
    f = hip.HipFilter.ibf_storage(BINS, TOTAL_ROWS, h)
    f.emplace_runs_window(runs, first_bin, per_bin, TOTAL_ROWS, 0)
    assert np.array_equal(f.download_rows(0, TOTAL_ROWS, 3), one_pass)
    f.free()


def test_a_slab_no_row_falls_into_stays_zero(hip):
    runs, first_bin, per_bin = [np.array([0x9E3779B97F4A7C15], dtype=U64)], [129], [1]
    ref = oracle_filter(runs, first_bin, per_bin, 5)
    slabs = slabs_of(hip, 5, runs, first_bin, per_bin, 0)
    assert np.array_equal(np.concatenate(slabs), ref) and ref.any()
    assert any(not s.any() for s in slabs), "one hash has at most five rows: not every slab holds one"


def test_window_refusals(hip):
    import ganon_amd
    f = hip.HipFilter.ibf_storage(BINS, 10, 3)
    one = [np.arange(5, dtype=U64)]
    for args, word in (((one, [0], [1], 9, 0), "rows"), ((one, [0], [1], 100, 91), "rows"), ((one, [0], [1], 2**32, 0), "2^32 - 1"),
                       ((one, [126], [1], 100, 0), "exceed the filter's 130 bins"), ((one, [0], [0], 100, 0), "bad argument")):
        with pytest.raises(ganon_amd.hip.GanonHipError) as e:
            f.emplace_runs_window(*args)
        assert word in str(e.value), (args[1:], str(e.value))
    assert not f.download_rows(0, 10, 3).any(), "a refused call writes nothing"
    f.free()


# ------------------------------------------------------------------------------------------------------------ the binary
def slab_lines(stderr):
    return [tuple(int(x) for x in m.groups()) for m in re.finditer(r"^slab (\d+): rows \[(\d+), (\d+)\) device (\d+)$", stderr, re.M)]


def build_in_slabs(d, tag, inp, budget, one_pass, rows, row_bytes, devices=(0,), **kw):
    """a build with --device-memory `budget` (None: not given) over `devices`: the same bytes, the slab lines of the restated plan"""
    sub = os.path.join(d, tag)
    os.mkdir(sub)
    extra = ["--verbose"] + (["--device-memory", str(budget)] if budget is not None else []) + ["--device", ",".join(map(str, devices))]
    out, p = run_build(sub, inp, extra=extra, **kw)
    assert filecmp.cmp(out, one_pass, shallow=False), tag
    if budget is None:
        assert slab_lines(p.stderr) == [(0, 0, rows, devices[0])], "what is free holds these few rows: the one-pass build"
        return out, 1
    P, per, slab = plan_rule(rows, row_bytes, budget, len(devices))
    assert slab_lines(p.stderr) == [(i, slab(i)[0], slab(i)[0] + slab(i)[1], devices[slab(i)[2]]) for i in range(P)], (tag, p.stderr)
    assert f"filled in {P} pass" in p.stderr and " hash bytes uploaded" in p.stderr
    return out, P


@pytest.mark.parametrize("case", ["one target each", "shared targets"])
def test_slab_builds_write_the_one_pass_file(hip, tmp_path, case):
    from ganon_amd import ibf_file
    d = str(tmp_path)
    seqs = SEQS if case == "one target each" else SEQS2
    targets = None if case == "one target each" else ["T1", "T9", "T1", "T8", "T1", "T1", "T1", "T1", "T4", "T1"]
    inp, _, names = write_inputs(d, seqs, targets)
    kw = dict(max_fp=0.05 if targets is None else 0.001)
    one_pass, _ = run_build(d, inp, **kw)
    m = check_filter(hip, one_pass, seqs, names, 19, 32, 4, kw["max_fp"], 0)
    rows, row_bytes = m.bin_size, m.bin_words * 8
    assert rows >= 50, "enough rows for seven slabs"
    three = next(P for P in (3, 4, 5) if rows % P)  # (equal slabs where 3 divides the rows: one more, so that the last one is shorter)
    seen = set()
    for tag, budget in (("a", -(-rows // three) * row_bytes), ("b", -(-rows // 7) * row_bytes), ("c", (rows - 1) * row_bytes)):
        out, P = build_in_slabs(d, tag, inp, budget, one_pass, rows, row_bytes, **kw)
        check_filter(hip, out, seqs, names, 19, 32, 4, kw["max_fp"], 0)
        seen.add(P)
    assert seen == {three, plan_rule(rows, row_bytes, -(-rows // 7) * row_bytes, 1)[0], 2} and rows % three and max(seen) >= 6


def test_slab_build_of_split_targets(hip, tmp_path):
    # the sizing splits no target of ten 80-mers; it does split the reference's 25 genomes at --mode smallest --filter-size 1
    # (127 bins, two words a row), so a target's run of bins and the word boundary go through the windowed insert of the binary
    d = str(tmp_path)
    inp = os.path.join(d, "mode_input.tsv")
    seqs, names = [], []
    with open(inp, "w") as o:
        for line in open(os.path.join(DATA, "mode_input.tsv")):
            f, t = line.rstrip("\n").split("\t")
            o.write(f"{os.path.join(DATA, f)}\t{t}\n")
            for s in read_fasta_gz(os.path.join(DATA, f)):
                seqs.append(s)
                names.append(t)
    kw = dict(extra=["--mode", "smallest", "--filter-size", "1"])
    from ganon_amd import ibf_file
    one_pass, _ = run_build(d, inp, **kw)
    m = ibf_file.read_ibf_meta(one_pass)
    assert m.bins > len(set(names)) and m.bin_words == 2, "targets with several bins"
    sub = os.path.join(d, "slabs")
    os.mkdir(sub)
    out, p = run_build(sub, inp, extra=kw["extra"] + ["--verbose", "--device-memory", str(-(-m.bin_size // 3) * m.bin_words * 8)])
    assert len(slab_lines(p.stderr)) == 3 and filecmp.cmp(out, one_pass, shallow=False)
    check_filter(hip, out, seqs, names, 19, 32, 4, 0.05, 1.0, "smallest")


def test_device_lists(hip, tmp_path):
    from ganon_amd import ibf_file
    d = str(tmp_path)
    inp, _, names = write_inputs(d, SEQS)
    one_pass, _ = run_build(d, inp)
    m = ibf_file.read_ibf_meta(one_pass)
    rows, row_bytes = m.bin_size, m.bin_words * 8
    out, P = build_in_slabs(d, "two_workers", inp, -(-rows // 3) * row_bytes, one_pass, rows, row_bytes, devices=(0, 0))
    assert P == 3
    check_filter(hip, out, SEQS, names, 19, 32, 4, 0.05, 0)
    build_in_slabs(d, "list_alone", inp, None, one_pass, rows, row_bytes, devices=(0, 0))
    # refusals: nothing is written
    absent = hip.device_count()
    for tag, extra, words in (("absent", ["--device", f"0,{absent}"], [f"--device {absent} does not exist"]),
                              ("no_row", ["--device-memory", str(row_bytes - 1)], [f"{row_bytes} bytes", "not one row fits"])):
        sub = os.path.join(d, tag)
        os.mkdir(sub)
        out, p = run_build(sub, inp, extra=extra, expect=1)
        assert all(w in p.stderr for w in words) and not os.path.exists(out), (tag, p.stderr)


def test_slab_built_filter_classifies_like_the_one_pass_file(hip, tmp_path):
    # the reads of test_build_gpu.test_built_filter_classifies_with_the_binary against a three-slab file
    import cli_util as cu
    from ganon_amd import ibf_file
    inp = str(tmp_path / "in.tsv")
    genomes = {}
    with open(inp, "w") as o:
        for line in open(os.path.join(DATA, "mode_input.tsv")):
            f, t = line.rstrip("\n").split("\t")
            o.write(f"{os.path.join(DATA, f)}\tG{t}\n")
            genomes[f"G{t}"] = "".join(read_fasta_gz(os.path.join(DATA, f)))
    files = {}
    for tag, extra in (("one_pass", []), ("slabs", None)):
        if extra is None:
            m = ibf_file.read_ibf_meta(files["one_pass"])
            extra = ["--device-memory", str(-(-m.bin_size // 3) * m.bin_words * 8), "--verbose"]
        files[tag] = str(tmp_path / f"{tag}.ibf")
        p = subprocess.run([BIN_BUILD, "-i", inp, "-o", files[tag], "--quiet", "-p", "0.01", "-t", "4"] + extra, capture_output=True, text=True)
        assert p.returncode == 0, p.stderr
        if tag == "slabs":
            assert len(slab_lines(p.stderr)) == 3
    assert filecmp.cmp(files["one_pass"], files["slabs"], shallow=False)
    rng = np.random.default_rng(4)
    fq = str(tmp_path / "reads.fq")
    with open(fq, "w") as o:
        for i in range(2000):
            g = genomes[f"G{i % 25}"]
            s = int(rng.integers(0, len(g) - 150))
            o.write(f"@r{i}\n{g[s:s + 150]}\n+\n{'I' * 150}\n")
    results = {}
    for tag, path in files.items():
        prefix = str(tmp_path / f"res_{tag}")
        cu.run(cu.BIN_HIP, ["--ibf", path, "--single-reads", fq, "-o", prefix, "--output-all", "--quiet", "--rel-cutoff", "0.9", "--skip-lca"])
        results[tag] = open(prefix + ".all").read()
    assert results["one_pass"] == results["slabs"] and results["slabs"].count("\n") >= 2000
