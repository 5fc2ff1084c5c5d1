"""Packed hash sets on the GPU: the device's packing (gn_stream_distinct_hashes_packed) against the restated format's encoding of
gn_stream_distinct_hashes; the packed insert (gn_filter_emplace_packed_window) whole and slab by slab against the raw windowed insert and
oracle.Ibf; and the binary with --hash-sets packed|spilled, in one pass, under budgets and over a device list: the file is byte for byte
the raw one-pass build's, and a spilled build leaves no file behind."""
import filecmp
import os
import re

import numpy as np
import pytest

import oracle
from test_build_cpu import DATA, read_fasta_gz
from test_build_gpu import SEQS, SEQS2, check_filter, hashes_of, hip, run_build, write_inputs  # noqa: F401  (hip: a fixture)
from test_build_packed_cpu import BLOCK_BYTES, ITEM_BYTES, encode, flat_runs, packed_inputs
from test_build_slabs_cpu import BINS, CUTS, TOTAL_ROWS, oracle_filter, plan_rule
from test_build_slabs_gpu import slab_lines

pytestmark = pytest.mark.gpu
U64 = np.uint64


def as_arrays(blocks, payload):
    from ganon_amd.hip import PACKED_BLOCK_DTYPE
    return np.array(blocks, dtype=PACKED_BLOCK_DTYPE).reshape(-1), np.array(payload, dtype=U64)


# ------------------------------------------------------------------------------------------------------------ the ABI: packing
def packed_and_raw(hip, pieces, k, w):
    bases = np.frombuffer(b"".join(pieces), dtype=np.uint8)
    off = np.zeros(len(pieces) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(x) for x in pieces])
    tmp = hip.HipFilter.ibf(None, 64, 64, 1)
    st = hip.HipStream(tmp, len(pieces), bases.size)
    st.upload(bases, off, None)
    st.minimisers(k, w)
    first = st.distinct_hashes_packed()  # (packs a set nobody asked for raw yet)
    raw = st.distinct_hashes()
    again = st.distinct_hashes_packed()  # (the packed form of an earlier call)
    st.destroy()
    tmp.free()
    assert first[0] == again[0] and np.array_equal(first[1], again[1]) and np.array_equal(first[2], again[2])
    return first, raw


@pytest.mark.parametrize("case", ["SEQS", "20 kbp at (19, 32)", "k = 32", "a few hashes"])
def test_device_packing_is_the_encoding_of_the_distinct_hashes(hip, case):
    rng = np.random.default_rng(3)
    letters = np.frombuffer(b"ACGT", dtype=np.uint8)
    if case == "SEQS":
        pieces, k, w = [s.encode() for s in SEQS], 19, 32
    elif case == "20 kbp at (19, 32)":
        pieces, k, w = [bytes(rng.choice(letters, size=20_000))], 19, 32
    elif case == "k = 32":
        pieces, k, w = [bytes(rng.choice(letters, size=6_000))], 32, 40
    else:
        pieces, k, w = [b"ACGTNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNN"], 19, 32
    (n, blocks, words), raw = packed_and_raw(hip, pieces, k, w)
    exp = np.unique(np.concatenate([oracle.minimiser_hash(oracle.to_ranks(p), k, w) for p in pieces]))
    assert np.array_equal(raw, exp) and n == len(raw)
    eb, ew = as_arrays(*encode([raw]))
    assert np.array_equal(blocks, eb) and np.array_equal(words, ew), case
    if case == "20 kbp at (19, 32)":
        assert len(blocks) >= 3 and blocks["cnt"][-1] < 512, "several blocks, the last one short"
    if case == "k = 32":
        assert len(blocks) >= 2 and blocks["width"].max() > 52, "hashes over all 64 bits"
    if case == "a few hashes":
        assert len(blocks) == 1 and 1 < blocks["cnt"][0] < 8, "one short block: most lanes hold nothing"


# ------------------------------------------------------------------------------------------------------------ the ABI: the insert
def packed_runs(runs):
    return [as_arrays(*encode(files)) for files in runs]


def slabs_of(hip, h, runs, first_bin, per_bin, chunk):
    out = []
    for a, b in zip(CUTS, CUTS[1:]):
        f = hip.HipFilter.ibf_storage(BINS, b - a, h)
        f.emplace_packed_window(runs, first_bin, per_bin, TOTAL_ROWS, a, chunk)
        out.append(f.download_rows(0, b - a, 3))
        f.free()
    return out


@pytest.mark.parametrize("h", [1, 3, 5])
def test_packed_insert_equals_the_raw_insert_and_the_oracle(hip, h):
    runs, first_bin, per_bin = packed_inputs()
    flat, packed = flat_runs(runs), packed_runs(runs)
    ref = oracle_filter(flat, first_bin, per_bin, h)
    f = hip.HipFilter.ibf_storage(BINS, TOTAL_ROWS, h)
    f.emplace_runs_window(flat, first_bin, per_bin, TOTAL_ROWS, 0)
    raw = f.download_rows(0, TOTAL_ROWS, 3)
    f.free()
    assert np.array_equal(raw, ref)
    f = hip.HipFilter.ibf_storage(BINS, TOTAL_ROWS, h)  # whole
    f.emplace_packed_window(packed, first_bin, per_bin, TOTAL_ROWS, 0)
    whole = f.download_rows(0, TOTAL_ROWS, 3)
    f.free()
    assert np.array_equal(whole, raw) and np.array_equal(whole, ref)
    for chunk in (0, 700):  # (700 words: the runs are cut into several staging chunks, the later blocks carry their index in the run)
        got = np.concatenate(slabs_of(hip, h, packed, first_bin, per_bin, chunk))
        assert np.array_equal(got, raw) and np.array_equal(got, ref), (h, chunk)


def test_a_slab_no_row_falls_into_stays_zero(hip):
    runs, first_bin, per_bin = [[np.array([0x9E3779B97F4A7C15], dtype=U64)]], [129], [1]
    ref = oracle_filter(flat_runs(runs), first_bin, per_bin, 5)
    slabs = slabs_of(hip, 5, packed_runs(runs), first_bin, per_bin, 0)
    assert np.array_equal(np.concatenate(slabs), ref) and ref.any()
    assert any(not s.any() for s in slabs), "one hash has at most five rows: not every slab holds one"


def test_packed_window_refusals(hip):
    import ganon_amd
    f = hip.HipFilter.ibf_storage(BINS, 10, 3)
    one = [as_arrays(*encode([np.arange(5, dtype=U64)]))]

    def bad(**kw):
        blocks, words = as_arrays(*encode([np.arange(5, dtype=U64)]))
        for key, v in kw.items():
            blocks[key][0] = v
        return [(blocks, words)]

    for args, word in (((one, [0], [1], 9, 0), "rows"), ((one, [0], [1], 100, 91), "rows"), ((one, [0], [1], 2**32, 0), "2^32 - 1"),
                       ((one, [126], [1], 100, 0), "exceed the filter's 130 bins"), ((one, [0], [0], 100, 0), "bad argument"),
                       ((bad(cnt=0), [0], [1], 100, 0), "block 0 of 0 hashes"), ((bad(cnt=513), [0], [1], 100, 0), "block 0 of 513 hashes"),
                       ((bad(width=65), [0], [1], 100, 0), "at 65 bits")):
        with pytest.raises(ganon_amd.hip.GanonHipError) as e:
            f.emplace_packed_window(*args)
        assert word in str(e.value), (args[1:], str(e.value))
    assert not f.download_rows(0, 10, 3).any(), "a refused call writes nothing"
    f.free()


# ------------------------------------------------------------------------------------------------------------ the binary
def hash_sets_line(stderr):
    m = re.search(r"^hash sets: (\d+) hashes held (\w+) in (\d+) bytes \(8 x hashes = (\d+) bytes\)(?:, (\d+) files in (.*))?$", stderr, re.M)
    assert m, stderr
    return int(m.group(1)), m.group(2), int(m.group(3)), int(m.group(4)), m.group(5), m.group(6)


def uploaded(stderr):
    m = re.search(r"^filled in (\d+) pass(?:es)? over the hash sets, (\d+) hash bytes uploaded$", stderr, re.M)
    assert m, stderr
    return int(m.group(1)), int(m.group(2))


def inputs_of(d, case):
    """-> input file, extra arguments, (seqs, names) or None"""
    if case == "split targets":
        inp = os.path.join(d, "mode_input.tsv")
        with open(inp, "w") as o:
            for line in open(os.path.join(DATA, "mode_input.tsv")):
                f, t = line.rstrip("\n").split("\t")
                o.write(f"{os.path.join(DATA, f)}\t{t}\n")
        return inp, dict(extra=["--mode", "smallest", "--filter-size", "1"]), None
    seqs = SEQS if case == "one target each" else SEQS2
    targets = None if case == "one target each" else ["T1", "T9", "T1", "T8", "T1", "T1", "T1", "T1", "T4", "T1"]
    inp, _, names = write_inputs(d, seqs, targets)
    return inp, dict(max_fp=0.05 if targets is None else 0.001), (seqs, names)


@pytest.mark.parametrize("mode", ["packed", "spilled"])
@pytest.mark.parametrize("case", ["one target each", "shared targets", "split targets"])
def test_packed_and_spilled_builds_write_the_raw_file(hip, tmp_path, case, mode):
    from ganon_amd import ibf_file
    d = str(tmp_path)
    inp, kw, known = inputs_of(d, case)
    extra = list(kw.pop("extra", []))
    raw, p = run_build(d, inp, extra=extra + ["--verbose"], **kw)
    m = ibf_file.read_ibf_meta(raw)
    rows, row_bytes = m.bin_size, m.bin_words * 8
    n_raw, how, held, eight, _, _ = hash_sets_line(p.stderr)
    assert how == "raw" and held == eight == 8 * n_raw and uploaded(p.stderr) == (1, 8 * n_raw) and re.search(r"^RssAnon after hashing: \d+ kB$", p.stderr, re.M)
    if case == "split targets":
        assert m.bins > len(set(t for _, t in m.bin_map)) and m.bin_words == 2, "targets with several bins"
    exp_held = exp_pass = None
    if known:  # what the restated format makes of the oracle's hash sets: a target's files behind each other
        per_target = {}
        for s, t in zip(*known):
            per_target.setdefault(t, []).append(np.unique(hashes_of(s, 19, 32)))
        enc = [encode(files) for files in per_target.values()]
        n_blocks, n_words = sum(len(b) for b, _ in enc), sum(len(w) for _, w in enc)
        assert n_raw == sum(len(x) for files in per_target.values() for x in files)
        exp_held, exp_pass = 8 * n_words + BLOCK_BYTES * n_blocks, 8 * n_words + ITEM_BYTES * n_blocks
    three = next(P for P in (3, 4, 5) if rows % P)
    builds = [("one_pass", None, (0,)), ("a", -(-rows // three) * row_bytes, (0,)), ("b", -(-rows // 7) * row_bytes, (0,)), ("c", (rows - 1) * row_bytes, (0,)),
              ("list", -(-rows // 3) * row_bytes, (0, 0))]
    for tag, budget, devices in builds:
        sub = os.path.join(d, tag)
        os.mkdir(sub)
        tmp = os.path.join(d, tag + "_tmp")
        more = ["--hash-sets", mode, "--verbose", "--device", ",".join(map(str, devices))] + (["--device-memory", str(budget)] if budget else [])
        if tag in ("a", "list"):  # (with and without --tmp-output-folder: a spilled build's files go there, else beside the output)
            os.mkdir(tmp)
            more += ["--tmp-output-folder", tmp]
        out, p = run_build(sub, inp, extra=extra + more, **kw)
        assert filecmp.cmp(out, raw, shallow=False), (case, mode, tag)
        P = plan_rule(rows, row_bytes, budget, len(devices))[0] if budget else 1
        assert len(slab_lines(p.stderr)) == P and (P > 1 or budget is None)
        n, how, held, eight, files, folder = hash_sets_line(p.stderr)
        assert (n, how, eight) == (n_raw, mode, 8 * n_raw) and re.search(r"^RssAnon after hashing: \d+ kB$", p.stderr, re.M)
        passes, sent = uploaded(p.stderr)
        assert passes == P and sent % P == 0
        if exp_held is not None:
            assert held == exp_held and sent == P * exp_pass, (tag, held, exp_held, sent, exp_pass)
        assert sorted(os.listdir(sub)) == ["case.ibf"], "nothing but the filter is left"
        if mode == "spilled":
            assert int(files) >= 1 and os.path.samefile(folder, tmp if os.path.isdir(tmp) else sub)
        else:
            assert files is None
        if os.path.isdir(tmp):
            assert os.listdir(tmp) == [], "no arena file remains"
    if case == "one target each" and mode == "spilled":
        check_filter(hip, os.path.join(d, "b", "case.ibf"), known[0], known[1], 19, 32, 4, 0.05, 0)


@pytest.mark.parametrize("mode", ["packed", "spilled"])
def test_a_file_of_several_flushes_is_packed_on_the_host(hip, tmp_path, mode):
    # a sequence shorter than the window is hashed in a batch of its own: the file's sets are united on the host, then packed
    d = str(tmp_path)
    fa = os.path.join(d, "two.fasta")
    open(fa, "w").write(f">long\n{SEQS[0]}\n>short\n{SEQS[1][:25]}\n")
    inp = os.path.join(d, "in.tsv")
    open(inp, "w").write(f"{fa}\tT\n{os.path.join(d, 'one.fasta')}\tT\n")
    open(os.path.join(d, "one.fasta"), "w").write(f">one\n{SEQS[2]}\n")
    raw, _ = run_build(d, inp)
    sub = os.path.join(d, mode)
    os.mkdir(sub)
    out, p = run_build(sub, inp, extra=["--hash-sets", mode, "--verbose"])
    assert filecmp.cmp(out, raw, shallow=False) and sorted(os.listdir(sub)) == ["case.ibf"]
    files = [np.unique(np.concatenate([hashes_of(SEQS[0], 19, 32), hashes_of(SEQS[1][:25], 19, 32)])), np.unique(hashes_of(SEQS[2], 19, 32))]
    blocks, words = encode(files)
    assert hash_sets_line(p.stderr)[:3] == (sum(len(x) for x in files), mode, 8 * len(words) + BLOCK_BYTES * len(blocks))


def test_a_failed_spilled_build_leaves_no_file(hip, tmp_path):
    d = str(tmp_path)
    inp, _, _ = write_inputs(d, SEQS)
    before = sorted(os.listdir(d))
    os.mkdir(os.path.join(d, "case.ibf"))  # the output path is a directory: hashing runs, the filter cannot be written
    out, p = run_build(d, inp, extra=["--hash-sets", "spilled"], expect=1)
    assert "cannot write" in p.stderr and os.path.isdir(out) and os.listdir(out) == []
    assert sorted(os.listdir(d)) == sorted(before + ["case.ibf"]), "no arena file remains after a failure"
    # a "folder" no file can be created in (it is a file): the command ends with the arena file named and no output written
    os.rmdir(out)
    not_a_folder = os.path.join(d, "plain")
    open(not_a_folder, "w").close()
    out, p = run_build(d, inp, extra=["--hash-sets", "spilled", "--tmp-output-folder", not_a_folder], expect=1)
    assert "cannot create " + os.path.join(not_a_folder, "case.ibf.hashsets.") in p.stderr and not os.path.exists(out), p.stderr
