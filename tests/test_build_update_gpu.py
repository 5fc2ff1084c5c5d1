"""`ganon-build --hibf --update`, the device side: set bits per technical bin (gn_filter_bin_popcounts) against numpy over the
downloaded rows, the move of an IBF into a wider one (gn_filter_copy_ibf), and the fill an insert is predicted to leave against the
fill it leaves; and the command: indexes built from half of a fixture's targets and updated with the rest, checked bit for bit
against the old file and the oracle's hashes along the reported paths, by `--verify-index` over all inputs, and by classification."""
import ctypes as C
import math

import numpy as np
import pytest

import ganon_fixtures as gf
from test_build_verify_gpu import hip, paths_of  # noqa: F401  (hip: the module fixture)

pytestmark = pytest.mark.gpu

U64 = np.uint64
BINS = (1, 63, 64, 65, 200, 1000, 1100)  # W = 1, 1, 1, 2, 4, 16, 18: row strides 1, 1, 1, 2, 4, 16, 32 in an HIBF
ROWS = (1, 2, 254, 255, 256, 511, 4099, 70001)  # around a flush of the bit planes (240 words) and past a tile (960 steps of a wave)


def column_sums(mat: np.ndarray, bins: int) -> np.ndarray:
    """set bits per bin of a downloaded matrix [rows, W]"""
    out = np.zeros(mat.shape[1] * 64, dtype=U64)
    for r in range(0, mat.shape[0], 8192):  # (bit 0 of word w is bin 64 w: little-endian bytes, least significant bit first)
        part = np.ascontiguousarray(mat[r:r + 8192]).view(np.uint8)
        out += np.unpackbits(part, axis=1, bitorder="little").sum(axis=0, dtype=U64)
    return out[:bins]


def one_ibf(hip, bins, rows, h=3):
    """an HIBF of one IBF (padded row stride), all zero"""
    return hip.HipFilter.hibf([(None, bins, rows, h)], [np.zeros(bins, np.int64)], [np.arange(bins, dtype=np.int64)], bins)


def storage_only(hip, bins, rows, h=3):
    """a flat filter created without a bin map: dense rows"""
    from ganon_amd import hip as H
    d = H._desc(None, bins, rows, h)
    handle = C.c_void_p()
    H._check(H.load_library().gn_filter_upload_ibf(0, C.byref(d), None, 0, C.byref(handle)))
    return hip.HipFilter(handle, bins=[bins])


def check(flt, bins, rows, what, ibf_idx=0):
    W = (bins + 63) >> 6
    got = flt.bin_popcounts(bins, ibf_idx)
    exp = column_sums(flt.download_rows(0, rows, W, ibf_idx), bins)
    assert got.dtype == U64 and np.array_equal(got, exp), f"{what}: bins {bins} rows {rows}: first difference at bin {int(np.argmax(got != exp))}"
    return got


@pytest.mark.parametrize("bins", BINS)
def test_bin_popcounts(hip, bins):
    from ganon_amd import hip as H
    W = (bins + 63) >> 6
    rng = np.random.default_rng(bins)
    for rows in ROWS:
        for make in (one_ibf, storage_only):
            flt = make(hip, bins, rows)
            assert not check(flt, bins, rows, "zeros").any()
            flt.fill_random(5 + rows, 1)
            got = check(flt, bins, rows, "density 1/2")
            assert abs(float(got.sum()) / (rows * bins) - 0.5) <= 3.0 / math.sqrt(rows * bins)  # (six standard deviations of the mean)
            flt.fill_random(6 + rows, H.FILL_3_OF_8)
            check(flt, bins, rows, "density 3/8")
            # every bit set, the padding bins of the last word too: every plane saturates at every flush, and no padding bin is reported
            flt.write_rows(0, np.full((rows, W), ~U64(0), dtype=U64))
            got = flt.bin_popcounts(bins)
            assert np.array_equal(got, np.full(bins, rows, dtype=U64)), f"ones: bins {bins} rows {rows}"
            flt.free()
        flt = one_ibf(hip, bins, rows)
        n = min(20000, 4 * rows)
        flt.emplace(rng.integers(0, 1 << 38, size=n, dtype=U64), rng.integers(0, bins, size=n).astype(np.uint32))
        got = check(flt, bins, rows, "emplace")
        assert got.any()
        flt.free()


def test_bin_popcounts_wide_rows(hip):
    """rows of more than 64 words are read in chunks of 64 word columns: one chunk and a bit, and a stride that is no multiple of 64"""
    for bins, rows in ((64 * 64 + 1, 1500), (64 * 70, 977), (64 * 129 - 5, 300)):
        for make in (one_ibf, storage_only):
            flt = make(hip, bins, rows)
            flt.fill_random(bins, 1)
            check(flt, bins, rows, "wide")
            flt.free()


def test_bin_popcounts_in_a_tree(hip):
    """every IBF of a three-level HIBF after an insert along whole paths"""
    rng = np.random.default_rng(3)
    hb = gf.random_hibf(40, 8, 3, seed=48, density=0.0, hash_funs=3, rows=(3000, 9000))
    sets = [np.unique(rng.integers(0, 1 << 38, size=200 + 37 * u, dtype=U64)) for u in range(40)]
    paths, _, _ = paths_of(hb, [len(x) for x in sets])
    flt = hip.HipFilter.hibf([(None, f.bins, f.bin_size, f.hash_funs) for f in hb.ibfs], hb.next_ibf_id, hb.bin_to_user, 40)
    flt.emplace_path(sets, paths)
    assert len(hb.ibfs) >= 3
    for i, f in enumerate(hb.ibfs):
        assert check(flt, f.bins, f.bin_size, f"ibf {i}", ibf_idx=i).any()
    flt.free()


def test_bin_popcounts_refusals(hip):
    from ganon_amd import hip as H
    L = H.load_library()
    flat, tree = hip.HipFilter.ibf(None, 64, 1000, 3), one_ibf(hip, 65, 100)
    out = np.zeros(65, dtype=U64)
    for call in (lambda: flat.bin_popcounts(64, 1), lambda: tree.bin_popcounts(65, 1), lambda: H._check(L.gn_filter_bin_popcounts(None, 0, H._p(out))),
                 lambda: H._check(L.gn_filter_bin_popcounts(tree._h, 0, None))):
        with pytest.raises(H.GanonHipError) as e:
            call()
        assert e.value.code == -22 and "gn_filter_bin_popcounts" in str(e.value)
    with pytest.raises(ValueError):
        tree.bin_popcounts(64)  # fewer bins than the IBF has: refused, the library would write 65 counts
    assert len(tree.bin_popcounts()) == 65
    flat.free()
    tree.free()


@pytest.mark.parametrize("w_src,w_dst", [(1, 1), (1, 2), (3, 4), (5, 9), (16, 17)])
def test_copy_ibf(hip, w_src, w_dst):
    for rows in (1, 4099):
        b_src, b_dst = 64 * w_src - 7, 64 * w_dst - (0 if w_dst == w_src + 1 else 7)
        src, dst = one_ibf(hip, b_src, rows), one_ibf(hip, b_dst, rows)
        src.fill_random(w_src * 100 + rows, 1)
        dst.fill_random(9, 1)  # what was there has to go, the words beyond the source's too
        dst.copy_ibf(0, src, 0)
        a, b = src.download_rows(0, rows, w_src), dst.download_rows(0, rows, w_dst)
        assert a.any() and np.array_equal(b[:, :w_src], a) and not b[:, w_src:].any()
        pa, pb = src.bin_popcounts(b_src), dst.bin_popcounts(b_dst)
        assert np.array_equal(pb[:b_src], pa) and not pb[b_src:].any()
        src.free()
        dst.free()


def test_copy_ibf_refusals(hip):
    from ganon_amd import hip as H
    a, wide, rows, hashes = one_ibf(hip, 65, 100), one_ibf(hip, 200, 100), one_ibf(hip, 200, 101), one_ibf(hip, 200, 100, h=2)
    flat = hip.HipFilter.ibf(None, 200, 100, 3)
    for call, word in ((lambda: flat.copy_ibf(0, a, 0), "HIBF"), (lambda: wide.copy_ibf(0, flat, 0), "HIBF"),  # not both HIBF filters
                       (lambda: rows.copy_ibf(0, a, 0), "rows"), (lambda: hashes.copy_ibf(0, a, 0), "hash functions"),  # another shape
                       (lambda: a.copy_ibf(0, wide, 0), "words"),  # narrower than the source
                       (lambda: wide.copy_ibf(1, a, 0), "ibf"), (lambda: wide.copy_ibf(0, a, 1), "ibf")):
        with pytest.raises(H.GanonHipError) as e:
            call()
        assert e.value.code == -22 and word in str(e.value), str(e.value)
    assert not wide.download_rows(0, 100, 4).any(), "a refused copy writes nothing"
    for f in (a, wide, rows, hashes, flat):
        f.free()


@pytest.mark.parametrize("rows", [4099, 1000003])
def test_fill_prediction(hip, rows):
    """the fill the update's placement predicts, rows * (1 - (1 - t / rows) * exp(-h n / rows)), against the insert: within 3 sqrt(rows).
    A set bit is new with probability 1 - t / rows whatever the others are, and the indicators of the rows a set hits are negatively
    associated, so the variance of the bit count is at most rows / 4: the bound is six standard deviations."""
    from ganon_amd import hip as H
    h, bins, b = 3, 65, 64
    flt = one_ibf(hip, bins, rows, h)
    flt.fill_random(rows, H.FILL_3_OF_16)
    before = int(flt.bin_popcounts(bins)[b])
    assert abs(before / rows - 3 / 16) < 0.03
    n = int(rows / h * math.log((1 - before / rows) / 0.7))  # to a fill of about 0.3
    hashes = np.unique(np.random.default_rng(rows).integers(0, 1 << 62, size=n + n // 8, dtype=U64))[:n]
    assert len(hashes) == n
    flt.emplace(hashes, np.full(n, b, dtype=np.uint32))
    after = flt.bin_popcounts(bins)
    predicted = rows * (1.0 - (1.0 - before / rows) * math.exp(-float(h) * n / rows))
    print(f"rows {rows}: {before} bits, {n} hashes, predicted {predicted:.1f}, found {int(after[b])}, bound {3 * math.sqrt(rows):.1f}")
    assert abs(int(after[b]) - predicted) <= 3 * math.sqrt(rows)
    assert abs(predicted / rows - 0.3) < 0.002, "the set was sized for a fill of 0.3"
    flt.free()


def test_bin_popcounts_dense_odd_strides(hip):
    """dense rows whose width does not divide 64: 21 rows of 3 words, 12 of 5, 9 of 7 a wave step, the other lanes idle, nothing folded"""
    for bins, rows in ((64 * 3 - 1, 4099), (64 * 5, 2000), (64 * 7 - 30, 70001)):
        flt = storage_only(hip, bins, rows)
        flt.fill_random(bins, 1)
        check(flt, bins, rows, "odd stride")
        flt.free()


# ------------------------------------------------------------------------------------------------------------ the command
import os  # noqa: E402
import subprocess  # noqa: E402

import cli_util as cu  # noqa: E402
from test_build_cpu import BIN_BUILD  # noqa: E402
from test_build_hibf_gpu import Inputs, K, W, build, cut_reads, genomes, hashes_of, short200  # noqa: E402,F401  (genomes, short200: fixtures)
from test_build_similarity_gpu import families36  # noqa: E402,F401  (a fixture)
from test_build_verify_gpu import check_report, rows_of, verify  # noqa: E402


def part(inp, names, path):
    """the lines of an input file that name one of `names`, as an input of their own"""
    keep = set(names)
    with open(path, "w") as o:
        for line in open(inp.tsv):
            if line.rstrip("\n").split("\t")[1] in keep:
                o.write(line)
    return Inputs(path, [t for t in inp.order if t in keep], inp.seqs)


def update(old, tsv, out, extra=(), expect=0):
    """-> (targets {name: dict}, ibfs {i: dict}, merged [(ibf, bin, before, predicted, after, warn)], result line)"""
    p = subprocess.run([BIN_BUILD, "--hibf", "--update", old, "-i", tsv, "-o", out, "-t", "2", "--verbose"] + list(extra), capture_output=True, text=True, timeout=300)
    assert p.returncode == expect, (p.returncode, p.stdout[-2000:], p.stderr[-2000:])
    if expect:
        return p
    lines = p.stdout.splitlines()
    assert lines[0].startswith("index\t") and lines[-1].startswith("result\tok\t")
    assert " - seconds: hash " in p.stderr and all(w in p.stderr for w in (" load ", " count ", " plan ", " copy ", " emplace ", " write "))
    targets, ibfs, merged = {}, {}, []
    for ln in lines[1:-1]:
        f = ln.split("\t")
        if f[0] == "target":
            assert len(f) == 9, ln
            targets[f[1]] = dict(user_bin=int(f[2]), n=int(f[3]), leaf=int(f[4]), first=int(f[5]), bins=int(f[6]), depth=int(f[7]),
                                 path=[tuple(int(x) for x in e.split(":")) for e in f[8].split(" ")])
        elif f[0] == "ibf":
            ibfs[int(f[1])] = dict(rows=int(f[2]), before=int(f[3]), after=int(f[4]), fill_before=float(f[5]), fill_after=float(f[6]))
        elif f[0] == "merged":
            merged.append((int(f[1]), int(f[2]), int(f[3]), float(f[4]), int(f[5]), len(f) > 6 and f[6] == "WARN fill"))
        else:
            assert ln.startswith("#"), ln
    return targets, ibfs, merged, lines[-1]


def check_update(old, new, inp_new, min_length, report):
    """the written bits equal the old file's, widened, with every new target's oracle hashes ORed along the path the report printed"""
    from ganon_amd import ibf_file
    targets, ibfs, merged, _ = report
    a, b = ibf_file.read_hibf_meta(old), ibf_file.read_hibf_meta(new)
    names, sets = inp_new.sets(min_length)
    assert list(targets) == names and [targets[t]["user_bin"] for t in names] == list(range(len(a.names), len(a.names) + len(names)))
    assert (b.kmer_size, b.window_size, b.fpr) == (a.kmer_size, a.window_size, a.fpr) and len(b.ibfs) == len(a.ibfs)
    assert b.bin_path[:len(a.names)] == a.bin_path and b.user_bin_filenames[:len(a.names)] == a.user_bin_filenames, "the file's strings, verbatim"
    assert b.names[:len(a.names)] == a.names and b.names[len(a.names):] == names, "old names and ids stay, new ones follow in input order"
    touched = [set() for _ in a.ibfs]
    exp = []
    for i, ((bins_a, rows_a, h, _), (bins_b, rows_b, h_b, _)) in enumerate(zip(a.ibfs, b.ibfs)):
        assert rows_b == rows_a and h_b == h and bins_b >= bins_a
        assert np.array_equal(np.asarray(b.next_ibf_id[i])[:bins_a], np.asarray(a.next_ibf_id[i])[:bins_a])
        assert np.array_equal(np.asarray(b.bin_to_user[i])[:bins_a], np.asarray(a.bin_to_user[i])[:bins_a])
        assert (i in ibfs) == (bins_b != bins_a or any(i in [e[0] for e in t["path"]] for t in targets.values()))
        if i in ibfs:
            assert (ibfs[i]["rows"], ibfs[i]["before"], ibfs[i]["after"]) == (rows_a, bins_a, bins_b)
        m = np.zeros((rows_a, (bins_b + 63) >> 6), dtype=U64)
        m[:, :(bins_a + 63) >> 6] = a.payload(old, i)
        exp.append(m)
    for t, hs in zip(names, sets):
        r = targets[t]
        assert r["n"] == len(hs) and r["path"][-1] == (r["leaf"], r["first"]) and r["depth"] == len(r["path"]) and r["path"][0][0] == 0
        for d, (i, first) in enumerate(r["path"]):
            leaf = d == len(r["path"]) - 1
            per = -(-len(hs) // r["bins"]) if leaf else 1
            bins = (first + np.arange(len(hs)) // per) if leaf else np.full(len(hs), first)
            assert not leaf or (int(np.asarray(b.bin_to_user[i])[first]) == r["user_bin"] and int(bins.max()) < first + r["bins"])
            assert leaf or int(np.asarray(b.next_ibf_id[i])[first]) == r["path"][d + 1][0]
            touched[i].update(range(first, first + (r["bins"] if leaf else 1)))
            for fn in range(a.ibfs[i][2]):
                np.bitwise_or.at(exp[i], (rows_of(hs, fn, a.ibfs[i][1]).astype(np.int64), bins >> 6), U64(1) << (bins & 63).astype(U64))
    for i in range(len(a.ibfs)):
        got = b.payload(new, i)
        assert np.array_equal(got, exp[i]), f"IBF {i}"
        was = a.payload(old, i)
        for bin_ in set(range(a.ibfs[i][0])) - touched[i]:  # a bin on no new path: its column as it was
            assert np.array_equal((got[:, bin_ >> 6] >> U64(bin_ & 63)) & U64(1), (was[:, bin_ >> 6] >> U64(bin_ & 63)) & U64(1)), (i, bin_)
    for i, bin_, before, predicted, after, warn in merged:
        rows = a.ibfs[i][1]
        print(f"merged ibf {i} bin {bin_}: {before} -> predicted {predicted} found {after} of {rows} rows{' WARN' if warn else ''}")
        assert after <= predicted + 3 * math.sqrt(rows) and bin_ in touched[i]
        assert after == int(((exp[i][:, bin_ >> 6] >> U64(bin_ & 63)) & U64(1)).sum())
    return a, b


def classify_finds_everything(index, inp, min_length, tmp_path, seed):
    reads = cut_reads(inp, min_length, np.random.default_rng(seed))
    fq = str(tmp_path / "reads.fq")
    gf.write_fastq(fq, [(rid, seq) for rid, seq, _ in reads])
    outs = {}
    for tag, binary in (("hip", cu.BIN_HIP), ("oracle", cu.build_oracle_binary())):
        prefix = str(tmp_path / tag)
        cu.run(binary, ["--ibf", index, "--hibf", "--single-reads", fq, "-o", prefix, "--output-all", "--skip-lca", "--rel-cutoff", "1", "--rel-filter", "1", "--quiet"])
        outs[tag] = (open(prefix + ".all", "rb").read(), open(prefix + ".rep", "rb").read())
    assert outs["hip"] == outs["oracle"], ".all / .rep"
    found = {}
    for line in outs["hip"][0].decode().splitlines():
        rid, target, count = line.split("\t")
        found.setdefault(rid, {})[target] = int(count)
    sources = set()
    for rid, seq, source in reads:
        if source is not None:
            sources.add(source)
            assert found.get(rid, {}).get(source) == len(hashes_of(seq)), (rid, source, found.get(rid))
    return sources


def all_ok(index, inp, min_length, extra=()):
    """`--verify-index` over all inputs: exit 0, every line `ok`, and every figure of the report equal to the restatement's"""
    got = verify(index, inp.tsv, extra=extra)
    _, lines, notes, result, _ = got
    print("verdicts:", {v: sum(r["verdict"] == v for r in lines.values()) for v in sorted({r["verdict"] for r in lines.values()})})
    assert not notes and result.startswith("result\tok\t")
    assert [t for t, r in lines.items() if r["verdict"] != "ok"] == [], "every line ok"
    check_report(index, inp, min_length, got)
    return lines


@pytest.mark.parametrize("which,tmax,s,max_fp,min_length,layout", [
    ("genomes", 8, 3, 0.001, 0, "rule"), ("genomes", 8, 0, 0.05, 0, "rule"), ("genomes", 8, 0, 0.05, 42000, "rule"),
    ("short200", 4, 3, 0.001, 0, "rule"), ("families36", 6, 3, 0.001, 0, "similarity")])
def test_update(hip, request, tmp_path, which, tmax, s, max_fp, min_length, layout):
    inp = request.getfixturevalue(which)
    half = len(inp.order) // 2
    first, rest = part(inp, inp.order[:half], str(tmp_path / "first.tsv")), part(inp, inp.order[half:], str(tmp_path / "rest.tsv"))
    old, new = str(tmp_path / "old.hibf"), str(tmp_path / "new.hibf")
    build(first, old, tmax, s, max_fp, min_length, extra=("--layout", layout))
    before = open(old, "rb").read()
    ml = ["--min-length", str(min_length)] if min_length else []
    report = update(old, rest.tsv, new, extra=ml)
    assert open(old, "rb").read() == before, "the index given is left as it is"
    a, b = check_update(old, new, rest, min_length, report)
    assert f"{len(b.names) - len(a.names)} user bin(s) added" in report[3] and f"{len(before)} -> {os.path.getsize(new)} bytes" in report[3]
    lines = all_ok(new, inp, min_length, extra=ml)
    named = set(inp.sets(min_length)[0])
    assert {t for t, r in lines.items() if r["user_bin"] != "-"} == named == set(b.names)
    assert classify_finds_everything(new, inp, min_length, tmp_path, tmax) == named, "reads from every old and every new target"


def test_update_of_an_update(hip, genomes, tmp_path):
    n = len(genomes.order)
    parts = [part(genomes, genomes.order[a:b], str(tmp_path / f"p{a}.tsv")) for a, b in ((0, n // 3), (n // 3, 2 * n // 3), (2 * n // 3, n))]
    files = [str(tmp_path / f"db{i}.hibf") for i in range(3)]
    build(parts[0], files[0], 4, 3, 0.001)
    for i in (1, 2):
        check_update(files[i - 1], files[i], parts[i], 0, update(files[i - 1], parts[i].tsv, files[i]))
    assert len(all_ok(files[2], genomes, 0)) == n


def test_update_refusals(hip, genomes, tmp_path):
    half = len(genomes.order) // 2
    first = part(genomes, genomes.order[:half], str(tmp_path / "first.tsv"))
    again = part(genomes, genomes.order[half - 1:], str(tmp_path / "again.tsv"))  # one target the index holds already
    old, new = str(tmp_path / "old.hibf"), str(tmp_path / "new.hibf")
    build(first, old, 8, 3, 0.001)
    p = update(old, again.tsv, new, expect=1)
    assert "already in the index" in p.stderr and genomes.order[half - 1] in p.stderr and p.stdout == "" and not os.path.exists(new)
    rest = part(genomes, genomes.order[half:], str(tmp_path / "rest.tsv"))
    p = update(old, rest.tsv, new, extra=["--min-length", "100000000"], expect=1)  # no sequence is that long: no target has a hash
    assert "No valid sequences to build" in p.stderr and not os.path.exists(new)
