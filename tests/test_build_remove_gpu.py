"""`ganon-build --hibf --update --remove` on the device: the column-compacting move of an IBF (gn_filter_copy_ibf_spans) against numpy's
gather over the downloaded rows, its bit counts, its refusals; and the command: indexes of a fixture's targets with some of them taken
out, checked column by column against the old file, by `--verify-index` over the surviving and over all inputs, and by classification."""
import os
import subprocess

import numpy as np
import pytest

import ganon_fixtures as gf
from test_build_remove_cpu import gather, span_cases
from test_build_update_gpu import hip, one_ibf  # noqa: F401  (hip: the module fixture)

pytestmark = pytest.mark.gpu

U64 = np.uint64
SRC_BINS = (1, 63, 64, 65, 200, 1100)  # W = 1, 1, 1, 2, 4, 18: row strides 1, 1, 1, 2, 4, 32
ROWS = (1, 255, 4099)


def mapped(counts, spans, bins_dst):
    out = np.zeros(bins_dst, dtype=U64)
    for s, d, n in spans:
        out[d:d + n] = counts[s:s + n]
    return out


def check_copy(hip, src, a, counts, B, rows, spans, bins_dst, what):
    """the spans' copy of `src` (rows `a`, bit counts `counts`) into a destination of bins_dst bins that held random bits"""
    W_dst = (bins_dst + 63) >> 6
    dst = one_ibf(hip, bins_dst, rows)
    dst.fill_random(bins_dst + 3 * rows, 1)  # what was there has to go
    dst.copy_ibf_spans(0, src, 0, spans)
    got = dst.download_rows(0, rows, W_dst)
    exp = gather(a, spans, W_dst)
    assert np.array_equal(got, exp), f"{what}: {B} -> {bins_dst} bins, {rows} rows: first difference in row {int(np.argmax((got != exp).any(axis=1)))}"
    assert np.array_equal(dst.bin_popcounts(bins_dst), mapped(counts, spans, bins_dst)), f"{what}: bit counts"
    return dst, got


@pytest.mark.parametrize("B", SRC_BINS)
def test_copy_ibf_spans(hip, B):
    W = (B + 63) >> 6
    for rows in ROWS:
        src = one_ibf(hip, B, rows)
        src.fill_random(B * 7 + rows, 1)
        a, counts = src.download_rows(0, rows, W), src.bin_popcounts(B)
        assert a.any() or rows * B < 64  # (a handful of random bits may all be clear)
        for name, spans in span_cases(B).items():
            used = max((d + n for _, d, n in spans), default=0)
            for extra in (0, 1, 70):
                dst, got = check_copy(hip, src, a, counts, B, rows, spans, max(used + extra, 1), name)
                if name == "identity":
                    plain = one_ibf(hip, used + extra, rows)
                    plain.fill_random(11, 1)
                    plain.copy_ibf(0, src, 0)
                    assert np.array_equal(plain.download_rows(0, rows, (used + extra + 63) >> 6), got), "the identity span is the plain copy"
                    plain.free()
                dst.free()
        src.free()


def test_copy_ibf_spans_padding_bins_do_not_travel(hip):
    """a source whose padding bins are set (rows written as they are): the destination's padding bins and further words stay clear"""
    for B in (1, 65, 200):
        W, rows = (B + 63) >> 6, 300
        src = one_ibf(hip, B, rows)
        a = np.full((rows, W), ~U64(0), dtype=U64)
        src.write_rows(0, a)
        for name, spans in span_cases(B).items():
            used = max((d + n for _, d, n in spans), default=0)
            dst, got = check_copy(hip, src, a, np.full(B, rows, dtype=U64), B, rows, spans, used + 70, name)
            assert int(np.unpackbits(got.view(np.uint8), axis=1, bitorder="little")[:, used:].sum()) == 0
            dst.free()
        src.free()


def test_copy_ibf_spans_wide_rows(hip):
    """rows of more than 64 words (a stride of 80): blocks along the row; and a destination narrower than the source by whole words"""
    B, rows = 64 * 70, 300
    src = one_ibf(hip, B, rows)
    src.fill_random(B, 1)
    a, counts = src.download_rows(0, rows, 70), src.bin_popcounts(B)
    cases = span_cases(B)
    cases["a narrow destination"] = [(64 * 40 + 7, 0, 100), (5, 100, 20)]
    for name, spans in cases.items():
        used = max((d + n for _, d, n in spans), default=0)
        check_copy(hip, src, a, counts, B, rows, spans, max(used, 1) + (70 if name == "one bin kept" else 0), name)[0].free()
    wide = 64 * 520 - 9  # (a stride of 528 words, 264 pairs: more than one block along the row)
    check_copy(hip, src, a, counts, B, rows, [(0, wide - B, B)], wide, "into the end of a wider IBF")[0].free()
    src.free()


def test_copy_ibf_spans_refusals(hip):
    from ganon_amd import hip as H
    a, wide, rows, hashes = one_ibf(hip, 65, 100), one_ibf(hip, 200, 100), one_ibf(hip, 200, 101), one_ibf(hip, 200, 100, h=2)
    flat = hip.HipFilter.ibf(None, 200, 100, 3)
    a.fill_random(1, 1)
    wide.fill_random(2, 1)
    before = wide.download_rows(0, 100, 4)
    one = [(0, 0, 65)]
    L = H.load_library()
    table = np.array([[0, 0, 65, 0]], dtype=np.uint32)
    for call, word in ((lambda: flat.copy_ibf_spans(0, a, 0, one), "HIBF"), (lambda: wide.copy_ibf_spans(0, flat, 0, one), "HIBF"),
                       (lambda: rows.copy_ibf_spans(0, a, 0, one), "rows"), (lambda: hashes.copy_ibf_spans(0, a, 0, one), "hash functions"),
                       (lambda: wide.copy_ibf_spans(1, a, 0, one), "ibf"), (lambda: wide.copy_ibf_spans(0, a, 1, one), "ibf"),
                       (lambda: wide.copy_ibf_spans(0, wide, 0, one), "onto itself"),
                       (lambda: wide.copy_ibf_spans(0, a, 0, [(0, 0, 0)]), "0 bins"),
                       (lambda: wide.copy_ibf_spans(0, a, 0, [(1, 0, 65)]), "beyond the source"),
                       (lambda: wide.copy_ibf_spans(0, a, 0, [(0, 136, 65)]), "beyond the destination"),
                       (lambda: wide.copy_ibf_spans(0, a, 0, [(0, 0, 10), (20, 9, 10)]), "overlap"),
                       (lambda: wide.copy_ibf_spans(0, a, 0, [(0, 50, 10), (20, 0, 10)]), "ascend"),
                       (lambda: H._check(L.gn_filter_copy_ibf_spans(None, 0, a._h, 0, H._p(table), 1)), "null"),
                       (lambda: H._check(L.gn_filter_copy_ibf_spans(wide._h, 0, None, 0, H._p(table), 1)), "null"),
                       (lambda: H._check(L.gn_filter_copy_ibf_spans(wide._h, 0, a._h, 0, None, 1)), "null")):
        with pytest.raises(H.GanonHipError) as e:
            call()
        assert e.value.code == -22 and word in str(e.value) and "gn_filter_copy_ibf_spans" in str(e.value), str(e.value)
        assert np.array_equal(wide.download_rows(0, 100, 4), before), "a refused copy writes nothing"
    wide.copy_ibf_spans(0, a, 0, [])  # no span: the destination is cleared
    assert not wide.download_rows(0, 100, 4).any() and not wide.bin_popcounts(200).any()
    for f in (a, wide, rows, hashes, flat):
        f.free()


# ------------------------------------------------------------------------------------------------------------ the command
import cli_util as cu  # noqa: E402
import hibf_checks as hc  # noqa: E402
from test_build_cpu import BIN_BUILD  # noqa: E402
from test_build_extend_gpu import MEMBERS, families, inputs, restated, union  # noqa: E402,F401  (families: a fixture)
from test_build_hibf_gpu import Inputs, build, cut_reads, genomes, short200  # noqa: E402,F401  (genomes, short200: fixtures)
from test_build_remove_cpu import plan  # noqa: E402  (the rule, restated)
from test_build_similarity_gpu import families36  # noqa: E402,F401  (a fixture)
from test_build_update_gpu import all_ok, classify_finds_everything, column_sums, part, update  # noqa: E402
from test_build_verify_gpu import verify  # noqa: E402


def remove(old, names, out, tmp_path, tsv=None, extra=(), expect=0):
    """-> dict(index, removed, dropped, stale, targets, result, lines) of the report, or the process when the command is to fail"""
    listed = str(tmp_path / (os.path.basename(out) + ".names.txt"))
    with open(listed, "w") as o:
        o.write("".join(n + "\n" for n in names) + "\n" + (names[0] + "\n" if names else ""))  # an empty line and a repeat: ignored
    args = [BIN_BUILD, "--hibf", "--update", old, "--remove", listed, "-o", out, "-t", "2", "--verbose"] + (["-i", tsv] if tsv else []) + list(extra)
    p = subprocess.run(args, capture_output=True, text=True, timeout=300)
    assert p.returncode == expect, (p.returncode, p.stdout[-2000:], p.stderr[-2000:])
    if expect:
        return p
    lines = p.stdout.splitlines()
    assert lines[0].startswith("index\t") and lines[-1].startswith("result\tok\t") and "--remove            " + listed in p.stderr
    rep = dict(index=lines[0], result=lines[-1], removed=[], dropped=[], stale=[], targets={}, extended={}, lines=lines)
    for ln in lines[1:-1]:
        f = ln.split("\t")
        if f[0] == "removed":
            assert len(f) == 9, ln
            rep["removed"].append((f[1], int(f[2]), int(f[3]), int(f[4]), int(f[5]), int(f[6]), f[7], [tuple(int(x) for x in e.split(":")) for e in f[8].split(" ")]))
        elif f[0] == "dropped":
            rep["dropped"].append(tuple(int(x) for x in f[1:]))
        elif f[0] == "stale":
            rep["stale"].append((int(f[1]), int(f[2]), int(f[3]), f[4]))
        elif f[0] == "target":
            rep["targets"][f[1]] = int(f[2])
        elif f[0] == "extended":
            rep["extended"][f[1]] = int(f[2])
    return rep


def tables(m):
    bins = [f[0] for f in m.ibfs]
    return bins, [f[1] for f in m.ibfs], [[int(x) for x in a[:b]] for a, b in zip(m.next_ibf_id, bins)], [[int(x) for x in a[:b]] for a, b in zip(m.bin_to_user, bins)]


def runs_of(m):
    """{user bin: (ibf, first, n)}, {ibf: (parent ibf, bin)}, {ibf: level}"""
    bins, _, nx, bu = tables(m)
    run, parent = {}, {}
    for i in range(len(bins)):
        for b in range(bins[i]):
            if bu[i][b] < 0:
                parent[nx[i][b]] = (i, b)
            else:
                run.setdefault(bu[i][b], [i, b, 0])[2] += 1
    level = {0: 0}
    for i in range(1, len(bins)):  # (a child's index is above its parent's in no particular order: walk up)
        at, d = i, 0
        while at != 0:
            at, d = parent[at][0], d + 1
        level[i] = d
    return {u: tuple(r) for u, r in run.items()}, parent, level


def columns(mat, first, n):
    return np.unpackbits(np.ascontiguousarray(mat[:, first >> 6:((first + n - 1) >> 6) + 1]).view(np.uint8), axis=1, bitorder="little")[:, first & 63:(first & 63) + n]


def names_below(m):
    """{(ibf, bin) of a merged bin: (level of its IBF, frozenset of the target names below it)}"""
    bins, _, nx, bu = tables(m)
    _, _, level = runs_of(m)

    def below(i):
        out = set()
        for b in range(bins[i]):
            out |= {m.names[bu[i][b]]} if bu[i][b] >= 0 else below(nx[i][b])
        return out
    return {(i, b): (level[i], frozenset(below(nx[i][b]))) for i in range(len(bins)) for b in range(bins[i]) if bu[i][b] < 0}


def choose(m, kind):
    """the names to remove, from the file's tables"""
    bins, _, nx, bu = tables(m)
    run, _, level = runs_of(m)
    n = len(m.names)
    if kind == "leaf":  # every user bin of one IBF of the lowest level: it drops
        lowest = [i for i in range(1, len(bins)) if level[i] == max(level.values()) and all(u >= 0 for u in bu[i])]
        i = min(lowest, key=lambda i: (len(set(bu[i])), i))
        users = sorted(set(bu[i]))
    elif kind == "ends":
        users = [0, n - 1]
    else:  # a split run
        users = [min(u for u, r in run.items() if r[2] >= 2)]
    return [m.names[u] for u in users], users


def check_remove(old, new, before, names, users, rep):
    """the file written against the file given: tables by the restated rule, columns bit for bit, strings verbatim, the report's figures"""
    from ganon_amd import ibf_file
    assert open(old, "rb").read() == before, "the index given is left as it is"
    assert os.path.getsize(new) < len(before), "the new file is strictly smaller"
    a, b = ibf_file.read_hibf_meta(old), ibf_file.read_hibf_meta(new)
    bins_a, rows_a, nx_a, bu_a = tables(a)
    bins_b, rows_b, nx_b, bu_b = tables(b)
    h = a.ibfs[0][2]
    mats_a = [a.payload(old, i) for i in range(len(bins_a))]
    mats_b = [b.payload(new, i) for i in range(len(bins_b))]
    pop_a = [[int(x) for x in column_sums(mats_a[i], bins_a[i])] for i in range(len(bins_a))]
    exp = plan(bins_a, nx_a, bu_a, len(a.names), users, rows_a, h, pop_a)
    assert (bins_b, nx_b, bu_b) == (exp["bins"], exp["nx"], exp["bu"]) and rows_b == [rows_a[i] for i in exp["old_ibf"]], "the tables after the removal"
    assert sum(bins_b) == sum(bins_a) - sum(r[3] for r in exp["removed"]) - len(exp["dropped"]), "bins per IBF add up to the survivors"
    hc.check_tree(bins_b, b.next_ibf_id, b.bin_to_user, len(b.names), max(bins_b), max_levels=64)
    keep = [u for u in range(len(a.names)) if exp["user_map"][u] >= 0]
    assert b.names == [a.names[u] for u in keep] and (b.kmer_size, b.window_size, b.fpr) == (a.kmer_size, a.window_size, a.fpr)
    assert b.bin_path == [a.bin_path[u] for u in keep] and b.user_bin_filenames == [a.user_bin_filenames[u] for u in keep], "the file's strings, verbatim"
    # every surviving target, found by name: its run's columns as they were
    run_a, _, _ = runs_of(a)
    run_b, _, _ = runs_of(b)
    for u_new, name in enumerate(b.names):
        (ia, fa, na), (ib, fb, nb) = run_a[a.names.index(name)], run_b[u_new]
        assert na == nb and np.array_equal(columns(mats_a[ia], fa, na), columns(mats_b[ib], fb, nb)), name
    # every surviving merged bin, found by the level of its IBF and the surviving names below it: likewise
    gone = set(names)
    was = {(lv, frozenset(s - gone)): at for at, (lv, s) in names_below(a).items() if s - gone}
    now = names_below(b)
    assert len(was) == len(now), "a merged bin with a target left below it survives, no other does"
    for (ib, bb), key in now.items():
        ia, ba = was[key]
        assert np.array_equal(columns(mats_a[ia], ba, 1), columns(mats_b[ib], bb, 1)), (ib, bb)
    # the report
    assert [r[0] for r in rep["removed"]] == [a.names[u] for u in sorted(users)]
    for got, e in zip(rep["removed"], exp["removed"]):
        assert got[1:6] == e[:5] and got[6] == ("full" if e[6] else str(e[5])), (got, e)
        assert got[7][-1] == (e[1], e[2]) and got[7][0][0] == 0
    assert rep["dropped"] == exp["dropped"]
    pop_b = [[int(x) for x in column_sums(mats_b[i], bins_b[i])] for i in range(len(bins_b))]
    assert rep["stale"] == [(s[2], s[3], pop_b[s[2]][s[3]], "full" if s[6] else str(s[5])) for s in exp["stale"]]
    assert f"ibfs={len(bins_a)}->{len(bins_b)} " in rep["index"] and f"user_bins={len(a.names)}->{len(b.names)} " in rep["index"]
    assert f"\t{len(users)} user bin(s) removed, {len(exp['dropped'])} IBF(s) dropped, " in rep["result"]
    return a, b, exp


def absent_from_classification(index, inp_removed, tmp_path):
    """reads cut from removed targets: no removed name in .all or .rep"""
    reads = cut_reads(inp_removed, 0, np.random.default_rng(9), n_random=0)
    fq = str(tmp_path / "removed_reads.fq")
    gf.write_fastq(fq, [(rid, seq) for rid, seq, _ in reads])
    prefix = str(tmp_path / "removed_hip")
    cu.run(cu.BIN_HIP, ["--ibf", index, "--hibf", "--single-reads", fq, "-o", prefix, "--output-all", "--skip-lca", "--rel-cutoff", "1", "--rel-filter", "1", "--quiet"])
    for ext in (".all", ".rep"):
        text = open(prefix + ext).read() if os.path.exists(prefix + ext) else ""
        for line in text.splitlines():
            assert not set(line.split("\t")) & set(inp_removed.order), (ext, line)


_index = {}


def index_of(request, tmp_path_factory, which, tmax, s, max_fp, layout):
    key = (which, tmax, s, max_fp, layout)
    if key not in _index:
        inp = request.getfixturevalue(which)
        out = str(tmp_path_factory.mktemp("remove_index") / "all.hibf")
        build(inp, out, tmax, s, max_fp, extra=("--layout", layout))
        _index[key] = (inp, out, open(out, "rb").read())
    return _index[key]


@pytest.mark.parametrize("which,tmax,s,max_fp,layout,kind", [
    ("genomes", 8, 3, 0.001, "rule", "leaf"), ("genomes", 8, 3, 0.001, "rule", "ends"), ("genomes", 8, 3, 0.001, "rule", "split"),
    ("short200", 4, 3, 0.001, "rule", "leaf"), ("families36", 6, 0, 0.05, "similarity", "ends")])
def test_remove(hip, request, tmp_path, tmp_path_factory, which, tmax, s, max_fp, layout, kind):
    """(genomes at tmax 8: 25 targets, 5 bins of the root are single, 3 are merged over 20 targets in leaves of 8 bins: a leaf of at most 6
    targets has spare bins, so a split run exists)"""
    from ganon_amd import ibf_file
    inp, old, before = index_of(request, tmp_path_factory, which, tmax, s, max_fp, layout)
    names, users = choose(ibf_file.read_hibf_meta(old), kind)
    new = str(tmp_path / "new.hibf")
    rep = remove(old, names, new, tmp_path)
    a, b, exp = check_remove(old, new, before, names, users, rep)
    print(f"{which} tmax {tmax} {kind}: {len(users)} of {len(a.names)} user bins removed, {len(exp['dropped'])} IBFs dropped, runs of "
          f"{[r[3] for r in exp['removed']]} bins, {len(exp['stale'])} stale merged bins")
    if kind == "leaf":
        assert exp["dropped"], "an IBF was dropped"
    if kind == "split":
        assert exp["removed"][0][3] >= 2, "a run of several bins was removed"
    survivors = part(inp, [t for t in inp.order if t not in names], str(tmp_path / "survivors.tsv"))
    lines = all_ok(new, survivors, 0)
    assert {t for t, r in lines.items() if r["user_bin"] != "-"} == set(b.names)
    _, rows, _, result, _ = verify(new, inp.tsv, expect=1)
    assert {t for t, r in rows.items() if r["verdict"] == "FAIL: no such user bin"} == set(names) and result.startswith("result\tFAIL")
    assert all(r["verdict"] in ("ok", "WARN fp") for t, r in rows.items() if t not in names)
    assert classify_finds_everything(new, survivors, 0, tmp_path, tmax) == set(b.names), "reads from every surviving target, found in full"
    absent_from_classification(new, part(inp, names, str(tmp_path / "removed.tsv")), tmp_path)


def test_remove_then_add_back(hip, request, genomes, tmp_path, tmp_path_factory):
    """the last targets of the input leave and come back with `--update`: the names are in the input's order again, and everything is found"""
    inp, old, before = index_of(request, tmp_path_factory, "genomes", 8, 3, 0.001, "rule")
    names = inp.order[-4:]
    less, again = str(tmp_path / "less.hibf"), str(tmp_path / "again.hibf")
    remove(old, names, less, tmp_path)
    back = part(inp, names, str(tmp_path / "back.tsv"))
    update(less, back.tsv, again)
    assert len(all_ok(again, inp, 0)) == len(inp.order)


def test_remove_add_and_extend_in_one_command(hip, families, tmp_path):
    """six families of four members each; one command takes a family out, gives the families the restated extension plan accepts their
    fifth member, and adds two new families.  (A removal changes no bit of a surviving bin, so what the plan accepts on the index given it
    accepts on the survivors; the family that leaves is one the plan rejects, where there is one.)"""
    from ganon_amd import ibf_file
    old_fams = [f"F{f}" for f in range(6)]
    base = inputs(families, {f: [0, 1, 2, 3] for f in old_fams}, str(tmp_path / "base.tsv"))
    old, new = str(tmp_path / "old.hibf"), str(tmp_path / "new.hibf")
    build(base, old, 4, 3, 0.05, extra=("--layout", "rule"))
    accepted = restated(old, {f: union(families, f, [4]) for f in old_fams})[0]
    assert len(accepted) >= 3, "the fixture is meant to leave room for at least three extensions"
    rejected = [f for f in old_fams if f not in accepted]
    gone = rejected[0] if rejected else accepted[-1]
    extended = [f for f in accepted if f != gone]
    members = {f: [4] for f in extended}
    members.update({"F6": list(range(MEMBERS)), "F7": list(range(MEMBERS))})
    rep = remove(old, [gone], new, tmp_path, tsv=inputs(families, members, str(tmp_path / "more.tsv")).tsv, extra=["--extend"])
    b = ibf_file.read_hibf_meta(new)
    kept = [f for f in old_fams if f != gone]
    assert b.names == kept + ["F6", "F7"] and [r[0] for r in rep["removed"]] == [gone]
    assert rep["extended"] == {f: kept.index(f) for f in extended} and rep["targets"] == {"F6": len(kept), "F7": len(kept) + 1}
    assert f"{len(extended)} user bin(s) extended, 2 user bin(s) added" in rep["result"] and "1 user bin(s) removed" in rep["result"]
    have = {f: [0, 1, 2, 3] + ([4] if f in extended else []) for f in kept}
    have.update({"F6": list(range(MEMBERS)), "F7": list(range(MEMBERS))})
    assert len(all_ok(new, inputs(families, have, str(tmp_path / "all.tsv"), order=b.names), 0)) == len(b.names)


def test_replacement(hip, request, genomes, tmp_path, tmp_path_factory):
    """a name in --remove and in the input: its user bin goes, another genome's sequences enter under the name as the last user bin"""
    from ganon_amd import ibf_file
    inp, old, before = index_of(request, tmp_path_factory, "genomes", 8, 3, 0.001, "rule")
    name, donor = inp.order[5], inp.order[11]
    tsv = str(tmp_path / "replace.tsv")
    with open(tsv, "w") as o:
        for line in open(inp.tsv):
            f, t = line.rstrip("\n").split("\t")
            if t == donor:
                o.write(f"{f}\t{name}\n")
    new = str(tmp_path / "replaced.hibf")
    rep = remove(old, [name], new, tmp_path, tsv=tsv)
    b = ibf_file.read_hibf_meta(new)
    others = [t for t in inp.order if t != name]
    assert b.names == others + [name] and rep["targets"] == {name: len(others)} and [r[0] for r in rep["removed"]] == [name]
    final = str(tmp_path / "final.tsv")
    with open(final, "w") as o:
        for line in open(inp.tsv):
            if line.rstrip("\n").split("\t")[1] != name:
                o.write(line)
        o.write(open(tsv).read())
    assert len(all_ok(new, Inputs(final, others + [name], {**inp.seqs, name: inp.seqs[donor]}), 0)) == len(inp.order)


def test_remove_from_an_updated_index(hip, genomes, tmp_path):
    from ganon_amd import ibf_file
    half = len(genomes.order) // 2
    first, rest = part(genomes, genomes.order[:half], str(tmp_path / "first.tsv")), part(genomes, genomes.order[half:], str(tmp_path / "rest.tsv"))
    files = [str(tmp_path / f"db{i}.hibf") for i in range(3)]
    build(first, files[0], 4, 3, 0.001)
    update(files[0], rest.tsv, files[1])
    before = open(files[1], "rb").read()
    m = ibf_file.read_hibf_meta(files[1])
    users = [1, half, len(m.names) - 1]  # one the build placed, two the update added
    names = [m.names[u] for u in users]
    check_remove(files[1], files[2], before, names, users, remove(files[1], names, files[2], tmp_path))
    all_ok(files[2], part(genomes, [t for t in genomes.order if t not in names], str(tmp_path / "survivors.tsv")), 0)


def test_remove_refusals(hip, request, genomes, tmp_path, tmp_path_factory):
    inp, old, before = index_of(request, tmp_path_factory, "genomes", 8, 3, 0.001, "rule")
    new = str(tmp_path / "new.hibf")
    p = remove(old, [inp.order[0], "not there", inp.order[1], "nor this"], new, tmp_path, expect=1)
    assert "not there" in p.stderr and "nor this" in p.stderr and "2 name(s) are not in the index" in p.stderr and "nothing written" in p.stderr
    assert p.stdout == "" and not os.path.exists(new)
    p = remove(old, list(inp.order), new, tmp_path, expect=1)
    assert "nothing would be left" in p.stderr and p.stdout == "" and not os.path.exists(new)
    listed = str(tmp_path / "names.txt")
    open(listed, "w").write(inp.order[0] + "\n")
    p = subprocess.run([BIN_BUILD, "--hibf", "-i", inp.tsv, "--remove", listed, "-o", new], capture_output=True, text=True)
    assert p.returncode == 1 and "--remove needs --update" in p.stderr and p.stdout == "" and not os.path.exists(new)
    assert open(old, "rb").read() == before
