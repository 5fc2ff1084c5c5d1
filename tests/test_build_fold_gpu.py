"""`ganon-build --hibf --update --fold` on the device: the OR of groups of columns of an IBF into one column each of another one
(gn_filter_fold_ibf) against numpy over the downloaded rows, and its refusals; and the command: indexes with a wide root folded to a
bound, checked column by column against the old file (every kept, every moved and every merged column), by `--verify-index` over all
inputs, and by classification against the index as it was."""
import math
import os
import subprocess

import numpy as np
import pytest

import ganon_fixtures as gf
from test_build_fold_cpu import member_cases
from test_build_remove_gpu import ROWS, SRC_BINS
from test_build_update_gpu import hip, one_ibf  # noqa: F401  (hip: the module fixture)

pytestmark = pytest.mark.gpu

U64 = np.uint64


def group_hits(a, n_groups, members):
    """numpy: [rows, n_groups] of 0 / 1, the OR of the members' columns of the rows `a` per group"""
    bits = np.unpackbits(np.ascontiguousarray(a).view(np.uint8), axis=1, bitorder="little")
    hits = np.zeros((a.shape[0], n_groups), dtype=np.uint8)
    for first, n, g in members:
        hits[:, g] |= bits[:, first] if n == 1 else bits[:, first:first + n].any(axis=1).astype(np.uint8)
    return hits


def placed(before, hits, dst_first):
    out = np.unpackbits(np.ascontiguousarray(before).view(np.uint8), axis=1, bitorder="little").copy()
    out[:, dst_first:dst_first + hits.shape[1]] |= hits
    return np.packbits(out, axis=1, bitorder="little").view(U64).reshape(before.shape)


def check_fold(hip, src, hits, B, rows, G, members, dst_first, bins_dst, what):
    """the fold of `src` into a destination of bins_dst bins that held random bits: the call is an OR"""
    W_dst = (bins_dst + 63) >> 6
    dst = one_ibf(hip, bins_dst, rows)
    dst.fill_random(bins_dst + 3 * rows + dst_first, 3)
    before = dst.download_rows(0, rows, W_dst)
    dst.fold_ibf(0, dst_first, G, src, 0, members)
    got, exp = dst.download_rows(0, rows, W_dst), placed(before, hits, dst_first)
    assert np.array_equal(got, exp), f"{what}: {B} bins, {G} groups at bin {dst_first} of {bins_dst}, {rows} rows: first difference in row {int(np.argmax((got != exp).any(axis=1)))}"
    dst.free()


def fold_cases(hip, B, rows_list, seed_density=3):
    W = (B + 63) >> 6
    for rows in rows_list:
        src = one_ibf(hip, B, rows)
        src.fill_random(B * 7 + rows, seed_density)
        a = src.download_rows(0, rows, W)
        assert a.any() or rows * B < 640  # (a handful of random bits may all be clear)
        for name, (G, members) in member_cases(B).items():
            hits = group_hits(a, G, members)
            for dst_first, extra in ((0, 70), (63, 0), (64, 1)):  # the groups' bits straddle destination words; a destination that ends with them
                check_fold(hip, src, hits, B, rows, G, members, dst_first, dst_first + G + extra, name)
        src.free()


@pytest.mark.parametrize("B", SRC_BINS + (64 * 70,))
def test_fold_ibf(hip, B):
    fold_cases(hip, B, ROWS)


def test_fold_ibf_rows_of_more_than_256_words(hip):
    """strides above 256 words: one row a step, the row in chunks by the same block"""
    for B in (64 * 300 - 9, 64 * 560 - 5):  # (an IBF on the device has at most 36864 bins, and every bin is a group in one of the cases)
        fold_cases(hip, B, (1, 301))


def test_fold_ibf_padding_bins_do_not_travel(hip):
    """a source whose padding bins alone are set (rows written as they are): no group hits"""
    for B in (1, 65, 200):
        W, rows = (B + 63) >> 6, 300
        src = one_ibf(hip, B, rows)
        a = np.zeros((rows, W), dtype=U64)
        a[:, -1] = ~U64(0) << U64(B & 63)
        src.write_rows(0, a)
        for name, (G, members) in member_cases(B).items():
            dst = one_ibf(hip, G + 70, rows)
            dst.fold_ibf(0, 3, G, src, 0, members)
            assert not dst.download_rows(0, rows, (G + 70 + 63) >> 6).any(), (B, name)
            dst.free()
        src.write_rows(0, np.full((rows, W), ~U64(0), dtype=U64))  # every bit: every group hits in every row, and nothing else is set
        G, members = member_cases(B)["every bin a group of its own"]
        dst = one_ibf(hip, G + 70, rows)
        dst.fold_ibf(0, 3, G, src, 0, members)
        assert np.array_equal(dst.bin_popcounts(G + 70), np.array([0] * 3 + [rows] * G + [0] * 67, dtype=U64))
        dst.free()
        src.free()


def test_fold_ibf_refusals(hip):
    from ganon_amd import hip as H
    a, wide, rows, hashes = one_ibf(hip, 65, 100), one_ibf(hip, 200, 100), one_ibf(hip, 200, 101), one_ibf(hip, 200, 100, h=2)
    flat = hip.HipFilter.ibf(None, 200, 100, 3)
    a.fill_random(1, 1)
    wide.fill_random(2, 1)
    before = wide.download_rows(0, 100, 4)
    one = [(0, 65, 0)]
    L = H.load_library()
    table = np.array([[0, 65, 0, 0]], dtype=np.uint32)
    for call, word in ((lambda: flat.fold_ibf(0, 0, 1, a, 0, one), "HIBF"), (lambda: wide.fold_ibf(0, 0, 1, flat, 0, one), "HIBF"),
                       (lambda: rows.fold_ibf(0, 0, 1, a, 0, one), "rows"), (lambda: hashes.fold_ibf(0, 0, 1, a, 0, one), "hash functions"),
                       (lambda: wide.fold_ibf(1, 0, 1, a, 0, one), "ibf"), (lambda: wide.fold_ibf(0, 0, 1, a, 1, one), "ibf"),
                       (lambda: wide.fold_ibf(0, 0, 1, wide, 0, one), "onto itself"),
                       (lambda: wide.fold_ibf(0, 0, 1, a, 0, [(0, 0, 0)]), "0 bins"),
                       (lambda: wide.fold_ibf(0, 0, 1, a, 0, [(1, 65, 0)]), "beyond the source"),
                       (lambda: wide.fold_ibf(0, 0, 1, a, 0, [(0, 10, 0), (9, 10, 0)]), "overlap"),
                       (lambda: wide.fold_ibf(0, 0, 1, a, 0, [(20, 10, 0), (0, 10, 0)]), "ascend"),
                       (lambda: wide.fold_ibf(0, 0, 1, a, 0, [(0, 10, 1)]), "at or beyond the number of groups"),
                       (lambda: wide.fold_ibf(0, 0, 3, a, 0, [(0, 10, 0), (20, 10, 2)]), "a group without a member"),
                       (lambda: wide.fold_ibf(0, 199, 2, a, 0, [(0, 10, 0), (20, 10, 1)]), "beyond the destination"),
                       (lambda: H._check(L.gn_filter_fold_ibf(None, 0, 0, 1, a._h, 0, H._p(table), 1)), "null"),
                       (lambda: H._check(L.gn_filter_fold_ibf(wide._h, 0, 0, 1, None, 0, H._p(table), 1)), "null"),
                       (lambda: H._check(L.gn_filter_fold_ibf(wide._h, 0, 0, 1, a._h, 0, None, 1)), "null")):
        with pytest.raises(H.GanonHipError) as e:
            call()
        assert e.value.code == -22 and word in str(e.value) and "gn_filter_fold_ibf" in str(e.value), str(e.value)
        assert np.array_equal(wide.download_rows(0, 100, 4), before), "a refused fold writes nothing"
    wide.fold_ibf(0, 0, 0, a, 0, [])  # no group: nothing to do
    assert np.array_equal(wide.download_rows(0, 100, 4), before)
    wide.fold_ibf(0, 198, 2, a, 0, [(0, 10, 0), (20, 10, 1)])  # the destination's last two bins
    assert not np.array_equal(wide.download_rows(0, 100, 4), before)
    for f in (a, wide, rows, hashes, flat):
        f.free()


# ------------------------------------------------------------------------------------------------------------ the command
import cli_util as cu  # noqa: E402
import hibf_checks as hc  # noqa: E402
from test_build_cpu import BIN_BUILD  # noqa: E402
from test_build_extend_gpu import MEMBERS, families, inputs, restated, union  # noqa: E402,F401  (families: a fixture)
from test_build_fold_cpu import plan as fold_plan  # noqa: E402  (the rule, restated)
from test_build_hibf_gpu import build, cut_reads, genomes, short200  # noqa: E402,F401  (genomes, short200: fixtures)
from test_build_remove_gpu import columns, names_below, runs_of, tables  # noqa: E402
from test_build_update_gpu import all_ok, classify_finds_everything, column_sums, part  # noqa: E402
from test_build_verify_gpu import rows_of  # noqa: E402


def fold(old, N, out, tsv=None, extra=(), expect=0):
    """-> dict(index, result, folded, targets, merged, lines, stderr) of the report, or the process when the command is to fail"""
    args = [BIN_BUILD, "--hibf", "--update", old, "--fold", str(N), "-o", out, "-t", "2", "--verbose"] + (["-i", tsv] if tsv else []) + list(extra)
    p = subprocess.run(args, capture_output=True, text=True, timeout=300)
    assert p.returncode == expect, (p.returncode, p.stdout[-2000:], p.stderr[-2000:])
    if expect:
        return p
    lines = p.stdout.splitlines()
    assert lines[0].startswith("index\t") and lines[-1].startswith("result\tok\t") and f"--fold              {N}" in p.stderr
    assert " - seconds: hash " in p.stderr and " copy " in p.stderr and " fold " in p.stderr, "the laps, with the fold's"
    rep = dict(index=lines[0], result=lines[-1], folded=[], targets={}, merged=[], ibfs={}, lines=lines, stderr=p.stderr)
    for ln in lines[1:-1]:
        f = ln.split("\t")
        if f[0] == "folded":
            rep["folded"].append(dict(parent=int(f[1]), bin=int(f[2]), ibf=int(f[3]), runs=int(f[4]), bins=int(f[5]), predicted=float(f[6]), found=int(f[7]),
                                      warn=len(f) > 8 and f[8] == "WARN fill"))
        elif f[0] == "target":
            rep["targets"][f[1]] = dict(user_bin=int(f[2]), n=int(f[3]), leaf=int(f[4]), first=int(f[5]), bins=int(f[6]), depth=int(f[7]),
                                        path=[tuple(int(x) for x in e.split(":")) for e in f[8].split(" ")])
        elif f[0] == "merged":
            rep["merged"].append((int(f[1]), int(f[2]), int(f[3]), float(f[4]), int(f[5])))
        elif f[0] == "ibf":
            rep["ibfs"][int(f[1])] = (int(f[2]), int(f[3]), int(f[4]))
    return rep


def file_fills(path):
    """-> (meta, payloads, bins, rows, nx, bu, fills): the tables of a file and the set bits of every bin, as floats"""
    from ganon_amd import ibf_file
    m = ibf_file.read_hibf_meta(path)
    bins, rows, nx, bu = tables(m)
    mats = [m.payload(path, i) for i in range(len(bins))]
    return m, mats, bins, rows, nx, bu, [[float(x) for x in column_sums(mats[i], bins[i])] for i in range(len(bins))]


def choose_bound(path, lowest=2):
    """the least N the restated rule reaches on the file as it is with at least two groups, one of them of three runs or more"""
    m, _, bins, rows, nx, bu, fills = file_fills(path)
    for N in range(lowest, max(bins)):
        exp = fold_plan(bins, rows, nx, bu, m.ibfs[0][2], m.fpr, fills, N)
        if not isinstance(exp, tuple) and len(exp["groups"]) >= 2 and max(g[3] for g in exp["groups"]) >= 3:
            return N, exp
    raise AssertionError(f"no bound folds {path}: IBFs of {bins} bins")


def check_fold_file(old, new, before, rep, N, new_sets=None, gone=()):
    """the file written against the file given, whatever the plan was: strings verbatim, every column of an old user bin as it was, every
    old merged bin as it was, every merged bin the fold made the OR of the columns below it -- and the new targets' oracle hashes ORed
    along the paths the report printed, in every IBF on them"""
    from ganon_amd import ibf_file
    assert open(old, "rb").read() == before, "the index given is left as it is"
    a, b = ibf_file.read_hibf_meta(old), ibf_file.read_hibf_meta(new)
    bins_a, rows_a, nx_a, bu_a = tables(a)
    bins_b, rows_b, nx_b, bu_b = tables(b)
    h = a.ibfs[0][2]
    new_sets = new_sets or {}
    kept = [t for t in a.names if t not in gone]
    assert b.names == kept + list(new_sets) and (b.kmer_size, b.window_size, b.fpr) == (a.kmer_size, a.window_size, a.fpr)
    keep_u = [u for u, t in enumerate(a.names) if t not in gone]
    assert b.bin_path[:len(kept)] == [a.bin_path[u] for u in keep_u] and b.user_bin_filenames[:len(kept)] == [a.user_bin_filenames[u] for u in keep_u], "the file's strings, verbatim"
    hc.check_tree(bins_b, b.next_ibf_id, b.bin_to_user, len(b.names), max(bins_b), max_levels=64)
    assert max(bins_b) <= N, "every IBF of the file written is within the bound"
    mats_a = [a.payload(old, i) for i in range(len(bins_a))]
    mats_b = [b.payload(new, i) for i in range(len(bins_b))]
    run_a, _, _ = runs_of(a)
    run_b, parent_b, _ = runs_of(b)
    exp = [np.zeros((rows_b[i], ((bins_b[i] + 63) >> 6) * 64), dtype=np.uint8) for i in range(len(bins_b))]  # one byte a bit

    def put(i, first, cols):
        exp[i][:, first:first + cols.shape[1]] |= cols
    # the old user bins: their runs as they were, wherever they are now
    for u_new, name in enumerate(kept):
        (ia, fa, na), (ib, fb, nb) = run_a[a.names.index(name)], run_b[u_new]
        assert na == nb and rows_b[ib] == rows_a[ia], name
        put(ib, fb, columns(mats_a[ia], fa, na))
    # the merged bins: an old one is found by its level and the old names below it; every other one the fold made
    old_names = set(kept)
    was = {(lv, frozenset(s & old_names)): at for at, (lv, s) in names_below(a).items() if s & old_names}
    made = []
    for (ib, bb), (lv, s) in sorted(names_below(b).items()):
        key = (lv, frozenset(s & old_names))
        if key in was:
            ia, ba = was.pop(key)
            put(ib, bb, columns(mats_a[ia], ba, 1))
        else:
            made.append((ib, bb, nx_b[ib][bb]))
    # the new targets along their printed paths
    for t, hs in new_sets.items():
        r = rep["targets"][t]
        assert r["n"] == len(hs) and r["path"][-1] == (r["leaf"], r["first"]) and r["depth"] == len(r["path"]) and r["path"][0][0] == 0 and r["user_bin"] == b.names.index(t)
        for d, (i, first) in enumerate(r["path"]):
            leaf = d == len(r["path"]) - 1
            per = -(-len(hs) // r["bins"]) if leaf else 1
            at = (first + np.arange(len(hs)) // per) if leaf else np.full(len(hs), first)
            assert not leaf or (bu_b[i][first] == r["user_bin"] and int(at.max()) < first + r["bins"])
            assert leaf or nx_b[i][first] == r["path"][d + 1][0]
            for fn in range(h):
                exp[i][rows_of(hs, fn, rows_b[i]).astype(np.int64), at] = 1
    # a merged bin the fold made: the OR of every column of its child (user bins only: one level a command)
    for ib, bb, child in made:
        assert all(u >= 0 for u in bu_b[child]) and rows_b[child] == rows_b[ib] and 2 <= bins_b[child] <= N, (ib, bb, child)
        put(ib, bb, exp[child][:, :bins_b[child]].any(axis=1).astype(np.uint8).reshape(-1, 1))
    for i in range(len(bins_b)):
        want = np.packbits(exp[i], axis=1, bitorder="little").view(U64).reshape(mats_b[i].shape)
        assert np.array_equal(mats_b[i], want), f"IBF {i}: first difference in row {int(np.argmax((mats_b[i] != want).any(axis=1)))}"
    # the report
    pop_b = [column_sums(mats_b[i], bins_b[i]) for i in range(len(bins_b))]
    assert sorted((f["parent"], f["bin"], f["ibf"]) for f in rep["folded"]) == sorted(made), "a `folded` line per merged bin the fold made"
    for f in rep["folded"]:
        child = f["ibf"]
        assert f["bins"] == bins_b[child] and f["runs"] == len(set(bu_b[child])) and f["found"] == int(pop_b[f["parent"]][f["bin"]]), f
        assert f["found"] <= f["predicted"] + 3 * math.sqrt(rows_b[child]), f
        assert f["warn"] == (f["found"] > b.fpr ** (1.0 / h) * rows_b[child])
    if rep["folded"]:
        print(f"{len(rep['folded'])} merged bins made: found - predicted bits from {min(f['found'] - f['predicted'] for f in rep['folded']):.1f} to "
              f"{max(f['found'] - f['predicted'] for f in rep['folded']):.1f}, 3 sqrt(rows) = {3 * math.sqrt(min(rows_b)):.1f}")
    assert f"ibfs={len(bins_a)}->{len(bins_b)} " in rep["index"] and f"user_bins={len(a.names)}->{len(b.names)} " in rep["index"]
    assert f"{len(made)} IBF(s) created under {len({m[0] for m in made})} folded, " in rep["result"]
    return a, b, made


def classify_all(index, fq, prefix):
    cu.run(cu.BIN_HIP, ["--ibf", index, "--hibf", "--single-reads", fq, "-o", prefix, "--output-all", "--skip-lca", "--rel-cutoff", "0.25", "--rel-filter", "1", "--quiet"])
    return [tuple(ln.split("\t")) for ln in open(prefix + ".all").read().splitlines()]


_index = {}


def index_of(request, tmp_path_factory, which, tmax, s, max_fp, names=None):
    key = (which, tmax, s, max_fp, None if names is None else len(names))
    if key not in _index:
        inp = request.getfixturevalue(which)
        d = tmp_path_factory.mktemp("fold_index")
        if names is not None:
            inp = part(inp, names, str(d / "part.tsv"))
        out = str(d / "all.hibf")
        build(inp, out, tmax, s, max_fp)
        _index[key] = (inp, out, open(out, "rb").read())
    return _index[key]


@pytest.mark.parametrize("which,tmax,s,max_fp", [("short200", 256, 3, 0.001), ("short200", 256, 0, 0.05)])
def test_fold(hip, request, tmp_path, tmp_path_factory, which, tmax, s, max_fp):
    """(a) fold only: no input file"""
    inp, old, before = index_of(request, tmp_path_factory, which, tmax, s, max_fp)
    N, exp = choose_bound(old)
    new = str(tmp_path / "new.hibf")
    rep = fold(old, N, new)
    a, b, made = check_fold_file(old, new, before, rep, N)
    bins_b, rows_b, nx_b, bu_b = tables(b)
    assert (bins_b, rows_b, nx_b, bu_b) == (exp["bins"], exp["rows"], exp["nx"], exp["bu"]), "the tables of the restated rule"
    assert [(f["parent"], f["bin"], f["ibf"], f["runs"], f["bins"]) for f in rep["folded"]] == [g[:5] for g in exp["groups"]]
    assert all(abs(f["predicted"] - g[5]) <= 0.051 for f, g in zip(rep["folded"], exp["groups"]))
    split = [n for g in exp["groups"] for _, n in g[6] if n > 1]
    print(f"{which} tmax {tmax} s {s} fpr {max_fp}: root of {tables(a)[0][0]} bins folded to {N}: {len(exp['groups'])} groups of {[g[3] for g in exp['groups']]} runs, "
          f"{len(split)} folded runs of several bins")
    assert len(made) >= 2 and max(g[3] for g in exp["groups"]) >= 3 and split, "groups, one of three runs or more, and a folded run of several bins"
    assert len(all_ok(new, inp, 0)) == len(inp.order)
    assert classify_finds_everything(new, inp, 0, tmp_path, tmax) == set(b.names), "reads from every target, found in full, on both backends"
    # the same reads against the index as it was: nothing is gained; where no folded run is split, nothing is lost either
    fq = str(tmp_path / "reads.fq")
    was, now = classify_all(old, fq, str(tmp_path / "was")), classify_all(new, fq, str(tmp_path / "now"))
    assert set(now) <= set(was) and len(now) == len(set(now)), "a subset, with equal counts"
    assert split or now == was
    print(f"  .all: {len(was)} lines before, {len(now)} after")


def restated_update_and_fold(old, counts, lowest=2):
    """plan_update and then plan_fold, restated, on a file and the hash counts of the new targets: the least bound that is reached with at
    least two groups, one of them of three runs or more -> (N, the fold's plan)"""
    from test_build_update_cpu import plan as update_plan, predict
    m, _, bins, rows, nx, bu, fills = file_fills(old)
    h = m.ibfs[0][2]
    pop = [[int(x) for x in f] for f in fills]
    u_bins, u_nx, u_bu, paths, touched = update_plan(bins, rows, nx, bu, len(m.names), h, m.fpr, pop, counts)
    for i in range(len(bins)):
        fills[i] += [0.0] * (u_bins[i] - bins[i])
    for i, b, _, predicted in touched:
        fills[i][b] = predicted
    for path in paths:
        i, first, n, per = path[0]
        fills[i][first:first + n] = [predict(0.0, per, rows[i], h)] * n
    for N in range(lowest, max(u_bins)):
        exp = fold_plan(u_bins, rows, u_nx, u_bu, h, m.fpr, fills, N)
        if not isinstance(exp, tuple) and len(exp["groups"]) >= 2 and max(g[3] for g in exp["groups"]) >= 3:
            return N, exp
    raise AssertionError(f"no bound folds the update of {old}: IBFs of {u_bins} bins")


@pytest.mark.parametrize("which,tmax,s,max_fp", [("short200", 256, 3, 0.001), ("short200", 256, 0, 0.05)])
def test_update_with_fold(hip, request, tmp_path, tmp_path_factory, which, tmax, s, max_fp):
    """(b) the first half of a fixture is built, the rest added with --fold: new user bins land in children"""
    full = request.getfixturevalue(which)
    half = len(full.order) // 2
    first, old, before = index_of(request, tmp_path_factory, which, tmax, s, max_fp, names=full.order[:half])
    rest = part(full, full.order[half:], str(tmp_path / "rest.tsv"))
    names, sets = rest.sets(0)
    N, exp = restated_update_and_fold(old, [len(x) for x in sets])
    new = str(tmp_path / "new.hibf")
    rep = fold(old, N, new, tsv=rest.tsv)
    a, b, made = check_fold_file(old, new, before, rep, N, new_sets=dict(zip(names, sets)))
    bins_b, rows_b, nx_b, bu_b = tables(b)
    assert (bins_b, rows_b, nx_b, bu_b) == (exp["bins"], exp["rows"], exp["nx"], exp["bu"]), "the tables of the restated rules"
    in_children = [t for t in names if rep["targets"][t]["leaf"] >= len(a.ibfs)]
    print(f"{which}: {len(names)} targets added, bound {N}: {len(made)} IBFs made, {len(in_children)} new user bins in them, levels {rep['index'].split('levels=')[1].split(' ')[0]}")
    assert in_children and len(made) >= 2 and max(g[3] for g in exp["groups"]) >= 3
    assert all(rep["targets"][t]["depth"] >= 2 and rep["targets"][t]["path"][-2][0] < len(a.ibfs) for t in in_children)
    assert len(all_ok(new, full, 0)) == len(full.order)


def test_remove_extend_and_fold_in_one_command(hip, families, tmp_path):
    """(c) six families of four members each behind one root; one command takes a family out, gives the others their fifth member where
    the restated extension plan accepts it, adds two families, and folds the root"""
    from ganon_amd import ibf_file
    old_fams = [f"F{f}" for f in range(6)]
    base = inputs(families, {f: [0, 1, 2, 3] for f in old_fams}, str(tmp_path / "base.tsv"))
    old, new = str(tmp_path / "old.hibf"), str(tmp_path / "new.hibf")
    build(base, old, 8, 3, 0.05, extra=("--layout", "rule"))
    before = open(old, "rb").read()
    accepted = restated(old, {f: union(families, f, [4]) for f in old_fams})[0]
    assert len(accepted) >= 3, "the fixture is meant to leave room for at least three extensions"
    gone = ([f for f in old_fams if f not in accepted] or accepted[-1:])[0]
    extended = [f for f in accepted if f != gone]
    members = {f: [4] for f in extended}
    members.update({"F6": list(range(MEMBERS)), "F7": list(range(MEMBERS))})
    listed = str(tmp_path / "gone.txt")
    open(listed, "w").write(gone + "\n")
    more = inputs(families, members, str(tmp_path / "more.tsv"))
    rep = None
    for N in range(2, 16):  # the least bound the command reaches (the fills after an extension are the extension plan's: not restated here)
        p = subprocess.run([BIN_BUILD, "--hibf", "--update", old, "--fold", str(N), "-o", new, "-t", "2", "-i", more.tsv, "--extend", "--remove", listed],
                           capture_output=True, text=True, timeout=300)
        if p.returncode == 0:
            rep = fold(old, N, new, tsv=more.tsv, extra=["--extend", "--remove", listed])
            break
        assert p.returncode == 1 and "rebuild or give a larger --fold" in p.stderr and not os.path.exists(new), p.stderr
    assert rep is not None and rep["folded"], "a bound below the root's bins that the rule reaches"
    b = ibf_file.read_hibf_meta(new)
    kept = [f for f in old_fams if f != gone]
    assert b.names == kept + ["F6", "F7"] and open(old, "rb").read() == before
    bins_b, _, _, _ = tables(b)
    hc.check_tree(bins_b, b.next_ibf_id, b.bin_to_user, len(b.names), max(bins_b), max_levels=64)
    assert max(bins_b) <= N and "1 user bin(s) removed" in rep["result"] and f"{len(extended)} user bin(s) extended, 2 user bin(s) added" in rep["result"]
    pop = [column_sums(b.payload(new, i), bins_b[i]) for i in range(len(bins_b))]
    assert all(f["found"] == int(pop[f["parent"]][f["bin"]]) for f in rep["folded"])
    have = {f: [0, 1, 2, 3] + ([4] if f in extended else []) for f in kept}
    have.update({"F6": list(range(MEMBERS)), "F7": list(range(MEMBERS))})
    assert len(all_ok(new, inputs(families, have, str(tmp_path / "all.tsv"), order=b.names), 0)) == len(b.names)


def test_update_of_a_folded_index_and_fold_of_a_folded_index(hip, request, short200, tmp_path, tmp_path_factory):
    """(d) a folded index is an ordinary one: it takes an update, and a second fold to a lower bound"""
    from test_build_update_gpu import check_update, update
    half = len(short200.order) // 2
    first, old, before = index_of(request, tmp_path_factory, "short200", 256, 3, 0.001, names=short200.order[:half])
    N, _ = choose_bound(old)
    files = [str(tmp_path / f"db{i}.hibf") for i in range(3)]
    N1 = N + 60  # (a bound that leaves most of the root's runs where they are: a merged bin is not folded again)
    check_fold_file(old, files[0], before, fold(old, N1, files[0]), N1)
    rest = part(short200, short200.order[half:], str(tmp_path / "rest.tsv"))
    check_update(files[0], files[1], rest, 0, update(files[0], rest.tsv, files[1]))
    assert len(all_ok(files[1], short200, 0)) == len(short200.order)
    again = open(files[0], "rb").read()
    N2, _ = choose_bound(files[0])
    assert N2 < N1
    a, b, made = check_fold_file(files[0], files[2], again, fold(files[0], N2, files[2]), N2)
    assert made and len(b.ibfs) > len(a.ibfs)
    assert len(all_ok(files[2], first, 0)) == half


def test_fold_refusals(hip, request, genomes, tmp_path, tmp_path_factory):
    """(e) each exits 1 with nothing written"""
    inp, old, before = index_of(request, tmp_path_factory, "genomes", 64, 3, 0.001)
    new = str(tmp_path / "new.hibf")
    for args, word in ((["--hibf", "-i", inp.tsv, "--fold", "8", "-o", new], "--fold needs --update"),
                       (["--hibf", "--update", old, "--fold", "1", "-o", new], "--fold has to be >= 2"),
                       (["--hibf", "--verify-index", old, "-i", inp.tsv, "--fold", "8"], "--fold cannot be used with --verify-index"),
                       (["--hibf", "--update", old, "--tmax", "8", "-o", new], "--update cannot be used with --tmax")):
        p = subprocess.run([BIN_BUILD] + args, capture_output=True, text=True, timeout=300)
        assert p.returncode == 1 and word in p.stderr and p.stdout == "" and not os.path.exists(new), (args, p.stderr)
    p = fold(old, 2, new, expect=1)  # a root of 25 runs whose largest fill their bins to the bound: two bins are out of reach
    assert "IBF 0 has" in p.stderr and ", not 2" in p.stderr and "rebuild or give a larger --fold" in p.stderr and "nothing written" in p.stderr
    assert p.stdout == "" and not os.path.exists(new) and open(old, "rb").read() == before
    assert "--fold arg" in subprocess.run([BIN_BUILD, "--help"], capture_output=True, text=True).stderr


def test_without_fold_nothing_changes(hip, request, genomes, tmp_path, tmp_path_factory):
    """the report and the laps of an update without --fold name no fold"""
    from test_build_update_gpu import update
    half = len(genomes.order) // 2
    first, old, _ = index_of(request, tmp_path_factory, "genomes", 64, 3, 0.001, names=genomes.order[:half])
    rest = part(genomes, genomes.order[half:], str(tmp_path / "rest.tsv"))
    p = subprocess.run([BIN_BUILD, "--hibf", "--update", old, "-i", rest.tsv, "-o", str(tmp_path / "new.hibf"), "-t", "2", "--verbose"], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "folded" not in p.stdout and "created" not in p.stdout and " fold " not in p.stderr and "--fold" not in p.stderr


@pytest.mark.parametrize("s,max_fp", [(3, 0.001), (0, 0.05)])
def test_fold_of_genomes_is_refused_as_restated(hip, request, tmp_path, tmp_path_factory, s, max_fp):
    """The 25 genomes hold 3397 .. 6059 distinct minimisers each: every bin of their index is filled to within a factor of two of the
    bin that sized the rows, so the OR of any two runs is over the merged-bin bound, and a split run is over it alone.  The rule folds
    nothing there at any bound, the restatement and the command agree on it for every bound below the root's bins, and at the root's own
    number of bins the command writes the index as it was."""
    inp, old, before = index_of(request, tmp_path_factory, "genomes", 64, s, max_fp)
    m, mats, bins, rows, nx, bu, fills = file_fills(old)
    new = str(tmp_path / "new.hibf")
    for N in (2, bins[0] // 2, bins[0] - 1):
        exp = fold_plan(bins, rows, nx, bu, m.ibfs[0][2], m.fpr, fills, N)
        assert exp == ("unreachable", 0, bins[0]), exp
        p = fold(old, N, new, expect=1)
        assert f"IBF 0 has {bins[0]} bins" in p.stderr and f"reaches {bins[0]} bins, not {N}" in p.stderr and p.stdout == "" and not os.path.exists(new)
    rep = fold(old, bins[0], new)
    a, b, made = check_fold_file(old, new, before, rep, bins[0])
    assert not made and tables(b) == tables(a) and all(np.array_equal(b.payload(new, i), mats[i]) for i in range(len(bins)))
    assert len(all_ok(new, inp, 0)) == len(inp.order)
