"""`ganon-build --hibf` in parts on the GPU: the storage-only HIBF and the windowed path insert against gn_filter_emplace_path and the
oracle (every IBF whole in one filter, every IBF alone, the root and a leaf in pieces), their refusals, and the binary under budgets that
cut the tree by IBF and by rows: the same bytes as the one-pass build, the parts of the restated plan, a budget that is kept."""
import ctypes as C
import filecmp
import os
import re
import subprocess

import numpy as np
import pytest

import cli_util as cu
import ganon_fixtures as gf
import oracle
from test_build_cpu import BIN_BUILD
from test_build_hibf_gpu import K, W, build, check_file, cut_reads, genomes, hip, paths_of, short200  # noqa: F401  (fixtures among them)
from test_build_hibf_parts_cpu import parts_of, plan_rule

pytestmark = pytest.mark.gpu

U64 = np.uint64
_TREES = {}


def tree(hip, n_ub, tmax, depth, h):  # noqa: F811
    """a random tree, its sets and paths, and every IBF after gn_filter_emplace_path: made once per shape, never changed"""
    key = (n_ub, tmax, depth, h)
    if key not in _TREES:
        rng = np.random.default_rng(n_ub * 7 + tmax + h)
        hb = gf.random_hibf(n_ub, tmax, depth, seed=n_ub + tmax, density=0.0, hash_funs=h, rows=(3000, 9000))
        sets = [np.unique(rng.integers(0, 1 << 38, size=int(rng.integers(1, 3000)), dtype=U64)) for _ in range(n_ub)]
        sets[1] = np.zeros(0, U64)                                             # an empty set between the others
        sets[2] = np.unique(rng.integers(0, 1 << 38, size=20000, dtype=U64))   # a set of many wave items, longer than a chunk of 700
        sets[3] = np.unique(rng.integers(0, 1 << 38, size=600, dtype=U64))[:512]  # exactly one full item
        assert len(sets[3]) == 512
        paths, where, parent = paths_of(hb, [len(x) for x in sets])
        shapes = [(f.bins, f.bin_size, h) for f in hb.ibfs]
        one = hip.HipFilter.hibf([(None,) + s for s in shapes], hb.next_ibf_id, hb.bin_to_user, n_ub)
        one.emplace_path(sets, paths)
        ref = [one.download_rows(0, r, (b + 63) // 64, ibf_idx=i) for i, (b, r, _) in enumerate(shapes)]
        one.free()
        assert all(r.any() for r in ref[:1])
        for r in ref:
            r.setflags(write=False)
        _TREES[key] = (hb, sets, paths, where, parent, shapes, ref)
    return _TREES[key]


def compact(paths, held):
    """the sets with an entry in one of the IBFs `held` (tree numbers, in the filter's order) and their paths cut down to those"""
    local = {t: j for j, t in enumerate(held)}
    out = np.zeros_like(paths)
    keep = []
    for u in range(paths.shape[0]):
        k = 0
        for d in range(paths.shape[1]):
            if paths[u, d]["n_bins"] == 0:
                break
            if int(paths[u, d]["ibf"]) in local:
                out[u, k] = paths[u, d]
                out[u, k]["ibf"] = local[int(paths[u, d]["ibf"])]
                k += 1
        if k:
            keep.append(u)
    return keep, out[keep]


def fill_pieces(hip, shapes, sets, paths, pieces, chunk=0):  # noqa: F811
    """a storage filter of `pieces` (tree ibf, row_begin, n_rows), filled through the windowed insert as the builder fills a part"""
    flt = hip.HipFilter.hibf_storage([(shapes[t][0], n, shapes[t][2]) for t, _, n in pieces])
    keep, cut = compact(paths, [t for t, _, _ in pieces])
    flt.emplace_path_window([sets[u] for u in keep], cut, [shapes[t][1] for t, _, _ in pieces], [a for _, a, _ in pieces], chunk)
    got = [flt.download_rows(0, n, (shapes[t][0] + 63) // 64, ibf_idx=j) for j, (t, _, n) in enumerate(pieces)]
    info = flt.info()
    flt.free()
    return got, info


SHAPES = [(40, 8, 3), (10, 4, 4)]


# ------------------------------------------------------------------------------------------------------------ the ABI
@pytest.mark.parametrize("h", [1, 3, 5])
@pytest.mark.parametrize("n_ub,tmax,depth", SHAPES)
def test_every_ibf_whole_in_one_storage_filter(hip, n_ub, tmax, depth, h):  # noqa: F811
    hb, sets, paths, where, parent, shapes, ref = tree(hip, n_ub, tmax, depth, h)
    got, info = fill_pieces(hip, shapes, sets, paths, [(t, 0, r) for t, (_, r, _) in enumerate(shapes)])
    assert info["is_hibf"] and info["n_ibf"] == len(shapes)
    L = hip.load_library()
    assert info["device_bytes"] == sum(r * L.gn_hibf_row_stride_words((b + 63) // 64) * 8 for b, r, _ in shapes), "rows padded as an uploaded HIBF's"
    for t in range(len(shapes)):
        assert np.array_equal(got[t], ref[t]), f"IBF {t}"


@pytest.mark.parametrize("h", [1, 3, 5])
@pytest.mark.parametrize("n_ub,tmax,depth", SHAPES)
def test_every_ibf_alone_with_compacted_paths(hip, n_ub, tmax, depth, h):  # noqa: F811
    hb, sets, paths, where, parent, shapes, ref = tree(hip, n_ub, tmax, depth, h)
    for t, (_, r, _) in enumerate(shapes):
        got, _ = fill_pieces(hip, shapes, sets, paths, [(t, 0, r)])
        assert np.array_equal(got[0], ref[t]), f"IBF {t}"


@pytest.mark.parametrize("chunk", [0, 700])
@pytest.mark.parametrize("h", [1, 3, 5])
@pytest.mark.parametrize("n_ub,tmax,depth", SHAPES)
def test_the_root_and_a_leaf_in_pieces(hip, n_ub, tmax, depth, h, chunk):  # noqa: F811
    hb, sets, paths, where, parent, shapes, ref = tree(hip, n_ub, tmax, depth, h)
    rows0 = shapes[0][1]
    cuts = [0, 1, 7, 512, 999, 1000, rows0 // 2, rows0 - 1, rows0]
    assert cuts == sorted(cuts)
    root = [fill_pieces(hip, shapes, sets, paths, [(0, a, b - a)], chunk)[0][0] for a, b in zip(cuts, cuts[1:])]
    assert np.array_equal(np.concatenate(root), ref[0]), "the pieces behind each other are the root"
    leaf = where[2][0]  # the IBF that holds the 20 000-hash set's run
    if leaf == 0:
        leaf = max(i for i, _, _ in where.values())
    half = shapes[leaf][1] // 2 + 1
    # the leaf's halves in filters of two pieces: beside a piece of the root, and beside another whole IBF
    other = next(t for t in range(1, len(shapes)) if t != leaf)
    (a0, a1), _ = fill_pieces(hip, shapes, sets, paths, [(0, 512, 487), (leaf, 0, half)], chunk)
    (b0, b1), _ = fill_pieces(hip, shapes, sets, paths, sorted([(other, 0, shapes[other][1]), (leaf, half, shapes[leaf][1] - half)]), chunk)
    if other > leaf:
        b0, b1 = b1, b0
    assert np.array_equal(a0, ref[0][512:999]) and np.array_equal(b0, ref[other])
    assert np.array_equal(np.concatenate([a1, b1]), ref[leaf]), "the leaf's halves"


def test_against_the_oracle(hip):  # noqa: F811
    hb, sets, paths, where, parent, shapes, ref = tree(hip, 10, 4, 4, 3)
    refs = [oracle.Ibf(b, r, h) for b, r, h in shapes]
    for u, hs in enumerate(sets):
        if len(hs) == 0:
            continue
        i, first, n = where[u]
        refs[i].emplace_many(hs, (first + np.arange(len(hs)) // ((len(hs) + n - 1) // n)).astype(np.uint32))
        at = i
        while at != 0:
            at, b = parent[at]
            refs[at].emplace_many(hs, np.full(len(hs), b, dtype=np.uint32))
    got, _ = fill_pieces(hip, shapes, sets, paths, [(t, 0, r) for t, (_, r, _) in enumerate(shapes)])
    for t in range(len(shapes)):
        assert np.array_equal(got[t], refs[t].data), f"IBF {t}"


def test_a_piece_no_row_falls_into_stays_zero(hip):  # noqa: F811
    hs = np.array([3, 1 << 20, (1 << 37) + 5], dtype=U64)
    whole = oracle.Ibf(70, 1000, 1)
    whole.emplace_many(hs, np.full(3, 69, dtype=np.uint32))
    used = np.nonzero(whole.data.any(axis=1))[0]
    assert 1 <= len(used) <= 3
    gaps = [(a + 1, b) for a, b in zip([-1] + used.tolist(), used.tolist() + [1000]) if b - a > 1]
    a, b = max(gaps, key=lambda g: g[1] - g[0])
    paths = np.zeros((1, 1), dtype=hip.hip.PATH_DTYPE)
    paths[0, 0] = (0, 69, 1, 0, 1)
    flt = hip.HipFilter.hibf_storage([(70, b - a, 1)])
    flt.emplace_path_window([hs], paths, [1000], [a])
    assert not flt.download_rows(0, b - a, 2).any()
    flt.free()
    r = int(used[0])  # and a piece of one row that a hash does fall into
    flt = hip.HipFilter.hibf_storage([(70, 1, 1)])
    flt.emplace_path_window([hs], paths, [1000], [r])
    assert np.array_equal(flt.download_rows(0, 1, 2), whole.data[r:r + 1])
    flt.free()


def test_refusals_write_nothing(hip):  # noqa: F811
    H = hip.hip
    hs = np.arange(1, 1001, dtype=U64) * U64(0x9E3779B97F4A7C15 % (1 << 38))
    hs.sort()
    flt = hip.HipFilter.hibf_storage([(70, 500, 3), (8, 300, 3)])

    def path(*entries):
        p = np.zeros((1, 2), dtype=H.PATH_DTYPE)
        for d, e in enumerate(entries):
            p[0, d] = e
        return p

    good = path((1, 2, 4, 0, 250), (0, 69, 1, 0, 1))
    cases = [("an IBF out of range", path((2, 0, 1, 0, 1)), [500, 300], [0, 0]),
             ("a bin out of range", path((1, 5, 4, 0, 250)), [500, 300], [0, 0]),
             ("a bin out of range above", path((1, 2, 4, 0, 250), (0, 70, 1, 0, 1)), [500, 300], [0, 0]),
             ("hashes that do not fit the run", path((1, 2, 4, 0, 249)), [500, 300], [0, 0]),
             ("no hashes a bin", path((1, 2, 4, 0, 0)), [500, 300], [0, 0]),
             ("row_begin + rows > total_rows", good, [500, 300], [0, 1]),
             ("rows > total_rows", good, [499, 300], [0, 0]),
             ("total_rows of 2^32", good, [1 << 32, 300], [0, 0]),
             ("total_rows of 0", good, [500, 0], [0, 0])]
    for what, p, total, begin in cases:
        with pytest.raises(hip.GanonHipError):
            flt.emplace_path_window([hs], p, total, begin)
        assert not flt.download_rows(0, 500, 2, ibf_idx=0).any() and not flt.download_rows(0, 300, 1, ibf_idx=1).any(), what
    # null arguments, through the library itself
    L = hip.load_library()
    ptrs = (C.c_void_p * 1)(hs.ctypes.data)
    sizes, total, begin = np.array([len(hs)], U64), np.array([500, 300], U64), np.array([0, 0], U64)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    full = [flt._h, ptrs, vp(sizes), 1, vp(good), 2, vp(total), vp(begin), 0]
    for k in (0, 1, 2, 4, 6, 7):
        args = list(full)
        args[k] = None
        assert L.gn_filter_emplace_path_window(*args) != 0, k
    args = list(full)
    args[5] = 0  # no depth
    assert L.gn_filter_emplace_path_window(*args) != 0
    assert not flt.download_rows(0, 500, 2, ibf_idx=0).any() and not flt.download_rows(0, 300, 1, ibf_idx=1).any()
    # a flat filter is no HIBF
    flat = hip.HipFilter.ibf_storage(70, 500, 3)
    with pytest.raises(hip.GanonHipError):
        flat.emplace_path_window([hs], path((0, 0, 1, 0, 1)), [500], [0])
    assert not flat.download_rows(0, 500, 2).any()
    flat.free()
    # and the call that is not refused writes
    flt.emplace_path_window([hs], good, [500, 300], [0, 0])
    assert flt.download_rows(0, 500, 2, ibf_idx=0).any() and flt.download_rows(0, 300, 1, ibf_idx=1).any()
    # a storage filter takes no rows at creation and no classify stream
    with pytest.raises(hip.GanonHipError):
        hip.HipStream(flt, 16, 4096)
    flt.free()
    d = H._desc(np.zeros(500 * 2, U64), 70, 500, 3)
    h = C.c_void_p()
    assert L.gn_filter_create_hibf_storage(0, 1, C.byref(d), C.byref(h)) != 0 and not h.value
    assert L.gn_filter_create_hibf_storage(0, 0, C.byref(d), C.byref(h)) != 0


# ------------------------------------------------------------------------------------------------------------ the binary
INPUTS = {"genomes": (4, 0, 0.001), "short200": (8, 0, 0.05)}  # tmax, -s, -p (genomes: three levels)
_ONE_PASS = {}


def one_pass(hip, request, tmp_path_factory, which):  # noqa: F811
    """the one-pass index of an input, its IBFs' (rows, device bytes a row) and the figure the one-pass build uploads"""
    if which not in _ONE_PASS:
        from ganon_amd import ibf_file
        inp = request.getfixturevalue(which)
        tmax, s, max_fp = INPUTS[which]
        out = str(tmp_path_factory.mktemp("hibf_parts_" + which) / "one.hibf")
        build(inp, out, tmax, s, max_fp)
        m =ibf_file.read_hibf_meta(out)
        L = hip.load_library()
        ibfs = [(rows, int(L.gn_hibf_row_stride_words((bins + 63) // 64)) * 8) for bins, rows, _, _ in m.ibfs]
        _ONE_PASS[which] = (inp, out, ibfs, 8 * sum(len(x) for x in inp.sets(0)[1]))
    return _ONE_PASS[which]


def beside(one, name):
    """a file in the one-pass index's folder: an index names its user bins' files by the folder it is written to"""
    return os.path.join(os.path.dirname(one), name)


def budget_of(ibfs, kind):
    rows, rb = max(ibfs, key=lambda x: x[0] * x[1])
    return {"whole": rows * rb, "three": -(-rows // 3) * rb, "two": (rows - 1) * rb}[kind]


def parse_verbose(stderr):
    pieces, parts, end = {}, {}, None
    for ln in stderr.splitlines():
        m = re.fullmatch(r"part (\d+) device (\d+): ibf (\d+) rows \[(\d+), (\d+)\)", ln)
        if m:
            p, d, i, a, b = map(int, m.groups())
            pieces.setdefault(p, []).append((d, i, a, b - a))
        m = re.match(r"part (\d+) entry (\d+): (\d+) device bytes, (\d+) sets taken, filled in \S+ s, written in \S+ s$", ln)
        if m:
            p, e, by, n = map(int, m.groups())
            assert p not in parts
            parts[p] = (e, by, n)
        m = re.fullmatch(r"filled in (\d+) parts?, (\d+) hash bytes uploaded(?: \(one pass: (\d+)\))?", ln)
        if m:
            assert end is None
            end = tuple(int(x) if x else None for x in m.groups())
    return pieces, parts, end


def check_parts(stderr, ibfs, budget, n_entries, one_pass_bytes):
    want = parts_of(plan_rule(ibfs, budget, n_entries), ibfs)
    pieces, parts, end = parse_verbose(stderr)
    assert sorted(pieces) == sorted(parts) == list(range(len(want))), (len(pieces), len(parts), len(want))
    for p, pc in enumerate(want):
        assert [x[1:] for x in pieces[p]] == pc, ("the part lines are those of the restated plan", p)
        e, by, n_sets = parts[p]
        assert e == p % n_entries, "parts dealt round robin"
        assert by == sum(n * ibfs[i][1] for i, _, n in pc) <= budget, (p, by, budget)
        assert n_sets >= 1
    assert end == (len(want), end[1], one_pass_bytes) and end[1] >= one_pass_bytes, end
    return want


@pytest.mark.parametrize("kind", ["whole", "three", "two"])
@pytest.mark.parametrize("which", ["genomes", "short200"])
def test_budgets(hip, request, tmp_path_factory, tmp_path, which, kind):  # noqa: F811
    inp, one, ibfs, one_pass_bytes = one_pass(hip, request, tmp_path_factory, which)
    tmax, s, max_fp = INPUTS[which]
    budget = budget_of(ibfs, kind)
    out = beside(one, f"budget_{kind}.hibf")
    p = build(inp, out, tmax, s, max_fp, extra=("--verbose", "--hibf-memory", str(budget)))
    want = check_parts(p.stderr, ibfs, budget, 1, one_pass_bytes)
    big = max(range(len(ibfs)), key=lambda i: ibfs[i][0] * ibfs[i][1])
    slabs = [pc for pc in want if pc[0][0] == big]
    if kind == "whole":
        assert len(want) > 1 and all(a == 0 and n == ibfs[i][0] for pc in want for i, a, n in pc), "every IBF whole, in several parts"
    else:
        assert len(slabs) == {"three": 3, "two": 2}[kind] and all(len(pc) == 1 for pc in slabs)
    assert filecmp.cmp(out, one, shallow=False), "byte for byte the one-pass file"
    check_file(out, inp, tmax, s, max_fp, 0)


@pytest.mark.parametrize("entries", ["0,0", "0,0,0"])
def test_parts_dealt_to_a_list(hip, request, tmp_path_factory, tmp_path, entries):  # noqa: F811
    inp, one, ibfs, one_pass_bytes = one_pass(hip, request, tmp_path_factory, "short200")
    tmax, s, max_fp = INPUTS["short200"]
    budget = budget_of(ibfs, "three")
    out = beside(one, f"list_{entries.count(',')}.hibf")
    p = build(inp, out, tmax, s, max_fp, extra=("--verbose", "--hibf-memory", str(budget), "--hibf-devices", entries))
    want = check_parts(p.stderr, ibfs, budget, entries.count(",") + 1, one_pass_bytes)
    assert len(want) > 3
    assert filecmp.cmp(out, one, shallow=False)


def test_one_part_is_the_one_pass_build(hip, request, tmp_path_factory, tmp_path):  # noqa: F811
    inp, one, ibfs, _ = one_pass(hip, request, tmp_path_factory, "short200")
    tmax, s, max_fp = INPUTS["short200"]
    args = [BIN_BUILD, "-i", inp.tsv, "-k", str(K), "-w", str(W), "-s", str(s), "-p", repr(max_fp), "--hibf", "--tmax", str(tmax), "-t", "2"]
    errs = []
    for tag, extra in (("plain", []), ("roomy", ["--hibf-memory", str(sum(r * b for r, b in ibfs)), "--hibf-devices", "0"])):
        out = beside(one, tag + ".hibf")
        p = subprocess.run(args + ["-o", out] + extra, capture_output=True, text=True, timeout=300)
        assert p.returncode == 0 and filecmp.cmp(out, one, shallow=False), p.stderr
        assert "part " not in p.stderr and "hash bytes" not in p.stderr
        errs.append(re.sub(r"[0-9][0-9.e+:-]*", "#", p.stderr))
    assert errs[0] == errs[1], "stderr without --verbose as before"
    assert "ganon-build processed" in errs[0] and " - hibf: " in errs[0] and " - seconds: hash " in errs[0]


def test_a_budget_below_one_row_is_refused(hip, request, tmp_path_factory, tmp_path):  # noqa: F811
    inp, one, ibfs, _ = one_pass(hip, request, tmp_path_factory, "short200")
    tmax, s, max_fp = INPUTS["short200"]
    widest = max(b for _, b in ibfs)
    out = str(tmp_path / "none.hibf")
    p = build(inp, out, tmax, s, max_fp, extra=("--hibf-memory", str(widest - 1)), expect=1)
    first = next(i for i, (_, b) in enumerate(ibfs) if b == widest)
    assert f"--hibf-memory: IBF {first}: " in p.stderr and f"{widest} bytes" in p.stderr and "not one row fits" in p.stderr, p.stderr
    assert not os.path.exists(out)


def test_classify_on_the_file_built_in_parts(hip, request, tmp_path_factory, tmp_path):  # noqa: F811
    inp, one, ibfs, _ = one_pass(hip, request, tmp_path_factory, "short200")
    tmax, s, max_fp = INPUTS["short200"]
    out = beside(one, "classify.hibf")
    build(inp, out, tmax, s, max_fp, extra=("--hibf-memory", str(budget_of(ibfs, "three")), "--hibf-devices", "0,0"))
    assert filecmp.cmp(out, one, shallow=False)
    fq = str(tmp_path / "reads.fq")
    gf.write_fastq(fq, [(rid, seq) for rid, seq, _ in cut_reads(inp, 0, np.random.default_rng(8), per_target=1, n_random=20)])
    outs = []
    for tag, index in (("parts", out), ("one", one)):
        prefix = str(tmp_path / tag)
        cu.run(cu.BIN_HIP, ["--ibf", index, "--hibf", "--single-reads", fq, "-o", prefix, "--output-all", "--skip-lca", "--rel-cutoff", "1", "--rel-filter", "1",
                            "--quiet"])
        outs.append((open(prefix + ".all", "rb").read(), open(prefix + ".rep", "rb").read()))
    assert outs[0] == outs[1] and outs[0][0]
