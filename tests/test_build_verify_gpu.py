"""`ganon-build --hibf --verify-index` on the GPU: gn_filter_probe_path and gn_filter_probe_paths_shared against a numpy restatement
of include/ganon_hip.h over the downloaded rows, and the command on indexes it built, on one built with another --min-length and on
deliberately damaged files."""
import math
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import ganon_fixtures as gf
import hibf_checks as hc
from test_build_cpu import BIN_BUILD
from test_build_hibf_gpu import Inputs, K, W, build, genomes, hip, paths_of, short200  # noqa: F401  (genomes, hip and short200 are fixtures)
from test_build_similarity_gpu import families36  # noqa: F401  (a fixture)

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
NONE = 0xFFFFFFFFFFFFFFFF
U64 = np.uint64


# ------------------------------------------------------------------------------------------------------------ the restatement
def _constants():
    text = open(os.path.join(HERE, "..", "include", "ganon_ibf_hash.h")).read()
    seeds = [int(x) for x in re.search(r"GN_IBF_SEED_LIST \{([^}]*)\}", text).group(1).replace("ULL", "").split(",")]
    return seeds, int(re.search(r"GN_IBF_MULTIPLIER (\d+)ULL", text).group(1))


SEEDS, MULTIPLIER = _constants()


def rows_of(v: np.ndarray, i: int, S: int) -> np.ndarray:
    """include/ganon_ibf_hash.h: row(v, i) = mulhi64((x ^ (x >> clz64(S))) * multiplier, S), x = v * seed[i]; for S below 2^32"""
    assert 0 < S < (1 << 32)
    with np.errstate(over="ignore"):
        x = v.astype(U64) * U64(SEEDS[i])
        x ^= x >> U64(64 - S.bit_length())
        x *= U64(MULTIPLIER)
        lo, hi = x & U64(0xFFFFFFFF), x >> U64(32)
        return (hi * U64(S) + ((lo * U64(S)) >> U64(32))) >> U64(32)


def contained(mats, h, v: np.ndarray, entry) -> np.ndarray:
    """bool per hash: for at least one bin of the entry's run, all h rows have the bin's bit set"""
    ibf, first, n = int(entry["ibf"]), int(entry["first_bin"]), int(entry["n_bins"])
    data = mats[ibf]
    hit = np.zeros(len(v), dtype=bool)
    for w in range(first >> 6, ((first + n - 1) >> 6) + 1):
        lo, hi = max(first, w * 64), min(first + n, w * 64 + 64)
        mask = U64(((1 << (hi - lo)) - 1) << (lo - w * 64))
        a = np.full(len(v), NONE, dtype=U64)
        for i in range(h):
            a &= data[rows_of(v, i, data.shape[0]), w]
        hit |= (a & mask) != 0
    return hit


def probe_path_ref(mats, h, sets, paths):
    """(found, lost_at, first_lost) as include/ganon_hip.h states them"""
    n, depth = paths.shape
    found, first = np.zeros(n, U64), np.full(n, NONE, U64)
    lost = np.zeros((n, depth), U64)
    for s, v in enumerate(sets):
        ok = np.ones(len(v), dtype=bool)
        for d in range(depth):
            if paths[s, d]["n_bins"] == 0:
                break
            c = contained(mats, h, v, paths[s, d])
            lost[s, d] = np.count_nonzero(~c)
            ok &= c
        found[s] = np.count_nonzero(ok)
        if not ok.all():
            first[s] = int(np.argmin(ok))
    return found, lost, first


def shared_ref(mats, h, probes, paths):
    memo, out = {}, np.zeros(len(paths), U64)
    for p in range(len(paths)):
        ok = np.ones(len(probes), dtype=bool)
        for e in paths[p]:
            if e["n_bins"] == 0:
                break
            key = (int(e["ibf"]), int(e["first_bin"]), int(e["n_bins"]))
            if key not in memo:
                memo[key] = contained(mats, h, probes, e)
            ok &= memo[key]
        out[p] = np.count_nonzero(ok)
    return out


def probes_of_the_command(P=65536):
    """include/ganon_hip.h: splitmix64 of i + 1 with bit 63 set"""
    with np.errstate(over="ignore"):
        z = (np.arange(P, dtype=U64) + U64(1)) * U64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> U64(30))) * U64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> U64(27))) * U64(0x94D049BB133111EB)
        z ^= z >> U64(31)
    return z | U64(1 << 63)


def test_the_restatement_against_the_oracle():
    import oracle
    ref = oracle.Ibf(70, 4099, 3)
    v = np.random.default_rng(1).integers(0, 1 << 63, size=200, dtype=U64) * U64(2) + U64(1)
    for i in range(3):
        assert rows_of(v, i, 4099).tolist() == [ref.row(int(x), i) for x in v]
    assert probes_of_the_command(3).tolist() == [0xE220A8397B1DCDAF | 1 << 63, 0x6E789E6AA1B965F4 | 1 << 63, 0x06C45D188009454F | 1 << 63]  # splitmix64(seed 0)


# ------------------------------------------------------------------------------------------------------------ the two device functions
SIZES = (0, 1, 63, 64, 65, 511, 512, 513, 1500)  # the insert's item boundaries
TREES = [(40, 8, 3), (150, 64, 2), (10, 4, 4), (30, 64, 1)]
_trees = {}


@pytest.fixture(scope="module")
def trees(hip):
    """tree -> (filter with every set inserted along its own path, sets, paths, downloaded matrices, hash functions, bins per IBF); built on demand"""
    def get(n_ub, tmax, depth):
        key = (n_ub, tmax, depth)
        if key not in _trees:
            rng = np.random.default_rng(n_ub * 7 + tmax)
            hb = gf.random_hibf(n_ub, tmax, depth, seed=n_ub + tmax, density=0.0, hash_funs=3, rows=(3000, 9000))
            sets = [np.unique(rng.integers(0, 1 << 38, size=4 * SIZES[u % len(SIZES)], dtype=U64))[:SIZES[u % len(SIZES)]] for u in range(n_ub)]
            assert [len(s) for s in sets] == [SIZES[u % len(SIZES)] for u in range(n_ub)]
            paths, _, _ = paths_of(hb, [len(x) for x in sets])
            flt = hip.HipFilter.hibf([(None, f.bins, f.bin_size, f.hash_funs) for f in hb.ibfs], hb.next_ibf_id, hb.bin_to_user, n_ub)
            flt.emplace_path(sets, paths)
            mats = [flt.download_rows(0, f.bin_size, f.bin_words, ibf_idx=i) for i, f in enumerate(hb.ibfs)]
            assert any(m.any() for m in mats)
            _trees[key] = (flt, sets, paths, mats, 3, [f.bins for f in hb.ibfs])
        return _trees[key]
    yield get
    for flt, *_ in _trees.values():
        flt.free()
    _trees.clear()


@pytest.mark.parametrize("n_ub,tmax,depth", TREES)
def test_probe_path(trees, n_ub, tmax, depth):
    flt, sets, paths, mats, h, bins = trees(n_ub, tmax, depth)
    sizes = np.array([len(s) for s in sets], U64)
    found, lost, first = flt.probe_path(sets, paths)
    assert np.array_equal(found, sizes) and not lost.any() and (first == U64(NONE)).all(), "every set along its own path"
    other = np.roll(paths, -1, axis=0)  # every set along the next user bin's path
    exp = probe_path_ref(mats, h, sets, other)
    assert (exp[0] < sizes).any() and exp[1].any(), "the case is meant to lose hashes"
    found, lost, first = flt.probe_path(sets, other)
    print(f"tree {n_ub}/{tmax}/{depth}: {int(sizes.sum())} hashes, {int(found.sum())} found along the neighbour's path, lost per level {lost.sum(axis=0).tolist()}")
    assert np.array_equal(found, exp[0]) and np.array_equal(lost, exp[1]) and np.array_equal(first, exp[2])
    found, lost, first = flt.probe_path(sets, other, with_lost_at=False)
    assert lost is None and np.array_equal(found, exp[0]) and np.array_equal(first, exp[2])


def test_probe_path_word_boundaries(hip):
    """an IBF of 192 bins under a root: runs that straddle a word, fill one exactly, reach the last bin; single bins at 63 and 191"""
    from ganon_amd import hip as H
    rng = np.random.default_rng(192)
    rows0, rows1, h = 4001, 7001, 3
    nx = [np.array([1], np.int64), np.full(192, 1, np.int64)]
    bu = [np.array([-1], np.int64), np.arange(192, dtype=np.int64)]
    flt = hip.HipFilter.hibf([(None, 1, rows0, h), (None, 192, rows1, h)], nx, bu, 192)
    runs = {"straddle": (60, 10), "word": (64, 64), "last": (127, 65), "bin63": (63, 1), "bin191": (191, 1)}
    sets = {name: np.unique(rng.integers(0, 1 << 38, size=n, dtype=U64)) for name, n in (("straddle", 700), ("last", 1300), ("bin63", 65), ("bin191", 513))}

    def path(name, size=0):
        first, n = runs[name]
        p = np.zeros(2, dtype=H.PATH_DTYPE)
        p[0] = (1, first, n, 0, max(1, (size + n - 1) // n))
        p[1] = (0, 0, 1, 0, 1)
        return p

    inserted = ["straddle", "last", "bin63", "bin191"]  # (not "word": it overlaps "straddle" on purpose and is only looked at)
    flt.emplace_path([sets[n] for n in inserted], np.stack([path(n, len(sets[n])) for n in inserted]))
    mats = [flt.download_rows(0, rows0, 1, ibf_idx=0), flt.download_rows(0, rows1, 3, ibf_idx=1)]
    own = np.stack([path(n) for n in inserted])
    found, lost, first = flt.probe_path([sets[n] for n in inserted], own)
    assert found.tolist() == [len(sets[n]) for n in inserted] and not lost.any() and (first == U64(NONE)).all()
    for name in ("straddle", "last"):  # one set against all five entries
        five = np.stack([path(n) for n in runs])
        exp = probe_path_ref(mats, h, [sets[name]] * 5, five)
        got = flt.probe_path([sets[name]] * 5, five)
        print(f"{name}: found per entry {dict(zip(runs, got[0].tolist()))}")
        for a, b in zip(got, exp):
            assert np.array_equal(a, b)
        assert got[0][list(runs).index(name)] == len(sets[name])
    word = flt.probe_path([sets["straddle"]], path("word")[None, :])[0][0]
    assert 6 * 70 <= word < len(sets["straddle"]), "the hashes dealt to bins 64..69 are in the run 64..127, those of bins 60..63 only by chance"
    # the root's rows zeroed: every set is lost at exactly that level
    flt.write_rows(0, np.zeros((rows0, 1), U64), ibf_idx=0)
    found, lost, first = flt.probe_path([sets[n] for n in inserted], own)
    assert not found.any() and not lost[:, 0].any() and lost[:, 1].tolist() == [len(sets[n]) for n in inserted] and not first.any()
    flt.free()


@pytest.mark.parametrize("n_ub,tmax,depth", TREES)
def test_probe_paths_shared(trees, n_ub, tmax, depth):
    flt, sets, paths, mats, h, bins = trees(n_ub, tmax, depth)
    rng = np.random.default_rng(n_ub)
    members = np.concatenate([s[:7] for s in sets])
    probes = np.concatenate([rng.integers(0, 1 << 38, size=1000 - min(300, len(members)), dtype=U64), members[:300]])
    probes = rng.permutation(probes)
    assert len(probes) == 1000  # not a multiple of 64
    for n_paths in (1, 63, 64, 65, 257):
        some = paths[np.arange(n_paths) % n_ub]  # (more paths than user bins: paths repeat)
        exp = shared_ref(mats, h, probes, some)
        got = flt.probe_paths_shared(probes, some)
        assert np.array_equal(got, exp), n_paths
        assert np.array_equal(flt.probe_path([probes] * n_paths, some)[0], exp), "the same probes as one set per path"
        perm = rng.permutation(n_paths)
        assert np.array_equal(flt.probe_paths_shared(probes, some[perm]), exp[perm]), "the order of the paths does not show"
    print(f"tree {n_ub}/{tmax}/{depth}: of 1000 probes, {int(exp.min())}..{int(exp.max())} contained per path")
    assert exp.max() > 0


def test_probe_refusals(hip, trees):
    from ganon_amd import hip as H
    flt, sets, paths, mats, h, bins = trees(10, 4, 4)
    probes = np.arange(100, dtype=U64)
    flat = hip.HipFilter.ibf(None, 64, 1000, 3)
    for call in (lambda: flat.probe_path(sets, paths), lambda: flat.probe_paths_shared(probes, paths)):
        with pytest.raises(H.GanonHipError) as e:
            call()
        assert e.value.code == -22 and "HIBF" in str(e.value)
    flat.free()
    n_ibf = len(mats)
    bad_ibf, bad_bin = paths.copy(), paths.copy()
    bad_ibf[3, 1]["ibf"] = n_ibf  # one past the end, on an entry above the leaf
    assert bad_ibf[3, 1]["n_bins"] == 1
    bad_bin[5, 0]["n_bins"] = bins[int(bad_bin[5, 0]["ibf"])] - int(bad_bin[5, 0]["first_bin"]) + 1  # a run one past the IBF's bins
    for bad in (bad_ibf, bad_bin):
        for call in (lambda: flt.probe_path(sets, bad), lambda: flt.probe_paths_shared(probes, bad)):
            with pytest.raises(H.GanonHipError) as e:
                call()
            assert e.value.code == -22, str(e.value)
    # nothing to do is legal
    found, lost, first = flt.probe_path([], np.zeros((0, 4), dtype=H.PATH_DTYPE))
    assert len(found) == 0 and len(first) == 0
    assert not flt.probe_paths_shared(np.zeros(0, U64), paths).any()
    found, lost, first = flt.probe_path([np.zeros(0, U64)] * len(sets), paths)
    assert not found.any() and not lost.any() and (first == U64(NONE)).all()
    assert np.array_equal(flt.probe_path(sets, paths)[0], [len(s) for s in sets]), "the filter still answers after the refusals"


# ------------------------------------------------------------------------------------------------------------ the command
P = 65536
HEAD = "#target\tuser_bin\tleaf_ibf\tbins\tdepth\tdistinct_hashes\tmissing\tfalse_hits\tobserved_fp\tverdict"


def verify(index, tsv, extra=(), expect=0):
    """-> (index line, {target: dict of its line}, {target: line after a FAIL}, result line, stderr)"""
    p = subprocess.run([BIN_BUILD, "--hibf", "--verify-index", index, "-i", tsv, "-t", "2"] + list(extra), capture_output=True, text=True, timeout=300)
    assert p.returncode == expect, (p.returncode, p.stdout[-2000:], p.stderr[-2000:])
    lines = p.stdout.splitlines()
    assert lines[0].startswith("index\t") and lines[1] == HEAD and lines[-1].startswith("result\t")
    rows, notes, last = {}, {}, None
    for ln in lines[2:-1]:
        if ln.startswith("  first false negative: "):
            notes[last] = ln
            continue
        f = ln.split("\t")
        assert len(f) == 10, ln
        last = f[0]
        rows[last] = dict(zip(HEAD[1:].split("\t"), f))
    return lines[0], rows, notes, lines[-1], p.stderr


def file_paths(m):
    """the paths of every user bin from the file's tables (hibf_checks.check_tree), as PATH_DTYPE [n_user, levels]"""
    from ganon_amd import hip as H
    bins = [f[0] for f in m.ibfs]
    runs, depth, below, where, parent = hc.check_tree(bins, m.next_ibf_id, m.bin_to_user, len(m.names), max(bins), max_levels=64)
    paths = np.zeros((len(m.names), max(depth) + 1), dtype=H.PATH_DTYPE)
    for u, (i, first, n) in where.items():
        paths[u, 0] = (i, first, n, 0, 0)
        at, d = i, 1
        while at != 0:
            at, b = parent[at]
            paths[u, d] = (at, b, 1, 0, 0)
            d += 1
    return paths


def warn_above(fpr):
    return math.ceil(P * fpr + 4 * math.sqrt(P * fpr * (1 - fpr)))


def check_report(index, inp, min_length, got, fpr=None):
    """every line of a passing report against the oracle's sets and a walk over the file's bits; -> (false hits per target, marks)"""
    from ganon_amd import ibf_file
    head, rows, notes, result, _ = got
    m = ibf_file.read_hibf_meta(index)
    fpr = m.fpr if fpr is None else fpr
    names, sets = inp.sets(min_length)
    assert m.names == names and not notes
    paths = file_paths(m)
    h = m.ibfs[0][2]
    assert head == f"index\t{index}\tk={K} w={W} h={h} ibfs={len(m.ibfs)} levels={paths.shape[1]} user_bins={len(names)} fpr={fpr:g}"
    hits = shared_ref([m.payload(index, i) for i in range(len(m.ibfs))], h, probes_of_the_command(), paths)
    marks = {}
    for u, t in enumerate(names):
        r = rows[t]
        used = int(np.count_nonzero(paths[u]["n_bins"]))
        assert (r["user_bin"], r["leaf_ibf"], r["bins"], r["depth"]) == (str(u), str(paths[u, 0]["ibf"]), str(paths[u, 0]["n_bins"]), str(used)), r
        assert int(r["distinct_hashes"]) == len(sets[u]) and r["missing"] == "0", r
        assert int(r["false_hits"]) == int(hits[u]), (t, r["false_hits"], int(hits[u]))
        assert r["observed_fp"] == f"{int(hits[u]) / P:.6f}"
        marks[t] = int(hits[u]) > warn_above(fpr)
        assert r["verdict"] == ("WARN fp" if marks[t] else "ok"), r
    for t in inp.order:  # a target without a hash has no user bin and nothing to look for
        if t not in names:
            assert rows[t]["verdict"] == "ok" and rows[t]["user_bin"] == "-" and rows[t]["distinct_hashes"] == "0"
    assert set(rows) == set(inp.order)
    assert result == (f"result\tok\t{len(names)} target(s) checked, 0 failing, 0 user bin(s) of the index not named by the input, "
                      f"{sum(len(s) for s in sets)} distinct minimisers looked up, max_observed_fp {int(hits.max()) / P:.6f}, "
                      f"mean_observed_fp {int(hits.sum()) / P / len(names):.6f}")
    print(f"{os.path.basename(index)}: {len(names)} user bins, fpr {fpr:g}: max_observed_fp {int(hits.max()) / P:.6f} mean_observed_fp "
          f"{int(hits.sum()) / P / len(names):.6f}, WARN above {warn_above(fpr)} hits: {sum(marks.values())} line(s)")
    return hits, marks


_built = {}


@pytest.fixture(scope="module")
def built(hip, request, tmp_path_factory):
    """(fixture name, tmax, s, max_fp, min_length, layout) -> (inputs, index), each built once"""
    d = tmp_path_factory.mktemp("verify_built")

    def get(which, tmax, s, max_fp, min_length=0, layout="rule"):
        key = (which, tmax, s, max_fp, min_length, layout)
        if key not in _built:
            inp = request.getfixturevalue(which)
            out = str(d / ("_".join(str(x) for x in key) + ".hibf"))
            build(inp, out, tmax, s, max_fp, min_length, extra=("--layout", layout))
            _built[key] = (inp, out)
        return _built[key]
    yield get
    _built.clear()


@pytest.mark.parametrize("which,tmax,s,max_fp,layout", [("genomes", 8, 0, 0.05, "rule"), ("short200", 4, 3, 0.001, "rule"), ("families36", 6, 3, 0.001, "similarity")])
def test_verify_built_indexes(built, which, tmax, s, max_fp, layout):
    inp, index = built(which, tmax, s, max_fp, 0, layout)
    got = verify(index, inp.tsv, extra=("--verbose",))
    check_report(index, inp, 0, got)
    assert re.search(r"^ - seconds: hash [0-9.e+-]+ load [0-9.e+-]+ membership [0-9.e+-]+ fp [0-9.e+-]+$", got[4], re.M), got[4]
    # the file's own k, w and hash functions may be given, and nothing was written
    verify(index, inp.tsv, extra=("-k", str(K), "-w", str(W), "-s", str(4 if s == 0 else s), "--quiet"))


def test_verify_min_length(built):
    """an index built with -y: verified with the same -y it passes; without, exactly the targets that own a hash of a dropped sequence fail"""
    inp, index = built("short200", 8, 3, 0.001, 1000)
    check_report(index, inp, 1000, verify(index, inp.tsv, extra=("--min-length", "1000")))
    names, kept = inp.sets(1000)
    all_names, full = inp.sets(0)
    extra = {t: len(full[all_names.index(t)]) - len(kept[u]) for u, t in enumerate(names)}
    assert 0 < sum(1 for x in extra.values() if x) < len(names), "the case is meant to drop sequences of some targets that keep others"
    _, rows, notes, result, _ = verify(index, inp.tsv, expect=1)
    for t in all_names:
        r = rows[t]
        if t not in extra:  # every sequence dropped: the index has no such user bin
            assert r["verdict"] == "FAIL: no such user bin", r
            continue
        assert int(r["distinct_hashes"]) == len(full[all_names.index(t)])
        assert (int(r["missing"]) > 0) == (extra[t] > 0) and int(r["missing"]) <= extra[t], (r, extra[t])
        assert r["verdict"] == ("FAIL" if extra[t] else "ok") or (r["verdict"] == "WARN fp" and not extra[t])
        assert (t in notes) == (extra[t] > 0)
    assert result.startswith("result\tFAIL\t")


def swapped_tsv(inp, path, a, b):
    with open(path, "w") as o:
        for line in open(inp.tsv):
            f, t = line.rstrip("\n").split("\t")
            o.write(f"{f}\t{b if t == a else a if t == b else t}\n")
    return path


NOTE = re.compile(r"^  first false negative: hash (\d+) \(index (\d+) of the sorted distinct hashes\); lost at level (\d+), ibf (\d+), bins (\d+)\.\.(\d+); rows((?: \d+)+); "
                  r"bits \[bin: one per hash function\]((?: \[\d+:(?: [01])+\])+)$")


def test_verify_swapped_targets(built, tmp_path):
    inp, index = built("genomes", 8, 0, 0.05)
    names, sets = inp.sets(0)
    a, b = names[0], names[-1]
    _, rows, notes, result, _ = verify(index, swapped_tsv(inp, str(tmp_path / "swapped.tsv"), a, b), expect=1)
    assert {t for t, r in rows.items() if r["verdict"] == "FAIL"} == {a, b}, "the two swapped targets, nobody else"
    assert result.startswith("result\tFAIL\t") and f"{len(names)} target(s) checked, 2 failing" in result
    for t, other in ((a, b), (b, a)):
        note = NOTE.match(notes[t])
        assert note, notes[t]
        hs = sets[names.index(other)]  # what the line `t` was given to look for
        assert int(rows[t]["missing"]) > 0 and int(note.group(3)) == 0, "lost in the user bin's own run: level 0"
        assert int(note.group(1)) == int(hs[int(note.group(2))])
        assert re.search(r"\[\d+:(?: 1)* 0", note.group(8)), "a bin of the run with a bit that is not set"


def test_verify_zeroed_root_row(built, tmp_path):
    """the row of the first target's first hash under hash function 0 zeroed in the ROOT IBF: every target with a hash on that row fails"""
    from ganon_amd import ibf_file
    inp, index = built("genomes", 8, 0, 0.05)
    names, sets = inp.sets(0)
    m = ibf_file.read_hibf_meta(index)
    bins, rows0, h, at = m.ibfs[0]
    Wd = (bins + 63) >> 6
    v = sets[0][:1]
    row = int(rows_of(v, 0, rows0)[0])
    bad = str(tmp_path / "zeroed.hibf")
    data = bytearray(open(index, "rb").read())
    assert any(data[at + row * Wd * 8:at + (row + 1) * Wd * 8])
    data[at + row * Wd * 8:at + (row + 1) * Wd * 8] = bytes(Wd * 8)
    open(bad, "wb").write(bytes(data))
    owners = {t for u, t in enumerate(names) if any((rows_of(sets[u], i, rows0) == U64(row)).any() for i in range(h))}
    assert names[0] in owners
    paths = file_paths(m)
    _, rows, notes, result, _ = verify(bad, inp.tsv, expect=1)
    assert {t for t, r in rows.items() if r["verdict"] == "FAIL"} == owners and set(notes) == owners
    note = NOTE.match(notes[names[0]])
    assert note, notes[names[0]]
    used = int(np.count_nonzero(paths[0]["n_bins"]))
    root = paths[0, used - 1]
    assert (int(note.group(1)), int(note.group(2))) == (int(v[0]), 0), "that hash, the first of the sorted set"
    assert (int(note.group(3)), int(note.group(4)), int(note.group(5)), int(note.group(6))) == (used - 1, 0, int(root["first_bin"]), int(root["first_bin"])), "the root entry"
    assert [int(x) for x in note.group(7).split()] == [int(rows_of(v, i, rows0)[0]) for i in range(h)] and int(note.group(7).split()[0]) == row
    assert re.search(rf"\[{int(root['first_bin'])}: 0", note.group(8)), "the bit of hash function 0 is gone"


def test_verify_patched_fpr(built, tmp_path):
    """the file's fpr patched from 0.05 to 0.0001: nothing is missing, the lines the restatement marks (more than 17 false hits) say WARN fp"""
    from ganon_amd import ibf_file
    inp, index = built("genomes", 8, 0, 0.05)
    m = ibf_file.read_hibf_meta(index)
    at = 30 + 8 + sum(8 + sum(8 + len(s.encode()) for s in lst) for lst in m.bin_path)
    data = bytearray(open(index, "rb").read())
    assert struct.unpack_from("<d", data, at)[0] == 0.05
    struct.pack_into("<d", data, at, 0.0001)
    bad = str(tmp_path / "fpr.hibf")
    open(bad, "wb").write(bytes(data))
    assert warn_above(0.0001) == 17
    hits, marks = check_report(bad, inp, 0, verify(bad, inp.tsv), fpr=0.0001)
    assert any(marks.values()), "the patched value is meant to mark at least one line"


def test_verify_unknown_target(built, tmp_path):
    inp, index = built("genomes", 8, 0, 0.05)
    names, _ = inp.sets(0)
    first = open(inp.tsv).readline().split("\t")[0]
    tsv = str(tmp_path / "more.tsv")
    open(tsv, "w").write(open(inp.tsv).read() + f"{first}\tnot in the index\n")
    _, rows, notes, result, _ = verify(index, tsv, expect=1)
    assert rows["not in the index"]["verdict"] == "FAIL: no such user bin" and int(rows["not in the index"]["distinct_hashes"]) > 0
    assert all(rows[t]["verdict"] in ("ok", "WARN fp") for t in names)
    assert result.startswith("result\tFAIL\t") and f"{len(names)} target(s) checked, 1 failing" in result
