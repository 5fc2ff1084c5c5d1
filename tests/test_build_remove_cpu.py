"""`ganon-build --hibf --update --remove` without a GPU: the tables after a removal (ganon_amd/host/hibf_remove.hpp) through a driver this
test compiles, against a Python restatement of the rule; the tables it leaves against derive_paths; the arithmetic the device's
column-compacting copy is made of (ganon_amd/csrc/gn_bin_spans.h: the segment table and the composition of a destination word, the
very functions the kernel calls) against numpy, under AddressSanitizer and UBSan with a source buffer of exactly rows * W_src words;
which user bins a list of names takes out; and the command's refusals that need no device."""
import math
import os
import subprocess

import numpy as np
import pytest

import ganon_fixtures as gf
import hibf_checks as hc
from test_build_update_cpu import derive

HERE = os.path.dirname(os.path.abspath(__file__))
U64 = np.uint64


@pytest.fixture(scope="module")
def drivers(tmp_path_factory):
    d = tmp_path_factory.mktemp("hibf_remove")
    rem, paths = str(d / "hibf_remove_driver"), str(d / "hibf_paths_driver")
    inc = ["-I", os.path.join(HERE, "..", "include")]
    # a stand-alone program: the sanitizers' runtimes are linked in, nothing is preloaded
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", rem,
                           os.path.join(HERE, "hibf_remove_driver.cpp")] + inc)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-o", paths, os.path.join(HERE, "hibf_paths_driver.cpp")] + inc)
    return rem, paths


def run(driver, text):
    p = subprocess.run([driver], input=text, capture_output=True, text=True)
    assert p.returncode == 0 and p.stderr == "", (p.returncode, p.stderr[-3000:])  # (a sanitizer report ends the program with a status)
    return p.stdout


# ------------------------------------------------------------------------------------------------------------ the rule, restated
def estimate(t, m, h):
    return None if t >= m else int(math.ceil(-(m / h) * math.log1p(-t / m)))


def plan(bins, nx, bu, n_user, remove, rows, h, pop):
    """-> None when IBF 0 is emptied, else a dict of everything the driver prints"""
    n_ibf = len(bins)
    run_of, parent = {}, {}
    for i in range(n_ibf):
        for b in range(bins[i]):
            if bu[i][b] < 0:
                parent[nx[i][b]] = (i, b)
            else:
                run_of.setdefault(bu[i][b], [i, b, 0])[2] += 1
    keep = [[True] * bins[i] for i in range(n_ibf)]
    for u in remove:
        i, first, n = run_of[u]
        keep[i][first:first + n] = [False] * n
    alive, changed = [True] * n_ibf, True
    while changed:
        changed = False
        for i in range(1, n_ibf):
            if alive[i] and not any(keep[i]):
                alive[i], changed = False, True
                keep[parent[i][0]][parent[i][1]] = False
    if not any(keep[0]):
        return None
    gone = set(remove)
    user_map = [-1 if u in gone else u - sum(1 for g in gone if g < u) for u in range(n_user)]
    ibf_map = [-1 if not alive[i] else sum(alive[:i]) for i in range(n_ibf)]
    out = dict(n_user=n_user - len(gone), ibf_map=ibf_map, user_map=user_map, old_ibf=[i for i in range(n_ibf) if alive[i]], bins=[], nx=[], bu=[], pop=[],
               spans=[], new_bin={})
    for i in out["old_ibf"]:
        kept = [b for b in range(bins[i]) if keep[i][b]]
        for to, b in enumerate(kept):
            out["new_bin"][(i, b)] = to
        out["bins"].append(len(kept))
        out["nx"].append([ibf_map[nx[i][b]] if bu[i][b] < 0 else ibf_map[i] for b in kept])
        out["bu"].append([bu[i][b] if bu[i][b] < 0 else user_map[bu[i][b]] for b in kept])
        out["pop"].append([pop[i][b] for b in kept])
        spans = []
        for to, b in enumerate(kept):
            if spans and spans[-1][0] + spans[-1][2] == b:
                spans[-1][2] += 1
            else:
                spans.append([b, to, 1])
        out["spans"].append([tuple(s) for s in spans])
    out["dropped"] = [(i,) + parent[i] for i in range(n_ibf) if not alive[i]]
    out["removed"], stale = [], {}
    for u in sorted(gone):
        i, first, n = run_of[u]
        est = [estimate(pop[i][b], rows[i], h) for b in range(first, first + n)]
        full = any(e is None for e in est)
        hashes = sum(e for e in est if e is not None)
        out["removed"].append((u, i, first, n, sum(pop[i][first:first + n]), hashes, int(full)))
        at = i
        while at != 0:
            pi, pb = parent[at]
            if keep[pi][pb]:
                s = stale.setdefault((ibf_map[pi], out["new_bin"][(pi, pb)]), [pi, pb, pop[pi][pb], 0, 0])
                s[3] += hashes
                s[4] |= int(full)
            at = pi
    out["stale"] = [(s[0], s[1], k[0], k[1], s[2], s[3], s[4]) for k, s in sorted(stale.items())]
    return out


def remove_line(h, n_user, bins, rows, nx, bu, pop, remove):
    parts = ["remove", str(h), str(n_user), str(len(bins))]
    for i in range(len(bins)):
        parts += [str(bins[i]), str(rows[i])] + [str(int(x)) for x in nx[i]] + [str(int(x)) for x in bu[i]] + [str(int(x)) for x in pop[i]]
    return " ".join(parts + [str(len(remove))] + [str(u) for u in remove]) + "\n"


def parse(text):
    lines = text.splitlines()
    if lines[0].startswith("refused"):
        return None
    head = lines[0].split()
    assert head[0] == "case"
    out = dict(n_ibf=int(head[1]), n_user=int(head[2]), old_ibf=[], bins=[], nx=[], bu=[], pop=[], spans=[], dropped=[], removed=[], stale=[])
    for ln in lines[1:]:
        f = ln.split()
        v = [int(x) for x in f[1:]]
        if f[0] == "table":
            B = v[2]
            assert v[0] == len(out["bins"]) and len(v) == 3 + 2 * B
            out["old_ibf"].append(v[1]), out["bins"].append(B), out["nx"].append(v[3:3 + B]), out["bu"].append(v[3 + B:]), out["spans"].append([])
        elif f[0] == "pop":
            out["pop"].append(v[1:])
        elif f[0] == "span":
            out["spans"][v[0]].append(tuple(v[1:]))
        elif f[0] in ("ibfmap", "usermap"):
            out["ibf_map" if f[0] == "ibfmap" else "user_map"] = v
        else:
            out[f[0]].append(tuple(v))
    assert len(out["bins"]) == out["n_ibf"]
    return out


def check_case(drivers, h, n_user, bins, rows, nx, bu, pop, remove):
    rem, paths_driver = drivers
    text = run(rem, remove_line(h, n_user, bins, rows, nx, bu, pop, remove))
    got, exp = parse(text), plan(bins, nx, bu, n_user, remove, rows, h, pop)
    if exp is None:
        assert got is None and "nothing would be left" in text, text[:300]
        return None
    assert got is not None, text[:300]
    for key in ("n_user", "old_ibf", "bins", "nx", "bu", "pop", "spans", "ibf_map", "user_map", "dropped", "removed", "stale"):
        assert got[key] == exp[key], (key, got[key], exp[key])
    # the spans: exactly the surviving bins, closed up to the left, one span per maximal run
    for new_i, i in enumerate(exp["old_ibf"]):
        src = [b for s, d, n in got["spans"][new_i] for b in range(s, s + n)]
        dst = [b for s, d, n in got["spans"][new_i] for b in range(d, d + n)]
        assert src == [b for b in range(bins[i]) if (i, b) in exp["new_bin"]] and dst == list(range(got["bins"][new_i]))
        assert all(a[0] + a[2] < b[0] for a, b in zip(got["spans"][new_i], got["spans"][new_i][1:])), "neighbouring spans would be one"
    # what a reader derives from the new tables: every surviving user bin's old path under the two maps
    depth_old, before = derive(paths_driver, n_user, bins, nx, bu)
    depth_new, after = derive(paths_driver, got["n_user"], got["bins"], got["nx"], got["bu"])
    assert depth_new <= depth_old and sorted(after) == list(range(got["n_user"]))
    for u in range(n_user):
        if exp["user_map"][u] >= 0:
            assert after[exp["user_map"][u]] == [(exp["ibf_map"][i], exp["new_bin"][(i, first)], n) for i, first, n in before[u]], u
    hc.check_tree(got["bins"], [np.array(a) for a in got["nx"]], [np.array(a) for a in got["bu"]], got["n_user"], max(got["bins"]), max_levels=depth_old)
    got["depth"] = (depth_old, depth_new)
    return got


# ------------------------------------------------------------------------------------------------------------ hand-made trees
def three_levels():
    """IBF 0: user bin 0 (2 bins), merged -> 1, user bin 5.  IBF 1: user bin 1, merged -> 2, user bin 4 (3 bins).  IBF 2: user bins 2, 3"""
    bins, rows = [4, 5, 2], [1000, 800, 600]
    nx, bu = [[0, 0, 1, 0], [1, 2, 1, 1, 1], [2, 2]], [[0, 0, -1, 5], [1, -1, 4, 4, 4], [2, 3]]
    pop = [[100, 110, 450, 90], [200, 300, 120, 130, 140], [250, 260]]
    return 6, bins, rows, nx, bu, pop


def test_child_emptied(drivers):
    n_user, *tree = three_levels()
    got = check_case(drivers, 3, n_user, *tree, [2, 3])
    assert got["dropped"] == [(2, 1, 1)] and got["old_ibf"] == [0, 1] and got["bins"] == [4, 4] and got["depth"] == (3, 2)
    assert got["bu"][1] == [1, 2, 2, 2] and got["spans"][1] == [(0, 0, 1), (2, 1, 3)]
    assert [s[:4] for s in got["stale"]] == [(0, 2, 0, 2)], "the merged bin of IBF 1 went with its child; the root's stays, and is stale"
    assert got["stale"][0][5] == sum(r[5] for r in got["removed"])


def test_cascade_through_two_levels(drivers):
    n_user, *tree = three_levels()
    got = check_case(drivers, 3, n_user, *tree, [4, 1, 3, 2])  # (the order of the list does not matter)
    assert got["dropped"] == [(1, 0, 2), (2, 1, 1)] and got["bins"] == [3] and got["nx"] == [[0, 0, 0]] and got["bu"] == [[0, 0, 1]]
    assert got["depth"] == (3, 1) and got["stale"] == [] and got["spans"] == [[(0, 0, 2), (3, 2, 1)]]


def test_first_last_and_a_run(drivers):
    n_user, *tree = three_levels()
    got = check_case(drivers, 3, n_user, *tree, [0, 5])
    assert got["bins"][0] == 1 and got["spans"][0] == [(2, 0, 1)] and got["user_map"] == [-1, 0, 1, 2, 3, -1] and not got["dropped"]
    got = check_case(drivers, 3, n_user, *tree, [4])
    assert got["removed"][0][:4] == (4, 1, 2, 3) and got["removed"][0][4] == 120 + 130 + 140 and got["spans"][1] == [(0, 0, 2)]
    assert got["removed"][0][5] == sum(estimate(t, 800, 3) for t in (120, 130, 140)) and [s[:4] for s in got["stale"]] == [(0, 2, 0, 2)]
    got = check_case(drivers, 3, n_user, *tree, [])
    assert got["bins"] == tree[0] and got["spans"] == [[(0, 0, 4)], [(0, 0, 5)], [(0, 0, 2)]] and not got["removed"]


def test_full_bins_have_no_estimate(drivers):
    n_user, bins, rows, nx, bu, pop = three_levels()
    pop[2][0] = 600
    got = check_case(drivers, 3, n_user, bins, rows, nx, bu, pop, [2])
    assert got["removed"] == [(2, 2, 0, 1, 600, 0, 1)] and [s[4:] for s in got["stale"]] == [(450, 0, 1), (300, 0, 1)]


def test_refusals_of_the_rule(drivers):
    n_user, *tree = three_levels()
    assert check_case(drivers, 3, n_user, *tree, [0, 1, 2, 3, 4, 5]) is None
    for remove, word in (([1, 1], "named twice"), ([6], "user bin 6 of 6")):
        text = run(drivers[0], remove_line(3, n_user, *tree, remove))
        assert text.startswith("refused") and word in text, text
    bins, rows, nx, bu, pop = tree
    text = run(drivers[0], remove_line(3, n_user, bins, rows, [[0, 0, 1, 0], [1, 1, 1, 1, 1], [2, 2]], bu, pop, [1]))  # a merged bin onto its own IBF
    assert text.startswith("refused HIBF tables"), text
    text = run(drivers[0], remove_line(3, n_user, bins, rows, nx, bu, [[100, 110, 1001, 90], pop[1], pop[2]], [1]))
    assert text.startswith("refused") and "bits set" in text, text


@pytest.mark.parametrize("seed", range(12))
def test_random_trees(drivers, seed):
    rng = np.random.default_rng(seed)
    n_user, depth = int(rng.integers(5, 61)), int(rng.integers(2, 5))
    hb = gf.random_hibf(n_user, int(rng.integers(4, 10)), depth, seed=seed, density=0.0, rows=(300, 900))
    bins, rows = [f.bins for f in hb.ibfs], [f.bin_size for f in hb.ibfs]
    nx, bu = [list(map(int, a)) for a in hb.next_ibf_id], [list(map(int, a)) for a in hb.bin_to_user]
    pop = [[int(x) for x in rng.integers(0, rows[i] + 1, size=bins[i])] for i in range(len(bins))]
    dropped = 0
    for k in (0, 1, n_user // 3, n_user - 1):
        remove = [int(u) for u in rng.choice(n_user, size=k, replace=False)]
        got = check_case(drivers, 3, n_user, bins, rows, nx, bu, pop, remove)
        dropped += len(got["dropped"])
    # every user bin of one lowest IBF
    leaf = max(range(len(bins)), key=lambda i: (all(u >= 0 for u in bu[i]), i))
    if leaf and all(u >= 0 for u in bu[leaf]):
        got = check_case(drivers, 3, n_user, bins, rows, nx, bu, pop, sorted(set(bu[leaf])))
        assert leaf in [d[0] for d in got["dropped"]]
    print(f"seed {seed}: {n_user} user bins, {len(bins)} IBFs, {dropped} IBFs dropped over the random removals")


# ------------------------------------------------------------------------------------------------------------ the names
def test_name_resolution(drivers):
    """targets a b c d; user bin 2 carries the name c twice over (with user bin 4), user bin 3 is listed under d AND b (a foreign file)"""
    index = "resolve 5 4 a 1 0 b 2 1 3 c 2 2 4 d 1 3"
    assert run(drivers[0], index + " 2 a c\n").splitlines() == ["resolved 0 2 4"], "a name several user bins hold removes all of them"
    assert run(drivers[0], index + " 3 a a a\n").splitlines() == ["resolved 0"]
    assert run(drivers[0], index + " 3 x a y\n").splitlines() == ["resolved 0", "unknown x", "unknown y"], "every unknown name is listed"
    assert run(drivers[0], index + " 1 d\n").splitlines() == ["resolved 3", "shared 3 b"], "user bin 3 also names b, which stays"
    assert run(drivers[0], index + " 2 d b\n").splitlines() == ["resolved 1 3"]


# ------------------------------------------------------------------------------------------------------------ the spans
SRC_BINS = (1, 63, 64, 65, 127, 128, 200, 1100)


def span_cases(B):
    """{name: [(src_first, dst_first, n_bins)]} for a source of B bins: the destinations closed up to the left"""
    def closed(runs):
        out, at = [], 0
        for s, n in runs:
            out.append((s, at, n))
            at += n
        return out
    cases = {"identity": closed([(0, B)]), "one bin kept": closed([(B // 2, 1)]), "none": []}
    if B > 1:
        cases["first bin dropped"] = closed([(1, B - 1)])
        cases["last bin dropped"] = closed([(0, B - 1)])
        cases["ends at the last bin at a shift"] = closed([(5, B - 5) if B > 5 else (1, B - 1)])
    if B > 71:
        cases["a run over a word boundary dropped"] = closed([(0, 60), (71, B - 71)])
    if B >= 128:
        cases["a whole word dropped"] = closed([(0, 64)] + ([(128, B - 128)] if B > 128 else []))
    if B >= 3:
        cases["every third bin dropped"] = closed([(b, min(2, B - b)) for b in range(1, B, 3)])
        a, b = B // 3, 2 * B // 3
        cases["runs in reverse order"] = closed([(b, B - b), (a, b - a), (0, a)])
    return cases


def gather(src, spans, words_dst):
    """numpy: the rows [rows, W_src] of a source with the spans' columns moved, [rows, words_dst]"""
    bits = np.unpackbits(np.ascontiguousarray(src).view(np.uint8), axis=1, bitorder="little")
    out = np.zeros((src.shape[0], words_dst * 64), dtype=np.uint8)
    for s, d, n in spans:
        out[:, d:d + n] = bits[:, s:s + n]
    return np.packbits(out, axis=1, bitorder="little").view(U64).reshape(src.shape[0], words_dst)


def spans_line(src, bins_src, bins_dst, words_dst, spans):
    parts = ["spans", str(src.shape[0]), str(bins_src), str(bins_dst), str(words_dst), str(len(spans))] + [f"{s} {d} {n}" for s, d, n in spans]
    return " ".join(parts + [format(int(x), "x") for x in src.reshape(-1)]) + "\n"


def compose(driver, src, bins_src, bins_dst, words_dst, spans):
    lines = run(driver, spans_line(src, bins_src, bins_dst, words_dst, spans)).splitlines()
    assert not lines[0].startswith("refused"), lines[0]
    assert len(lines) == src.shape[0] + 1 and lines[-1].startswith("segments ")
    return np.array([[int(x, 16) for x in ln.split()] for ln in lines[:-1]], dtype=U64).reshape(src.shape[0], words_dst), int(lines[-1].split()[1])


@pytest.mark.parametrize("B", SRC_BINS)
def test_span_cases(drivers, B):
    rng = np.random.default_rng(B)
    W = (B + 63) >> 6
    src = rng.integers(0, 1 << 64, size=(7, W), dtype=U64)  # the padding bins of the last word are set too: they must not travel
    for name, spans in span_cases(B).items():
        used = sum(n for _, _, n in spans)
        for bins_dst in sorted({max(used, 1), used + 1, used + 70}):
            for words_dst in ((bins_dst + 63) >> 6, ((bins_dst + 63) >> 6) + 3):
                got, n_seg = compose(drivers[0], src, B, bins_dst, words_dst, spans)
                assert np.array_equal(got, gather(src, spans, words_dst)), (name, B, bins_dst, words_dst)
        if name == "identity":
            exp = src.copy()
            if B & 63:
                exp[:, -1] &= U64((1 << (B & 63)) - 1)
            assert np.array_equal(got[:, :W], exp) and not got[:, W:].any() and n_seg == W, "whole words are one segment each"


@pytest.mark.parametrize("seed", range(8))
def test_random_spans(drivers, seed):
    """random span lists: ascending, disjoint destinations with gaps, free source positions (overlapping and out of order)"""
    rng = np.random.default_rng(100 + seed)
    B = int(rng.choice(SRC_BINS[1:])) if seed else 1100
    W = (B + 63) >> 6
    src = rng.integers(0, 1 << 64, size=(5, W), dtype=U64)
    spans, at = [], 0
    for _ in range(int(rng.integers(1, 40))):
        at += int(rng.integers(0, 70)) * int(rng.integers(0, 2))
        n = int(rng.integers(1, min(B, 150) + 1))
        spans.append((int(rng.integers(0, B - n + 1)), at, n))
        at += n
    words_dst = ((at + 63) >> 6) + int(rng.integers(0, 3))
    got, _ = compose(drivers[0], src, B, at, words_dst, spans)
    assert np.array_equal(got, gather(src, spans, words_dst))


def test_span_refusals(drivers):
    src = np.zeros((1, 2), dtype=U64)
    for spans, word in (([(0, 0, 0)], "0 bins"), ([(60, 0, 11)], "beyond the source"), ([(0, 90, 11)], "beyond the destination"),
                        ([(0, 0, 10), (20, 9, 5)], "overlap"), ([(0, 20, 10), (20, 0, 5)], "ascend")):
        text = run(drivers[0], spans_line(src, 70, 100, 2, spans))
        assert text.startswith("refused") and word in text, (spans, text)


# ------------------------------------------------------------------------------------------------------------ the command's refusals
from test_build_cpu import BIN_BUILD  # noqa: E402
from test_build_hibf_cpu import tiny_input  # noqa: E402,F401  (a fixture)
from test_build_verify_cpu import tiny_index  # noqa: E402,F401  (a fixture)


def test_remove_needs_update(tiny_input, tiny_index, tmp_path):
    inp, out = tiny_input
    names = tmp_path / "names.txt"
    names.write_text("a\n")
    p = subprocess.run([BIN_BUILD, "-i", inp, "--hibf", "-o", out, "--remove", str(names)], capture_output=True, text=True)
    assert p.returncode == 1 and "--remove needs --update" in p.stderr and p.stdout == "" and not os.path.exists(out), p.stderr
    p = subprocess.run([BIN_BUILD, "--hibf", "--update", tiny_index, "-o", out, "--remove", str(tmp_path / "no_such.txt")], capture_output=True, text=True)
    assert p.returncode == 1 and "--remove" in p.stderr and "no_such.txt" in p.stderr and p.stdout == "" and not os.path.exists(out), p.stderr
    p = subprocess.run([BIN_BUILD, "--hibf", "--update", tiny_index, "-o", out], capture_output=True, text=True)  # no input and no --remove: as before
    assert p.returncode == 1 and p.stdout == "" and not os.path.exists(out), p.stderr
    p = subprocess.run([BIN_BUILD, "--help"], capture_output=True, text=True)
    assert "--remove arg" in p.stdout + p.stderr
