"""`ganon-build --hibf --layout similarity` without a GPU: the similarity order and the layout chosen with it
(ganon_amd/host/hibf_layout_similarity.hpp) through a driver this test compiles, fed exact unions of explicit sets as its estimates:
families of related sets end up side by side and the tree gets smaller, unrelated sets leave `--layout sketch`'s tree as it is, the
intervals and the threshold are what the header says, and the command line refuses what it cannot do."""
import os
import random
import subprocess

import pytest

import hibf_checks as hc
from test_build_cpu import BIN_BUILD
from test_build_hibf_cpu import cases, parse, tables, tiny_input  # noqa: F401  (tiny_input is a fixture)

HERE = os.path.dirname(os.path.abspath(__file__))
HOST = os.path.join(HERE, "..", "ganon_amd", "host")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("hibf_layout_similarity") / "hibf_layout_similarity_driver")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-o", out, os.path.join(HERE, "hibf_layout_similarity_driver.cpp"),
                           os.path.join(HOST, "build_params.cpp")])
    return out


@pytest.fixture(scope="module")
def sketch_driver(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("hibf_layout_sketch_again") / "hibf_layout_sketch_driver")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-o", out, os.path.join(HERE, "hibf_layout_sketch_driver.cpp"), os.path.join(HOST, "build_params.cpp")])
    return out


def families(seed, n_families=8, members=8, lengths=None, keep=0.7, drop=0.1):
    """the model the layout was tried on: an ancestor of random 64-bit values per family; a member loses a random 0 .. `drop` of
    them (so that the sizes of the families interleave) and keeps each of the others with probability `keep`, drawing a fresh
    value otherwise.  Member i of family f is user bin i * n_families + f."""
    rng = random.Random(seed)
    sets = [None] * (n_families * members)
    for f in range(n_families):
        ancestor = [rng.getrandbits(64) for _ in range(lengths[f] if lengths else 2000)]
        for i in range(members):
            d = rng.random() * drop
            sets[i * n_families + f] = sorted({x if rng.random() < keep else rng.getrandbits(64) for x in ancestor if rng.random() >= d})
    return sets


_memo = {}


def run(driver, mode, tmax, counts, sets=None, matrix=None, max_fp=0.001, h=3, noisy=False):
    """-> (stdout, stderr); one run per input is kept"""
    source = "sets" if sets is not None else "matrix" if matrix is not None else "noisy" if noisy else "disjoint"
    words = [mode, str(tmax), repr(max_fp), str(h), str(len(counts)), source] + [str(c) for c in counts]
    if sets is not None:
        words += [str(v) for s in sets for v in s]
    if matrix is not None:
        words += [str(v) for row in matrix for v in row]
    text = " ".join(words) + "\n"
    key = (driver, text)
    if key not in _memo:
        p = subprocess.run([driver], input=text, capture_output=True, text=True, check=True)
        _memo[key] = (p.stdout, p.stderr)
    return _memo[key]


def order_of(driver, counts, sets=None, matrix=None):
    """-> (starts of the intervals, order, pair tables asked for, the largest of them)"""
    lines = run(driver, "order", 8, counts, sets, matrix)[0].splitlines()
    assert [ln.split()[0] for ln in lines] == ["intervals", "order", "tables"]
    starts = [int(x) for x in lines[0].split()[2:]]
    assert len(starts) == int(lines[0].split()[1])
    order = [int(x) for x in lines[1].split()[1:]]
    assert sorted(order) == list(range(len(counts))), "a permutation of the user bins"
    n_tables, largest = (int(x) for x in lines[2].split()[1:])
    return starts, order, n_tables, largest


def order_of_noisy(driver, counts):
    lines = run(driver, "order", 8, counts, noisy=True)[0].splitlines()
    starts = [int(x) for x in lines[0].split()[2:]]
    n_tables, largest = (int(x) for x in lines[2].split()[1:])
    return starts, [int(x) for x in lines[1].split()[1:]], n_tables, largest


def size_order(counts):
    return sorted(range(len(counts)), key=lambda u: (-counts[u], u))


_chains = {}


def chain(counts, sets):
    """the order as the header states it, restated with Python integers and exact unions; computed once per input"""
    key = (tuple(counts), tuple(s[0] for s in sets))
    if key not in _chains:
        _chains[key] = _chain(counts, [set(s) for s in sets])
    return _chains[key]


def _chain(counts, sets):
    order, out, n, a = size_order(counts), [], len(counts), 0
    while a < n:
        b = a + 1
        while b < n and b - a < 1024 and 2 * counts[order[b]] >= counts[order[a]]:
            b += 1
        placed, left = [order[a]], order[a + 1:b]
        while left:
            last, best = placed[-1], None
            for c in left:
                total = counts[last] + counts[c]
                union = len(sets[last] | sets[c])
                shared = total - union
                if shared > 0 and 8 * shared >= min(counts[last], counts[c]) and (best is None or total * best[1] > best[0] * union):
                    best = (total, union, c)
            placed.append(best[2] if best else left[0])
            left.remove(placed[-1])
        out += placed
        a = b
    return out


def contiguous(order, n_families=8):
    """every family (user bin modulo n_families) is one run of the order"""
    runs = [f for j, f in enumerate(u % n_families for u in order) if j == 0 or f != order[j - 1] % n_families]
    return len(runs) == n_families


# ------------------------------------------------------------------------------------------------------------ families
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_families_end_up_side_by_side(driver, seed):
    sets = families(seed)
    counts = [len(s) for s in sets]
    assert not contiguous(size_order(counts)), "the sizes of the families interleave: the size order mixes them"
    starts, order, n_tables, largest = order_of(driver, counts, sets)
    assert starts == [0] and (n_tables, largest) == (1, 64), "all within a factor of two: one interval, one table"
    assert order[0] == size_order(counts)[0], "the largest stays first"
    assert contiguous(order), [u % 8 for u in order]
    assert order == chain(counts, sets)


@pytest.mark.parametrize("tmax", [2, 4, 8, 16])
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_families_get_a_smaller_tree(driver, seed, tmax):
    """by the (exact) estimates, at most 0.9 of what the size order takes; measured with this random stream: 0.71 .. 0.85"""
    sets = families(seed)
    counts = [len(s) for s in sets]
    out, err = run(driver, "similarity", tmax, counts, sets)
    word, intervals, moved, kept, bits = err.split()
    assert (word, intervals, kept) == ("similarity", "1", "similarity") and int(moved) > 32
    sketch_bits = int(run(driver, "sketch", tmax, counts, sets)[1].split()[1])
    print(f"seed {seed} tmax {tmax}: similarity {bits} sketch {sketch_bits} ratio {int(bits) / sketch_bits:.3f}")
    assert int(bits) <= 0.9 * sketch_bits
    lines = out.splitlines()
    asked, longest, width = (int(x) for x in lines.pop().split()[1:])
    assert longest <= width
    levels, L, ibfs = parse("\n".join(lines))
    assert L == hc.levels_for(64, tmax)
    nx, bu = tables(ibfs)
    runs, depth, below, where, parent = hc.check_tree([f["bins"] for f in ibfs], nx, bu, 64, tmax)
    assert levels == max(depth) + 1 <= L
    order = order_of(driver, counts, sets)[1]
    at = {u: j for j, u in enumerate(order)}
    for i, f in enumerate(ibfs):
        assert f["depth"] == depth[i] and (f["parent"], f["parent_bin"]) == (parent[i] if i else (-1, 0))
        for (first, n, user, child), got in zip(runs[i], f["runs"]):
            if user < 0:  # the members of a merged bin are neighbours in the similarity order, and it holds their exact union
                members = sorted(below[child], key=lambda u: at[u])
                assert len(members) >= 2 and order[at[members[0]]:at[members[0]] + len(members)] == members
                assert got[4] == len(set().union(*(sets[u] for u in members)))


@pytest.mark.parametrize("tmax", [2, 4, 8, 16])
def test_families_that_differ_in_size(driver, tmax):
    """ancestors of different lengths and no drop: every member of a family has its ancestor's length, so the size order groups the
    families already.  The order keeps the families where the size order has them and the tree is `sketch`'s, line for line.
    (Inside a family all counts are equal, and the chain then goes by similarity, as its step 4 says, where the size order goes by
    index: the order of the members of one family may differ, the sequence of families may not.)"""
    sets = families(5, lengths=[2000 + 300 * f for f in range(8)], drop=0.0)
    counts = [len(s) for s in sets]
    by_size = size_order(counts)
    assert contiguous(by_size)
    starts, order, _, _ = order_of(driver, counts, sets)
    assert len(starts) == 2, "4100 is more than twice 2000"
    assert contiguous(order) and [u % 8 for u in order] == [u % 8 for u in by_size]
    assert order == chain(counts, sets)
    out, err = run(driver, "similarity", tmax, counts, sets)
    assert err.split()[3] == "sketch"
    assert out.splitlines()[:-1] == run(driver, "sketch", tmax, counts, sets)[0].splitlines()[:-1]


def test_nested_families_keep_the_whole_size_order(driver):
    """as above, with distinct counts inside a family: member i is the first len - 10 * i values of its ancestor, so the closest
    unplaced relative of a member is always the next smaller one, which is the next of the size order.  The two orders are equal,
    position for position, and so are the trees."""
    rng = random.Random(6)
    sets = [None] * 64
    for f in range(8):
        ancestor = sorted({rng.getrandbits(64) for _ in range(2000 + 300 * f)})
        for i in range(8):
            sets[i * 8 + f] = ancestor[:len(ancestor) - 10 * i]
    counts = [len(s) for s in sets]
    assert len(set(counts)) == 64 and contiguous(size_order(counts))
    starts, order, _, _ = order_of(driver, counts, sets)
    assert len(starts) == 2 and order == size_order(counts) == chain(counts, sets)
    for tmax in (2, 4, 8, 16):
        out, err = run(driver, "similarity", tmax, counts, sets)
        assert err.split()[2:4] == ["0", "sketch"]
        assert out.splitlines()[:-1] == run(driver, "sketch", tmax, counts, sets)[0].splitlines()[:-1]


# ------------------------------------------------------------------------------------------------------------ unrelated bins
def unrelated():
    return [(f"{name}/tmax{t}", counts, t) for name, counts, _ in cases() for t in (2, 4, 8, 64)]


@pytest.mark.parametrize("name,counts,tmax", unrelated(), ids=[c[0] for c in unrelated()])
def test_unrelated_bins_give_the_sketch_layout(driver, sketch_driver, name, counts, tmax):
    """disjoint sets: nothing moves, and the output is hibf_layout_sketch_driver's line for line -- so never above `sketch` or the rule"""
    assert order_of(driver, counts)[1] == size_order(counts)
    out, err = run(driver, "similarity", tmax, counts, max_fp=0.05, h=4)
    assert err.split()[2] == "0" and err.split()[3] in ("sketch", "rule")
    line = f"sketch {tmax} 0.05 4 {len(counts)} " + " ".join(str(c) for c in counts) + "\n"
    assert out == subprocess.run([sketch_driver], input=line, capture_output=True, text=True, check=True).stdout


def strangers():
    """one interval of user bins of nearly one size that share nothing: 1024 (a whole window), and 512 as the build benchmark has"""
    return [("1024", [200000 - u * 7919 % 1000 for u in range(1024)], t) for t in (4, 8, 16, 64)] + \
           [("512", [150000 - u * 7919 % 3000 for u in range(512)], t) for t in (4, 16)]


@pytest.mark.parametrize("name,counts,tmax", strangers(), ids=[f"{c[0]}/tmax{c[2]}" for c in strangers()])
def test_strangers_with_noisy_estimates_give_the_sketch_layout(driver, name, counts, tmax):
    """estimates as a sketch gives them for strangers -- the sum, off by a standard error of 1 / 64: of the 131 000 or 524 000 pairs
    of the interval a few are four standard errors low and pass the threshold, so the chain moves user bins and the second search
    runs.  What it gains or loses is noise, well under the margin of one standard error: the tree stays the size order's."""
    starts, order, n_tables, largest = order_of_noisy(driver, counts)
    assert starts == [0] and (n_tables, largest) == (1, len(counts))
    assert order != size_order(counts), "no pair passed the threshold: the case shows nothing"
    out, err = run(driver, "similarity", tmax, counts, noisy=True)
    word, intervals, moved, kept, bits = err.split()
    assert int(moved) > 0 and kept in ("sketch", "rule"), err
    sketch_out, sketch_err = run(driver, "sketch", tmax, counts, noisy=True)
    assert sketch_err.split()[1:] == [bits, kept]
    assert out.splitlines()[:-1] == sketch_out.splitlines()[:-1]  # (the last line counts the estimates asked for: two searches here)


# ------------------------------------------------------------------------------------------------------------ intervals, threshold
def test_a_count_below_half_the_first_starts_an_interval(driver):
    counts = [1000, 999, 500, 499, 498, 250, 249, 248]
    starts, order, n_tables, largest = order_of(driver, counts)
    assert starts == [0, 3, 6] and order == list(range(8))
    assert (n_tables, largest) == (2, 3), "500 is still within half of 1000, 499 is not; 250 is still within half of 499; two members ask for no table"
    assert order_of(driver, [7])[0] == [0] and order_of(driver, [])[0] == []


def test_1025_equal_counts_are_two_intervals(driver):
    starts, order, n_tables, largest = order_of(driver, [777] * 1025)
    assert starts == [0, 1024] and order == list(range(1025))
    assert (n_tables, largest) == (1, 1024), "an interval of one asks for no table"


def related(rng, base, shared, size):
    """`size` values, `shared` of them from `base`"""
    return sorted(set(rng.sample(base, shared)) | {rng.getrandbits(64) for _ in range(size - shared)})


def test_a_related_bin_outside_the_interval_is_not_pulled_in(driver):
    rng = random.Random(7)
    a = sorted(rng.getrandbits(64) for _ in range(1000))
    b, c = ([rng.getrandbits(64) for _ in range(n)] for n in (900, 800))
    inside, outside = related(rng, a, 500, 600), related(rng, a, 450, 499)  # both share most of what they hold with a
    assert order_of(driver, [1000, 900, 800, 600], [a, b, c, inside])[:2] == ([0], [0, 3, 1, 2])
    assert order_of(driver, [1000, 900, 800, 499], [a, b, c, outside])[:2] == ([0, 3], [0, 1, 2, 3])


def test_threshold(driver):
    """a pair that shares a sixteenth of the smaller set stays apart, a pair that shares a quarter becomes neighbours"""
    rng = random.Random(8)
    x = sorted(rng.getrandbits(64) for _ in range(1000))
    y = [rng.getrandbits(64) for _ in range(990)]
    assert order_of(driver, [1000, 990, 976], [x, y, related(rng, x, 61, 976)])[1] == [0, 1, 2]
    assert order_of(driver, [1000, 990, 976], [x, y, related(rng, x, 244, 976)])[1] == [0, 2, 1]
    assert order_of(driver, [1000, 990, 976], [x, y, related(rng, x, 121, 976)])[1] == [0, 1, 2], "8 * 121 < 976"
    assert order_of(driver, [1000, 990, 976], [x, y, related(rng, x, 122, 976)])[1] == [0, 2, 1], "8 * 122 >= 976"


def test_the_closest_relative_comes_next_and_ties_keep_the_size_order(driver):
    rng = random.Random(9)
    x = sorted(rng.getrandbits(64) for _ in range(1000))
    far, near = related(rng, x, 300, 990), related(rng, x, 600, 980)
    assert order_of(driver, [1000, 990, 980], [x, far, near])[1] == [0, 2, 1]
    matrix = [[1000, 1400, 1400], [1400, 900, 1800], [1400, 1800, 900]]  # both as close to 0: the earlier one is taken
    assert order_of(driver, [1000, 900, 900], matrix=matrix)[1] == [0, 1, 2]
    matrix = [[1000, 1401, 1400], [1401, 900, 1800], [1400, 1800, 900]]
    assert order_of(driver, [1000, 900, 900], matrix=matrix)[1] == [0, 2, 1]


def test_same_input_same_bytes(driver):
    sets = families(2)
    counts = [len(s) for s in sets]
    first = (run(driver, "order", 8, counts, sets), run(driver, "similarity", 8, counts, sets))
    _memo.clear()
    assert (run(driver, "order", 8, counts, sets), run(driver, "similarity", 8, counts, sets)) == first


# ------------------------------------------------------------------------------------------------------------ the command line
@pytest.mark.parametrize("extra,words", [(["--layout", "similarity"], ["--hibf"]), (["--hibf", "--layout", "nearest"], ["rule", "sketch", "similarity"]),
                                         (["--hibf", "--layout", "Similarity"], ["rule", "sketch", "similarity"])])
def test_refusals(tiny_input, extra, words):
    assert os.path.exists(BIN_BUILD), "ganon-build is built by __graft_entry__.build()"
    inp, out = tiny_input
    p = subprocess.run([BIN_BUILD, "-i", inp, "-o", out] + extra, capture_output=True, text=True)
    assert p.returncode == 1, (p.returncode, p.stderr)
    assert "--layout" in p.stderr and all(w in p.stderr for w in words) and "device" not in p.stderr.lower(), p.stderr  # before the device is touched
    assert not os.path.exists(out)


def test_help_names_the_layout():
    p = subprocess.run([BIN_BUILD, "--help"], capture_output=True, text=True)
    assert "similarity" in p.stdout + p.stderr
