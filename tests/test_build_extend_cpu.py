"""Extending user bins an index holds already, without a GPU: deal_run and plan_extend (ganon_amd/host/hibf_update.hpp) through a
driver this test compiles, against a Python restatement that uses the same double expressions in the same order, and plan_update
started from the fills the extensions leave."""
import math
import os
import subprocess

import numpy as np
import pytest

from test_build_update_cpu import plan as plan_new, predict

HERE = os.path.dirname(os.path.abspath(__file__))
HOST = os.path.join(HERE, "..", "ganon_amd", "host")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("hibf_extend") / "hibf_extend_driver")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-o", exe, os.path.join(HERE, "hibf_extend_driver.cpp"), os.path.join(HOST, "build_params.cpp"),
                           "-I", os.path.join(HERE, "..", "include")])
    return exe


def run(driver, line):
    return subprocess.run([driver], input=line, capture_output=True, text=True, check=True).stdout


# ------------------------------------------------------------------------------------------------------------ the rule, restated
def on_the_edge(t, m, h):
    """the estimate before its ceiling is within 1e-9 (relative) of an integer: C++ and Python may round apart"""
    x = -(float(m) / h) * math.log1p(-float(t) / m)
    return x != 0.0 and abs(x - round(x)) <= 1e-9 * max(1.0, abs(x))


def estimate(t, m, h):
    """hashes a bin with t of m rows set holds"""
    assert not on_the_edge(t, m, h), "a case on the edge"
    return math.ceil(-(float(m) / h) * math.log1p(-float(t) / m))


def deal(t, m, h, a):
    """-> (quotas, estimates, level)"""
    e = [estimate(x, m, h) for x in t]
    cost = lambda level: sum(max(0, level - x) for x in e)
    lo, hi = min(e), max(e) + a + 1   # cost(lo) = 0 <= a < cost(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if cost(mid) <= a else (lo, mid)
    level = lo
    q = [max(0, level - x) for x in e]
    for j in sorted(range(len(e)), key=lambda j: (e[j], j)):
        if sum(q) == a:
            break
        if e[j] <= level:
            q[j] += 1
    assert sum(q) == a
    return q, e, level


def check_deal(driver, t, m, h, a):
    text = run(driver, " ".join(["deal", str(m), str(h), str(a), str(len(t))] + [str(x) for x in t]) + "\n")
    assert text.startswith("quotas"), text
    got = [int(x) for x in text.split()[1:]]
    q, e, level = deal(t, m, h, a)
    assert got == q, (t, m, h, a, got, q)
    assert sum(got) == a and len(got) == len(t)
    ends = [e[j] + got[j] for j in range(len(t)) if got[j]]
    assert all(level <= x <= level + 1 for x in ends), "receiving bins end within one hash of the level"
    assert all(e[j] >= level for j in range(len(t)) if not got[j]), "a bin that receives nothing is at the level or above"
    return got, e, level


def run_bound(fpr, s, h, m):
    return math.pow(1.0 - math.exp(math.log(1.0 - fpr) / s), 1.0 / h) * m


def plan_extend(paths, rows, h, fpr, pop, ext):
    """paths[user] = [(ibf, first, n_bins)] leaf first; ext = [(user, hashes, lost_at)] -> (quotas, run, merged, over, fills), the
    numbers as the driver prints them.  Asserts that no prediction is within 1e-9 of its bound."""
    fills = [[float(x) for x in p] for p in pop]
    quotas, run_bins, merged, at, over = [], [], [], {}, []
    for x, (u, n, lost) in enumerate(ext):
        (i, first, s), above = paths[u][0], paths[u][1:]
        m = rows[i]
        t = pop[i][first:first + s]
        q = deal(t, m, h, lost[0])[0]
        quotas.append(q)
        bound = run_bound(fpr, s, h, m)
        for j in range(s):
            fill = predict(t[j], q[j], m, h)
            assert abs(fill - bound) > 1e-9 * bound
            run_bins.append((i, first + j, q[j], t[j], fill))
            fills[i][first + j] = fill
            if not fill <= bound:
                over.append((x, i, first + j, fill, bound))
        for d, (i, b, _) in enumerate(above, start=1):
            bound = math.pow(fpr, 1.0 / h) * rows[i]
            fill = predict(fills[i][b], lost[d], rows[i], h)
            assert abs(fill - bound) > 1e-9 * bound
            if (i, b) not in at:
                at[(i, b)] = len(merged)
                merged.append([i, b, pop[i][b], 0.0])
            fills[i][b] = fill
            merged[at[(i, b)]][3] = fill
            if not fill <= bound:
                over.append((x, i, b, fill, bound))
    return quotas, run_bins, [tuple(t) for t in merged], over, fills


def extend_line(fpr, h, n_user, bins, rows, nx, bu, pop, depth, ext, fresh):
    parts = ["extend", repr(fpr), str(h), str(n_user), str(len(bins))]
    for i in range(len(bins)):
        parts += [str(bins[i]), str(rows[i])] + [str(int(x)) for x in nx[i]] + [str(int(x)) for x in bu[i]] + [str(int(x)) for x in pop[i]]
    parts += [str(len(ext)), str(depth)]
    for u, n, lost in ext:
        parts += [str(u), str(n)] + [str(x) for x in list(lost) + [0] * (depth - len(lost))]
    return " ".join(parts + [str(len(fresh))] + [str(c) for c in fresh]) + "\n"


def parse(text):
    lines = text.splitlines()
    if lines[0].startswith("refused"):
        return None
    assert lines[0].startswith("case")
    out = dict(depth=int(lines[0].split()[1]), n_user=int(lines[0].split()[2]), quotas=[], run=[], merged=[], over=[], paths={}, touched=[])
    for ln in lines[1:]:
        f = ln.split()
        if f[0] == "quota":
            assert int(f[1]) == len(out["quotas"])
            out["quotas"].append([int(x) for x in f[2:]])
        elif f[0] == "run":
            out["run"].append((int(f[1]), int(f[2]), int(f[3]), int(f[4]), float(f[5])))
        elif f[0] in ("merged", "touched"):
            out[f[0]].append((int(f[1]), int(f[2]), int(f[3]), float(f[4])))
        elif f[0] == "over":
            out["over"].append((int(f[1]), int(f[2]), int(f[3]), float(f[4]), float(f[5])))
        else:
            assert f[0] == "path"
            out["paths"].setdefault(int(f[1]), []).append(tuple(int(x) for x in f[3:7]))
    return out


def check_case(driver, fpr, h, n_user, bins, rows, nx, bu, pop, paths, ext, fresh=()):
    depth = max(len(p) for p in paths.values())
    got = parse(run(driver, extend_line(fpr, h, n_user, bins, rows, nx, bu, pop, depth, ext, list(fresh))))
    assert got is not None
    quotas, run_bins, merged, over, fills = plan_extend(paths, rows, h, fpr, pop, ext)
    assert got["depth"] == depth and got["quotas"] == quotas
    assert got["run"] == run_bins and got["merged"] == merged and got["over"] == over  # (printed with 17 digits: the same doubles)
    for x, (u, n, lost) in enumerate(ext):
        assert sum(quotas[x]) == lost[0]
    # the new user bins: plan_update's rule, restated in test_build_update_cpu.py, started from the fills the extensions leave
    e_bins, e_nx, e_bu, e_paths, e_touched = plan_new(bins, rows, nx, bu, n_user, h, fpr, fills, list(fresh))
    for k in range(len(fresh)):
        assert [e for e in got["paths"][k] if e[2] != 0] == e_paths[k]
    assert [(t[0], t[1], t[3]) for t in got["touched"]] == [(t[0], t[1], t[3]) for t in e_touched]
    assert all(t[2] == pop[t[0]][t[1]] for t in got["touched"]), "bits_before is the bit count, not the carried fill"
    return got


# ------------------------------------------------------------------------------------------------------------ deal_run
M, H = 10007, 3


def test_deal_an_empty_run(driver):
    q, e, level = check_deal(driver, [0, 0, 0, 0], M, H, 1001)
    assert e == [0, 0, 0, 0] and q == [251, 250, 250, 250]


def test_deal_equal_fills(driver):
    q, e, _ = check_deal(driver, [1200] * 7, M, H, 3000)
    assert len(set(e)) == 1 and q == [429, 429, 429, 429, 428, 428, 428]


def test_deal_one_bin_far_fuller_gets_nothing(driver):
    q, e, level = check_deal(driver, [500, 6000, 520, 480], M, H, 900)
    assert q[1] == 0 and e[1] > level + 1 and all(x > 0 for x in (q[0], q[2], q[3]))
    assert q[3] > q[0] > q[2], "the emptier a bin, the more it takes"


def test_deal_fewer_hashes_than_bins(driver):
    q, e, _ = check_deal(driver, [300, 100, 300, 100, 300, 100], M, H, 2)
    assert q == [0, 1, 0, 1, 0, 0], "one each to the emptiest, the lower bin first"
    q, _, _ = check_deal(driver, [100] * 6, M, H, 4)
    assert q == [1, 1, 1, 1, 0, 0]


def test_deal_nothing(driver):
    assert check_deal(driver, [300, 100, 200], M, H, 0)[0] == [0, 0, 0]


def test_deal_a_full_bin_is_refused(driver):
    text = run(driver, f"deal {M} {H} 10 3 100 {M} 100\n")
    assert text.startswith("refused") and "full" in text and "bin 1" in text
    assert run(driver, f"deal {M} {H} 10 0\n").startswith("refused")
    assert run(driver, f"deal {M} {H} 10 3 100 100\n").startswith("refused"), "a line that ends early"


def test_deal_random_runs(driver):
    rng = np.random.default_rng(300)
    for case in range(50):
        s = int(rng.integers(1, 301))
        m = int(rng.integers(1000, 200000))
        h = int(rng.integers(2, 6))
        top = int(m * rng.uniform(0.05, 0.9))
        t = [int(x) for x in rng.integers(0, top + 1, size=s)]
        t = [x + 1 if on_the_edge(x, m, h) else x for x in t]  # (the inputs are chosen off the edge; estimate() asserts it)
        a = int(rng.integers(0, 4 * m // h))
        check_deal(driver, t, m, h, a)


# ------------------------------------------------------------------------------------------------------------ plan_extend on hand-made trees
FPR = 0.05


def tree(t1=1000, t2=1200, root_rows=10000, child_rows=(6000, 6000)):
    """root: user bin 0 (bin 0), merged bins 1 and 2; IBF 1: user bins 1 (bins 0..2, a split run) and 2 (bin 3); IBF 2: user bins 3 and 4"""
    bins, rows = [3, 4, 2], [root_rows, child_rows[0], child_rows[1]]
    nx, bu = [[0, 1, 2], [1, 1, 1, 1], [2, 2]], [[0, -1, -1], [1, 1, 1, 2], [3, 4]]
    pop = [[900, t1, t2], [500, 650, 300, 600], [700, 800]]
    paths = {0: [(0, 0, 1)], 1: [(1, 0, 3), (0, 1, 1)], 2: [(1, 3, 1), (0, 1, 1)], 3: [(2, 0, 1), (0, 2, 1)], 4: [(2, 1, 1), (0, 2, 1)]}
    return 5, bins, rows, nx, bu, pop, paths


def test_two_extensions_under_one_merged_bin(driver):
    n_user, bins, rows, nx, bu, pop, paths = tree()
    got = check_case(driver, FPR, H, n_user, bins, rows, nx, bu, pop, paths, [(1, 400, [250, 300]), (2, 200, [120, 150])])
    assert len(got["merged"]) == 1 and got["merged"][0][:3] == (0, 1, 1000)
    first = predict(1000, 300, 10000, H)
    assert got["merged"][0][3] == predict(first, 150, 10000, H) > first, "the second extension sees the first's prediction"
    assert [r[:2] for r in got["run"]] == [(1, 0), (1, 1), (1, 2), (1, 3)] and not got["over"]
    assert got["quotas"][0][2] > got["quotas"][0][0] > got["quotas"][0][1], "300, 500 and 650 bits: the emptiest bin of the run takes most"


def test_an_extension_takes_the_room_of_a_new_user_bin(driver):
    n_user, bins, rows, nx, bu, pop, paths = tree(t1=2000, t2=4700)
    alone = check_case(driver, FPR, H, n_user, bins, rows, nx, bu, pop, paths, [], fresh=[700])
    assert [e for e in alone["paths"][0] if e[2]] == [(1, 4, 1, 700), (0, 1, 1, 1)], "without the extension the merged bin 0:1 has room for 700"
    both = check_case(driver, FPR, H, n_user, bins, rows, nx, bu, pop, paths, [(2, 900, [500, 600])], fresh=[700])
    assert [e for e in both["paths"][0] if e[2]] == [(0, 3, 1, 700)], "600 more hashes in it first: the new user bin widens the root"
    assert not both["over"] and both["n_user"] == 6


def test_bins_over_their_bound_are_listed(driver):
    n_user, bins, rows, nx, bu, pop, paths = tree()
    got = check_case(driver, FPR, H, n_user, bins, rows, nx, bu, pop, paths, [(2, 3000, [2500, 100])])   # a run bin: 2500 hashes into 6000 rows
    assert [o[:3] for o in got["over"]] == [(0, 1, 3)] and got["over"][0][3] > got["over"][0][4] == run_bound(FPR, 1, H, 6000)
    got = check_case(driver, FPR, H, n_user, bins, rows, nx, bu, pop, paths, [(3, 3000, [10, 2500])])    # a merged bin: 2500 into 10000 rows at 1200
    assert [o[:3] for o in got["over"]] == [(0, 0, 2)] and got["over"][0][4] == math.pow(FPR, 1.0 / H) * 10000
    got = check_case(driver, FPR, H, n_user, bins, rows, nx, bu, pop, paths, [(1, 2400, [2100, 10])])    # a split run: the bound of a bin of three
    assert {o[:3] for o in got["over"]} == {(0, 1, 0), (0, 1, 1), (0, 1, 2)} and got["over"][0][4] == run_bound(FPR, 3, H, 6000) < run_bound(FPR, 1, H, 6000)


def test_refusals_of_the_plan(driver):
    n_user, bins, rows, nx, bu, pop, paths = tree()

    def refused(ext, depth=2, **kw):
        a = dict(fpr=FPR, h=H, n_user=n_user, bins=bins, rows=rows, nx=nx, bu=bu, pop=pop, depth=depth, ext=ext, fresh=[])
        a.update(kw)
        text = run(driver, extend_line(**a))
        assert text.startswith("refused"), text[:200]
        return text

    assert "user bin 5" in refused([(5, 10, [1, 1])])
    assert "twice" in refused([(2, 10, [1, 1]), (2, 10, [1, 1])])
    assert "entry 0" in refused([(2, 10, [11, 1])]), "more absent than the set has"
    assert "entry 1" in refused([(0, 10, [5, 5])]), "a count for an entry the path does not have"
    assert "counts for a path" in refused([(2, 10, [1])], depth=1)
    assert "full" in refused([(2, 10, [5, 5])], pop=[[900, 1000, 1200], [500, 650, 300, 6000], [700, 800]])
    assert "HIBF tables" in refused([(2, 10, [5, 5])], nx=[[0, 1, 1], [1, 1, 1, 1], [2, 2]])
    assert "out of range" in refused([(2, 10, [5, 5])], h=6)
    assert refused([], depth=65).startswith("refused driver")


# ------------------------------------------------------------------------------------------------------------ the command's refusals
# (Without --extend a held target still gets the message it always got and nothing is written: run_update hashes on the device before it
# reads the index's names, so that case is in tests/test_build_extend_gpu.py, test_extend_over_the_bound, as is a name two user bins hold.)
from test_build_cpu import BIN_BUILD  # noqa: E402
from test_build_hibf_cpu import tiny_input  # noqa: E402,F401  (a fixture)
from test_build_verify_cpu import tiny_index  # noqa: E402,F401  (a fixture: k 19, w 32, h 3, fpr 0.05)


@pytest.mark.parametrize("args", [["--extend"], ["--hibf", "--extend"], ["--hibf", "--extend", "--verify-index", "INDEX"]])
def test_extend_needs_update(tiny_input, tiny_index, args):
    assert os.path.exists(BIN_BUILD), "ganon-build is built by __graft_entry__.build()"
    inp, out = tiny_input
    args = [tiny_index if a == "INDEX" else a for a in args]
    p = subprocess.run([BIN_BUILD, "-i", inp] + ([] if "--verify-index" in args else ["-o", out]) + args, capture_output=True, text=True)
    assert p.returncode == 1 and "--extend needs --update" in p.stderr, (p.returncode, p.stderr)
    assert "device" not in p.stderr.lower() and p.stdout == "" and not os.path.exists(out)


def test_extend_keeps_the_refusals_of_update(tiny_input, tiny_index):
    inp, out = tiny_input
    size = os.path.getsize(tiny_index)
    for extra, word in ((["--tmax", "64"], "--tmax"), (["--layout", "rule"], "--layout"), (["-k", "21"], "--kmer-size")):
        p = subprocess.run([BIN_BUILD, "-i", inp, "--hibf", "--update", tiny_index, "--extend", "-o", out] + extra, capture_output=True, text=True)
        assert p.returncode == 1 and "--update" in p.stderr and word in p.stderr, (p.returncode, p.stderr)
        assert "device" not in p.stderr.lower() and p.stdout == "" and not os.path.exists(out) and os.path.getsize(tiny_index) == size
    help_text = subprocess.run([BIN_BUILD, "--help"], capture_output=True, text=True)
    assert "--extend" in help_text.stderr + help_text.stdout
