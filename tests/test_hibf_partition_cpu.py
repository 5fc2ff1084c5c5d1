"""The plan that spreads an HIBF over several devices by subtree (ganon_amd/host/hibf_partition.hpp), run on the CPU through a stand-alone
program built with the sanitizers, against a Python restatement (tests/hibf_partition_checks.py): hand-made trees and 200 random ones.

Decided here, as the header states it: parts go to the budgets IN ORDER; a budget that cannot take the next unit is skipped, and when
the units run out the trailing budgets stay empty and unused (no refusal for more devices than units)."""
import os
import subprocess

import numpy as np
import pytest

import ganon_fixtures as gf
import hibf_partition_checks as hp
import oracle

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("hibf_partition") / "hibf_partition_driver")
    # a stand-alone program: the sanitizers' runtimes are linked in, nothing is preloaded
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                           os.path.join(HERE, "hibf_partition_driver.cpp"), "-I", os.path.join(HERE, "..", "include")])
    return exe


def case_text(h, budgets):
    out = [f"{len(h.ibfs)} {h.n_user_bins}"]
    for i, f in enumerate(h.ibfs):
        out.append(f"{f.bins} {f.bin_size}")
        out.append(" ".join(f"{int(n)} {int(u)}" for n, u in zip(h.next_ibf_id[i], h.bin_to_user[i])))
    out.append(f"{len(budgets)} " + " ".join(str(int(b)) for b in budgets))
    return "\n".join(out) + "\n"


def run(driver, text):
    p = subprocess.run([driver], input=text, capture_output=True, text=True)
    assert p.returncode == 0 and p.stderr == "", (p.returncode, p.stderr[-3000:])  # (a sanitizer report ends the program with a status)
    return p.stdout


def parse(out):
    """-> list per case: a refusal string, or a list of part dicts"""
    cases, lines, i = [], out.splitlines(), 0
    while i < len(lines):
        if lines[i].startswith("refusal "):
            cases.append(lines[i][8:])
            i += 1
            continue
        head = lines[i].split()
        assert head[0] == "parts" and head[2] == "units"
        parts, i = [], i + 1
        for _ in range(int(head[1])):
            v = [int(x) for x in lines[i].split()[1:]]
            p = dict(zip(["slot", "unit_lo", "unit_hi", "bin_lo", "bin_hi", "word_lo", "word_hi", "bytes", "n_ibf", "n_user"], v))
            p["ibf_global"] = [int(x) for x in lines[i + 1].split()[1:]]
            p["user_global"] = [int(x) for x in lines[i + 2].split()[1:]]
            i += 3
            p["shapes"], p["next_ibf_id"], p["bin_to_user"] = [], [], []
            for _ in range(p["n_ibf"]):
                bins, words, rows = [int(x) for x in lines[i].split()[1:]]
                p["shapes"].append((bins, words, rows))
                p["next_ibf_id"].append([int(x) for x in lines[i + 1].split()[1:]])
                p["bin_to_user"].append([int(x) for x in lines[i + 2].split()[1:]])
                i += 3
            parts.append(p)
        cases.append(dict(units=int(head[3]), parts=parts))
    return cases


def check_plan(h, budgets, got):
    """every invariant of a plan that was not refused"""
    units = hp.units_of(h)
    C = hp.cost_matrix(h, units)
    best = hp.optimum(C, budgets)
    assert best is not None and not isinstance(got, str), got
    assert got["units"] == len(units)
    parts = got["parts"]
    B = h.ibfs[0].bins
    # every root bin is owned by exactly one part; parts are contiguous unit ranges, in budget order; a (split) user bin is in one part
    at, slot = 0, -1
    for p in parts:
        assert p["unit_lo"] == at and p["unit_hi"] > at and p["slot"] > slot
        at, slot = p["unit_hi"], p["slot"]
        assert (p["bin_lo"], p["bin_hi"]) == (units[p["unit_lo"]][0], units[p["unit_hi"] - 1][1])
        assert (p["word_lo"], p["word_hi"]) == (p["bin_lo"] >> 6, (p["bin_hi"] + 63) >> 6)
    assert at == len(units) and parts[-1]["bin_hi"] == B and parts[0]["bin_lo"] == 0
    # every non-root IBF is in exactly one part, the one that owns the merged bin of the root above it
    seen = {}
    for k, p in enumerate(parts):
        assert p["ibf_global"][0] == 0
        for g in p["ibf_global"][1:]:
            assert g not in seen
            seen[g] = k
    assert sorted(seen) == list(range(1, len(h.ibfs)))
    for k, p in enumerate(parts):
        for u in units[p["unit_lo"]:p["unit_hi"]]:
            assert all(seen[g] == k for g in u[2])
    users = [u for p in parts for u in p["user_global"]]
    assert len(users) == len(set(users)) and set(users) == {int(u) for a in h.bin_to_user for u in a if u >= 0}
    for p in parts:
        # bytes within the budget and as the restatement counts them; maps strictly increasing; the trees as restated (absent bins in
        # the boundary words included)
        assert p["bytes"] == int(C[p["unit_lo"], p["unit_hi"]]) <= budgets[p["slot"]]
        assert all(a < b for a, b in zip(p["ibf_global"], p["ibf_global"][1:]))
        assert all(a < b for a, b in zip(p["user_global"], p["user_global"][1:]))
        ref = hp.build_part(h, units, p["unit_lo"], p["unit_hi"])
        assert p["ibf_global"] == ref["ibf_global"] and p["user_global"] == ref["user_global"]
        assert p["next_ibf_id"] == ref["next_ibf_id"] and p["bin_to_user"] == ref["bin_to_user"]
        assert [(s[0], s[2]) for s in p["shapes"]] == [(s[0], s[1]) for s in ref["shapes"]]
        first = p["word_lo"] * 64
        for t in range(p["shapes"][0][0]):
            absent = p["next_ibf_id"][0][t] == -1 and p["bin_to_user"][0][t] == -1
            assert absent == (not p["bin_lo"] <= first + t < p["bin_hi"])
    # the largest part is as small as it can be
    assert max(p["bytes"] for p in parts) == best
    return parts


def tiny(rows=16):
    return dict(density=0.5, rows=(rows, rows + 1))


def hand_made():
    """a root of 70 bins = two words: bins 0-59 single user bins, a user bin split over 62-64 across the word boundary, merged bins"""
    rng = np.random.default_rng(1)
    nxt0, b2u0 = [], []
    for b in range(60):
        nxt0.append(0)
        b2u0.append(b)
    nxt0 += [1, 2]  # bins 60, 61: merged
    b2u0 += [-1, -1]
    for _ in range(3):  # bins 62..64: one user bin, split
        nxt0.append(0)
        b2u0.append(60)
    nxt0 += [3]
    b2u0 += [-1]
    for b in range(66, 70):
        nxt0.append(0)
        b2u0.append(61 + b - 66)
    ibfs = [gf.random_ibf(70, 64, 2, 0.5, 1)]
    nxt, b2u, ub = [nxt0], [b2u0], 65
    for child, bins in ((1, 100), (2, 30), (3, 200)):
        ibfs.append(gf.random_ibf(bins, 32 * child, 2, 0.5, child))
        nxt.append([child] * bins)
        b2u.append(list(range(ub, ub + bins)))
        ub += bins
    return oracle.Hibf(ibfs, nxt, b2u, ub)


def test_hand_made(driver):
    h = hand_made()
    units = hp.units_of(h)
    assert len(units) == 60 + 2 + 1 + 1 + 4 and (62, 65, []) in units
    C = hp.cost_matrix(h, units)
    whole = int(C[0, len(units)])
    cases = [[whole] * 2, [whole // 2 + 4096] * 2, [whole // 2 + 4096] * 3, [whole, 1, whole], [hp.optimum(C, [whole] * 4)] * 4,
             [30000, whole, 30000, whole]]
    got = parse(run(driver, "".join(case_text(h, b) for b in cases)))
    for b, g in zip(cases, got):
        parts = check_plan(h, b, g)
        for p in parts:  # the split user bin 60 (root bins 62..64, over the word boundary) is whole in one part
            assert not (p["bin_lo"] in (63, 64) or p["bin_hi"] in (63, 64))
    assert len(got[0]["parts"]) == 2 and len(got[4]["parts"]) >= 2  # (the largest part as small as possible: two parts even where one would fit)
    assert [p["slot"] for p in got[3]["parts"]] == [0, 2] and [p["slot"] for p in got[5]["parts"]][0] in (0, 1)


def test_refusals(driver):
    h = hand_made()
    units = hp.units_of(h)
    C = hp.cost_matrix(h, units)
    largest = max(int(C[a, a + 1]) for a in range(len(units)))
    cases = [[largest - 1] * 8,  # a unit over every budget
             [0, 0],  # budget 0
             [],  # no device
             [largest, 1]]  # every unit fits the first budget, but no assignment in order does
    assert hp.optimum(C, cases[3]) is None
    got = parse(run(driver, "".join(case_text(h, b) for b in cases)))
    for g in got:
        assert isinstance(g, str) and "does not fit" in g and "cannot be partitioned" in g, g
    big = max(range(len(units)), key=lambda a: int(C[a, a + 1]))
    assert f"the subtree under root bin {units[big][0]} takes" in got[0] and f"({largest} bytes" in got[0]
    assert "no assignment" in got[3]
    # more devices than units: the trailing devices stay empty and unused
    h2 = gf.random_hibf(12, 4, 2, seed=2, hash_funs=2, **tiny())
    u2 = hp.units_of(h2)
    C2 = hp.cost_matrix(h2, u2)
    assert 2 <= len(u2) < 8
    b2 = [max(int(C2[a, a + 1]) for a in range(len(u2)))] * 8
    parts = check_plan(h2, b2, parse(run(driver, case_text(h2, b2)))[0])
    assert 2 <= len(parts) <= len(u2) and all(p["slot"] == i for i, p in enumerate(parts))


def test_random_trees(driver):
    rng = np.random.default_rng(11)
    trees, budgets, text = [], [], []
    for c in range(200):
        n = int(rng.integers(2, 260))
        h = gf.random_hibf(n, int(rng.choice([64, 100, 128, 192])), int(rng.integers(1, 4)), seed=1000 + c, hash_funs=2, **tiny(int(rng.integers(8, 40))))
        if c % 2:
            h, _ = hp.permuted(h, c)
        units = hp.units_of(h)
        C = hp.cost_matrix(h, units)
        k = int(rng.integers(2, 9))
        tight = hp.optimum(C, [np.iinfo(np.int64).max - 1] * k)
        if c % 3 == 0:
            b = [tight] * k  # equal, the tightest that places k parts
        elif c % 3 == 1:
            b = [int(tight * rng.uniform(0.3, 2.0)) for _ in range(k)]  # unequal, some too small for anything
        else:
            b = [int(tight * rng.uniform(1.0, 1.5)) for _ in range(k)]
        trees.append(h)
        budgets.append(b)
        text.append(case_text(h, b))
    got = parse(run(driver, "".join(text)))
    assert len(got) == 200
    n_ok = n_multiword = 0
    for h, b, g in zip(trees, budgets, got):
        if hp.optimum(hp.cost_matrix(h, hp.units_of(h)), b) is None:
            assert isinstance(g, str) and "does not fit" in g and "cannot be partitioned" in g
            continue
        parts = check_plan(h, b, g)
        n_ok += 1
        n_multiword += any(p["bin_lo"] & 63 for p in parts)
    assert n_ok >= 120 and n_multiword >= 20  # (the cases are not all refusals, and cuts inside a word occur)
