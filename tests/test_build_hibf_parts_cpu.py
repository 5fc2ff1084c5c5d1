"""`ganon-build --hibf` in parts, without a GPU: the plan (ganon_amd/host/hibf_build_parts.hpp) against a Python restatement of its rule and
its four properties on random trees; the path compaction; the item builder and the arithmetic of the windowed path insert
(ganon_amd/csrc/gn_path_window.h with gn_emplace_window.h, the very functions the kernel and its host call) on a host model of the kernel
against oracle.Ibf; and the command's refusals.  The driver is a stand-alone program under AddressSanitizer and UBSan with buffers of exactly
the words there are; nothing is preloaded."""
import os
import subprocess

import numpy as np
import pytest

import oracle
from test_build_cpu import BIN_BUILD
from test_build_hibf_cpu import tiny_input  # noqa: F401  (a fixture)
from test_build_verify_cpu import tiny_index  # noqa: F401  (a fixture)

HERE = os.path.dirname(os.path.abspath(__file__))
U64 = np.uint64


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("build_hibf_parts") / "build_hibf_parts_driver")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                           os.path.join(HERE, "build_hibf_parts_driver.cpp"), "-I", os.path.join(HERE, "..", "include")])
    return exe


def run(driver, text):
    p = subprocess.run([driver], input=text, capture_output=True, text=True)
    assert p.returncode == 0 and p.stderr == "", (p.returncode, p.stderr[-3000:])  # (a sanitizer report ends the program with a status)
    return p.stdout


# ------------------------------------------------------------------------------------------------------------ the plan
def plan_rule(ibfs, budget, n_devices):
    """the rule of the plan, restated.  ibfs: (rows, device bytes a row) in file order.  Returns ("refused", ibf) or a list of groups in
    part order: ("whole", [(ibf, 0, rows) ...]) is one part, ("cut", ibf, P, r) stands for P parts of one piece (ibf, j * r, min(r, rows - j * r))"""
    groups, cur, left = [], [], budget
    for i, (rows, rb) in enumerate(ibfs):
        need = rows * rb
        if need <= left:
            cur.append((i, 0, rows))
            left -= need
        elif need <= budget:
            groups.append(("whole", cur))
            cur, left = [(i, 0, rows)], budget - need
        else:
            if cur:
                groups.append(("whole", cur))
            per = budget // rb
            if per == 0:
                return ("refused", i)
            P = -(-rows // per)
            groups.append(("cut", i, P, -(-rows // P)))
            cur, left = [], budget
    if cur:
        groups.append(("whole", cur))
    return groups


def n_parts_of(groups):
    return sum(1 if g[0] == "whole" else g[2] for g in groups)


def parts_of(groups, ibfs):
    """every part of a plan as its list of pieces (only where the parts are few enough to list)"""
    out = []
    for g in groups:
        if g[0] == "whole":
            out.append(g[1])
        else:
            _, i, P, r = g
            out += [[(i, j * r, min(r, ibfs[i][0] - j * r))] for j in range(P)]
    return out


def plan_line(ibfs, budget, n_devices, asked=()):
    return f"plan {budget} {n_devices} {len(ibfs)} " + " ".join(f"{r} {b}" for r, b in ibfs) + "".join(f" {p}" for p in asked) + "\n"


def parse_plan(text):
    lines = text.splitlines()
    assert lines[0].split()[0] == "plan", text[:300]
    parts = {}
    for f in (ln.split() for ln in lines[1:]):
        assert f[0] == "piece"
        parts.setdefault(int(f[1]), (int(f[2]), []))[1].append((int(f[3]), int(f[4]), int(f[5])))
    return int(lines[0].split()[1]), parts


def check_plan(driver, ibfs, budget, n_devices, what=""):
    exp = plan_rule(ibfs, budget, n_devices)
    assert exp[0] != "refused", what
    n, got = parse_plan(run(driver, plan_line(ibfs, budget, n_devices)))
    want = parts_of(exp, ibfs)
    assert n == len(want) == n_parts_of(exp), (what, n, len(want))
    assert sorted(got) == list(range(n)), "no empty part"
    for p, pieces in enumerate(want):
        assert got[p] == (p % n_devices, pieces), (what, p, got[p], pieces)
    return want


@pytest.mark.parametrize("n_devices", [1, 2, 3])
def test_plan_cases(driver, n_devices):
    rb = 32  # 130 bins: three words, padded to four on the device
    a, b, c = (1000, rb), (300, 8), (700, 16)
    whole = lambda t: sum(r * w for r, w in t)  # noqa: E731
    cases = [("one IBF", [a], whole([a])), ("one IBF under twice its bytes", [a], 2 * whole([a])),
             ("every IBF whole in one part", [a, b, c], whole([a, b, c])),
             ("every IBF alone", [a, (600, rb), (900, rb)], 1000 * rb),  # (each over half the budget)
             ("an IBF of exactly the budget", [b, a, c], 1000 * rb),
             ("an IBF one byte over the budget", [b, a, c], 1000 * rb - 1),
             ("an IBF over the budget between two that fit", [b, (5000, rb), c], 700 * 16),
             ("budgets of one row", [b, a, c], rb), ("a budget of one row of every IBF", [(3, 8), (2, 8), (1, 8)], 8)]
    for what, ibfs, budget in cases:
        parts = check_plan(driver, ibfs, budget, n_devices, what)
        if what == "every IBF whole in one part":
            assert parts == [[(0, 0, 1000), (1, 0, 300), (2, 0, 700)]]
        if what == "every IBF alone":
            assert parts == [[(0, 0, 1000)], [(1, 0, 600)], [(2, 0, 900)]]
        if what == "an IBF of exactly the budget":
            assert parts == [[(0, 0, 300)], [(1, 0, 1000)], [(2, 0, 700)]]
        if what == "an IBF one byte over the budget":
            assert parts == [[(0, 0, 300)], [(1, 0, 500)], [(1, 500, 500)], [(2, 0, 700)]], "two slabs, never more than needed"
        if what == "an IBF over the budget between two that fit":
            assert parts[0] == [(0, 0, 300)] and parts[-1] == [(2, 0, 700)] and len(parts) == 2 + 15 and parts[1] == [(1, 0, 334)]
        if what == "budgets of one row":
            assert len(parts) == 300 // 4 + 1000 + 700 // 2 and parts[0] == [(0, 0, 4)]


@pytest.mark.parametrize("n_devices", [1, 2, 3])
def test_plan_of_the_largest_ibf_under_a_budget_of_one_row(driver, n_devices):
    big = 2**32 - 1
    ibfs = [(10, 8), (big, 24), (10, 8)]
    exp = plan_rule(ibfs, 80, n_devices)  # three rows of the large one fit
    assert exp == [("whole", [(0, 0, 10)]), ("cut", 1, -(-big // 3), 3), ("whole", [(2, 0, 10)])]
    P = exp[1][2]
    asked = [0, 1, 2, P // 2, P - 1, P, P + 1]
    n, got = parse_plan(run(driver, plan_line(ibfs, 80, n_devices, asked)))
    assert n == P + 2
    assert got[0] == (0, [(0, 0, 10)]) and got[P + 1] == ((P + 1) % n_devices, [(2, 0, 10)])
    for p in (1, 2, P // 2, P - 1, P):
        j = p - 1
        assert got[p] == (p % n_devices, [(1, 3 * j, min(3, big - 3 * j))]), p
    assert got[P][1][0][1] + got[P][1][0][2] == big, "the last slab ends the IBF"
    # one row: as many parts as rows
    n, got = parse_plan(run(driver, plan_line([(big, 24)], 24, n_devices, [0, big - 1])))
    assert n == big and got[0] == (0, [(0, 0, 1)]) and got[big - 1] == ((big - 1) % n_devices, [(0, big - 1, 1)])


def test_plan_refuses_when_not_one_row_fits(driver):
    text = run(driver, plan_line([(300, 8), (1000, 32), (700, 16)], 31, 2))
    assert plan_rule([(300, 8), (1000, 32), (700, 16)], 31, 2) == ("refused", 1)
    assert text.startswith("refused") and "IBF 1" in text and "32 bytes" in text and " 31 " in text and "not one row fits" in text, text


@pytest.mark.parametrize("seed", [1, 2, 3, 4, 5, 6])
def test_plan_properties_on_random_trees(driver, seed):
    rng = np.random.default_rng(seed)
    ibfs = [(int(rng.integers(1, 4000)), 8 * int(rng.choice([1, 2, 4, 8, 16, 32]))) for _ in range(int(rng.integers(1, 40)))]
    largest = max(r * b for r, b in ibfs)
    for budget in (max(b for _, b in ibfs), largest // 7 + 1, largest - 1, largest, 3 * largest, sum(r * b for r, b in ibfs)):
        for n_devices in (1, 3):
            parts = check_plan(driver, ibfs, budget, n_devices, (seed, budget))
            assert all(parts) and all(n >= 1 for pc in parts for _, _, n in pc), "no empty part, no empty piece"
            assert all(sum(n * ibfs[i][1] for i, _, n in pc) <= budget for pc in parts), "no part holds more than the budget"
            covered = {}
            for pc in parts:
                assert len({i for i, _, _ in pc}) == len(pc), "an IBF is in a part once"
                for i, a, n in pc:
                    covered.setdefault(i, []).append((a, a + n))
            assert sorted(covered) == list(range(len(ibfs)))
            for i, spans in covered.items():
                spans.sort()
                assert spans[0][0] == 0 and spans[-1][1] == ibfs[i][0] and all(x[1] == y[0] for x, y in zip(spans, spans[1:])), \
                    "every row of every IBF lies in exactly one piece"
                per = budget // ibfs[i][1]
                assert len(spans) == 1 if ibfs[i][0] <= per else (len(spans) - 1) * per < ibfs[i][0], "never more slabs of an IBF than needed"
            order = [(i, a) for pc in parts for i, a, _ in pc]
            assert order == sorted(order), "file order"


# ------------------------------------------------------------------------------------------------------------ the paths
@pytest.mark.parametrize("depth", [1, 2, 3, 4])
def test_path_compaction(driver, depth):
    rng = np.random.default_rng(depth)
    n_ibf = 9
    for used in range(0, depth + 1):  # used entries; the rest end the path
        ibf_of = [int(x) for x in rng.permutation(n_ibf)[:used]]
        path = [(ibf_of[d], 3 + d, 5 if d == 0 else 1, 77 if d == 0 else 1) for d in range(used)] + [(0, 0, 0, 0)] * (depth - used)
        for held in ([], ibf_of, ibf_of[::2], ibf_of[1:], [i for i in range(n_ibf) if i not in ibf_of], list(range(n_ibf))):
            held = sorted(set(held))
            local = [held.index(i) if i in held else -1 for i in range(n_ibf)]
            text = run(driver, f"compact {depth} {n_ibf} " + " ".join(map(str, local)) + " " + " ".join(" ".join(map(str, e)) for e in path) + "\n")
            lines = [ln.split() for ln in text.splitlines()]
            want = [(local[i], f, n, per) for i, f, n, per in path[:used] if local[i] >= 0]
            assert lines[0] == ["kept", str(len(want))], (path, held, text)
            got = [tuple(int(x) for x in f[1:]) for f in lines[1:]]
            assert len(got) == depth and got[:len(want)] == want, "the entries of the part's IBFs in their order, renumbered to the part's filter"
            assert all(e == (0, 0, 0, 0) for e in got[len(want):]), "ended with n_bins = 0"


# ------------------------------------------------------------------------------------------------------------ the items
def test_items_of_a_set_longer_than_a_chunk(driver):
    sizes = [0, 1300, 0, 64]
    chunks = []
    for ln in run(driver, "items 700 1048576 4 " + " ".join(map(str, sizes)) + "\n").splitlines():
        f = ln.split()
        if f[0] == "chunk":
            chunks.append((int(f[1]), []))
        else:
            chunks[-1][1].append(tuple(int(x) for x in f[1:]))
    assert [t for t, _ in chunks] == [700, 664]
    seen = [np.zeros(n, dtype=np.int64) for n in sizes]
    for taken, items in chunks:
        at = 0
        for s, cnt, begin, stage_at in items:
            assert 1 <= cnt <= 512 and begin + cnt <= sizes[s] and stage_at == at
            seen[s][begin:begin + cnt] += 1
            at += cnt
        assert at == taken
    assert all((x == 1).all() for x in seen), "every hash of every set is in exactly one item"
    assert chunks[0][1] == [(1, 512, 0, 0), (1, 188, 512, 512)]
    assert chunks[1][1][0] == (1, 512, 700, 0) and chunks[1][1][1] == (1, 88, 1212, 512), "the later items carry the index in the SET"


# ------------------------------------------------------------------------------------------------------------ the kernel's model
# IBF 0 is the root: 1000 rows of 130 bins, cut into pieces; IBFs 1 .. 3 are whole: 5, 64 and 65 bins
MODEL_IBFS = [(130, 1000), (5, 300), (64, 257), (65, 123)]
CUTS = [0, 1, 7, 512, 999, 1000]
SET_SIZES = (0, 1, 64, 513, 1300, 700)


def model_inputs(seed=11):
    """(sets, paths): paths[s] = up to two entries (ibf, first_bin, n_bins, per_bin); per_bin of a single bin is 1, as the library resolves it"""
    rng = np.random.default_rng(seed)
    sets = [np.unique(rng.integers(0, 1 << 62, size=n, dtype=U64)) for n in SET_SIZES]
    sets = [s if len(s) == n else np.arange(n, dtype=U64) * U64(977) for s, n in zip(sets, SET_SIZES)]
    sets[3][0] = 0  # the value 0 among the hashes
    paths = [[(1, 0, 1, 1), (0, 3, 1, 1)],            # an empty set
             [(1, 4, 1, 1), (0, 3, 1, 1)],            # one hash: bin 4 of 5, below merged bin 3 of the root
             [(2, 60, 4, 16), (0, 64, 1, 1)],         # 64 hashes at 16 a bin: bins 60 .. 63 of 64, the last word's last bit
             [(3, 54, 11, 47), (0, 129, 1, 1)],       # 513 at 47 a bin: bins 54 .. 64 of 65, over a word boundary; the root's last bin
             [(0, 126, 3, 600), (0, 0, 0, 0)],        # 1300 at 600 a bin in the root itself: bins 126 .. 128, a path of one entry
             [(3, 0, 2, 350), (0, 129, 1, 1)]]        # 700 at 350 a bin
    return sets, paths


def model_oracle(sets, paths, h):
    refs = [oracle.Ibf(b, r, h) for b, r in MODEL_IBFS]
    for s, path in zip(sets, paths):
        for ibf, first, n, per in path:
            if n and len(s):
                refs[ibf].emplace_many(s, (first + (np.arange(len(s)) // per if n > 1 else np.zeros(len(s), np.int64))).astype(np.uint32))
    return [r.data for r in refs]


def window_line(h, cap, pieces, sets, paths):
    """pieces: per IBF of the model's filter (tree ibf, row_begin, n_rows); the paths are compacted to them as the builder does"""
    local = {t: j for j, (t, _, _) in enumerate(pieces)}
    parts = ["window", str(h), str(cap), str(len(pieces))]
    for t, a, n in pieces:
        parts += [str(MODEL_IBFS[t][0]), str(MODEL_IBFS[t][1]), str(a), str(n)]
    taken = [(s, [e for e in p if e[2] and e[0] in local]) for s, p in zip(sets, paths)]
    taken = [(s, p) for s, p in taken if p]
    parts += ["2", str(len(taken))]
    for s, p in taken:
        for ibf, first, n, per in p + [(0, 0, 0, 0)] * (2 - len(p)):
            parts += [str(local.get(ibf, 0)), str(first), str(n), str(per)]
        parts += [str(len(s))] + [format(int(x), "x") for x in s]
    return " ".join(parts) + "\n"


def parse_window(text, pieces):
    assert not text.startswith("refused"), text
    out, lines = [], text.splitlines()
    at = 0
    for j, (t, a, n) in enumerate(pieces):
        assert lines[at] == f"ibf {j}"
        W = (MODEL_IBFS[t][0] + 63) // 64
        out.append(np.array([[int(x, 16) for x in ln.split()] for ln in lines[at + 1:at + 1 + n]], dtype=U64).reshape(n, W))
        at += 1 + n
    assert at == len(lines)
    return out


@pytest.mark.parametrize("cap", [700, 1 << 20])
def test_window_model_equals_the_oracle(driver, cap):
    h = 5
    sets, paths = model_inputs()
    ref = model_oracle(sets, paths, h)
    assert all(r.any() for r in ref)
    root = []
    for a, b in zip(CUTS, CUTS[1:]):  # a piece of the root with the three others whole
        pieces = [(0, a, b - a), (1, 0, 300), (2, 0, 257), (3, 0, 123)]
        got = parse_window(run(driver, window_line(h, cap, pieces, sets, paths)), pieces)
        root.append(got[0])
        for t in (1, 2, 3):
            assert np.array_equal(got[t], ref[t]), f"IBF {t} whole beside rows [{a}, {b}) of the root"
    assert np.array_equal(np.concatenate(root), ref[0]), "the pieces behind each other are the root"
    for t in range(4):  # every IBF alone, its paths compacted to it
        pieces = [(t, 0, MODEL_IBFS[t][1])]
        assert np.array_equal(parse_window(run(driver, window_line(h, cap, pieces, sets, paths)), pieces)[0], ref[t]), f"IBF {t} alone"
    assert not (ref[0][:, 2] >> U64(130 - 128)).any() and not (ref[3][:, 1] >> U64(1)).any(), "the padding bits of the last word stay zero"


# ------------------------------------------------------------------------------------------------------------ the command's refusals
def test_refusals_that_need_no_device(tiny_input, tiny_index, tmp_path):
    inp, out = tiny_input
    flat = str(tmp_path / "x.ibf")
    for args, word in ((["-i", inp, "-o", flat, "--hibf-memory", "1000"], "--hibf-memory needs --hibf"),
                       (["-i", inp, "-o", flat, "--hibf-devices", "0,0"], "--hibf-devices needs --hibf"),
                       (["-i", inp, "--hibf", "--update", tiny_index, "-o", out, "--hibf-memory", "1000"], "--hibf-memory cannot be used with --update"),
                       (["-i", inp, "--hibf", "--update", tiny_index, "-o", out, "--hibf-devices", "0,0"], "--hibf-devices cannot be used with --update"),
                       (["-i", inp, "--hibf", "--verify-index", tiny_index, "--hibf-memory", "1000"], "--hibf-memory cannot be used with --verify-index"),
                       (["-i", inp, "--hibf", "--verify-index", tiny_index, "--hibf-devices", "0"], "--hibf-devices cannot be used with --verify-index"),
                       (["-i", inp, "--hibf", "-o", out, "--hibf-memory", "0"], "--hibf-memory has to be > 0"),
                       (["-i", inp, "--hibf", "-o", out, "--hibf-memory", "-5"], "failed to parse"),
                       (["-i", inp, "--hibf", "-o", out, "--hibf-memory", "1k"], "failed to parse"),
                       (["-i", inp, "--hibf", "-o", out, "--hibf-devices", "0,"], "failed to parse"),
                       (["-i", inp, "--hibf", "-o", out, "--hibf-devices", "0,,1"], "failed to parse"),
                       (["-i", inp, "--hibf", "-o", out, "--hibf-devices", "a"], "failed to parse")):
        p = subprocess.run([BIN_BUILD] + args, capture_output=True, text=True)
        assert p.returncode == 1 and word in p.stderr and p.stdout == "" and not os.path.exists(out) and not os.path.exists(flat), (args, p.stderr)
    p = subprocess.run([BIN_BUILD, "--help"], capture_output=True, text=True)
    assert "--hibf-memory arg" in p.stderr and "--hibf-devices arg" in p.stderr and "Two families" in p.stderr
