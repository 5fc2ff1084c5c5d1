"""`ganon-build --hibf --update --fold` without a GPU: the tables after a fold (ganon_amd/host/hibf_fold.hpp) through a driver this test
compiles, against a Python restatement of the rule; the tables it leaves against derive_paths; the paths it rewrites; and the arithmetic
the device's fold is made of (ganon_amd/csrc/gn_fold_table.h: the segment table, the hits of a row and the composition of a destination
word, the very functions the kernel calls) against numpy, under AddressSanitizer and UBSan with buffers of exactly the words there are."""
import os
import subprocess

import numpy as np
import pytest

import ganon_fixtures as gf
import hibf_checks as hc
from test_build_remove_gpu import SRC_BINS
from test_build_update_cpu import derive

HERE = os.path.dirname(os.path.abspath(__file__))
U64 = np.uint64


@pytest.fixture(scope="module")
def drivers(tmp_path_factory):
    d = tmp_path_factory.mktemp("hibf_fold")
    fold, paths = str(d / "hibf_fold_driver"), str(d / "hibf_paths_driver")
    inc = ["-I", os.path.join(HERE, "..", "include")]
    # a stand-alone program: the sanitizers' runtimes are linked in, nothing is preloaded
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", fold,
                           os.path.join(HERE, "hibf_fold_driver.cpp")] + inc)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-o", paths, os.path.join(HERE, "hibf_paths_driver.cpp")] + inc)
    return fold, paths


def run(driver, text):
    p = subprocess.run([driver], input=text, capture_output=True, text=True)
    assert p.returncode == 0 and p.stderr == "", (p.returncode, p.stderr[-3000:])  # (a sanitizer report ends the program with a status)
    return p.stdout


# ------------------------------------------------------------------------------------------------------------ the rule, restated
def runs_in(bu_i):
    """[(first, n)] of the runs of user bins of one IBF"""
    out, b = [], 0
    while b < len(bu_i):
        e = b + 1
        if bu_i[b] >= 0:
            while e < len(bu_i) and bu_i[e] == bu_i[b]:
                e += 1
            out.append((b, e - b))
        b = e
    return out


def or_fill(prod, t, m, first, n):
    for b in range(first, first + n):
        prod *= 1.0 - t[b] / m
    return prod


def groups_of(bu_i, t, m, h, fpr, N):
    """-> (groups [[(first, n)] ascending], predicted bits per group, bins left) of one IBF of more than N bins"""
    keyed = []
    for first, n in runs_in(bu_i):
        key = t[first]
        for b in range(first + 1, first + n):
            key += t[b]
        keyed.append((key, first, n))
    keyed.sort()
    bound = fpr ** (1.0 / h) * m
    groups, predicted, left = [], [], len(bu_i)
    open_, open_bins, open_prod = [], 0, 1.0

    def close():
        nonlocal open_, open_bins, open_prod, left
        if open_bins > 1:
            left -= open_bins - 1
            groups.append(sorted(open_))
            predicted.append(m * (1.0 - open_prod))
        open_, open_bins, open_prod = [], 0, 1.0
    for _, first, n in keyed:
        alone = or_fill(1.0, t, m, first, n)
        if n > N or not m * (1.0 - alone) <= bound:
            break
        both = or_fill(open_prod, t, m, first, n)
        if open_ and (open_bins + n > N or not m * (1.0 - both) <= bound):
            close()
            both = alone
        open_.append((first, n))
        open_bins, open_prod = open_bins + n, both
        if left - (open_bins - 1) <= N:
            break
    close()
    return groups, predicted, left


def plan(bins, rows, nx, bu, h, fpr, fills, N):
    """-> ("unreachable", ibf, bins left) or a dict of everything the driver prints"""
    n_ibf = len(bins)
    out = dict(src=list(range(n_ibf)), bins=[0] * n_ibf, rows=list(rows), nx=[None] * n_ibf, bu=[None] * n_ibf, fills=[None] * n_ibf,
               spans=[None] * n_ibf, groups=[], folded=[], where={})
    for i in range(n_ibf):
        groups, predicted = [], []
        if bins[i] > N:
            groups, predicted, left = groups_of(bu[i][:bins[i]], fills[i], rows[i], h, fpr, N)
            if left > N:
                return ("unreachable", i, left)
            out["folded"].append(i)
        moved = {b for g in groups for first, n in g for b in range(first, first + n)}
        kept = [b for b in range(bins[i]) if b not in moved]
        for to, b in enumerate(kept):
            out["where"][(i, b)] = (i, to, None)
        p_nx, p_bu, p_fill = [nx[i][b] for b in kept], [bu[i][b] for b in kept], [fills[i][b] for b in kept]
        for g, pred in zip(groups, predicted):
            child, merged = len(out["bins"]), len(p_nx)
            members = [b for first, n in g for b in range(first, first + n)]
            for to, b in enumerate(members):
                out["where"][(i, b)] = (child, to, merged)
            out["groups"].append((i, merged, child, len(g), len(members), pred, g))
            p_nx.append(child), p_bu.append(-1), p_fill.append(pred)
            out["src"].append(i), out["bins"].append(len(members)), out["rows"].append(rows[i])
            out["nx"].append([child] * len(members)), out["bu"].append([bu[i][b] for b in members]), out["fills"].append([fills[i][b] for b in members])
            out["spans"].append(spans_of(members))
        out["bins"][i], out["nx"][i], out["bu"][i], out["fills"][i], out["spans"][i] = len(p_nx), p_nx, p_bu, p_fill, spans_of(kept)
    return out


def spans_of(src_bins):
    """the bins of a source, in order, closed up to the left: one span per maximal run"""
    spans = []
    for to, b in enumerate(src_bins):
        if spans and spans[-1][0] + spans[-1][2] == b:
            spans[-1][2] += 1
        else:
            spans.append([b, to, 1])
    return [tuple(s) for s in spans]


def fold_line(h, fpr, N, n_user, bins, rows, nx, bu, fills):
    parts = ["fold", str(h), repr(float(fpr)), str(N), str(n_user), str(len(bins))]
    for i in range(len(bins)):
        parts += [str(bins[i]), str(rows[i])] + [str(int(x)) for x in nx[i]] + [str(int(x)) for x in bu[i]] + [repr(float(x)) for x in fills[i]]
    return " ".join(parts) + "\n"


def parse(text):
    lines = text.splitlines()
    if lines[0].startswith(("refused", "unreachable")):
        return None
    head = lines[0].split()
    assert head[0] == "case"
    out = dict(n_ibf=int(head[1]), depth=int(head[2]), src=[], bins=[], rows=[], nx=[], bu=[], fills=[], spans=[], groups=[], folded=[], paths={})
    for ln in lines[1:]:
        f = ln.split()
        if f[0] == "table":
            v = [int(x) for x in f[1:]]
            B = v[2]
            assert v[0] == len(out["bins"]) and len(v) == 4 + 2 * B
            out["src"].append(v[1]), out["bins"].append(B), out["rows"].append(v[3]), out["nx"].append(v[4:4 + B]), out["bu"].append(v[4 + B:]), out["spans"].append([])
        elif f[0] == "fills":
            out["fills"].append([float(x) for x in f[2:]])
        elif f[0] == "span":
            out["spans"][int(f[1])].append(tuple(int(x) for x in f[2:]))
        elif f[0] == "group":
            r = [int(x) for x in f[7:]]
            out["groups"].append((int(f[1]), int(f[2]), int(f[3]), int(f[4]), int(f[5]), float(f[6]), list(zip(r[0::2], r[1::2]))))
        elif f[0] == "folded":
            out["folded"] = [int(x) for x in f[1:]]
        elif f[0] == "path":
            v = [int(x) for x in f[2:]]
            out["paths"][int(f[1])] = list(zip(v[0::3], v[1::3], v[2::3]))
    assert len(out["bins"]) == out["n_ibf"]
    return out


def check_case(drivers, h, fpr, N, n_user, bins, rows, nx, bu, fills):
    """-> the parsed plan, or ("unreachable", ibf, left) when the driver and the restatement both refuse"""
    fold, paths_driver = drivers
    text = run(fold, fold_line(h, fpr, N, n_user, bins, rows, nx, bu, fills))
    got, exp = parse(text), plan(bins, rows, nx, bu, h, fpr, fills, N)
    if isinstance(exp, tuple):
        _, i, left = exp
        assert got is None and text.startswith("unreachable") and f"IBF {i} has {bins[i]} bins" in text and f"reaches {left} bins, not {N}" in text \
            and "rebuild or give a larger --fold" in text, text[:400]
        return exp
    assert got is not None, text[:400]
    for key in ("src", "bins", "rows", "nx", "bu", "fills", "spans", "groups", "folded"):
        assert got[key] == exp[key], (key, got[key], exp[key])
    # every folded parent and every child is within the bound; nothing else changed
    for i in exp["folded"]:
        assert got["bins"][i] <= N < bins[i]
    for i in range(len(bins), got["n_ibf"]):
        assert 2 <= got["bins"][i] <= N and all(u >= 0 for u in got["bu"][i]) and got["rows"][i] == rows[got["src"][i]]
    for i in range(len(bins)):
        if i not in exp["folded"]:
            assert (got["bins"][i], got["nx"][i], got["bu"][i], got["spans"][i]) == (bins[i], nx[i][:bins[i]], bu[i][:bins[i]], [(0, 0, bins[i])])
    # what a reader derives from the new tables: every user bin's old path under the map, the merged entry above a folded run
    depth_old, before = derive(paths_driver, n_user, bins, nx, bu)
    depth_new, after = derive(paths_driver, n_user, got["bins"], got["nx"], got["bu"])
    assert depth_new == got["depth"] and depth_old <= depth_new <= depth_old + 1 and sorted(after) == list(range(n_user)), "user bin ids are unchanged"
    for u in range(n_user):
        want = []
        for d, (i, first, n) in enumerate(before[u]):
            ni, nb, merged = exp["where"][(i, first)]
            want.append((ni, nb, n))
            if merged is not None:
                assert d == 0, "only a run of user bins moves"
                want.append((i, merged, 1))
        assert after[u] == want and got["paths"][u] == want, (u, after[u], got["paths"][u], want)
    hc.check_tree(got["bins"], [np.array(a) for a in got["nx"]], [np.array(a) for a in got["bu"]], n_user, max(got["bins"]), max_levels=depth_old + 1)
    return got


# ------------------------------------------------------------------------------------------------------------ hand-made trees
def wide_root(last=100.0):
    """IBF 0: user bins 0..5 (one bin each), user bin 6 (3 bins), merged -> 1.  IBF 1: user bins 7, 8.  1000 rows, h 3, fpr 0.05: the
    merged-bin bound is 368.4 bits.  User bins 1 and 6 tie at 60 bits: the lower bin first."""
    bins, rows = [10, 2], [1000, 700]
    nx, bu = [[0] * 9 + [1], [1, 1]], [[0, 1, 2, 3, 4, 5, 6, 6, 6, -1], [7, 8]]
    fills = [[50.0, 60.0, 70.0, 80.0, 90.0, last, 20.0, 20.0, 20.0, 300.0], [100.0, 120.0]]
    return 9, bins, rows, nx, bu, fills


def test_exactly_reachable_with_a_run_of_several_bins(drivers):
    n_user, *tree = wide_root()
    got = check_case(drivers, 3, 0.05, 4, n_user, *tree)
    assert got["folded"] == [0] and got["bins"] == [4, 2, 2, 4, 3], "the root lands on exactly 4 bins; IBF 1 had 2 and is untouched"
    assert [g[6] for g in got["groups"]] == [[(0, 1), (1, 1)], [(2, 1), (6, 3)], [(3, 1), (4, 1), (5, 1)]]
    assert got["bu"][0] == [-1, -1, -1, -1] and got["nx"][0] == [1, 2, 3, 4] and got["bu"][3] == [2, 6, 6, 6]
    assert got["spans"][3] == [(2, 0, 1), (6, 1, 3)] and got["spans"][0] == [(9, 0, 1)] and got["spans"][4] == [(3, 0, 3)]
    assert got["paths"][6] == [(3, 1, 3), (0, 2, 1)] and got["paths"][7] == [(1, 0, 1), (0, 0, 1)]
    assert abs(got["groups"][0][5] - 1000 * (1 - 0.95 * 0.94)) < 1e-9 and got["fills"][0][1] == got["groups"][0][5]


def test_one_below_reachable_is_refused(drivers):
    n_user, *tree = wide_root()
    assert check_case(drivers, 3, 0.05, 3, n_user, *tree) == ("unreachable", 0, 5)


def test_a_run_over_the_bound_alone_ends_the_candidates(drivers):
    n_user, *tree = wide_root(last=400.0)
    assert check_case(drivers, 3, 0.05, 4, n_user, *tree) == ("unreachable", 0, 5), "user bin 5 cannot be folded: the root stays at 5"
    got = check_case(drivers, 3, 0.05, 5, n_user, *tree)
    assert got["bins"][0] == 5 and 5 in got["bu"][0], "it stays in the root"


def test_merged_bins_only(drivers):
    bins, rows = [3, 1, 1, 1], [500] * 4
    nx, bu = [[1, 2, 3], [1], [2], [3]], [[-1, -1, -1], [0], [1], [2]]
    fills = [[10.0, 10.0, 10.0], [5.0], [5.0], [5.0]]
    assert check_case(drivers, 3, 0.05, 2, 3, bins, rows, nx, bu, fills) == ("unreachable", 0, 3)
    got = check_case(drivers, 3, 0.05, 3, 3, bins, rows, nx, bu, fills)
    assert got["folded"] == [] and got["groups"] == [] and got["depth"] == 2


def test_folding_the_output_again(drivers):
    n_user, *tree = wide_root()
    once = check_case(drivers, 3, 0.05, 5, n_user, *tree)
    assert once["bins"][0] == 5
    again = check_case(drivers, 3, 0.05, 5, n_user, once["bins"], once["rows"], once["nx"], once["bu"], once["fills"])
    assert again["folded"] == [] and (again["bins"], again["nx"], again["bu"]) == (once["bins"], once["nx"], once["bu"]), "within the bound: nothing to do"
    # a lower bound: the children are folded in their turn (their runs are user bins), the root's merged bins are not
    lower = check_case(drivers, 3, 0.05, 4, n_user, once["bins"], once["rows"], once["nx"], once["bu"], once["fills"])
    assert lower["folded"] == [0, 2] and lower["depth"] == 3 and max(lower["bins"]) == 4


def test_refusals_of_the_rule(drivers):
    n_user, bins, rows, nx, bu, fills = wide_root()
    for line, word in ((fold_line(3, 0.05, 1, n_user, bins, rows, nx, bu, fills), "at least 2"),
                       (fold_line(3, 0.05, 4, n_user, bins, rows, [[0] * 9 + [0], [1, 1]], bu, fills), "HIBF tables"),
                       (fold_line(3, 0.05, 4, n_user, bins, rows, nx, bu, [fills[0][:9] + [1001.0], fills[1]]), "a fill of"),
                       (fold_line(6, 0.05, 4, n_user, bins, rows, nx, bu, fills), "hash functions"),
                       (fold_line(3, 0.05, 4, n_user, bins, [1000, 0], nx, bu, fills), "no rows")):
        text = run(drivers[0], line)
        assert text.startswith("refused") and word in text, text


@pytest.mark.parametrize("seed", range(25))
def test_random_trees(drivers, seed):
    """a random tree whose root an update has widened by runs of new user bins, at eight bounds and fill scales: 200 cases"""
    rng = np.random.default_rng(seed)
    n_user, depth = int(rng.integers(5, 41)), int(rng.integers(1, 4))
    hb = gf.random_hibf(n_user, int(rng.integers(4, 10)), depth, seed=seed, density=0.0, rows=(300, 900))
    bins, rows = [f.bins for f in hb.ibfs], [f.bin_size for f in hb.ibfs]
    nx, bu = [list(map(int, a[:b])) for a, b in zip(hb.next_ibf_id, bins)], [list(map(int, a[:b])) for a, b in zip(hb.bin_to_user, bins)]
    for _ in range(int(rng.integers(3, 30))):  # the update's runs, at the end of the root
        n = int(rng.choice([1, 1, 1, 2, 3]))
        nx[0] += [0] * n
        bu[0] += [n_user] * n
        bins[0] += n
        n_user += 1
    folded = refused = 0
    for k in range(8):
        scale = (0.02, 0.1, 0.3, 0.9)[k % 4]
        fills = [[float(x) if k < 4 else float(x) + 0.37 for x in rng.integers(0, int(rows[i] * scale) + 1, size=bins[i])] for i in range(len(bins))]
        N = int(rng.integers(2, max(bins) + 2))
        got = check_case(drivers, 3, 0.05, N, n_user, bins, rows, nx, bu, fills)
        if isinstance(got, tuple):
            refused += 1
            continue
        folded += len(got["groups"])
        again = check_case(drivers, 3, 0.05, N, n_user, got["bins"], got["rows"], got["nx"], got["bu"], got["fills"])  # legal, and nothing to do
        assert again["groups"] == []
        if N > 2:
            check_case(drivers, 3, 0.05, N - 1, n_user, got["bins"], got["rows"], got["nx"], got["bu"], got["fills"])  # a plan or a refusal, as restated
    print(f"seed {seed}: {n_user} user bins, {len(bins)} IBFs of up to {max(bins)} bins: {folded} groups, {refused} of 8 refused")


# ------------------------------------------------------------------------------------------------------------ the rows
def member_cases(B):
    """{name: (n_groups, [(src_first, n_bins, group)])} for a source of B bins"""
    def spread(G, skip):
        w = B // G
        return G, [(k * w, max(w - skip, 1), (k * 7) % G) for k in range(G)]  # (7 has no factor in common with 64, 65 or 130: a permutation)
    cases = {"one group of everything": (1, [(0, B, 0)]), "every bin a group of its own": (B, [(b, 1, B - 1 - b) for b in range(B)])}
    if B >= 2:
        cases["alternating members"] = (2, [(b, 1, b & 1) for b in range(B)])
        cases["one bin of the last word"] = (1, [(B - 1, 1, 0)])
    if B > 130:
        cases["a member across a word boundary"] = (2, [(3, 2, 1), (60, 11, 0), (127, 2, 1)])
    for G in (64, 65, 130):
        if B >= G:
            cases[f"{G} groups"] = spread(G, 0)
        if B >= 2 * G:
            cases[f"{G} groups with gaps"] = spread(G, 1)
    return cases


def fold_np(dst, src, n_groups, dst_first, members):
    """numpy: the destination rows [rows, W_dst] after the fold of the source rows [rows, W_src]"""
    bits = np.unpackbits(np.ascontiguousarray(src).view(np.uint8), axis=1, bitorder="little")
    out = np.unpackbits(np.ascontiguousarray(dst).view(np.uint8), axis=1, bitorder="little").copy()
    for first, n, g in members:
        out[:, dst_first + g] |= bits[:, first:first + n].any(axis=1).astype(np.uint8)
    return np.packbits(out, axis=1, bitorder="little").view(U64).reshape(dst.shape)


def rows_line(src, dst, bins_src, bins_dst, dst_first, n_groups, members):
    parts = ["rows", str(src.shape[0]), str(bins_src), str(bins_dst), str(dst.shape[1]), str(dst_first), str(n_groups), str(len(members))] + [f"{s} {n} {g}" for s, n, g in members]
    return " ".join(parts + [format(int(x), "x") for x in src.reshape(-1)] + [format(int(x), "x") for x in dst.reshape(-1)]) + "\n"


def compose(driver, src, dst, bins_src, bins_dst, dst_first, n_groups, members):
    lines = run(driver, rows_line(src, dst, bins_src, bins_dst, dst_first, n_groups, members)).splitlines()
    assert not lines[0].startswith("refused"), lines[0]
    assert len(lines) == src.shape[0] + 1 and lines[-1].startswith("segments ")
    return np.array([[int(x, 16) for x in ln.split()] for ln in lines[:-1]], dtype=U64).reshape(dst.shape), int(lines[-1].split()[1])


@pytest.mark.parametrize("B", SRC_BINS + (64 * 70,))
def test_rows(drivers, B):
    rng = np.random.default_rng(B)
    W = (B + 63) >> 6
    src = rng.integers(0, 1 << 64, size=(5, W), dtype=U64) & rng.integers(0, 1 << 64, size=(5, W), dtype=U64) & rng.integers(0, 1 << 64, size=(5, W), dtype=U64)
    src[0] = 0  # (a row without a bit; the padding bins of the last word are set in the others: they must not travel)
    src[1] = ~U64(0)
    for name, (G, members) in member_cases(B).items():
        for dst_first in (0, 63, 64):
            for extra in (0, 70):
                bins_dst = dst_first + G + extra
                dst = rng.integers(0, 1 << 64, size=(5, (bins_dst + 63) >> 6), dtype=U64) & rng.integers(0, 1 << 64, size=(5, (bins_dst + 63) >> 6), dtype=U64)
                got, n_seg = compose(drivers[0], src, dst, B, bins_dst, dst_first, G, members)
                assert np.array_equal(got, fold_np(dst, src, G, dst_first, members)), (name, B, dst_first, bins_dst)
        if name == "one group of everything":
            assert n_seg == W, "a group's bins of one word are one segment"
        if name == "alternating members":
            assert n_seg == B, "neighbouring members of different groups stay apart"


def test_row_refusals(drivers):
    src, dst = np.zeros((1, 2), dtype=U64), np.zeros((1, 2), dtype=U64)
    for G, dst_first, members, word in ((1, 0, [(0, 0, 0)], "0 bins"), (1, 0, [(60, 11, 0)], "beyond the source"), (2, 99, [(0, 1, 0), (1, 1, 1)], "beyond the destination"),
                                        (1, 0, [(0, 10, 0), (9, 5, 0)], "overlap"), (1, 0, [(20, 10, 0), (0, 5, 0)], "ascend"), (1, 0, [(0, 1, 1)], "at or beyond the number of groups"),
                                        (2, 0, [(0, 5, 1)], "without a member")):
        text = run(drivers[0], rows_line(src, dst, 70, 100, dst_first, G, members))
        assert text.startswith("refused") and word in text, (members, text)


# ------------------------------------------------------------------------------------------------------------ the command's refusals
from test_build_cpu import BIN_BUILD  # noqa: E402
from test_build_hibf_cpu import tiny_input  # noqa: E402,F401  (a fixture)
from test_build_verify_cpu import tiny_index  # noqa: E402,F401  (a fixture)


def test_fold_refusals_that_need_no_device(tiny_input, tiny_index, tmp_path):
    inp, out = tiny_input
    for args, word in ((["-i", inp, "--hibf", "-o", out, "--fold", "8"], "--fold needs --update"),
                       (["--hibf", "--update", tiny_index, "-o", out, "--fold", "1"], "--fold has to be >= 2"),
                       (["--hibf", "--update", tiny_index, "-o", out, "--fold", "x"], "failed to parse"),
                       (["--hibf", "--verify-index", tiny_index, "-i", inp, "--fold", "8"], "--fold cannot be used with --verify-index"),
                       (["--hibf", "--update", tiny_index, "-o", out, "--tmax", "8", "-i", inp], "--update cannot be used with --tmax")):
        p = subprocess.run([BIN_BUILD] + args, capture_output=True, text=True)
        assert p.returncode == 1 and word in p.stderr and p.stdout == "" and not os.path.exists(out), (args, p.stderr)
    p = subprocess.run([BIN_BUILD, "--help"], capture_output=True, text=True)
    assert "--fold arg" in p.stdout + p.stderr
