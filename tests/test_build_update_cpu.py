"""`ganon-build --hibf --update` without a GPU: the placement of new user bins (ganon_amd/host/hibf_update.hpp) through a driver this
test compiles, against a Python restatement of the rule that uses the same two double expressions in the same order; the tables it
leaves against derive_paths (ganon_amd/host/hibf_paths.hpp) and the tree invariants."""
import math
import os
import subprocess

import numpy as np
import pytest

import hibf_checks as hc

HERE = os.path.dirname(os.path.abspath(__file__))
HOST = os.path.join(HERE, "..", "ganon_amd", "host")
MAX_COUNT, MAX_SPLIT = 1 << 48, 1 << 16


@pytest.fixture(scope="module")
def drivers(tmp_path_factory):
    d = tmp_path_factory.mktemp("hibf_update")
    upd, paths = str(d / "hibf_update_driver"), str(d / "hibf_paths_driver")
    inc = ["-I", os.path.join(HERE, "..", "include")]
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-o", upd, os.path.join(HERE, "hibf_update_driver.cpp"), os.path.join(HOST, "build_params.cpp")] + inc)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-o", paths, os.path.join(HERE, "hibf_paths_driver.cpp")] + inc)
    return upd, paths


# ------------------------------------------------------------------------------------------------------------ the rule, restated
def predict(t, n, m, h):
    return m * (1.0 - (1.0 - float(t) / m) * math.exp(-float(h) * n / m))


def plan(bins, rows, nx, bu, n_user, h, fpr, pop, fresh):
    """-> (bins after, next_ibf_id after, bin_to_user after, path per new user bin as [(ibf, first, n_bins, hashes_per_bin)] leaf
    first, touched as [(ibf, bin, before, predicted)]).  Asserts that no decision is within 1e-9 of the eligibility bound."""
    bins, nx, bu = list(bins), [list(a) for a in nx], [list(a) for a in bu]
    old_bins = list(bins)
    t_now = [[float(x) for x in p] for p in pop]
    touched, at = [], {}
    paths = [None] * len(fresh)
    fits = lambda n, s, i: hc.run_bits(n, s, fpr, h) <= rows[i]
    for k in sorted(range(len(fresh)), key=lambda k: (-fresh[k], k)):
        n, i, down = fresh[k], 0, []
        while True:
            bound = math.pow(fpr, 1.0 / h) * rows[i]
            best = None
            for b in range(old_bins[i]):
                if bu[i][b] >= 0:
                    continue
                fill = predict(t_now[i][b], n, rows[i], h)
                assert abs(fill - bound) > 1e-9 * bound, "a case on the edge: C++ and Python may round apart"
                if fill <= bound and fits(n, 1, nx[i][b]) and (best is None or fill < best[1]):
                    best = (b, fill)
            if best is None:
                break
            b, fill = best
            if (i, b) not in at:
                at[(i, b)] = len(touched)
                touched.append([i, b, pop[i][b], 0.0])
            t_now[i][b] = fill
            touched[at[(i, b)]][3] = fill
            down.append((i, b, 1, 1))
            i = nx[i][b]
        s = 1
        while s <= MAX_SPLIT and s <= n and not fits(n, s, i):
            s += 1
        assert s <= MAX_SPLIT and s <= n
        paths[k] = [(i, bins[i], s, (n + s - 1) // s)] + down[::-1]
        bins[i] += s
        nx[i] += [i] * s
        bu[i] += [n_user + k] * s
    return bins, nx, bu, paths, [tuple(t) for t in touched]


# ------------------------------------------------------------------------------------------------------------ the driver
def update_line(fpr, h, n_user, bins, rows, nx, bu, pop, fresh):
    parts = ["update", repr(fpr), str(h), str(n_user), str(len(bins))]
    for i in range(len(bins)):
        parts += [str(bins[i]), str(rows[i])] + [str(int(x)) for x in nx[i]] + [str(int(x)) for x in bu[i]] + [str(int(x)) for x in pop[i]]
    return " ".join(parts + [str(len(fresh))] + [str(c) for c in fresh]) + "\n"


def parse(text):
    lines = text.splitlines()
    if lines[0].startswith("refused"):
        return None
    head = lines[0].split()
    assert head[0] == "case"
    out = dict(n_ibf=int(head[1]), depth=int(head[2]), n_user=int(head[3]), bins=[], rows=[], nx=[], bu=[], paths={}, touched=[], pop=[], old=[])
    for ln in lines[1:]:
        f = ln.split()
        if f[0] == "table":
            B = int(f[2])
            out["bins"].append(B), out["rows"].append(int(f[3]))
            out["nx"].append([int(x) for x in f[4:4 + B]]), out["bu"].append([int(x) for x in f[4 + B:4 + 2 * B]])
            assert len(f) == 4 + 2 * B
        elif f[0] == "pop":
            out["pop"].append([int(x) for x in f[2:]])
        elif f[0] == "old":
            B = int(f[2])
            out["old"].append((B, [int(x) for x in f[3:3 + B]], [int(x) for x in f[3 + B:3 + 2 * B]]))
        elif f[0] == "path":
            out["paths"].setdefault(int(f[1]), []).append(tuple(int(x) for x in f[3:7]))
        else:
            assert f[0] == "touched"
            out["touched"].append((int(f[1]), int(f[2]), int(f[3]), float(f[4])))
    assert len(out["bins"]) == out["n_ibf"]
    return out


def derive(paths_driver, n_user, bins, nx, bu):
    """derive_paths of the product on tables -> (depth, {user: [(ibf, first, n_bins)] with the unused entries dropped})"""
    parts = ["tables", str(n_user), str(len(bins))]
    for i in range(len(bins)):
        parts += [str(bins[i])] + [str(x) for x in nx[i]] + [str(x) for x in bu[i]]
    text = subprocess.run([paths_driver], input=" ".join(parts) + "\n", capture_output=True, text=True, check=True).stdout
    lines = text.splitlines()
    assert lines[0].startswith("case"), text[:300]
    out = {}
    for ln in lines[1:]:
        f = ln.split()
        if f[0] == "derived" and int(f[5]) != 0:
            out.setdefault(int(f[1]), []).append((int(f[3]), int(f[4]), int(f[5])))
    return int(lines[0].split()[1]), out


def check_case(drivers, fpr, h, n_user, bins, rows, nx, bu, pop, fresh, text=None):
    upd, paths_driver = drivers
    if text is None:
        text = subprocess.run([upd], input=update_line(fpr, h, n_user, bins, rows, nx, bu, pop, fresh), capture_output=True, text=True, check=True).stdout
    got = parse(text)
    assert got is not None, text
    e_bins, e_nx, e_bu, e_paths, e_touched = plan(bins, rows, nx, bu, n_user, h, fpr, pop, fresh)
    assert got["bins"] == e_bins and got["nx"] == e_nx and got["bu"] == e_bu and got["rows"] == list(rows)
    assert got["n_user"] == n_user + len(fresh)
    for k in range(len(fresh)):
        used = [e for e in got["paths"][k] if e[2] != 0]
        assert used == e_paths[k], (k, used, e_paths[k])
        assert len(got["paths"][k]) == got["depth"] and all(e[2] == 0 for e in got["paths"][k][len(used):])
    assert got["touched"] == e_touched  # (the prediction printed with 17 digits: the same double)
    # the tables the plan leaves are what a reader derives the same paths from, and the old user bins stay where they were
    depth_old, before = derive(paths_driver, n_user, bins, nx, bu)
    depth_new, after = derive(paths_driver, n_user + len(fresh), e_bins, e_nx, e_bu)
    assert depth_new == depth_old == got["depth"]
    for u in range(n_user):
        assert after[u] == before[u]
    for k in range(len(fresh)):
        assert after[n_user + k] == [e[:3] for e in e_paths[k]]
    hc.check_tree(e_bins, [np.array(a) for a in e_nx], [np.array(a) for a in e_bu], n_user + len(fresh), max(e_bins), max_levels=depth_old)
    return got, e_paths, e_touched


# ------------------------------------------------------------------------------------------------------------ hand-made trees
FPR, H = 0.05, 4  # one bin is at FPR when pow(0.05, 1/4) = 0.4729 of its rows are set; a set of n needs 6.2472 n rows unsplit


def two_children(t1, t2, child_rows=(6000, 6000), root_rows=10000):
    """root: user bin 0, merged bins 1 and 2 over two leaf IBFs of two user bins each"""
    bins, rows = [3, 2, 2], [root_rows, child_rows[0], child_rows[1]]
    nx, bu = [[0, 1, 2], [1, 1], [2, 2]], [[0, -1, -1], [1, 2], [3, 4]]
    pop = [[900, t1, t2], [500, 600], [700, 800]]
    return 5, bins, rows, nx, bu, pop


def test_leaf_only_tree(drivers):
    got, paths, touched = check_case(drivers, FPR, H, 3, [3], [1000], [[0, 0, 0]], [[0, 1, 2]], [[100, 200, 300]], [50, 160])
    assert not touched and paths[1] == [(0, 3, 1, 160)] and paths[0] == [(0, 4, 1, 50)]  # the larger first, ids by input order


def test_split_run_at_the_root(drivers):
    got, paths, _ = check_case(drivers, FPR, H, 3, [3], [1000], [[0, 0, 0]], [[0, 1, 2]], [[100, 200, 300]], [400])
    (ibf, first, s, share), = paths[0]
    assert (ibf, first) == (0, 3) and s > 1 and share == -(-400 // s)
    assert hc.run_bits(400, s, FPR, H) <= 1000 < hc.run_bits(400, s - 1, FPR, H)


def test_merged_bin_with_room_and_one_without(drivers):
    n_user, *tree = two_children(1000, 4700)
    got, paths, touched = check_case(drivers, FPR, H, n_user, *tree, [500])
    assert paths[0] == [(1, 2, 1, 500), (0, 1, 1, 1)] and [t[:3] for t in touched] == [(0, 1, 1000)]
    n_user, *tree = two_children(4700, 1000)
    got, paths, touched = check_case(drivers, FPR, H, n_user, *tree, [500])
    assert paths[0] == [(2, 2, 1, 500), (0, 2, 1, 1)]
    n_user, *tree = two_children(1000, 900)  # both have room: the lower predicted fill
    assert check_case(drivers, FPR, H, n_user, *tree, [500])[1][0][1] == (0, 2, 1, 1)
    n_user, *tree = two_children(900, 900)  # ... and the lower bin on a tie
    assert check_case(drivers, FPR, H, n_user, *tree, [500])[1][0][1] == (0, 1, 1, 1)


def test_the_first_uses_up_the_room(drivers):
    n_user, *tree = two_children(2000, 4700)
    got, paths, touched = check_case(drivers, FPR, H, n_user, *tree, [700, 800])
    assert paths[1] == [(1, 2, 1, 800), (0, 1, 1, 1)], "800 hashes raise 2000 bits of 10000 to about 4191: below 4729"
    assert paths[0] == [(0, 3, 1, 700)], "another 700 would raise them to about 5610: a new run at the root"
    assert len(touched) == 1 and 4100 < touched[0][3] < 4300


def test_fits_the_fill_but_not_the_child(drivers):
    n_user, *tree = two_children(1000, 4700, child_rows=(2000, 6000))
    got, paths, touched = check_case(drivers, FPR, H, n_user, *tree, [500])
    assert paths[0] == [(0, 3, 1, 500)] and not touched, "500 hashes need 3124 rows unsplit, the child has 2000"


def test_three_level_descent(drivers):
    bins, rows = [2, 2, 2], [20000, 9000, 4000]
    nx, bu = [[0, 1], [1, 2], [2, 2]], [[0, -1], [1, -1], [2, 3]]
    pop = [[3000, 2500], [900, 1200], [300, 400]]
    got, paths, touched = check_case(drivers, FPR, H, 4, bins, rows, nx, bu, pop, [600, 100])
    assert paths[0] == [(2, 2, 1, 600), (1, 1, 1, 1), (0, 1, 1, 1)] and paths[1] == [(2, 3, 1, 100), (1, 1, 1, 1), (0, 1, 1, 1)]
    assert [t[:2] for t in touched] == [(0, 1), (1, 1)] and got["depth"] == 3


def test_equal_counts_and_determinism(drivers):
    n_user, *tree = two_children(1000, 4700)
    line = update_line(FPR, H, n_user, *tree, [300, 300, 300])
    a = subprocess.run([drivers[0]], input=line + line, capture_output=True, text=True, check=True).stdout
    assert a[:len(a) // 2] == a[len(a) // 2:], "same input, same plan"
    got, paths, _ = check_case(drivers, FPR, H, n_user, *tree, [300, 300, 300], text=a[:len(a) // 2])
    assert [p[0][1] for p in paths] == [2, 3, 4] and all(p[0][0] == 1 for p in paths), "input order decides among equal counts"


def lognormal(n, seed):
    rng = np.random.default_rng(seed)
    return [max(1, int(x)) for x in rng.lognormal(mean=8.0, sigma=1.5, size=n)]


@pytest.mark.parametrize("tmax", [2, 4, 8, 64])
@pytest.mark.parametrize("percent", [40, 100])
def test_layouts(drivers, tmax, percent):
    """trees of the builder's own rule, filled to `percent` of the textbook fill, updated with a fifth as many user bins again"""
    n = {2: 11, 4: 40, 8: 150, 64: 300}[tmax]
    counts, fresh = lognormal(n, n + tmax), lognormal(max(3, n // 5), 7 * n + tmax)
    fpr, h = (0.05, 4) if tmax != 8 else (0.001, 3)
    line = " ".join(["layout", repr(fpr), str(h), str(tmax), str(percent), str(n)] + [str(c) for c in counts] + [str(len(fresh))] + [str(c) for c in fresh]) + "\n"
    text = subprocess.run([drivers[0]], input=line, capture_output=True, text=True, check=True).stdout
    got = parse(text)
    assert got is not None, text
    bins, nx, bu = [o[0] for o in got["old"]], [o[1] for o in got["old"]], [o[2] for o in got["old"]]
    assert max(bins) <= tmax
    _, paths, touched = check_case(drivers, fpr, h, n, bins, got["rows"], nx, bu, got["pop"], fresh, text=text)
    deepest = max(len(p) for p in paths)
    print(f"tmax {tmax} at {percent}%: {len(bins)} IBFs, depth {got['depth']}, {len(fresh)} new user bins, {len(touched)} merged bins touched, deepest new path {deepest}, "
          f"root {bins[0]} -> {got['bins'][0]} bins")
    if percent == 40 and tmax < 64:
        assert touched and deepest > 1, "at 40% of the textbook fill some new user bin finds room below the root"


def test_refusals_of_the_rule(drivers):
    n_user, bins, rows, nx, bu, pop = two_children(1000, 4700)

    def refused(**kw):
        a = dict(fpr=FPR, h=H, n_user=n_user, bins=bins, rows=rows, nx=nx, bu=bu, pop=pop, fresh=[500])
        a.update(kw)
        text = subprocess.run([drivers[0]], input=update_line(**a), capture_output=True, text=True, check=True).stdout
        assert text.startswith("refused"), text[:200]
        return text

    assert "HIBF tables" in refused(nx=[[0, 1, 1], [1, 1], [2, 2]])  # two parents: through derive_paths
    assert "HIBF tables" in refused(bu=[[0, -1, -1], [1, 2], [3, 3]])
    assert "distinct hashes" in refused(fresh=[0]) and "distinct hashes" in refused(fresh=[1 << 62])
    assert "bits set" in refused(pop=[[900, 10001, 4700], [500, 600], [700, 800]])
    assert "no rows" in refused(rows=[10000, 0, 6000])
    assert "rebuild" in refused(rows=[1, 1, 1], pop=[[0, 0, 0], [0, 0], [0, 0]])  # rows of 1: no run holds a hash at 0.05
    assert "out of range" in refused(h=6) and "out of range" in refused(fpr=1.0)


# ------------------------------------------------------------------------------------------------------------ the command's refusals
from test_build_cpu import BIN_BUILD  # noqa: E402
from test_build_hibf_cpu import tiny_input  # noqa: E402,F401  (a fixture)
from test_build_verify_cpu import tiny_index  # noqa: E402,F401  (a fixture: k 19, w 32, h 3, fpr 0.05)


@pytest.mark.parametrize("case,words", [
    ("no --hibf", ["--update", "--hibf"]),
    ("no --output-file", ["--update", "--output-file"]),
    ("with --verify-index", ["--update", "--verify-index"]),
    ("with --layout", ["--update", "--layout"]),
    ("with --tmax", ["--update", "--tmax"]),
    ("with --filter-size", ["--update", "--filter-size"]),
    ("with --mode", ["--update", "--mode"]),
    ("missing file", ["--update", "not found", "no_such.hibf"]),
    ("-k differs", ["--update", "--kmer-size", "21", "19"]),
    ("-w differs", ["--update", "--window-size", "35", "32"]),
    ("-s differs", ["--update", "--hash-functions", "4", "3"]),
    ("-p differs", ["--update", "--max-fp", "0.01", "0.05"]),
    ("output is the input", ["--update", "--output-file", "the index itself"]),
])
def test_refusals_of_the_command(tiny_input, tiny_index, case, words):
    assert os.path.exists(BIN_BUILD), "ganon-build is built by __graft_entry__.build()"
    inp, out = tiny_input
    missing = os.path.join(os.path.dirname(tiny_index), "no_such.hibf")
    size = os.path.getsize(tiny_index)
    upd = ["--hibf", "--update", tiny_index, "-o", out]
    args = {"no --hibf": ["--update", tiny_index, "-o", out],
            "no --output-file": ["--hibf", "--update", tiny_index],
            "with --verify-index": upd + ["--verify-index", tiny_index],
            "with --layout": upd + ["--layout", "rule"],
            "with --tmax": upd + ["--tmax", "64"],
            "with --filter-size": upd + ["--filter-size", "1"],
            "with --mode": upd + ["--mode", "avg"],
            "missing file": ["--hibf", "--update", missing, "-o", out],
            "-k differs": upd + ["-k", "21"],
            "-w differs": upd + ["-w", "35"],
            "-s differs": upd + ["-s", "4"],
            "-p differs": upd + ["-p", "0.01"],
            "output is the input": ["--hibf", "--update", tiny_index, "-o", os.path.join(os.path.dirname(tiny_index), ".", "tiny.hibf")]}[case]
    p = subprocess.run([BIN_BUILD, "-i", inp] + args, capture_output=True, text=True)
    assert p.returncode == 1, (p.returncode, p.stderr)
    for w in words:
        assert w in p.stderr, (w, p.stderr)
    assert "device" not in p.stderr.lower(), p.stderr  # refused before the device is touched
    assert p.stdout == "" and not os.path.exists(out) and os.path.getsize(tiny_index) == size
