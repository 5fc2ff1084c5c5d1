"""`ganon-build --hibf --verify-index` without a GPU: the paths derived from an index's tables (ganon_amd/host/hibf_paths.hpp) through
a driver this test compiles -- against the paths the builder inserts along, and against hand-made tables that must be refused -- and
the command line's refusals, which come before any device is asked for."""
import os
import struct
import subprocess

import pytest

from test_build_cpu import BIN_BUILD
from test_build_hibf_cpu import tiny_input  # noqa: F401  (a fixture)
from test_build_sketch_cpu import TMAX, count_sets

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("hibf_paths") / "hibf_paths_driver")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", os.path.join(HERE, "..", "include"), "-o", out, os.path.join(HERE, "hibf_paths_driver.cpp")])
    return out


def run_driver(driver, line):
    """-> ("refused", message) or ("case", depth, levels, derived, built) with derived / built = {(user, entry): (ibf, first_bin, n_bins)}"""
    lines = subprocess.run([driver], input=line + "\n", capture_output=True, text=True, check=True).stdout.splitlines()
    if lines[0].startswith("refused "):
        return ("refused", lines[0][len("refused "):])
    head = lines[0].split()
    assert head[0] == "case"
    got = {"derived": {}, "built": {}}
    for ln in lines[1:]:
        f = ln.split()
        got[f[0]][(int(f[1]), int(f[2]))] = tuple(int(x) for x in f[3:])
    return ("case", int(head[1]), int(head[2]), got["derived"], got["built"])


GRID = [(f"{name}/tmax{t}", counts, t) for name, counts, _ in count_sets() for t in TMAX]


@pytest.mark.parametrize("name,counts,tmax", GRID, ids=[g[0] for g in GRID])
def test_round_trip(driver, name, counts, tmax):
    """layout -> tables -> derived paths == the paths the builder inserts along, entry for entry; depth == the layout's levels"""
    kind, depth, levels, derived, built = run_driver(driver, f"layout {tmax} {len(counts)} " + " ".join(str(c) for c in counts))
    assert kind == "case"
    assert depth == levels >= 1
    assert len(built) == len(counts) * depth and derived == built
    assert all(derived[(u, 0)][2] >= 1 for u in range(len(counts))), "entry 0 is the user bin's run"


def valid_tables():
    """three levels, six user bins: [(next_ibf_id, bin_to_user)] of IBF 0 (the root), 1 and 2"""
    return [([0, 0, 0, 1], [0, 1, 1, -1]),       # user bin 0, user bin 1 on two bins, a merged bin -> IBF 1
            ([1, 2, 1], [2, -1, 3]),             # user bin 2, a merged bin -> IBF 2, user bin 3
            ([2, 2, 2, 2], [4, 4, 4, 5])]        # user bin 4 on three bins, user bin 5


def tables_line(tabs, n_user=6):
    return f"tables {n_user} {len(tabs)} " + " ".join(f"{len(nx)} " + " ".join(map(str, nx)) + " " + " ".join(map(str, bu)) for nx, bu in tabs)


def test_valid_tables(driver):
    kind, depth, _, derived, _ = run_driver(driver, tables_line(valid_tables()))
    assert kind == "case" and depth == 3
    paths = {u: [derived[(u, d)] for d in range(3)] for u in range(6)}
    assert paths[0] == [(0, 0, 1), (0, 0, 0), (0, 0, 0)]
    assert paths[1] == [(0, 1, 2), (0, 0, 0), (0, 0, 0)]
    assert paths[2] == [(1, 0, 1), (0, 3, 1), (0, 0, 0)]
    assert paths[3] == [(1, 2, 1), (0, 3, 1), (0, 0, 0)]
    assert paths[4] == [(2, 0, 3), (1, 1, 1), (0, 3, 1)]
    assert paths[5] == [(2, 3, 1), (1, 1, 1), (0, 3, 1)]


# (what, [(ibf, table: 0 next_ibf_id | 1 bin_to_user, bin, new value)], words the refusal has to hold).  One field changed wherever one
# field makes exactly that fault; an IBF without a parent takes both fields of one bin (one field alone is another fault first), and
# a cycle in which every IBF still has exactly one parent takes two bins: user bin 5 moves from IBF 2 bin 3 to IBF 0 bin 3, which led
# to IBF 1, and IBF 2 bin 3 leads to IBF 1 instead.
MALFORMED = [
    ("no run", [(2, 1, 3, 4)], ["user bin 5", "no run"]),
    ("two runs", [(1, 1, 2, 0)], ["IBF 1 bin 2", "user bin 0", "two runs", "IBF 0 bin 0"]),
    ("not contiguous", [(2, 1, 1, 5)], ["IBF 2 bin 2", "user bin 4", "not contiguous", "IBF 2 bin 0"]),
    ("single bin, foreign next_ibf_id", [(1, 0, 0, 0)], ["IBF 1 bin 0", "not its own IBF"]),
    ("split bin, foreign next_ibf_id", [(2, 0, 1, 1)], ["IBF 2 bin 1", "not its own IBF"]),
    ("child out of range", [(0, 0, 3, 3)], ["IBF 0 bin 3", "IBF 3", "out of range"]),
    ("child negative", [(1, 0, 1, -7)], ["IBF 1 bin 1", "IBF -7", "out of range"]),
    ("child is IBF 0", [(1, 0, 1, 0)], ["IBF 1 bin 1", "IBF 0", "out of range"]),
    ("child is itself", [(1, 0, 1, 1)], ["IBF 1 bin 1", "its own IBF"]),
    ("two parents", [(0, 0, 3, 2)], ["IBF 1 bin 1", "IBF 2", "two parents", "IBF 0 bin 3"]),
    ("no parent", [(1, 1, 1, 3), (1, 0, 1, 1)], ["IBF 2", "no parent"]),
    ("cycle", [(0, 1, 3, 5), (0, 0, 3, 0), (2, 1, 3, -1), (2, 0, 3, 1)], ["cycle", "IBF 1", "IBF 2 bin 3"]),
    ("user bin out of range", [(2, 1, 3, 6)], ["IBF 2 bin 3", "user bin 6"]),
]


def malformed_line(changes):
    tabs = valid_tables()
    for ibf, table, b, value in changes:
        tabs[ibf][table][b] = value
    return tables_line(tabs)


@pytest.mark.parametrize("what,changes,words", MALFORMED, ids=[m[0] for m in MALFORMED])
def test_malformed_tables_are_refused(driver, what, changes, words):
    got = run_driver(driver, malformed_line(changes))
    assert got[0] == "refused", got
    for w in words:
        assert w in got[1], (w, got[1])


def test_a_user_bin_the_tables_never_name(driver):
    kind, msg = run_driver(driver, tables_line(valid_tables(), n_user=7))
    assert kind == "refused" and "user bin 6" in msg and "no run" in msg


def write_tiny_hibf(path, k=19, w=32, h=3, rows=64, name="A"):
    """a raptor 3.0.1 index of one IBF with one bin and no bit set (the layout ganon_amd/ibf_file.py:save_hibf writes)"""
    fn = ("/db/" + name + ".minimiser").encode()
    with open(path, "wb") as f:
        f.write(struct.pack("<IQQQBB", 1, w, k, (1 << k) - 1, 1, 0))
        f.write(struct.pack("<QQQ", 1, 1, len(fn)) + fn)
        f.write(struct.pack("<dBQ", 0.05, 1, 1))
        f.write(struct.pack("<6Q", 1, 64, rows, 64 - rows.bit_length(), 1, h))
        f.write(struct.pack("<BfQ", 1, 1.5, 64 * rows) + bytes(rows * 8))
        f.write(struct.pack("<QQq", 1, 1, 0))
        f.write(struct.pack("<QQ", 1, len(fn)) + fn)
        f.write(struct.pack("<QQq", 1, 1, 0))


@pytest.fixture(scope="module")
def tiny_index(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("verify_cli") / "tiny.hibf")
    write_tiny_hibf(path)
    from ganon_amd import ibf_file
    m = ibf_file.read_hibf_meta(path)
    assert (m.kmer_size, m.window_size, m.names, m.ibfs[0][:3]) == (19, 32, ["A"], (1, 64, 3))
    return path


@pytest.mark.parametrize("case,words", [
    ("no --hibf", ["--verify-index", "--hibf", "ganon-classify --verify-filter"]),
    ("with --output-file", ["--verify-index", "--output-file"]),
    ("missing file", ["--verify-index", "not found", "no_such.hibf"]),
    ("-k differs", ["--kmer-size", "21", "19"]),
    ("-w differs", ["--window-size", "35", "32"]),
    ("-s differs", ["--hash-functions", "4", "3"]),
])
def test_refusals(tiny_input, tiny_index, case, words):
    assert os.path.exists(BIN_BUILD), "ganon-build is built by __graft_entry__.build()"
    inp, out = tiny_input
    missing = os.path.join(os.path.dirname(tiny_index), "no_such.hibf")
    args = {"no --hibf": ["--verify-index", tiny_index],
            "with --output-file": ["--hibf", "--verify-index", tiny_index, "-o", out],
            "missing file": ["--hibf", "--verify-index", missing],
            "-k differs": ["--hibf", "--verify-index", tiny_index, "-k", "21"],
            "-w differs": ["--hibf", "--verify-index", tiny_index, "-w", "35"],
            "-s differs": ["--hibf", "--verify-index", tiny_index, "-s", "4"]}[case]
    p = subprocess.run([BIN_BUILD, "-i", inp] + args, capture_output=True, text=True)
    assert p.returncode == 1, (p.returncode, p.stderr)
    for w in words:
        assert w in p.stderr, (w, p.stderr)
    assert "device" not in p.stderr.lower(), p.stderr  # refused before the device is touched
    assert p.stdout == "" and not os.path.exists(out)
