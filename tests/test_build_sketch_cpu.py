"""`ganon-build --hibf --layout sketch` without a GPU: the size-aware layout (ganon_amd/host/hibf_layout_sketch.hpp) through a driver
this test compiles, fed exact sums as its union estimates (disjoint sets), against the invariants every HIBF layout keeps and
against the rule's tree (hibf_layout.hpp) on the same counts; and the command line's two refusals."""
import os
import subprocess

import pytest

import hibf_checks as hc
from test_build_cpu import BIN_BUILD
from test_build_hibf_cpu import cases, lognormal, parse, tables, tiny_input  # noqa: F401  (tiny_input is a fixture)

HERE = os.path.dirname(os.path.abspath(__file__))
TMAX = (2, 4, 8, 64)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("hibf_layout_sketch") / "hibf_layout_sketch_driver")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-o", out, os.path.join(HERE, "hibf_layout_sketch_driver.cpp"),
                           os.path.join(HERE, "..", "ganon_amd", "host", "build_params.cpp")])
    return out


def count_sets():
    """the rule's 31 count sets (each with the tmax it is tested at there), and the one-large-bin set of the size tests"""
    out = list(cases())
    out.append(("one-large-39-small@8", [64000] + [1000] * 39, 8))
    return out


def grid():
    """every count set at its own tmax and at 2, 4, 8, 64"""
    return [(f"{name}/tmax{t}", counts, t) for name, counts, own in count_sets() for t in sorted(set(TMAX) | {own})]


_memo = {}


def run_driver(driver, layout, counts, tmax, max_fp=0.05, h=4):
    """-> (text, (levels, L, ibfs), asked | None); one run per input is kept"""
    key = (layout, tuple(counts), tmax, max_fp, h)
    if key not in _memo:
        line = f"{layout} {tmax} {max_fp!r} {h} {len(counts)} " + " ".join(str(c) for c in counts) + "\n"
        text = subprocess.run([driver], input=line, capture_output=True, text=True, check=True).stdout
        lines = text.splitlines()
        asked = None
        if lines and lines[-1].startswith("asked "):
            asked = tuple(int(x) for x in lines.pop().split()[1:])
        _memo[key] = (text, parse("\n".join(lines)), asked)
    return _memo[key]


def total_bits(ibfs):
    """what the builder allocates and writes: rows times the bins rounded up to whole 64-bit words, over every IBF"""
    return sum(f["rows"] * ((f["bins"] + 63) // 64 * 64) for f in ibfs)


@pytest.mark.parametrize("name,counts,tmax", grid(), ids=[c[0] for c in grid()])
def test_layout_invariants(driver, name, counts, tmax):
    text, (levels, L, ibfs), asked = run_driver(driver, "sketch", counts, tmax)
    assert L == hc.levels_for(len(counts), tmax)
    nx, bu = tables(ibfs)
    runs, depth, below, where, parent = hc.check_tree([f["bins"] for f in ibfs], nx, bu, len(counts), tmax)
    assert levels == max(depth) + 1 <= L
    order = sorted(range(len(counts)), key=lambda u: (-counts[u], u))
    at = {u: j for j, u in enumerate(order)}
    for i, f in enumerate(ibfs):
        assert f["depth"] == depth[i]
        assert (f["parent"], f["parent_bin"]) == (parent[i] if i else (-1, 0))
        for (first, n, user, child), got in zip(runs[i], f["runs"]):
            if user < 0:  # a merged bin is never spent on one user bin, and its members are neighbours in the sorted order
                members = sorted(below[child], key=lambda u: at[u])
                assert len(members) >= 2
                assert order[at[members[0]]:at[members[0]] + len(members)] == members
                assert got[4] == sum(counts[u] for u in members)
    if len(counts) <= tmax:
        assert len(ibfs) == 1
    n_asked, longest, width = asked
    assert longest <= width, "no union longer than the table the builder computes"
    if L == 1:
        assert n_asked == 0, "one IBF: no estimate is needed"


@pytest.mark.parametrize("name,counts,tmax", grid()[::7], ids=[c[0] for c in grid()[::7]])
def test_same_input_same_tree(driver, name, counts, tmax):
    text = run_driver(driver, "sketch", counts, tmax)[0]
    _memo.clear()
    assert run_driver(driver, "sketch", counts, tmax)[0] == text


@pytest.mark.parametrize("name,counts,tmax", grid(), ids=[c[0] for c in grid()])
@pytest.mark.parametrize("max_fp,h", [(0.05, 4), (0.001, 3)])
def test_never_larger_than_the_rule(driver, name, counts, tmax, max_fp, h):
    sketch = total_bits(run_driver(driver, "sketch", counts, tmax, max_fp, h)[1][2])
    rule = total_bits(run_driver(driver, "rule", counts, tmax, max_fp, h)[1][2])
    print(f"{name} max_fp {max_fp} h {h}: sketch {sketch} rule {rule} ratio {sketch / rule:.3f}")
    assert sketch <= rule


@pytest.mark.parametrize("name,counts", [("lognormal25", lognormal(25, 33)), ("lognormal200", lognormal(200, 208)), ("lognormal5000", lognormal(5000, 5008)),
                                         ("giant100", [3] * 50 + [3_000_000] + [3] * 49), ("one-large-39-small", [64000] + [1000] * 39)])
@pytest.mark.parametrize("max_fp,h", [(0.05, 4), (0.001, 3)])
def test_strictly_smaller_at_tmax_8(driver, name, counts, max_fp, h):
    sketch = total_bits(run_driver(driver, "sketch", counts, 8, max_fp, h)[1][2])
    rule = total_bits(run_driver(driver, "rule", counts, 8, max_fp, h)[1][2])
    print(f"{name} max_fp {max_fp} h {h}: sketch {sketch} rule {rule} ratio {sketch / rule:.3f}")
    assert sketch < rule


@pytest.mark.parametrize("extra,word", [(["--layout", "sketch"], "--hibf"), (["--layout", "rule"], "--hibf"), (["--hibf", "--layout", "chopper"], "--layout"),
                                        (["--hibf", "--layout", ""], "--layout")])
def test_refusals(tiny_input, extra, word):
    assert os.path.exists(BIN_BUILD), "ganon-build is built by __graft_entry__.build()"
    inp, out = tiny_input
    p = subprocess.run([BIN_BUILD, "-i", inp, "-o", out] + extra, capture_output=True, text=True)
    assert p.returncode == 1, (p.returncode, p.stderr)
    assert "--layout" in p.stderr and word in p.stderr and "device" not in p.stderr.lower(), p.stderr  # refused before the device is touched
    assert not os.path.exists(out)
