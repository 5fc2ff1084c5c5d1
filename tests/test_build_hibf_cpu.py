"""`ganon-build --hibf` without a GPU: the layout rule (ganon_amd/host/hibf_layout.hpp) through a driver this test compiles, the
sizing of the IBFs against a Python restatement, and the command line's refusals."""
import math
import os
import subprocess

import numpy as np
import pytest

import hibf_checks as hc
from test_build_cpu import BIN_BUILD

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("hibf_layout") / "hibf_layout_driver")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-o", out, os.path.join(HERE, "hibf_layout_driver.cpp"),
                           os.path.join(HERE, "..", "ganon_amd", "host", "build_params.cpp")])
    return out


def lognormal(n, seed):
    rng = np.random.default_rng(seed)
    return [max(1, int(x)) for x in rng.lognormal(mean=8.0, sigma=1.5, size=n)]


def cases():
    out = [(f"{n}@64", [1000 + 7 * i for i in range(n)], 64) for n in (1, 2, 63, 64, 65, 1000)]
    out += [(f"{n}@4", [50 + i for i in range(n)], 4) for n in (16, 17)]
    out += [(f"lognormal{n}@{t}", lognormal(n, n + t), t) for n in (25, 200, 5000) for t in (4, 8, 64)]
    out += [(f"equal{n}@{t}", [777] * n, t) for n, t in ((200, 8), (70, 64), (9, 4))]
    out += [(f"giant{n}@{t}", [3] * (n // 2) + [3_000_000] + [3] * (n - n // 2 - 1), t) for n, t in ((100, 8), (30, 64), (300, 4))]
    out += [("tiny@2", [5, 4, 3, 2, 1], 2), ("few-hashes@64", [1, 2, 70], 64)]
    return out


def run_driver(driver, counts, tmax, max_fp=0.05, h=4, shared=25):
    line = f"{tmax} {max_fp!r} {h} {shared} {len(counts)} " + " ".join(str(c) for c in counts) + "\n"
    p = subprocess.run([driver], input=line, capture_output=True, text=True, check=True)
    return p.stdout


def parse(text):
    """-> (levels, L, per IBF dict(bins, rows, parent, parent_bin, depth, runs=[(first, n_bins, user, child, hashes)]))"""
    lines = text.splitlines()
    head = lines[0].split()
    assert head[0] == "case"
    ibfs = []
    for ln in lines[1:]:
        f = ln.split()
        if f[0] == "ibf":
            ibfs.append(dict(bins=int(f[2]), rows=int(f[3]), parent=int(f[4]), parent_bin=int(f[5]), depth=int(f[6]), n_runs=int(f[7]), runs=[]))
        else:
            assert f[0] == "run"
            ibfs[-1]["runs"].append(tuple(int(x) for x in f[1:]))
    assert len(ibfs) == int(head[1])
    return int(head[2]), int(head[3]), ibfs


def tables(ibfs):
    nx, bu = [], []
    for i, f in enumerate(ibfs):
        assert len(f["runs"]) == f["n_runs"]
        a, b = np.full(f["bins"], i, dtype=np.int64), np.full(f["bins"], -1, dtype=np.int64)
        at = 0
        for first, n, user, child, _ in f["runs"]:
            assert first == at and n >= 1, "runs cover the bins in ascending order without gaps"
            at += n
            a[first:first + n] = child if user < 0 else i
            b[first:first + n] = user
        assert at == f["bins"]
        nx.append(a)
        bu.append(b)
    return nx, bu


@pytest.mark.parametrize("name,counts,tmax", cases(), ids=[c[0] for c in cases()])
def test_layout_invariants(driver, name, counts, tmax):
    text = run_driver(driver, counts, tmax)
    assert run_driver(driver, counts, tmax) == text, "same input, same tree"
    levels, L, ibfs = parse(text)
    assert L == hc.levels_for(len(counts), tmax)
    nx, bu = tables(ibfs)
    runs, depth, below, where, parent = hc.check_tree([f["bins"] for f in ibfs], nx, bu, len(counts), tmax)
    assert levels == max(depth) + 1 <= L
    for i, f in enumerate(ibfs):  # what the builder derives from the layout agrees with the tables
        assert f["depth"] == depth[i]
        assert (f["parent"], f["parent_bin"]) == (parent[i] if i else (-1, 0))
    if len(counts) <= tmax:
        assert len(ibfs) == 1 and ibfs[0]["bins"] <= max(tmax, 1)


@pytest.mark.parametrize("name,counts,tmax", cases(), ids=[c[0] for c in cases()])
@pytest.mark.parametrize("max_fp,h", [(0.05, 4), (0.001, 4), (0.05, 3), (0.001, 1), (0.3, 5)])
def test_sizing(driver, name, counts, tmax, max_fp, h):
    shared = 25
    _, _, ibfs = parse(run_driver(driver, counts, tmax, max_fp, h, shared))
    nx, bu = tables(ibfs)
    runs, _, below, where, _ = hc.check_tree([f["bins"] for f in ibfs], nx, bu, len(counts), tmax)
    for i, f in enumerate(ibfs):
        need = 0
        for (first, n, user, child), got in zip(runs[i], f["runs"]):
            if user >= 0:
                card = counts[user]
            else:  # the made-up cardinality of a merged bin: a quarter of the hashes below it shared
                members = [counts[u] for u in below[child]]
                card = max(max(members), sum(members) * (100 - shared) // 100)
            assert got[4] == card
            need = max(need, hc.run_bits(card, n, max_fp, h))
        assert f["rows"] == need, (i, f["rows"], need)
    from ganon_amd.ibf_file import false_positive
    for u, (i, first, s) in where.items():
        share = (counts[u] + s - 1) // s
        fp = 1.0 - (1.0 - false_positive(ibfs[i]["rows"], h, share)) ** s
        # the rows are rounded UP, so the rate is at most max_fp in exact arithmetic; the chain of log / exp / pow that
        # evaluates it is good to a few units in the last place of a double
        assert fp <= max_fp * (1 + 1e-12), (u, fp, max_fp)


@pytest.fixture(scope="module")
def tiny_input(tmp_path_factory):
    d = tmp_path_factory.mktemp("hibf_cli")
    fa = d / "a.fasta"
    fa.write_text(">a\n" + "ACGTTGCATGACCGTAGGCTAAGCTTAGGATCCATGCAAGTCGGATTACA" * 2 + "\n")
    inp = d / "in.tsv"
    inp.write_text(f"{fa}\tA\n")
    return str(inp), str(d / "out.hibf")


@pytest.mark.parametrize("extra,word", [(["--hibf", "--filter-size", "1"], "--filter-size"), (["--hibf", "--mode", "smaller"], "--mode"),
                                        (["--hibf", "--tmax", "1"], "--tmax"), (["--tmax", "64"], "--hibf")])
def test_refusals(tiny_input, extra, word):
    assert os.path.exists(BIN_BUILD), "ganon-build is built by __graft_entry__.build()"
    inp, out = tiny_input
    p = subprocess.run([BIN_BUILD, "-i", inp, "-o", out] + extra, capture_output=True, text=True)
    assert p.returncode == 1, (p.returncode, p.stderr)
    assert word in p.stderr and "device" not in p.stderr.lower(), p.stderr  # refused before the device is touched
    assert not os.path.exists(out)
