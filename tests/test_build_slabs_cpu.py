"""A flat `ganon-build` in row slabs, without a GPU: the slab plan (ganon_amd/host/build_slabs.hpp) against a Python restatement of its rule;
the item builder and the window arithmetic of the windowed insert (ganon_amd/csrc/gn_emplace_window.h, the very functions the kernel and
its host call) on a host model of the kernel against oracle.Ibf; and the command's refusals.  The driver is a stand-alone program under
AddressSanitizer and UBSan with buffers of exactly the words there are; nothing is preloaded."""
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

# the shape the GPU test (test_build_slabs_gpu.py) uses too
TOTAL_ROWS, BINS, CUTS = 1000, 130, [0, 1, 7, 512, 999, 1000]
RUN_SIZES = (0, 1, 64, 513, 1300)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("build_slabs") / "build_slabs_driver")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                           os.path.join(HERE, "build_slabs_driver.cpp"), "-I", os.path.join(HERE, "..", "include")])
    return exe


def run(driver, text):
    p = subprocess.run([driver], input=text, capture_output=True, text=True)
    assert p.returncode == 0 and p.stderr == "", (p.returncode, p.stderr[-3000:])  # (a sanitizer report ends the program with a status)
    return p.stdout


# ------------------------------------------------------------------------------------------------------------ the plan
def plan_rule(total_rows, row_bytes, budget, n_devices):
    """the rule of the plan, restated: None when one row does not fit, else (P, rows per slab, slab(i) -> (row_begin, n_rows, entry))"""
    per = budget // row_bytes
    if per == 0:
        return None
    P = -(-total_rows // per)
    per = -(-total_rows // P)
    return P, per, lambda i: (i * per, min(per, total_rows - i * per), i % n_devices)


@pytest.mark.parametrize("total_rows", [1, 2, 1000, 2**32 - 1])
@pytest.mark.parametrize("n_devices", [1, 2, 3])
def test_plan(driver, total_rows, n_devices):
    row_bytes = 24  # 130 bins: three words
    whole = total_rows * row_bytes
    for what, budget in (("one row", row_bytes), ("one byte short of one row", row_bytes - 1), ("one row short of the whole", whole - row_bytes),
                         ("the whole", whole), ("twice the whole", 2 * whole)):
        exp = plan_rule(total_rows, row_bytes, budget, n_devices)
        if budget < row_bytes:  # (one row short of the whole is no row when the whole is one row)
            text = run(driver, f"plan {total_rows} {row_bytes} {budget} {n_devices}\n")
            assert exp is None and text.startswith("refused") and f"{row_bytes} bytes" in text and "not one row fits" in text, (what, text)
            continue
        P, per, slab = exp
        # every slab when there are few, else both ends and slabs spread over the plan (the plan is a rule: slab i alone says where it lies)
        asked = list(range(P)) if P <= 5000 else sorted({0, 1, 2, P // 3, P // 2, P - 3, P - 2, P - 1})
        lines = run(driver, f"plan {total_rows} {row_bytes} {budget} {n_devices} " + " ".join(map(str, asked)) + "\n").splitlines()
        assert lines[0].split() == ["plan", str(P), str(per)], (what, lines[0], P, per)
        got = {int(f[1]): (int(f[2]), int(f[3]), int(f[4])) for f in (ln.split() for ln in lines[1:])}
        assert sorted(got) == asked
        for i in asked:
            assert got[i] == slab(i), (what, i)
            begin, n, entry = got[i]
            assert n >= 1 and n * row_bytes <= budget and entry == i % n_devices, (what, i, got[i])
            if i + 1 in got:
                assert begin + n == got[i + 1][0], "no gap, no overlap"
        assert got[0][0] == 0 and got[P - 1][0] + got[P - 1][1] == total_rows, "the slabs tile [0, total_rows)"
        assert (P - 1) * per < total_rows <= P * per, "equal slabs but for a shorter last one, which is not empty"
        assert P == 1 or (P - 1) * (budget // row_bytes) < total_rows, "P is minimal: P - 1 slabs of the budget's rows do not hold the matrix"
        if budget >= whole:
            assert P == 1 and got[0] == (0, total_rows, 0), "the one-pass build: one slab on the first entry"


# ------------------------------------------------------------------------------------------------------------ the items
def parse_chunks(text):
    chunks = []
    for ln in text.splitlines():
        f = ln.split()
        if f[0] == "chunk":
            chunks.append((int(f[1]), []))
        else:
            assert f[0] == "item"
            chunks[-1][1].append(tuple(int(x) for x in f[1:]))
    return chunks


@pytest.mark.parametrize("cap_items", [1 << 20, 3])
def test_items(driver, cap_items):
    sizes = list(RUN_SIZES) + [0, 700, 0]
    chunks = parse_chunks(run(driver, f"items 700 {cap_items} {len(sizes)} " + " ".join(map(str, sizes)) + "\n"))
    seen = [np.zeros(n, dtype=np.int64) for n in sizes]
    for taken, items in chunks:
        assert 1 <= taken <= 700 and 1 <= len(items) <= cap_items
        at = 0
        for run_, cnt, begin, stage_at in items:
            assert 1 <= cnt <= 512 and begin + cnt <= sizes[run_], "an item lies in one run and holds at most 512 hashes"
            assert stage_at == at, "the items of a chunk lie behind each other in the staging buffer"
            seen[run_][begin:begin + cnt] += 1  # (begin is the index in the RUN: a later piece of a long run does not start at 0)
            at += cnt
        assert at == taken
    assert all((s == 1).all() for s in seen), "every hash of every run is in exactly one item"
    order = [(r, b) for _, items in chunks for r, _, b, _ in items]
    assert order == sorted(order), "runs in order, a run's pieces ascending"
    if cap_items == 1 << 20:
        assert [t for t, _ in chunks] == [700, 700, 700, 478], "chunks are full but for the last"
        assert any(b > 0 and b % 512 != 0 for _, items in chunks for r, _, b, _ in items if r == 4), "the 1300-hash run is cut by a chunk boundary"


# ------------------------------------------------------------------------------------------------------------ the window
def window_inputs(seed=5):
    """runs of 0, 1, 64, 513 and 1300 hashes, the value 0 among them; one run crosses a word boundary (bins 60 .. 70), one ends in bin 129"""
    rng = np.random.default_rng(seed)
    runs = [rng.integers(0, 1 << 64, size=n, dtype=U64) for n in RUN_SIZES]
    runs[3][7] = 0
    first_bin = [5, 6, 7, 60, 127]
    per_bin = [1, 1, 64, 47, 600]  # 513 hashes at 47 a bin: bins 60 .. 70; 1300 at 600: bins 127 .. 129
    assert 60 + (513 - 1) // 47 == 70 and 127 + (1300 - 1) // 600 == 129
    return runs, first_bin, per_bin


def oracle_filter(runs, first_bin, per_bin, h):
    ref = oracle.Ibf(BINS, TOTAL_ROWS, h)
    for r, f, p in zip(runs, first_bin, per_bin):
        if len(r):
            ref.emplace_many(r, (f + np.arange(len(r)) // p).astype(np.uint32))
    return ref.data


def window_line(h, row_begin, n_rows, cap, runs, first_bin, per_bin):
    parts = ["window", str(TOTAL_ROWS), str(BINS), str(h), str(row_begin), str(n_rows), str(cap), str(len(runs))]
    for r, f, p in zip(runs, first_bin, per_bin):
        parts += [str(f), str(p), str(len(r))] + [format(int(x), "x") for x in r]
    return " ".join(parts) + "\n"


@pytest.mark.parametrize("cap", [700, 1 << 20])
def test_window_model_equals_the_oracle(driver, cap):
    h = 5
    runs, first_bin, per_bin = window_inputs()
    ref = oracle_filter(runs, first_bin, per_bin, h)
    slabs = []
    for a, b in zip(CUTS, CUTS[1:]):
        text = run(driver, window_line(h, a, b - a, cap, runs, first_bin, per_bin))
        assert not text.startswith("refused"), text
        slabs.append(np.array([[int(x, 16) for x in ln.split()] for ln in text.splitlines()], dtype=U64).reshape(b - a, 3))
    got = np.concatenate(slabs)
    assert np.array_equal(got, ref), "the slabs behind each other are the filter"
    assert ref.any() and not (got[:, 2] >> U64(BINS - 128)).any(), "the padding bits of the last word stay zero"


# ------------------------------------------------------------------------------------------------------------ the command's refusals
def test_refusals_that_need_no_device(tiny_input, tiny_index, tmp_path):
    inp, out = tiny_input
    flat = str(tmp_path / "x.ibf")
    for args, word in ((["-i", inp, "--hibf", "-o", out, "--device-memory", "1000"], "--device-memory cannot be used with --hibf"),
                       (["-i", inp, "--hibf", "-o", out, "--device", "0,0"], "--device takes one device with --hibf"),
                       (["-i", inp, "--hibf", "--verify-index", tiny_index, "--device-memory", "1000"], "--device-memory cannot be used with --verify-index"),
                       (["-i", inp, "--hibf", "--verify-index", tiny_index, "--device", "0,1"], "--device takes one device with --verify-index"),
                       (["-i", inp, "--hibf", "--update", tiny_index, "-o", out, "--device-memory", "1000"], "--device-memory cannot be used with --update"),
                       (["-i", inp, "--hibf", "--update", tiny_index, "-o", out, "--device", "0,0"], "--device takes one device with --update"),
                       (["-i", inp, "-o", flat, "--device-memory", "0"], "--device-memory has to be > 0"),
                       (["-i", inp, "-o", flat, "--device-memory", "-5"], "failed to parse"),
                       (["-i", inp, "-o", flat, "--device-memory", "1k"], "failed to parse"),
                       (["-i", inp, "-o", flat, "--device", "0,"], "failed to parse"),
                       (["-i", inp, "-o", flat, "--device", "0,,1"], "failed to parse"),
                       (["-i", inp, "-o", flat, "--device", "a"], "failed to parse")):
        p = subprocess.run([BIN_BUILD] + args, capture_output=True, text=True)
        assert p.returncode == 1 and word in p.stderr and p.stdout == "" and not os.path.exists(out) and not os.path.exists(flat), (args, p.stderr)
    p = subprocess.run([BIN_BUILD, "--help"], capture_output=True, text=True)
    assert "--device-memory arg" in p.stderr and "A list a,b,..." in p.stderr
