"""`ganon-build --hibf --hibf-hash-sets packed|spilled` without a GPU: a host model of the packed path insert's kernel, built from the
functions the kernel and its host call (ganon_amd/csrc/gn_packed_set.h, gn_path_window.h, gn_emplace_window.h), against the oracle model of
the parts test; the union of packed runs against the restated format of the packed test; and the command's refusals.  The driver is a
stand-alone program under AddressSanitizer and UBSan with buffers of exactly the words there are; nothing is preloaded."""
import os
import subprocess

import numpy as np
import pytest

from test_build_cpu import BIN_BUILD
from test_build_hibf_cpu import tiny_input  # noqa: F401  (a fixture)
from test_build_hibf_parts_cpu import CUTS, MODEL_IBFS, model_inputs, model_oracle, parse_window
from test_build_packed_cpu import M64, ascending, encode, of_width, run_text
from test_build_verify_cpu import tiny_index  # noqa: F401  (a fixture)

HERE = os.path.dirname(os.path.abspath(__file__))
U64 = np.uint64


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("build_hibf_packed") / "build_hibf_packed_driver")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                           os.path.join(HERE, "build_hibf_packed_driver.cpp"), "-I", os.path.join(HERE, "..", "include")])
    return exe


def run(driver, text):
    p = subprocess.run([driver], input=text, capture_output=True, text=True)
    assert p.returncode == 0 and p.stderr == "", (p.returncode, p.stderr[-3000:])  # (a sanitizer report ends the program with a status)
    return p.stdout


# ------------------------------------------------------------------------------------------------------------ the kernel's model
def packed_model_inputs():
    """(runs, paths): the sets of the parts test's model -- none, 1 hash, 64, 513, 1300 over 62 bits (three blocks of some 400 words: longer
    than a chunk of 700 words) and 700 -- each as a run of one file, and behind them 512 hashes, a run of two files (300 + 513: a short
    block in the middle), consecutive values (width 1), deltas of 63 bits, and the triple whose deltas take all 64"""
    rng = np.random.default_rng(23)
    sets, paths = model_inputs()
    runs = [[s] if len(s) else [] for s in sets]
    runs += [[ascending(rng, 512, 1 << 62)], [ascending(rng, 300, 1 << 64), ascending(rng, 513, 1 << 40)], [np.arange(5000, 5600, dtype=U64)],
             [np.array(of_width(rng, 40, 63), dtype=U64)], [np.array([0, 1 << 63, M64], dtype=U64)]]
    paths = paths + [[(2, 0, 8, 64), (0, 64, 1, 1)],      # 512 at 64 a bin: bins 0 .. 7 of 64
                     [(3, 20, 11, 74), (0, 129, 1, 1)],   # 813 at 74 a bin: bins 20 .. 30, the files' boundary inside bin 24
                     [(1, 0, 3, 200), (0, 3, 1, 1)],      # 600 at 200 a bin
                     [(1, 3, 1, 1), (0, 10, 2, 20)],      # 40: a single bin below, a run of two bins in the root
                     [(2, 10, 3, 1), (0, 3, 1, 1)]]       # 3 at one a bin
    return runs, paths


def flat(files):
    return np.concatenate([np.asarray(v, dtype=U64) for v in files]) if files else np.zeros(0, U64)


def test_the_model_inputs_are_what_they_say():
    runs, paths = packed_model_inputs()
    enc = [encode(files) for files in runs]
    assert [sum(b[2] for b in e[0]) for e in enc] == [0, 1, 64, 513, 1300, 700, 512, 813, 600, 40, 3] and len(paths) == len(runs)
    assert [b[2] for b in enc[7][0]] == [300, 512, 1], "a short block in the middle of a run"
    assert len(enc[4][1]) > 700 and [b[2] for b in enc[6][0]] == [512] and [b[2] for b in enc[3][0]] == [512, 1]
    widths = {b[3] for e in enc for b in e[0]}
    assert {0, 1, 63, 64} <= widths, widths
    assert (enc[1][0][0][3], enc[8][0][0][3], enc[9][0][0][3], enc[10][0][0][3]) == (0, 1, 63, 64)


def window_line(h, cap, pieces, runs, paths):
    """pieces: per IBF of the model's filter (tree ibf, row_begin, n_rows); the paths are compacted to them as the builder does"""
    local = {t: j for j, (t, _, _) in enumerate(pieces)}
    parts = ["window", str(h), str(cap), str(len(pieces))]
    for t, a, n in pieces:
        parts += [str(MODEL_IBFS[t][0]), str(MODEL_IBFS[t][1]), str(a), str(n)]
    taken = [(files, [e for e in p if e[2] and e[0] in local]) for files, p in zip(runs, paths)]
    taken = [(files, p) for files, p in taken if p]
    parts += ["2", str(len(taken))]
    for files, p in taken:
        for ibf, first, n, per in p + [(0, 0, 0, 0)] * (2 - len(p)):
            parts += [str(local.get(ibf, 0)), str(first), str(n), str(per)]
        parts.append(run_text(files))
    return " ".join(parts) + "\n"


@pytest.mark.parametrize("h", [1, 3, 5])
@pytest.mark.parametrize("cap", [700, 1 << 20])
def test_window_model_equals_the_oracle(driver, cap, h):
    runs, paths = packed_model_inputs()
    ref = model_oracle([flat(files) for files in runs], paths, h)
    assert all(r.any() for r in ref)
    whole = [(t, 0, r) for t, (_, r) in enumerate(MODEL_IBFS)]
    got = parse_window(run(driver, window_line(h, cap, whole, runs, paths)), whole)
    for t in range(4):
        assert np.array_equal(got[t], ref[t]), f"IBF {t}, every IBF whole"
    for t in range(4):  # every IBF alone, its paths compacted to it
        pieces = [(t, 0, MODEL_IBFS[t][1])]
        assert np.array_equal(parse_window(run(driver, window_line(h, cap, pieces, runs, paths)), pieces)[0], ref[t]), f"IBF {t} alone"
    root = []
    for a, b in zip(CUTS, CUTS[1:]):  # the root in pieces
        pieces = [(0, a, b - a)]
        root.append(parse_window(run(driver, window_line(h, cap, pieces, runs, paths)), pieces)[0])
    assert np.array_equal(np.concatenate(root), ref[0]), "the pieces behind each other are the root"
    assert not (ref[0][:, 2] >> U64(130 - 128)).any() and not (ref[3][:, 1] >> U64(1)).any(), "the padding bits of the last word stay zero"


# ------------------------------------------------------------------------------------------------------------ the union's model
def union_cases():
    rng = np.random.default_rng(31)
    a, b = ascending(rng, 700, 1 << 38), ascending(rng, 1300, 1 << 38)
    return [("no run", []), ("an empty run", [[]]), ("one run of one file", [[a]]),
            ("a target's two files as one run, hashes shared", [[a, np.sort(np.concatenate([a[::3], b[:100]]))]]),
            ("runs with duplicates and an empty one between", [[a], [], [a[100:400]], [b, a[:5]]]),
            ("all 64 bits", [[np.array([0, 1 << 63, M64], dtype=U64)], [ascending(rng, 513, 1 << 64)]]),
            ("512 and one more", [[np.arange(0, 512, dtype=U64)], [np.array([512], dtype=U64)]])]


def test_union_model_equals_the_restated_format(driver):
    cases = union_cases()
    text = run(driver, "".join(f"union {len(runs)} " + " ".join(run_text(files) for files in runs) + "\n" for _, runs in cases))
    got = []
    for ln in text.splitlines():
        f = ln.split()
        assert f[0] != "refused", ln
        if f[0] == "union":
            got.append(dict(sizes=tuple(int(x) for x in f[1:]), blocks=[], payload=None))
        elif f[0] == "block":
            got[-1]["blocks"].append((int(f[1], 16), int(f[2]), int(f[3]), int(f[4])))
        else:
            got[-1]["payload"] = [int(x, 16) for x in f[1:]]
    assert len(got) == len(cases)
    for (name, runs), g in zip(cases, got):
        all_ = np.unique(np.concatenate([flat(files) for files in runs] + [np.zeros(0, U64)]))
        blocks, payload = encode([all_])
        assert g["blocks"] == blocks and g["payload"] == payload and g["sizes"] == (len(all_), len(blocks), len(payload)), name
    assert got[-1]["sizes"][:2] == (513, 2) and got[3]["sizes"][0] == 800


# ------------------------------------------------------------------------------------------------------------ the command's refusals
def test_refusals_that_need_no_device(tiny_input, tiny_index, tmp_path):
    inp, out = tiny_input
    flat_out = str(tmp_path / "x.ibf")
    cases = [(["-i", inp, "-o", flat_out, "--hibf-hash-sets", "packed"], "--hibf-hash-sets needs --hibf"),
             (["-i", inp, "-o", flat_out, "--hibf-hash-sets", "raw"], "--hibf-hash-sets needs --hibf"),
             (["-i", inp, "--hibf", "-o", out, "--hibf-hash-sets", "zip"], "--hibf-hash-sets has to be raw, packed or spilled"),
             (["-i", inp, "--hibf", "-o", out, "--hibf-hash-sets", ""], "--hibf-hash-sets has to be raw, packed or spilled"),
             (["-i", inp, "--hibf", "-o", out, "--hibf-hash-sets"], "is missing an argument")]
    for mode in ("raw", "packed", "spilled"):
        cases += [(["-i", inp, "--hibf", "--update", tiny_index, "-o", out, "--hibf-hash-sets", mode], f"--hibf-hash-sets {mode} cannot be used with --update"),
                  (["-i", inp, "--hibf", "--verify-index", tiny_index, "--hibf-hash-sets", mode], f"--hibf-hash-sets {mode} cannot be used with --verify-index")]
    for args, word in cases:
        p = subprocess.run([BIN_BUILD] + args, capture_output=True, text=True)
        assert p.returncode == 1 and word in p.stderr and p.stdout == "", (args, p.stderr)
        assert "device" not in p.stderr.lower(), "refused before the device is touched"
        assert not os.path.exists(out) and not os.path.exists(flat_out) and os.listdir(str(tmp_path)) == [], args
    # --hash-sets stays refused with --hibf, and says where to go
    p = subprocess.run([BIN_BUILD, "-i", inp, "--hibf", "-o", out, "--hash-sets", "packed"], capture_output=True, text=True)
    assert p.returncode == 1 and "unions, sketches and probes read raw sets" in p.stderr and "use --hibf-hash-sets" in p.stderr
    # raw is the command line of before: not refused for the switch (another refusal ends it here)
    p = subprocess.run([BIN_BUILD, "-i", inp, "--hibf", "-o", out, "--hibf-hash-sets", "raw", "--tmax", "1"], capture_output=True, text=True)
    assert p.returncode == 1 and "--tmax" in p.stderr and "--hibf-hash-sets" not in p.stderr and not os.path.exists(out)
    p = subprocess.run([BIN_BUILD, "--help"], capture_output=True, text=True)
    assert p.returncode == 0 and "--hibf-hash-sets arg" in p.stderr and "Two families" in p.stderr
