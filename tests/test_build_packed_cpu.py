"""Packed hash sets (`ganon-build --hash-sets packed|spilled`) without a GPU: the format of ganon_amd/csrc/gn_packed_set.h -- the host encoder
and decoder, the bit-extract, the bounds and the item builder, the very functions the kernels and their host call -- against a Python
restatement of the format that lives here; a host model of the insert kernel built from the header's functions against oracle.Ibf; and the
command's refusals.  The driver is a stand-alone program under AddressSanitizer and UBSan with buffers of exactly the words there are;
nothing is preloaded."""
import os
import subprocess

import numpy as np
import pytest

from test_build_cpu import BIN_BUILD
from test_build_hibf_cpu import tiny_input  # noqa: F401  (a fixture)
from test_build_slabs_cpu import BINS, CUTS, TOTAL_ROWS, oracle_filter
from test_build_verify_cpu import tiny_index  # noqa: F401  (a fixture)

HERE = os.path.dirname(os.path.abspath(__file__))
U64 = np.uint64
M64 = (1 << 64) - 1
BLOCK_BYTES, ITEM_BYTES = 24, 48  # a block of the block list; a block's entry in the table a pass uploads


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("build_packed") / "build_packed_driver")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                           os.path.join(HERE, "build_packed_driver.cpp"), "-I", os.path.join(HERE, "..", "include")])
    return exe


def run(driver, text):
    p = subprocess.run([driver], input=text, capture_output=True, text=True)
    assert p.returncode == 0 and p.stderr == "", (p.returncode, p.stderr[-3000:])  # (a sanitizer report ends the program with a status)
    return p.stdout


# ------------------------------------------------------------------------------------------------------------ the format, restated
def encode(files):
    """the format, independent of the header: a run = its files' sets behind each other, each cut every 512 hashes from its start ->
    (blocks as (first, word_at, cnt, width), payload words)"""
    blocks, payload = [], []
    for v in files:
        v = [int(x) for x in v]
        assert all(a < b for a, b in zip(v, v[1:])), "a set is strictly ascending"
        for at in range(0, len(v), 512):
            blk = v[at:at + 512]
            deltas = [b - a for a, b in zip(blk, blk[1:])]
            width = max(deltas).bit_length() if deltas else 0
            bits = 0
            for i, d in enumerate(deltas):
                bits |= d << (i * width)  # delta i at bits [i * width, (i + 1) * width), LSB first
            n_words = -(-len(deltas) * width // 64)
            blocks.append((blk[0], len(payload), len(blk), width))
            payload += [(bits >> (64 * w)) & M64 for w in range(n_words)]  # (the padding bits of the last word are zero)
    return blocks, payload


def run_text(files):
    return " ".join([str(len(files))] + [" ".join([str(len(v))] + [format(int(x), "x") for x in v]) for v in files])


def ascending(rng, n, hi):
    """n distinct values below hi, ascending"""
    out = np.unique(rng.integers(0, hi, size=n + n // 8 + 8, dtype=U64, endpoint=False))
    assert len(out) >= n
    return np.sort(rng.choice(out, size=n, replace=False))


def of_width(rng, n, width, start=3):
    """n hashes whose largest delta has exactly `width` bits: one delta has its top bit set, the others are anything of that width that
    keeps the sum below 2^64"""
    room = min(1 << width, ((1 << 64) - start - (1 << width)) // max(n, 1))
    deltas = [int(rng.integers(1, room)) for _ in range(n - 1)]
    if deltas:
        deltas[int(rng.integers(0, len(deltas)))] = (1 << (width - 1)) | int(rng.integers(0, 1 << min(width - 1, 62)))
    v = [start]
    for d in deltas:
        v.append(v[-1] + d)
    assert v[-1] <= M64 and (not deltas or max(deltas).bit_length() == width)
    return v


SIZES = (0, 1, 2, 64, 511, 512, 513, 1300)


def format_cases():
    rng = np.random.default_rng(11)
    cases = []
    for n in SIZES:
        cases.append((f"consecutive {n}", [list(range(1000, 1000 + n))]))
        cases.append((f"below 2^38 {n}", [ascending(rng, n, 1 << 38)]))
        cases.append((f"all 64 bits {n}", [ascending(rng, n, 1 << 64)]))
    cases.append(("two files 300 + 513", [ascending(rng, 300, 1 << 64), ascending(rng, 513, 1 << 38)]))
    cases.append(("width 64", [[0, 1 << 63, M64]]))
    for width in (7, 13, 33, 63):
        cases.append((f"width {width}", [of_width(rng, 600 if width < 63 else 40, width)]))
    cases.append(("ends on a word boundary", [of_width(rng, 65, 13)]))  # 64 deltas of 13 bits: 13 words exactly
    cases.append(("an empty file among files", [[], [5, 9], [], [7]]))
    return cases


def test_format_cases_are_what_they_say():
    by_name = {name: encode(files) for name, files in format_cases()}
    assert {w for _, _, c, w in by_name["consecutive 1300"][0]} == {1}
    assert [(c, w) for _, _, c, w in by_name["width 64"][0]] == [(3, 64)] and len(by_name["width 64"][1]) == 2
    assert [c for _, _, c, _ in by_name["two files 300 + 513"][0]] == [300, 512, 1], "a short block in the middle of the run"
    for width in (7, 13, 33, 63):
        assert by_name[f"width {width}"][0][0][3] == width
    (_, _, cnt, width), = by_name["ends on a word boundary"][0]
    assert (cnt - 1) * width % 64 == 0 and len(by_name["ends on a word boundary"][1]) == 13
    assert by_name["consecutive 1"][0] == [(1000, 0, 1, 0)] and by_name["consecutive 1"][1] == [] and by_name["consecutive 0"] == ([], [])
    assert [b[1] for b in by_name["below 2^38 1300"][0]][0] == 0 and max(w for _, _, _, w in by_name["all 64 bits 1300"][0]) > 50


def parse_encode(text):
    runs = []
    for ln in text.splitlines():
        f = ln.split()
        assert f[0] != "refused", ln
        if f[0] == "run":
            runs.append(dict(sizes=tuple(int(x) for x in f[1:]), blocks=[], payload=None, decoded=None))
        elif f[0] == "block":
            runs[-1]["blocks"].append((int(f[1], 16), int(f[2]), int(f[3]), int(f[4])))
        else:
            runs[-1][f[0]] = [int(x, 16) for x in f[1:]]
    return runs


def test_encoder_equals_the_restated_format_and_decodes_to_the_input(driver):
    cases = format_cases()
    got = parse_encode(run(driver, "encode " + str(len(cases)) + " " + " ".join(run_text(files) for _, files in cases) + "\n"))
    assert len(got) == len(cases)
    for (name, files), g in zip(cases, got):
        blocks, payload = encode(files)
        flat = [int(x) for v in files for x in v]
        assert g["blocks"] == blocks and g["payload"] == payload, name
        assert g["decoded"] == flat, name  # encode then decode is the identity
        assert g["sizes"] == (len(flat), len(blocks), len(payload)), name
        for (_, at, cnt, width), nxt in zip(blocks, blocks[1:] + [(0, len(payload), 0, 0)]):
            assert 1 <= cnt <= 512 and 0 <= width <= 64 and nxt[1] - at == -(-(cnt - 1) * width // 64), name


# ------------------------------------------------------------------------------------------------------------ the items
def packed_inputs(seed=5):
    """runs as the flat build has them, each a list of files: none, one hash, 64, two files of 300 + 513 over all 64 bits (a short block
    in the middle; crosses a word boundary of the bins, 60 .. 70), 1300 below 2^38 (ends in bin 129), the width-64 triple, 511 consecutive"""
    rng = np.random.default_rng(seed)
    runs = [[], [ascending(rng, 1, 1 << 64)], [ascending(rng, 64, 1 << 38)], [ascending(rng, 300, 1 << 64), ascending(rng, 513, 1 << 64)],
            [ascending(rng, 1300, 1 << 38)], [np.array([0, 1 << 63, M64], dtype=U64)], [np.arange(77, 77 + 511, dtype=U64)]]
    first_bin = [5, 6, 7, 60, 127, 20, 30]
    per_bin = [1, 1, 64, 74, 600, 1, 100]
    assert 60 + (813 - 1) // 74 == 70 and 127 + (1300 - 1) // 600 == 129
    return runs, first_bin, per_bin


def flat_runs(runs):
    return [np.concatenate([np.asarray(v, dtype=U64) for v in files]) if files else np.zeros(0, U64) for files in runs]


@pytest.mark.parametrize("cap_words,cap_items", [(700, 1 << 20), (1 << 20, 1 << 20), (700, 3), (511, 1)])
def test_items(driver, cap_words, cap_items):
    runs, _, _ = packed_inputs()
    enc = [encode(files) for files in runs]
    text = run(driver, f"items {cap_words} {cap_items} {len(runs)} " + " ".join(run_text(files) for files in runs) + "\n")
    chunks = []
    for ln in text.splitlines():
        f = ln.split()
        if f[0] == "chunk":
            chunks.append((int(f[1]), int(f[2]), []))
        else:
            assert f[0] == "item", ln
            chunks[-1][2].append((int(f[1]), int(f[2]), int(f[3]), int(f[4], 16), int(f[5]), int(f[6]), int(f[7])))
    seen = []
    for n_items, words, items in chunks:
        assert n_items == len(items) and 1 <= n_items <= cap_items and words <= cap_words, "both caps hold"
        at = 0
        for r, cnt, width, first, begin, stage_at, block in items:
            assert (first, cnt, width) == (enc[r][0][block][0], enc[r][0][block][2], enc[r][0][block][3]), "an item is one whole block"
            assert begin == sum(b[2] for b in enc[r][0][:block]), "begin is the index of the block's first hash in the RUN"
            assert stage_at == at, "the payloads of a chunk lie behind each other in the staging buffer"
            at += -(-(cnt - 1) * width // 64)
            seen.append((r, block))
        assert at == words
    assert seen == [(r, b) for r, (blocks, _) in enumerate(enc) for b in range(len(blocks))], "every block once, runs in order"
    if (cap_words, cap_items) == (700, 1 << 20):
        assert len(chunks) >= 3 and any(begin % 512 for _, _, items in chunks for r, _, _, _, begin, _, _ in items if r == 3), \
            "a payload cap of 700 words cuts the runs into several chunks; behind the short block begin is no multiple of 512"


# ------------------------------------------------------------------------------------------------------------ the window
def window_line(h, row_begin, n_rows, cap, runs, first_bin, per_bin):
    parts = ["window", str(TOTAL_ROWS), str(BINS), str(h), str(row_begin), str(n_rows), str(cap), str(len(runs))]
    for files, f, p in zip(runs, first_bin, per_bin):
        parts += [str(f), str(p), run_text(files)]
    return " ".join(parts) + "\n"


@pytest.mark.parametrize("h", [1, 3, 5])
@pytest.mark.parametrize("cap", [700, 1 << 20])
def test_window_model_equals_the_oracle(driver, cap, h):
    runs, first_bin, per_bin = packed_inputs()
    ref = oracle_filter(flat_runs(runs), first_bin, per_bin, h)
    text = run(driver, "".join(window_line(h, a, b - a, cap, runs, first_bin, per_bin) for a, b in zip(CUTS, CUTS[1:])))
    assert "refused" not in text, text
    got = np.array([[int(x, 16) for x in ln.split()] for ln in text.splitlines()], dtype=U64).reshape(TOTAL_ROWS, 3)
    assert np.array_equal(got, ref), "the slabs behind each other are the filter"
    assert ref.any() and not (got[:, 2] >> U64(BINS - 128)).any(), "the padding bits of the last word stay zero"


# ------------------------------------------------------------------------------------------------------------ the command's refusals
def test_refusals_that_need_no_device(tiny_input, tiny_index, tmp_path):
    inp, out = tiny_input
    flat = str(tmp_path / "x.ibf")
    why = "unions, sketches and probes read raw sets"
    for args, words in ((["-i", inp, "--hibf", "-o", out, "--hash-sets", "packed"], ["--hash-sets packed cannot be used with --hibf", why]),
                        (["-i", inp, "--hibf", "-o", out, "--hash-sets", "spilled"], ["--hash-sets spilled cannot be used with --hibf", why]),
                        (["-i", inp, "--hibf", "--verify-index", tiny_index, "--hash-sets", "packed"], ["--hash-sets packed cannot be used with --verify-index", why]),
                        (["-i", inp, "--hibf", "--update", tiny_index, "-o", out, "--hash-sets", "spilled"], ["--hash-sets spilled cannot be used with --update", why]),
                        (["-i", inp, "-o", flat, "--hash-sets", "zip"], ["--hash-sets has to be raw, packed or spilled"]),
                        (["-i", inp, "-o", flat, "--hash-sets", ""], ["--hash-sets has to be raw, packed or spilled"]),
                        (["-i", inp, "-o", flat, "--hash-sets"], ["is missing an argument"])):
        p = subprocess.run([BIN_BUILD] + args, capture_output=True, text=True)
        assert p.returncode == 1 and all(w in p.stderr for w in words) and p.stdout == "", (args, p.stderr)
        assert "device" not in p.stderr.lower().replace("--device", ""), "refused before the device is touched"
        assert not os.path.exists(out) and not os.path.exists(flat) and os.listdir(str(tmp_path)) == [], args
    # raw with the hierarchical modes is the command line of before: not refused for the switch (another refusal ends it here)
    p = subprocess.run([BIN_BUILD, "-i", inp, "--hibf", "-o", out, "--hash-sets", "raw", "--tmax", "1"], capture_output=True, text=True)
    assert p.returncode == 1 and "--tmax" in p.stderr and "--hash-sets" not in p.stderr
    p = subprocess.run([BIN_BUILD, "--help"], capture_output=True, text=True)
    assert p.returncode == 0 and "--hash-sets arg" in p.stderr and "raw (8 bytes a hash" in p.stderr and "spilled (packed, in one file per" in p.stderr
    assert "Default: raw; not with" in p.stderr
