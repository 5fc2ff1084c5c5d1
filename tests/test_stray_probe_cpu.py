"""The staged probe of the fast count kernel's finish (ganon_amd/csrc/gn_stray_probe.h) without a GPU.

The drop tests -- the very functions both finish sites call -- run in a stand-alone driver (tests/stray_probe_driver.cpp) under
AddressSanitizer and UBSan, nothing preloaded: by brute force over hit patterns for n <= 12 (stage 1 drops exactly when no completion
of the bits it has not seen reaches T; stage 2 never drops a bin that can), and by counts for n <= 127.  On the words both see, the
staged rule is the one-stage rule made tighter by what stage 1 counted: whatever one stage dropped, stage 2 drops (the other direction
does not hold, and is not meant to: e <= the hashes below F' with rows 2 and 3).

The Python restatement of the whole flow (tests/stray_probe_model.py), which the GPU test uses as the expected byte tally, is held
here against the header's screen table, against the oracle's matches on the reads of test_gpu_row_screen.py, and against itself with
F = 0: the same reports, no more words, and strays that fall in stage 1."""
import os
import subprocess

import numpy as np
import pytest

import gpu_util as gu
import oracle
import stray_probe_model as model
from ganon_amd import build as B
from test_gpu_row_screen import K, W, _workload

HERE = os.path.dirname(os.path.abspath(__file__))
CUTOFFS = (0.55, 0.75, 0.9, 1.0)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("stray_probe") / "stray_probe_driver")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                           os.path.join(HERE, "stray_probe_driver.cpp"), "-I", B.CSRC])
    return exe


def _run(driver, *args):
    p = subprocess.run([driver, *args], capture_output=True, text=True)
    assert p.returncode == 0 and p.stderr == "", (p.returncode, p.stdout[-500:], p.stderr[-3000:])  # (a sanitizer report ends the program with a status)
    return p.stdout


def test_the_bound_by_patterns(driver):
    out = _run(driver, "bound").split()
    assert out[0] == "ok" and int(out[1]) > 1_000_000 and int(out[3]) == model.PROBE_HASHES


def test_the_bound_by_counts(driver):
    out = _run(driver, "counts").split()
    assert out[0] == "ok" and int(out[1]) > 10_000_000


@pytest.mark.parametrize("cutoff", CUTOFFS + (0.2,))
@pytest.mark.parametrize("bins", [64, 4096, 8192])
def test_the_restated_table_is_the_headers(driver, cutoff, bins):
    vals = [int(x) for x in _run(driver, "table", repr(cutoff), "4", str(bins)).split()]
    assert [0] + vals[0::2] == model.screen_table(cutoff, 4, bins)


@pytest.fixture(scope="module")
def restated():
    ibf, reads, _, _, expect = _workload(4096, 5003, 4, 0.5)
    hashes = [oracle.minimiser_hash(oracle.to_ranks(s), K, W) for s in reads]
    return (ibf, hashes, expect) + model.batch(ibf, hashes, CUTOFFS, 1)


@pytest.mark.parametrize("cutoff", CUTOFFS)
def test_restatement_reports_what_the_oracle_reports(restated, cutoff):
    ibf, hashes, _, _, _, reports = restated
    b2t = np.arange(ibf.bins, dtype=np.uint32)
    for r, hs in enumerate(hashes):
        assert reports[cutoff][r] == gu.oracle_matches(ibf, b2t, ibf.bins, hs, cutoff)[0], (cutoff, r)


def test_staged_probe_loads_less_and_decides_the_same(restated):
    _, hashes, expect, skipped, tally, _ = restated
    for cutoff in CUTOFFS:
        new, old = tally[(cutoff, model.PROBE_HASHES)], tally[(cutoff, 0)]
        print(cutoff, {k: v for k, v in new.items() if k != "trace"}, {k: v for k, v in old.items() if k != "trace"})
        for k in ("unscreened", "dead", "aborted", "finish", "clean"):
            assert new[k] == old[k], (cutoff, k)
        assert old["drop1"] == 0 and old["stage1_words"] == 0, "one stage: nothing is known, nothing is loaded first"
        assert new["drop1"] + new["drop2"] >= old["drop2"] and new["full"] <= old["full"]
        assert skipped[(cutoff, model.PROBE_HASHES)] >= skipped[(cutoff, 0)]
    new, old = tally[(0.75, model.PROBE_HASHES)], tally[(0.75, 0)]
    assert new["finish"] > 100 and new["clean"] > 50 and new["drop1"] > 20, "error-free reads, and strays that fall on their first hashes"
    assert skipped[(0.75, model.PROBE_HASHES)] > skipped[(0.75, 0)]
    # a bin that falls in stage 1 cost 2 m <= 2 F words where one stage cost 2 ds (the probed bins of this batch are strays and the
    # bins of mutated reads, which pass both stages: the mean is over both kinds)
    lines_new = (new["stage1_words"] + new["stage2_words"]) / (new["drop1"] + new["drop2"] + new["full"])
    lines_old = old["stage2_words"] / (old["drop2"] + old["full"])
    print(f"words a probed bin: {lines_new:.1f} staged, {lines_old:.1f} in one stage")
    assert lines_new < lines_old
    assert all(m <= model.PROBE_HASHES and e <= m for _, _, stage, m, e in new["trace"])
    # the adversaries of test_gpu_row_screen.py (every hash hits rows 0 and 1: c2 == ds) take no probe at all
    clean = {(at[0], b) for at, b, stage, _, _ in new["trace"] if stage == "clean"}
    for r, b, _ in expect[:8]:
        assert (r, b) in clean
