"""An HIBF over one device's budget as a feature of the product binary: it is dealt to the --device entries by subtree (root bins with
everything below them, ganon_amd/host/hibf_partition.hpp), every part classifies every batch, and the parts' matches are merged on
the batch's owner device (gn_gather_create_merged).  The reference loads a filter of any size (GanonClassify.cpp:875-938), so every
output byte must be the one the unpartitioned run and the oracle-backend twin write.

One GPU on the test box: $GANON_DEVICE_BUDGET turns every --device ENTRY into a placement device with that budget."""
import os
import subprocess

import numpy as np
import pytest

import cli_util as cu
import ganon_fixtures as gf
import hibf_partition_checks as hp
from test_cli_kat import oracle_bin  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

EXTS = (".all", ".unc", ".rep")
BIG = np.iinfo(np.int64).max - 1


def _db(d, n_user_bins, tmax, seed, name="ub"):
    h, reads, _ = hp.planted_fixture(n_user_bins, tmax, seed, n_planted=300, n_random=100)
    path = os.path.join(d, "x.hibf")
    gf.write_hibf(path, h, [[f"/x/{name}{i}.minimiser"] for i in range(n_user_bins)], hp.K, hp.W, 0.05)
    fq, fq2 = os.path.join(d, "r.fq"), os.path.join(d, "r2.fq")
    gf.write_fastq(fq, [(f"r{i}", s) for i, s in enumerate(reads)])
    gf.write_fastq(fq2, [(f"r{i}", hp.revcomp(s)) for i, s in enumerate(reads)])
    units = hp.units_of(h)
    C = hp.cost_matrix(h, units)
    three = hp.optimum(C, [BIG] * 3)  # the smallest budget at which the restated plan places three parts
    largest_unit = max(int(C[a, a + 1]) for a in range(len(units)))
    return dict(ibf=path, fq=fq, fq2=fq2, budget=str(three), below=str(largest_unit - 1), hibf=h, bytes=sum(hp.ibf_bytes(h, i) for i in range(len(h.ibfs))))


@pytest.fixture(scope="module")
def wide_hibf(tmp_path_factory):
    return _db(str(tmp_path_factory.mktemp("hibf_wide")), 600, 192, 7)  # a root of three words


@pytest.fixture(scope="module")
def small_hibf(tmp_path_factory):
    return _db(str(tmp_path_factory.mktemp("hibf_small")), 20, 64, 3, name="other")


@pytest.fixture(scope="module")
def narrow_hibf(tmp_path_factory):
    return _db(str(tmp_path_factory.mktemp("hibf_narrow")), 200, 64, 9)  # a root of one word: every part holds it whole


def _run(binary, db, out, extra=(), env=None, check=True, paired=False):
    e = dict(os.environ)
    e.update(env or {})
    cutoff = [] if "--rel-cutoff" in extra else ["--rel-cutoff", "0.3"]
    reads = ["--paired-reads", db["fq"] + "," + db["fq2"]] if paired else ["--single-reads", db["fq"]]
    p = subprocess.run([binary, "--ibf", db["ibf"], "--hibf"] + reads + ["-o", out, "--output-all", "--output-unclassified", "--quiet"]
                       + cutoff + list(extra), capture_output=True, text=True, env=e, timeout=900)
    if check:
        assert p.returncode == 0, p.stderr
    return p


def _same(a, b, exts=EXTS):
    for ext in exts:
        assert open(a + ext, "rb").read() == open(b + ext, "rb").read(), ext


def _spread_env(db, **more):
    return dict({"GANON_DEVICE_BUDGET": db["budget"], "GANON_HOST_TIMING": "1"}, **more)


def test_hibf_over_budget_is_spread_by_subtree_and_changes_no_output_byte(oracle_bin, wide_hibf, tmp_path):
    db = wide_hibf
    whole, ora = str(tmp_path / "whole"), str(tmp_path / "ora")
    _run(cu.BIN_HIP, db, whole)
    _run(oracle_bin, db, ora)
    _same(whole, ora)
    assert os.path.getsize(whole + ".all") > 1000
    for name, devs, env in (("three", "0,0,0", {}), ("four", "0,0,0,0", {}), ("copies", "0,0,0", {"GANON_HIP_ABLATE": "gather_copy"}),
                            ("batches", "0,0,0", {"GANON_HOST_BATCH_READS": "37"}),
                            ("one_worker", "0,0,0", {"GANON_PARTITION_WORKERS": "1", "GANON_HOST_BATCH_READS": "100"}),
                            # the reads as pieces of FASTQ text, records found on the device (the part that takes a batch takes the text)
                            ("text", "0,0,0", {"GANON_HOST_PARALLEL_MIN": "0", "GANON_HOST_SLAB_BYTES": "65536", "GANON_HOST_PARSE_THREADS": "3"})):
        out = str(tmp_path / name)
        p = _run(cu.BIN_HIP, db, out, ["--device", devs], _spread_env(db, **env))
        assert "partitioned by subtree: [root bins 0-" in p.stderr and 3 <= p.stderr.count("-> device 0]") <= len(devs.split(",")), p.stderr
        _same(out, whole)
        if "GANON_HIP_ABLATE" in env:
            assert "moved between devices" in p.stderr and "MiB of matches gathered" in p.stderr, p.stderr[-800:]
        assert ("tokenised on the device" in p.stderr) == (name == "text"), p.stderr[-500:]
    # without the budget the same command line replicates, and its log is what it was
    p = _run(cu.BIN_HIP, db, str(tmp_path / "repl"), ["--device", "0,0,0"], {"GANON_HOST_TIMING": "1"})
    assert "replicated on 1 device(s)" in p.stderr and "partitioned" not in p.stderr
    _same(str(tmp_path / "repl"), whole)


def test_spread_hibf_with_paired_reads(oracle_bin, wide_hibf, tmp_path):
    db = wide_hibf
    ora, got = str(tmp_path / "ora"), str(tmp_path / "got")
    _run(oracle_bin, db, ora, paired=True)
    p = _run(cu.BIN_HIP, db, got, ["--device", "0,0,0"], _spread_env(db), paired=True)
    assert "partitioned by subtree" in p.stderr
    _same(got, ora)
    _run(cu.BIN_HIP, db, got + "_whole", paired=True)
    _same(got, got + "_whole")


def test_spread_hibf_with_the_filter_matches_prepass(oracle_bin, wide_hibf, tmp_path):
    # the parts take part in ONE joint device pre-pass (their targets are disjoint), survivors only are merged; .sta carries the
    # discarded-match totals
    db = wide_hibf
    thr = ["--rel-cutoff", "0.2", "--rel-filter", "0.1", "--fpr-query", "1e-5", "--output-stats"]
    ora, whole, got = str(tmp_path / "ora"), str(tmp_path / "whole"), str(tmp_path / "got")
    _run(oracle_bin, db, ora, thr)
    _run(cu.BIN_HIP, db, whole, thr)
    _same(whole, ora, EXTS + (".sta",))
    p = _run(cu.BIN_HIP, db, got, thr + ["--device", "0,0,0"], _spread_env(db))
    assert "partitioned by subtree" in p.stderr and "pre-pass on the device on (1 filter(s)" in p.stderr, p.stderr
    _same(got, ora, EXTS + (".sta",))
    # and with the pre-pass off (everything judged on the host): the same bytes
    p = _run(cu.BIN_HIP, db, got + "_host", thr + ["--device", "0,0,0"], _spread_env(db, GANON_HOST_NO_PREFILTER="1"))
    assert "partitioned by subtree" in p.stderr
    _same(got + "_host", ora, EXTS + (".sta",))


def test_level_with_a_replicated_and_a_spread_hibf(oracle_bin, wide_hibf, small_hibf, tmp_path):
    # two filters on one hierarchy level (disjoint target names): the small one fits everywhere and is replicated, the large one is spread
    # over what the devices have left.  (--hibf holds for every filter of a run, as in the reference: a flat .ibf cannot share the run.)
    db = wide_hibf
    args = lambda out: ["--ibf", small_hibf["ibf"] + "," + db["ibf"], "--hibf", "--single-reads", db["fq"] + "," + small_hibf["fq"], "-o", out,  # noqa: E731
                        "--output-all", "--output-unclassified", "--output-stats", "--rel-cutoff", "0.3", "--rel-filter", "0.2", "--quiet"]
    ora, got = str(tmp_path / "ora"), str(tmp_path / "got")
    cu.run(oracle_bin, args(ora))
    env = dict(os.environ, GANON_DEVICE_BUDGET=str(int(db["budget"]) + small_hibf["bytes"]), GANON_HOST_TIMING="1", GANON_HOST_BATCH_READS="300")
    p = subprocess.run([cu.BIN_HIP] + args(got) + ["--device", "0,0,0"], capture_output=True, text=True, env=env, timeout=900)
    assert p.returncode == 0, p.stderr
    assert "replicated on 1 device(s)" in p.stderr and "partitioned by subtree" in p.stderr, p.stderr
    _same(got, ora, EXTS + (".sta",))


def test_root_of_one_word_is_held_by_every_part(oracle_bin, narrow_hibf, tmp_path):
    db = narrow_hibf
    ora, got = str(tmp_path / "ora"), str(tmp_path / "got")
    _run(oracle_bin, db, ora)
    p = _run(cu.BIN_HIP, db, got, ["--device", "0,0,0"], _spread_env(db))
    assert "partitioned by subtree: [root bins 0-" in p.stderr and p.stderr.count("-> device 0]") >= 2, p.stderr
    _same(got, ora)
    _run(cu.BIN_HIP, db, got + "_whole")
    _same(got, got + "_whole")


def test_hibf_that_cannot_be_placed_is_refused_with_the_piece_named(wide_hibf, tmp_path):
    db = wide_hibf
    out = str(tmp_path / "x")
    p = _run(cu.BIN_HIP, db, out, ["--device", "0,0,0"], {"GANON_DEVICE_BUDGET": db["below"]}, check=False)
    assert p.returncode != 0 and "does not fit" in p.stderr and "cannot be partitioned" in p.stderr, p.stderr
    assert "the subtree under root bin" in p.stderr
    assert not [f for f in os.listdir(str(tmp_path)) if f.startswith("x.")]  # no output file is written
