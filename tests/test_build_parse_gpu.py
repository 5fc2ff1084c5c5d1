"""`ganon-build --parse device` on the GPU: the genomes travel as text and are tokenised there (csrc/gn_genome.hip, host/hasher.hpp
hash_text_file).  The host path stays the authority: every file written, stdout, the totals and the `Error parsing file` lines have to be
those of `--parse host` -- with the default chunk and with chunks of 4 KiB, which cut every genome into many texts and open records."""
import filecmp
import gzip
import os
import re
import subprocess

import numpy as np
import pytest

from test_build_cpu import BIN_BUILD, DATA

pytestmark = pytest.mark.gpu

MODES = {"flat": [], "hibf": ["--hibf"], "packed": ["--hash-sets", "packed"], "hibf_packed": ["--hibf", "--hibf-hash-sets", "packed"],
         "min_length": ["--min-length", "500"]}


def dna(rng, n, alphabet="ACGT"):
    return "".join(rng.choice(list(alphabet), n))


def wrap(s, width, eol="\n"):
    return "".join(s[i:i + width] + eol for i in range(0, len(s), width))


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    """the 25 genomes of the reference's build tests, and crafted files with what genome files come with"""
    import ganon_amd
    ganon_amd.load_library()
    assert ganon_amd.device_count() >= 1 and os.path.exists(BIN_BUILD)
    d = tmp_path_factory.mktemp("build_parse")
    rng = np.random.default_rng(17)
    rows = []
    for line in open(os.path.join(DATA, "mode_input.tsv")):
        f, t = line.split()
        rows.append((os.path.join(DATA, f), f"G{t}"))

    def put(name, text, target, binary=False):
        path = str(d / name)
        data = text if binary else text.encode()
        (gzip.open if name.endswith(".gz") else open)(path, "wb").write(data)
        rows.append((path, target))

    put("crlf.fna", ">c1 crlf\r\n" + wrap(dna(rng, 3000), 60, "\r\n") + ">c2\r\n" + wrap(dna(rng, 900), 70, "\r\n"), "CRLF")
    put("digits.fasta", ">d1 numbered\n" + "".join(f"{i + 1:9d} {s[:10]} {s[10:20]} {s[20:30]}\n" for i, s in
                                                  ((i, dna(rng, 30)) for i in range(0, 2400, 30))), "DIGITS")
    put("short.fa", ">s1 below k\nACGTACGTAC\n>s2 between k and w\n" + dna(rng, 25) + "\n>s3\n" + wrap(dna(rng, 2000), 80) + ">s4 empty\n>s5 also short\n"
        + dna(rng, 30) + "\n>s6 exactly w\n" + dna(rng, 31) + "\n", "SHORT")
    put("odd.fna", "\n\n;a comment header\n" + wrap(dna(rng, 1500, "ACGTacgtNRYKM"), 61) + "\n\n>o2 ACGT>ACGT\n" + wrap(dna(rng, 700), 7)
        + ">o3 no newline at the end\n" + wrap(dna(rng, 1300), 70)[:-1], "ODD")
    put("longline.fna", ">l1 one line\n" + dna(rng, 10000) + "\n>l2\n" + wrap(dna(rng, 800), 60), "LONG")
    put("wrapped.fna", ">w1 a genome as it comes\n" + wrap(dna(rng, 30000), 70) + ">w2 plasmid\n" + wrap(dna(rng, 12000), 70) + ">w3\n" + wrap(dna(rng, 5000), 70), "WRAPPED")
    put("wrapped80.fna.gz", ">x1\n" + wrap(dna(rng, 50000, "ACGTN"), 80) + ">x2\n" + wrap(dna(rng, 400), 80), "WRAPPED80")
    put("two.a.fna", ">t1\n" + wrap(dna(rng, 2500), 60), "TWO")
    put("two.b.fna.gz", ">t2\n" + wrap(dna(rng, 1800), 60) + ">t3\n" + wrap(dna(rng, 600), 60), "TWO")
    put("bad.good.fna", ">b0\n" + wrap(dna(rng, 1200), 60), "BAD")
    put("bad.fna", ">b1\n" + wrap(dna(rng, 1000), 60) + ">b2\n" + wrap(dna(rng, 500), 60) + "ACGTEACGT\n" + wrap(dna(rng, 500), 60), "BAD")
    put("nohdr.good.fna", ">n0\n" + wrap(dna(rng, 1100), 60), "NOHDR")
    put("nohdr.fna", wrap(dna(rng, 300), 60) + ">n1\n" + wrap(dna(rng, 900), 60), "NOHDR")
    fq = "".join(f"@r{i}\n{s}\n+\n{'I' * len(s)}\n" for i, s in ((i, dna(rng, 150)) for i in range(20)))
    put("reads.fastq", fq, "FASTQ")
    tsv = str(d / "input.tsv")
    open(tsv, "w").write("".join(f"{f}\t{t}\n" for f, t in rows))
    return d, tsv


def build(d, tsv, name, mode, parse, chunk=None, verbose=False):
    out = str(d / f"{name}.{parse}{'.chunked' if chunk else ''}.{'hibf' if '--hibf' in mode else 'ibf'}")
    env = dict(os.environ)
    env.pop("GANON_BUILD_PARSE_CHUNK", None)
    if chunk:
        env["GANON_BUILD_PARSE_CHUNK"] = str(chunk)
    args = [BIN_BUILD, "-i", tsv, "-o", out, "--max-fp", "0.05", "-t", "2", "--parse", parse] + mode + (["--verbose"] if verbose else [])
    p = subprocess.run(args, capture_output=True, text=True, timeout=300, env=env)
    assert p.returncode == 0, (args, p.stderr[-3000:])
    return out, p


def said(stderr):
    """what of stderr does not depend on the clock: the parse errors (in any order: two hashing threads) and the totals"""
    errors = sorted(ln for ln in stderr.splitlines() if ln.startswith("Error parsing file"))
    totals = re.search(r"processed (\d+) sequences / (\d+) files \(([^ ]+) Mbp\)", stderr)
    skipped = re.search(r" - (\d+) sequences skipped", stderr)
    assert totals, stderr[-2000:]
    return errors, totals.groups(), skipped.group(1) if skipped else None


@pytest.mark.parametrize("name", list(MODES))
def test_device_parse_writes_the_host_parse_file(inputs, name):
    d, tsv = inputs
    host, ph = build(d, tsv, name, MODES[name], "host")
    dev, pd = build(d, tsv, name, MODES[name], "device", verbose=name == "flat")
    assert filecmp.cmp(host, dev, shallow=False)
    assert pd.stdout == ph.stdout
    assert said(pd.stderr) == said(ph.stderr)
    assert len(said(ph.stderr)[0]) == 2 and "bad.fna" in said(ph.stderr)[0][0] and "nohdr.fna" in said(ph.stderr)[0][1]
    if name == "flat":
        # 25 + crlf, digits, short, odd, longline, wrapped, wrapped80, two.a, two.b, bad.good, nohdr.good on the device; bad and nohdr read
        # again; the FASTQ name never tried
        m = re.search(r"parse device: (\d+) files tokenised on the device, (\d+) fell back to the host reader, (\d+) not eligible, (\d+) text bytes", pd.stderr)
        assert m and [int(x) for x in m.groups()[:3]] == [36, 2, 1] and int(m.group(4)) > 25 * 10000, pd.stderr[-3000:]
        assert "--parse             device" in pd.stderr
    # many chunks and open records: the same file, the same words
    chunked, pc = build(d, tsv, name, MODES[name], "device", chunk=4096, verbose=name == "flat")
    assert filecmp.cmp(host, chunked, shallow=False)
    assert pc.stdout == ph.stdout and said(pc.stderr) == said(ph.stderr)
    if name == "flat":
        # bad and nohdr are read again, and so is every file with a line longer than a chunk (no newline in a buffer): longline and the
        # 25 genomes of the reference's tests, which hold their sequence on one line.  The wrapped files stay on the device in many chunks, their
        # long records open across several: a record cut with fewer than w letters so far would need a
        # 4 KiB buffer of little but header, blank and ignored bytes
        m = re.search(r"parse device: (\d+) files tokenised on the device, (\d+) fell back", pc.stderr)
        assert m and [int(x) for x in m.groups()] == [10, 28], pc.stderr[-3000:]


def test_verify_index_with_device_parse(inputs):
    d, tsv = inputs
    index, _ = build(d, tsv, "verify", ["--hibf"], "host")
    reports = []
    for parse, chunk in (("host", None), ("device", None), ("device", 4096)):
        env = dict(os.environ)
        env.pop("GANON_BUILD_PARSE_CHUNK", None)
        if chunk:
            env["GANON_BUILD_PARSE_CHUNK"] = str(chunk)
        p = subprocess.run([BIN_BUILD, "--hibf", "--verify-index", index, "-i", tsv, "-t", "2", "--parse", parse], capture_output=True, text=True, timeout=300, env=env)
        assert p.returncode == 0, p.stderr[-3000:]
        reports.append((p.stdout, sorted(ln for ln in p.stderr.splitlines() if ln.startswith("Error parsing file"))))
    assert reports[0][0].splitlines()[-1].startswith("result\t") and len(reports[0][1]) == 2
    assert reports[1] == reports[0] and reports[2] == reports[0]
