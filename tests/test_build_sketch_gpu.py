"""`ganon-build --hibf --layout sketch` on the GPU: the HyperLogLog registers and the union table against a restatement of
include/ganon_hip.h in numpy / Python integers / float64, the estimate's accuracy, and the written index: every check of
test_build_hibf_gpu.check_file (sizing and payload are exact whatever the layout), no false negatives through ganon-classify, and
the size against the rule's index."""
import math
import os
import subprocess

import numpy as np
import pytest

import cli_util as cu
import ganon_fixtures as gf
import gpu_util as gu
import hibf_checks as hc
from test_build_cpu import BIN_BUILD
from test_build_hibf_gpu import (CASES, K, W, Inputs, build, check_file, cut_reads, genomes, hashes_of, hip, read_tree,  # noqa: F401
                                 short200)  # (genomes, short200 and hip are fixtures)

pytestmark = pytest.mark.gpu

M = 4096
NUM = (0.7213 / (1.0 + 1.079 / 4096.0)) * 2.0 ** 76
SMALL = [0.0] + [4096.0 * math.log(4096.0 / z) for z in range(1, M + 1)]


# ------------------------------------------------------------------------------------------------------------ the restatement
def mix(h):
    with np.errstate(over="ignore"):
        h = h ^ (h >> np.uint64(33))
        h = h * np.uint64(0xff51afd7ed558ccd)
        h = h ^ (h >> np.uint64(33))
        h = h * np.uint64(0xc4ceb9fe1a85ec53)
        h = h ^ (h >> np.uint64(33))
    return h


def registers(hashes):
    regs = np.zeros(M, dtype=np.uint8)
    if len(hashes) == 0:
        return regs
    x = mix(np.asarray(hashes, dtype=np.uint64))
    idx = (x >> np.uint64(52)).astype(np.int64)
    rest = x & np.uint64((1 << 52) - 1)
    bit_length = np.frexp(rest.astype(np.float64))[1]  # exact: rest is below 2^52
    rank = np.where(rest == 0, 52, 52 - bit_length + 1)
    for v in range(1, 53):  # ascending: the larger rank stays
        regs[idx[rank == v]] = v
    return regs


def estimate(u):
    z = int(np.count_nonzero(u == 0))
    if z == M:
        return 0
    s = sum(int(c) << (52 - v) for v, c in enumerate(np.bincount(u, minlength=53)))
    raw = NUM / float(s)
    return round(SMALL[z] if raw <= 10240.0 and z > 0 else raw)


def union_table(regs, order, width, j0, j1):
    n = len(order)
    out = np.zeros((j1 - j0, width), dtype=np.uint64)
    for j in range(j0, j1):
        u, best = np.zeros(M, dtype=np.uint8), 0
        for l in range(1, min(width, n - j) + 1):
            u = np.maximum(u, regs[order[j + l - 1]])
            best = max(best, estimate(u))
            out[j - j0, l - 1] = best
    return out


def random_set(rng, size, bits=38):
    return np.unique(rng.integers(0, 1 << bits, size=size, dtype=np.uint64))


# ------------------------------------------------------------------------------------------------------------ device steps
def test_registers(hip):
    from ganon_amd import hip as H
    rng = np.random.default_rng(11)
    top = random_set(rng, 70000, 63) * np.uint64(2) + np.uint64(1) + np.uint64(1 << 63)  # bit 63 set; several blocks
    sets = [random_set(rng, n) for n in (0, 1, 63, 64, 65, 5000)] + [top]
    sets += [sets[5], np.array([0], np.uint64), np.array([0xFFFFFFFFFFFFFFFF], np.uint64), top[:9000]]  # a set twice; 0 and ~0; two blocks
    sk = H.HipSketches(sets)
    got = sk.download()
    assert got.shape == (len(sets), M) and got.dtype == np.uint8
    for i, hs in enumerate(sets):
        assert np.array_equal(got[i], registers(hs)), (i, len(hs))
    assert not got[0].any() and got[6].max() <= 52 and np.array_equal(got[5], got[7])
    assert np.array_equal(sk.download(2, 3), got[2:5])
    with pytest.raises(H.GanonHipError):
        sk.download(len(sets), 1)
    sk.free()
    none = H.HipSketches([])
    assert none.download().shape == (0, M)
    none.free()


def test_registers_of_a_set_cut_by_a_round(hip):
    """more hashes than one upload holds: the middle set is cut by the end of the first round, the last set starts the second"""
    from ganon_amd import hip as H
    rng = np.random.default_rng(12)
    big = rng.integers(0, 1 << 62, size=(8 << 20) + 4000, dtype=np.uint64)  # (not unique, not sorted: neither matters to a sketch)
    sets = [random_set(rng, 3000), big, random_set(rng, 2000), random_set(rng, 20000)]
    sk = H.HipSketches(sets)
    got = sk.download()
    for i, hs in enumerate(sets):
        assert np.array_equal(got[i], registers(hs)), i
    sk.free()


@pytest.fixture(scope="module")
def seventy(hip):
    """70 sketches: small sets (the small-range branch), sets of 30 000 and more (the raw branch), an empty one in the middle,
    identical neighbours"""
    from ganon_amd import hip as H
    rng = np.random.default_rng(13)
    sets = [random_set(rng, int(rng.integers(1, 3000))) for _ in range(70)]
    sets[0] = random_set(rng, 40)
    for i in (5, 6, 40):
        sets[i] = random_set(rng, 30000 + 10000 * (i % 5))
    sets[35] = np.zeros(0, np.uint64)
    sets[20] = sets[19]
    sets[21] = sets[19]
    sets[41] = sets[40]
    sk = H.HipSketches(sets)
    regs = sk.download()
    for i in (0, 5, 19, 35, 69):
        assert np.array_equal(regs[i], registers(sets[i]))
    yield sk, regs, sets
    sk.free()


@pytest.mark.parametrize("width", [1, 3, 70])
def test_union_table(seventy, width):
    sk, regs, sets = seventy
    order = np.random.default_rng(width).permutation(70).astype(np.uint32)
    order[10:13] = (19, 20, 21)  # identical neighbours: the row stays flat
    order[30:33] = (7, 35, 8)    # the empty sketch in the middle
    order[50:52] = (40, 41)
    order[60] = 0                # 40 hashes
    got = sk.union_table(order, width)
    exp = union_table(regs, order, width, 0, 70)
    assert got.shape == (70, width) and np.array_equal(got, exp)
    if width == 70:
        assert got[10, 0] == got[10, 1] == got[10, 2] and got[30, 0] == got[30, 1] < got[30, 2]
        assert (got[69, 1:] == 0).all() and got[0, 69] > 0, "entries past the end are 0"
        raw = [j for j in range(70) if len(sets[order[j]]) >= 30000]
        assert raw and all(got[j, 0] > 10240 for j in raw) and got[60, 0] < 100, "both branches of the estimate"
    for j in range(70):
        row = got[j, :min(width, 70 - j)]
        assert (np.diff(row.astype(np.int64)) >= 0).all(), j


def test_union_table_tile_and_single(seventy):
    from ganon_amd import hip as H
    sk, regs, sets = seventy
    order = np.arange(70, dtype=np.uint32)[::-1].copy()
    whole = sk.union_table(order, 9)
    assert np.array_equal(sk.union_table(order, 9, 17, 43), whole[17:43]), "a tile strictly inside"
    assert np.array_equal(whole[17:43], union_table(regs, order, 9, 17, 43))
    assert sk.union_table(order, 9, 5, 5).shape == (0, 9)
    one = sk.union_table(np.array([6], np.uint32), 4)  # n = 1
    assert one.tolist() == [[estimate(regs[6]), 0, 0, 0]]
    same = sk.union_table(np.array([6, 6, 6], np.uint32), 3)  # a sketch may be named more than once
    assert same[0].tolist() == [estimate(regs[6])] * 3
    too_wide = H.SKETCH_TABLE_MAX // 70 + 1
    with pytest.raises(H.GanonHipError) as e:
        sk.union_table(order, too_wide)
    assert e.value.code == -34, "GN_ERANGE above the stated number of entries"
    assert sk.union_table(order, H.SKETCH_TABLE_MAX // 70, 69, 70).shape == (1, H.SKETCH_TABLE_MAX // 70)  # (the limit is per call)
    for bad in (np.array([70], np.uint32), np.array([3, 0xFFFFFFFF], np.uint32)):  # no such sketch: refused before the launch
        with pytest.raises(H.GanonHipError):
            sk.union_table(bad, 2)
    with pytest.raises(H.GanonHipError):
        sk.union_table(order, 2, 3, 71)


def test_estimates_are_within_five_standard_errors(hip):
    """20 unions of 10 000 hashes and more, of sets that share hashes: within 8 % = 5 * 1.04 / sqrt(4096) of the exact size"""
    from ganon_amd import hip as H
    rng = np.random.default_rng(14)
    common = random_set(rng, 6000)
    sets = [np.union1d(random_set(rng, int(rng.integers(4000, 60000))), common[: int(rng.integers(0, 6000))]) for _ in range(24)]
    sk = H.HipSketches(sets)
    table = sk.union_table(np.arange(24, dtype=np.uint32), 5)
    checked = 0
    for j in range(20):
        exact = len(np.unique(np.concatenate(sets[j:j + 5])))
        assert exact >= 10000
        err = abs(int(table[j, 4]) - exact) / exact
        print(f"union {j}: exact {exact} estimate {int(table[j, 4])} error {err:.4f}")
        assert err <= 0.08
        checked += 1
    assert checked == 20
    sk.free()


# ------------------------------------------------------------------------------------------------------------ the written index
SKETCH = ("--layout", "sketch")


@pytest.fixture(scope="module")
def large40(tmp_path_factory):
    """one target of 64 kbp and 39 of 1 kbp: at tmax 8 the large one is split in the root, beside merged bins"""
    d = tmp_path_factory.mktemp("hibf_large40")
    rng = np.random.default_rng(40)
    tsv = str(d / "large_input.tsv")
    order, seqs = [], {}
    with open(tsv, "w") as o:
        for t in range(40):
            name = f"L{t}"
            order.append(name)
            seqs[name] = [gu.random_seq(rng, 64000 if t == 3 else 1000).decode()]
            path = str(d / f"{name}.fasta")
            gf.write_fasta(path, [(name, seqs[name][0])])
            o.write(f"{path}\t{name}\n")
    return Inputs(tsv, order, seqs)


@pytest.fixture(scope="module")
def equal40(tmp_path_factory):
    d = tmp_path_factory.mktemp("hibf_equal40")
    rng = np.random.default_rng(41)
    tsv = str(d / "equal_input.tsv")
    order, seqs = [], {}
    with open(tsv, "w") as o:
        for t in range(40):
            name = f"E{t}"
            order.append(name)
            seqs[name] = [gu.random_seq(rng, 2000).decode()]
            path = str(d / f"{name}.fasta")
            gf.write_fasta(path, [(name, seqs[name][0])])
            o.write(f"{path}\t{name}\n")
    return Inputs(tsv, order, seqs)


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    """index files by (input, layout, tmax, s, max_fp, min_length): the size tests and the index tests share their builds"""
    d = tmp_path_factory.mktemp("hibf_sketch_built")
    made = {}

    def get(inp, layout, tmax, s, max_fp, min_length=0):
        key = (id(inp), layout, tmax, s, max_fp, min_length)
        if key not in made:
            out = str(d / f"db{len(made)}.hibf")
            build(inp, out, tmax, s, max_fp, min_length, extra=SKETCH if layout == "sketch" else ())
            made[key] = out
        return made[key]
    return get


@pytest.mark.parametrize("which,tmax,s,max_fp,min_length", CASES + [("large40", 8, 3, 0.001, 0), ("short200", 8, 3, 0.001, 0)])
def test_index_against_the_oracle(hip, request, built, which, tmax, s, max_fp, min_length):
    inp = request.getfixturevalue(which)
    out = built(inp, "sketch", tmax, s, max_fp, min_length)
    m, hb, depth = check_file(out, inp, tmax, s, max_fp, min_length)
    names, _ = inp.sets(min_length)
    assert max(depth) + 1 <= hc.levels_for(len(names), tmax) and (len(names) > tmax or len(m.ibfs) == 1)
    if (which, tmax) in (("genomes", 8), ("short200", 4), ("large40", 8)):  # two builds of one input: the same bytes
        again = out + ".again"  # (beside the first: the index names files in the directory it is written to)
        build(inp, again, tmax, s, max_fp, min_length, extra=SKETCH)
        assert open(out, "rb").read() == open(again, "rb").read()
    if which == "large40":
        _, runs, _, _, where = read_tree(out, len(names), tmax)
        i, first, n = where[names.index("L3")]
        assert i == 0 and n >= 2, "the large user bin is split in the root"
        assert any(user < 0 for _, _, user, _ in runs[0]), "... beside merged bins"


def test_verbose_names_the_layout(hip, short200, tmp_path):
    a, b = str(tmp_path / "a.hibf"), str(tmp_path / "b.hibf")
    for extra, word, out in ((SKETCH, "sketch", str(tmp_path / "v.hibf")), ((), "rule", a)):
        p = build(short200, out, 8, extra=tuple(extra) + ("--verbose",))
        block = p.stderr[p.stderr.index("hibf_config:"):]
        assert f"layout         {word}\n" in block, block[:400]
    build(short200, b, 8, extra=("--layout", "rule"))
    assert open(a, "rb").read() == open(b, "rb").read(), "rule is the default"


def test_no_false_negatives_and_the_classify_side_agrees(hip, short200, built, tmp_path):
    tmax, s, max_fp = 8, 3, 0.001
    out = built(short200, "sketch", tmax, s, max_fp)
    names, sets = short200.sets(0)
    reads = cut_reads(short200, 0, np.random.default_rng(tmax))
    assert {t for _, _, t in reads if t} == set(names), "reads from every target"
    fq = str(tmp_path / "reads.fq")
    gf.write_fastq(fq, [(rid, seq) for rid, seq, _ in reads])
    outs = {}
    for tag, binary in (("hip", cu.BIN_HIP), ("oracle", cu.build_oracle_binary())):
        prefix = str(tmp_path / tag)
        cu.run(binary, ["--ibf", out, "--hibf", "--single-reads", fq, "-o", prefix, "--output-all", "--skip-lca", "--rel-cutoff", "1",
                        "--rel-filter", "1", "--quiet"])
        outs[tag] = (open(prefix + ".all", "rb").read(), open(prefix + ".rep", "rb").read())
    assert outs["hip"][0] == outs["oracle"][0], ".all"
    assert outs["hip"][1] == outs["oracle"][1], ".rep"
    found = {}
    for line in outs["hip"][0].decode().splitlines():
        rid, target, count = line.split("\t")
        found.setdefault(rid, {})[target] = int(count)
    for rid, seq, source in reads:
        if source is not None:  # every hash of the read is in its source's user bin: it is reported, with all of them
            assert found.get(rid, {}).get(source) == len(hashes_of(seq)), (rid, source, found.get(rid))


@pytest.mark.parametrize("which,tmax,bound", [("short200", 8, 0.8), ("short200", 64, 0.8), ("large40", 8, 0.8), ("genomes", 8, 1.02), ("genomes", 64, 1.02),
                                              ("equal40", 8, 1.02)])
def test_size_against_the_rule(hip, request, built, which, tmax, bound):
    inp = request.getfixturevalue(which)
    sketch = os.path.getsize(built(inp, "sketch", tmax, 3, 0.001))
    rule = os.path.getsize(built(inp, "rule", tmax, 3, 0.001))
    print(f"{which} tmax {tmax}: sketch {sketch} bytes, rule {rule} bytes, ratio {sketch / rule:.3f}")
    assert sketch <= bound * rule
