"""`ganon-build --hibf --layout similarity` on the GPU: gn_sketches_pair_table against a restatement of include/ganon_hip.h in
Python integers / float64 over the downloaded registers, the estimate's accuracy on pairs of known overlap, the similarity order
computed from the device's estimates, and the written index: every check of test_build_hibf_gpu.check_file, the size against
`--layout sketch`'s index, no false negatives through ganon-classify."""
import os
import re

import numpy as np
import pytest

import cli_util as cu
import ganon_fixtures as gf
import gpu_util as gu
from test_build_hibf_gpu import Inputs, build, check_file, cut_reads, hashes_of, hip, short200  # noqa: F401  (hip and short200 are fixtures)
from test_build_similarity_cpu import contiguous, driver, families, order_of  # noqa: F401  (driver is a fixture)
from test_build_sketch_gpu import M, estimate, large40, random_set, registers  # noqa: F401  (large40 is a fixture)

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------------------ the pair table
def pair_table(regs, idx):
    """include/ganon_hip.h: E of the registers' maximum, for every two of idx; every pair is computed on its own, both ways round"""
    out = np.zeros((len(idx), len(idx)), dtype=np.uint64)
    for a, i in enumerate(idx):
        for b, j in enumerate(idx):
            out[a, b] = estimate(np.maximum(regs[i], regs[j]))
    return out


@pytest.fixture(scope="module")
def sixty_five(hip):
    """65 sketches: an empty set, sets of 1, 5 and 300 hashes (the small-range branch), two of 70 000 (the raw branch), a set twice,
    and sets of up to 3000 hashes"""
    from ganon_amd import hip as H
    rng = np.random.default_rng(21)
    sets = [random_set(rng, int(rng.integers(1, 3000))) for _ in range(65)]
    sets[0] = np.zeros(0, np.uint64)
    sets[1], sets[2], sets[3] = random_set(rng, 1), random_set(rng, 5), random_set(rng, 300)
    sets[4], sets[5] = random_set(rng, 70000, 50), random_set(rng, 70000, 50)
    sets[6] = np.zeros(0, np.uint64)
    sets[30] = sets[29]
    sk = H.HipSketches(sets)
    regs = sk.download()
    for i in (0, 1, 4, 29, 64):
        assert np.array_equal(regs[i], registers(sets[i]))
    yield sk, regs, sets
    sk.free()


@pytest.mark.parametrize("m", [1, 2, 17, 65])
def test_pair_table(sixty_five, m):
    sk, regs, sets = sixty_five
    idx = np.arange(m, dtype=np.uint32) if m != 2 else np.array([4, 3], np.uint32)
    got = sk.pair_table(idx)
    assert got.shape == (m, m) and got.dtype == np.uint64
    assert np.array_equal(got, pair_table(regs, idx))
    assert np.array_equal(got, got.T), "symmetric"
    assert [int(got[a, a]) for a in range(m)] == [estimate(regs[i]) for i in idx], "the diagonal is E of the one sketch"
    if m >= 17:
        assert got[0, 0] == 0 and got[0, 6] == 0, "two empty sets"
        assert got[0, 4] == got[4, 4] == got[4, 0] > 10240, "an empty set beside a full one; the raw branch"
        assert got[4, 5] > got[4, 4] and got[1, 1] == 1 and got[2, 2] == 5 and 280 <= got[3, 3] <= 320 and got[1, 2] == 6
    if m == 65:
        assert got[29, 30] == got[29, 29], "a set and its copy"


def test_pair_table_repeats_and_descending(sixty_five):
    sk, regs, sets = sixty_five
    idx = np.array([64, 40, 40, 5, 4, 3, 3, 0, 64], np.uint32)
    got = sk.pair_table(idx)
    assert np.array_equal(got, pair_table(regs, idx))
    assert got[1, 2] == got[1, 1] == got[2, 2] and got[0, 8] == got[0, 0]
    whole = sk.pair_table(np.arange(65, dtype=np.uint32)[::-1].copy())
    assert np.array_equal(whole[::-1, ::-1], sk.pair_table(np.arange(65, dtype=np.uint32)))
    assert whole[64 - 4, 64 - 5] == got[4, 3]


def test_pair_table_limits(sixty_five):
    from ganon_amd import hip as H
    sk, regs, sets = sixty_five
    assert sk.pair_table(np.zeros(0, np.uint32)).shape == (0, 0)
    with pytest.raises(H.GanonHipError) as e:
        sk.pair_table(np.zeros(4097, np.uint32))
    assert e.value.code == -34, "GN_ERANGE above GN_SKETCH_TABLE_MAX entries"
    for bad in (np.array([65], np.uint32), np.array([3, 64, 65], np.uint32), np.array([0xFFFFFFFF], np.uint32)):  # no such sketch
        with pytest.raises(H.GanonHipError) as e:
            sk.pair_table(bad)
        assert e.value.code == -22, "GN_EINVAL: refused on the host, before a kernel could read past the sketches"
        assert f"idx[{len(bad) - 1}] = {int(bad[-1])} of 65 sketches" in str(e.value)
    assert sk.pair_table(np.array([64], np.uint32))[0, 0] == estimate(regs[64])


def test_pair_estimates_are_within_five_standard_errors(hip):
    """20 pairs of sets that share a known part: the union is within 8 % = 5 * 1.04 / sqrt(4096) of its exact size"""
    from ganon_amd import hip as H
    rng = np.random.default_rng(22)
    sets, exact = [], []
    for p in range(20):
        n_a, n_b = int(rng.integers(6000, 60000)), int(rng.integers(6000, 60000))
        shared = int(rng.integers(0, min(n_a, n_b)))
        pool = random_set(rng, n_a + n_b + 1000, 60)[:n_a + n_b - shared]
        assert len(pool) == n_a + n_b - shared
        pool = rng.permutation(pool)
        sets += [pool[:n_a], pool[n_a - shared:]]
        exact.append(len(pool))
    sk = H.HipSketches(sets)
    table = sk.pair_table(np.arange(40, dtype=np.uint32))
    for p in range(20):
        err = abs(int(table[2 * p, 2 * p + 1]) - exact[p]) / exact[p]
        print(f"pair {p}: sets {len(sets[2 * p])} {len(sets[2 * p + 1])} exact union {exact[p]} estimate {int(table[2 * p, 2 * p + 1])} error {err:.4f}")
        assert err <= 0.08
    sk.free()


@pytest.mark.parametrize("seed", [1, 2])
def test_order_from_the_device_estimates(hip, driver, seed):
    """the families of the CPU test as hash sets on the device: with the device's estimates every family is one run of the order"""
    from ganon_amd import hip as H
    sets = families(seed)
    counts = [len(s) for s in sets]
    sk = H.HipSketches([np.array(s, dtype=np.uint64) for s in sets])
    matrix = sk.pair_table(np.arange(64, dtype=np.uint32)).tolist()
    sk.free()
    starts, order, n_tables, largest = order_of(driver, counts, matrix=matrix)
    assert starts == [0] and (n_tables, largest) == (1, 64)
    assert contiguous(order), [u % 8 for u in order]


# ------------------------------------------------------------------------------------------------------------ the written index
TMAX, S, MAX_FP = 6, 3, 0.001
LINE = re.compile(r"^layout similarity: (\d+) intervals, (\d+) of (\d+) user bins moved, kept (sketch|similarity|rule)$", re.M)


@pytest.fixture(scope="module")
def families36(tmp_path_factory):
    """6 families of 6 members: an ancestor of 30 kbp, a member = the ancestor with every base substituted with probability 0.01 and
    a random 0 .. 10 % cut from its end; one target per member, listed family after family member by member, so that neither the
    input order nor the size order has a family together"""
    d = tmp_path_factory.mktemp("hibf_families36")
    rng = np.random.default_rng(36)
    ancestors = [np.frombuffer(gu.random_seq(rng, 30000), dtype=np.uint8) for _ in range(6)]
    tsv = str(d / "families_input.tsv")
    order, seqs = [], {}
    with open(tsv, "w") as o:
        for i in range(6):
            for f in range(6):
                seq = ancestors[f].copy()
                hit = np.nonzero(rng.random(len(seq)) < 0.01)[0]
                for at in hit:  # another base
                    seq[at] = [c for c in b"ACGT" if c != seq[at]][int(rng.integers(0, 3))]
                seq = seq[:len(seq) - int(rng.random() * 0.1 * len(seq))]
                name = f"F{f}m{i}"
                order.append(name)
                seqs[name] = [seq.tobytes().decode()]
                path = str(d / f"{name}.fasta")
                gf.write_fasta(path, [(name, seqs[name][0])])
                o.write(f"{path}\t{name}\n")
    return Inputs(tsv, order, seqs)


@pytest.fixture(scope="module")
def built36(hip, families36, tmp_path_factory):
    d = tmp_path_factory.mktemp("hibf_similarity_built")
    out = {name: str(d / f"{name}.hibf") for name in ("similarity", "sketch")}
    p = build(families36, out["similarity"], TMAX, S, MAX_FP, extra=("--layout", "similarity", "--verbose"))
    build(families36, out["sketch"], TMAX, S, MAX_FP, extra=("--layout", "sketch"))
    return out, p.stderr


def test_families_index(hip, families36, built36):
    out, stderr = built36
    m, hb, depth = check_file(out["similarity"], families36, TMAX, S, MAX_FP, 0)
    assert max(depth) + 1 == 2, "36 user bins at tmax 6: two levels"
    line = LINE.search(stderr)
    assert line, stderr[-600:]
    assert line.group(1, 3, 4) == ("1", "36", "similarity") and int(line.group(2)) > 18
    assert "layout         similarity\n" in stderr[stderr.index("hibf_config:"):]
    similarity, sketch = os.path.getsize(out["similarity"]), os.path.getsize(out["sketch"])
    print(f"families36 tmax {TMAX}: similarity {similarity} bytes, sketch {sketch} bytes, ratio {similarity / sketch:.3f}")
    assert similarity < sketch
    again = out["similarity"] + ".again"  # (beside the first: the index names files in the directory it is written to)
    build(families36, again, TMAX, S, MAX_FP, extra=("--layout", "similarity"))
    assert open(again, "rb").read() == open(out["similarity"], "rb").read(), "two builds of one input: the same bytes"


def test_families_reads_are_found(hip, families36, built36, tmp_path):
    out, _ = built36
    names, sets = families36.sets(0)
    reads = cut_reads(families36, 0, np.random.default_rng(TMAX))
    assert {t for _, _, t in reads if t} == set(names), "reads from every member"
    fq = str(tmp_path / "reads.fq")
    gf.write_fastq(fq, [(rid, seq) for rid, seq, _ in reads])
    outs = {}
    for tag, binary in (("hip", cu.BIN_HIP), ("oracle", cu.build_oracle_binary())):
        prefix = str(tmp_path / tag)
        cu.run(binary, ["--ibf", out["similarity"], "--hibf", "--single-reads", fq, "-o", prefix, "--output-all", "--skip-lca", "--rel-cutoff", "1",
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


@pytest.mark.parametrize("which", ["short200", "large40"])
def test_unrelated_fixtures(hip, request, tmp_path, which):
    """targets that share nothing: the index is sound, and what the estimates chose is never worse than `sketch` -- the search over
    the size order is kept, byte for byte, unless the line says that the similarity tree was estimated smaller"""
    inp = request.getfixturevalue(which)
    out, sketch = str(tmp_path / "similarity.hibf"), str(tmp_path / "sketch.hibf")
    p = build(inp, out, 8, S, MAX_FP, extra=("--layout", "similarity", "--verbose"))
    check_file(out, inp, 8, S, MAX_FP, 0)
    line = LINE.search(p.stderr)
    assert line, p.stderr[-600:]
    assert int(line.group(3)) == len(inp.sets(0)[0]) and int(line.group(1)) >= 2
    print(f"{which}: {line.group(0)}")
    if line.group(4) != "similarity":
        build(inp, sketch, 8, S, MAX_FP, extra=("--layout", "sketch"))
        assert open(out, "rb").read() == open(sketch, "rb").read()  # (in one directory: the index names the files of its directory)
