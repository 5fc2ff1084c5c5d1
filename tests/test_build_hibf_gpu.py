"""`ganon-build --hibf` on the GPU: the two device steps against numpy / the one-IBF-at-a-time emplace, the written index
against the oracle (header, names, tree invariants, rows of every IBF, every payload bit), and the classify side on a filter
built from sequences: a read is found in the user bin it came from."""
import math
import os
import subprocess

import numpy as np
import pytest

import cli_util as cu
import ganon_fixtures as gf
import gpu_util as gu
import hibf_checks as hc
import oracle
from test_build_cpu import BIN_BUILD, DATA, read_fasta_gz

pytestmark = pytest.mark.gpu

K, W = 19, 32


@pytest.fixture(scope="module")
def hip():
    import ganon_amd
    ganon_amd.load_library()
    assert ganon_amd.device_count() >= 1, "no HIP device: the product path has no CPU fallback"
    assert os.path.exists(BIN_BUILD), "ganon-build is built by __graft_entry__.build()"
    return ganon_amd


def hashes_of(seq: str):
    r = oracle.to_ranks(seq.encode())
    if len(r) < K:
        return np.zeros(0, np.uint64)
    return oracle.minimiser_hash(r, K, min(W, len(r)))  # a range shorter than the window: the window shrinks to it


class Inputs:
    """targets in first-appearance order: name -> its sequences; and the input file of ganon-build"""

    def __init__(self, tsv, order, seqs):
        self.tsv, self.order, self.seqs = tsv, order, seqs
        self._sets = {}

    def sets(self, min_length):
        """(names of the user bins, their distinct minimiser sets, ascending) as the oracle computes them"""
        if min_length not in self._sets:
            names, sets = [], []
            for t in self.order:
                hs = [hashes_of(s) for s in self.seqs[t] if len(s) >= min_length]
                hs = np.unique(np.concatenate(hs)) if hs else np.zeros(0, np.uint64)
                if len(hs):
                    names.append(t)
                    sets.append(hs)
            self._sets[min_length] = (names, sets)
        return self._sets[min_length]


@pytest.fixture(scope="module")
def genomes(tmp_path_factory):
    d = tmp_path_factory.mktemp("hibf_genomes")
    tsv = str(d / "mode_input.tsv")
    order, seqs = [], {}
    with open(tsv, "w") as o:
        for line in open(os.path.join(DATA, "mode_input.tsv")):
            f, t = line.rstrip("\n").split("\t")
            t = f"G.{t} x"  # a '.' and a space in every name: both have to come back from the file names
            o.write(f"{os.path.join(DATA, f)}\t{t}\n")
            if t not in seqs:
                order.append(t)
                seqs[t] = []
            seqs[t] += read_fasta_gz(os.path.join(DATA, f))
    return Inputs(tsv, order, seqs)


@pytest.fixture(scope="module")
def short200(tmp_path_factory):
    """200 targets of log-normal length (200 bp .. 60 kbp), one to three sequences each, a few of them in two files"""
    d = tmp_path_factory.mktemp("hibf_short")
    rng = np.random.default_rng(200)
    tsv = str(d / "short_input.tsv")
    order, seqs = [], {}
    with open(tsv, "w") as o:
        for t in range(200):
            name = f"T{t}"
            total = int(min(60000, max(200, rng.lognormal(math.log(2000), 1.0))))
            cuts = sorted(int(x) for x in rng.integers(150, max(151, total), size=int(rng.integers(0, 3))))
            whole = gu.random_seq(rng, total).decode()
            parts = [p for p in (whole[a:b] for a, b in zip([0] + cuts, cuts + [total])) if p]
            order.append(name)
            seqs[name] = parts
            files = [parts] if t % 9 else [parts[:1], parts[1:] + [whole[:170]]]  # a second file that shares hashes with the first
            if len(files) == 2:
                seqs[name] = files[0] + files[1]
            for j, recs in enumerate(files):
                path = str(d / f"{name}_{j}.fasta")
                gf.write_fasta(path, [(f"{name}_{j}_{i}", s) for i, s in enumerate(recs)])
                o.write(f"{path}\t{name}\n")
    return Inputs(tsv, order, seqs)


def build(inp, out, tmax, s=0, max_fp=0.05, min_length=0, extra=(), expect=0):
    args = [BIN_BUILD, "-i", inp.tsv if isinstance(inp, Inputs) else inp, "-o", out, "--quiet", "-k", str(K), "-w", str(W), "-s", str(s), "-p", repr(max_fp),
            "--hibf", "--tmax", str(tmax), "-t", "2"]
    if min_length:
        args += ["--min-length", str(min_length)]
    p = subprocess.run(args + list(extra), capture_output=True, text=True, timeout=300)
    assert p.returncode == expect, p.stderr
    return p


def read_tree(path, n_user, tmax):
    from ganon_amd import ibf_file
    m = ibf_file.read_hibf_meta(path)
    runs, depth, below, where, parent = hc.check_tree([f[0] for f in m.ibfs], m.next_ibf_id, m.bin_to_user, n_user, tmax)
    return m, runs, depth, below, where


def check_file(path, inp, tmax, s, max_fp, min_length):
    """header, names, invariants, rows per IBF and every payload bit of a `ganon-build --hibf` index against the oracle"""
    names, sets = inp.sets(min_length)
    h = 4 if s == 0 else s
    m, runs, depth, below, where = read_tree(path, len(names), tmax)
    assert (m.version, m.window_size, m.kmer_size, m.shape_bits, m.parts, m.compressed, m.is_hibf) == (1, W, K, (1 << K) - 1, 1, 0, 1)
    assert m.fpr == max_fp
    assert m.names == names, "one user bin per target with a hash, in first-appearance order"
    assert all(len(lst) == 1 for lst in m.bin_path) and m.user_bin_filenames == [lst[0] for lst in m.bin_path]
    ibfs = []
    for i, (bins, rows, hf, _) in enumerate(m.ibfs):
        assert hf == h
        ref = oracle.Ibf(bins, rows, h)
        need = 0
        for first, n, user, child in runs[i]:
            if user >= 0:
                hs = sets[user]
                per = (len(hs) + n - 1) // n
                ref.emplace_many(hs, (first + np.arange(len(hs)) // per).astype(np.uint32))
                need = max(need, hc.run_bits(len(hs), n, max_fp, h))
            else:
                members = [sets[u] for u in below[child]]
                for hs in members:
                    ref.emplace_many(hs, first)
                need = max(need, hc.run_bits(len(np.unique(np.concatenate(members))), 1, max_fp, h))
        assert rows == need, (i, rows, need)
        assert np.array_equal(m.payload(path, i), ref.data), f"payload of IBF {i}"
        ibfs.append(ref)
    return m, oracle.Hibf(ibfs, [a.tolist() for a in m.next_ibf_id], [a.tolist() for a in m.bin_to_user], len(names)), depth


# ------------------------------------------------------------------------------------------------------------ device steps
def test_hashes_union(hip):
    from ganon_amd import hip as H
    rng = np.random.default_rng(5)
    a = np.unique(rng.integers(0, 1 << 38, size=5000, dtype=np.uint64))
    b = np.unique(np.concatenate([a[::3], rng.integers(0, 1 << 38, size=3000, dtype=np.uint64)]))
    c = np.unique(rng.integers(0, 1 << 63, size=70000, dtype=np.uint64)) * np.uint64(2) + np.uint64(1)  # values with bit 63 set
    empty = np.zeros(0, np.uint64)
    for sets in ([a, b, c], [a, empty, b], [a, a, a], [a], [empty], [empty, empty], [np.array([7], np.uint64), np.array([7], np.uint64)], []):
        exp = np.zeros(0, np.uint64)
        for x in sets:
            exp = np.union1d(exp, x)
        got = H.hashes_union(sets)
        assert got.dtype == np.uint64 and np.array_equal(got, exp), [len(x) for x in sets]
        assert H.hashes_union(sets, size_only=True) == len(exp)


def paths_of(hb: oracle.Hibf, sizes):
    """the root-to-leaf path of every user bin of an oracle.Hibf, as gn_filter_emplace_path takes it"""
    from ganon_amd import hip as H
    bins = [f.bins for f in hb.ibfs]
    runs, depth, below, where, parent = hc.check_tree(bins, [np.asarray(a) for a in hb.next_ibf_id], [np.asarray(a) for a in hb.bin_to_user],
                                                      hb.n_user_bins, max(bins), max_levels=64)
    levels = max(depth) + 1
    paths = np.zeros((hb.n_user_bins, levels), dtype=H.PATH_DTYPE)
    for u, (i, first, n) in where.items():
        paths[u, 0] = (i, first, n, 0, max(1, (sizes[u] + n - 1) // n))
        at, d = i, 1
        while at != 0:
            at, b = parent[at]
            paths[u, d] = (at, b, 1, 0, 1)
            d += 1
    return paths, where, parent


@pytest.mark.parametrize("n_ub,tmax,depth", [(40, 8, 3), (150, 64, 2), (10, 4, 4), (30, 64, 1)])
def test_emplace_path_equals_emplace_per_ibf(hip, n_ub, tmax, depth):
    rng = np.random.default_rng(n_ub * 7 + tmax)
    hb = gf.random_hibf(n_ub, tmax, depth, seed=n_ub + tmax, density=0.0, hash_funs=3, rows=(3000, 9000))
    sets = [np.unique(rng.integers(0, 1 << 38, size=int(rng.integers(1, 3000)), dtype=np.uint64)) for _ in range(n_ub)]
    sets[1] = np.zeros(0, np.uint64)                                             # an empty set between the others
    sets[2] = np.unique(rng.integers(0, 1 << 38, size=20000, dtype=np.uint64))   # a set of many wave items
    sets[3] = sets[3][:512] if len(sets[3]) >= 512 else sets[3]
    paths, where, parent = paths_of(hb, [len(x) for x in sets])
    shapes = [(None, f.bins, f.bin_size, f.hash_funs) for f in hb.ibfs]
    one = hip.HipFilter.hibf(shapes, hb.next_ibf_id, hb.bin_to_user, n_ub)
    one.emplace_path(sets, paths)
    ref = hip.HipFilter.hibf(shapes, hb.next_ibf_id, hb.bin_to_user, n_ub)
    per_ibf = {}
    for u, hs in enumerate(sets):
        if len(hs) == 0:
            continue
        i, first, n = where[u]
        per = (len(hs) + n - 1) // n
        per_ibf.setdefault(i, []).append((hs, (first + np.arange(len(hs)) // per).astype(np.uint32)))
        at = i
        while at != 0:
            at, b = parent[at]
            per_ibf.setdefault(at, []).append((hs, np.full(len(hs), b, dtype=np.uint32)))
    for i, lst in per_ibf.items():
        ref.emplace(np.concatenate([x for x, _ in lst]), np.concatenate([b for _, b in lst]), ibf_idx=i)
    some = False
    for i, f in enumerate(hb.ibfs):
        a = one.download_rows(0, f.bin_size, f.bin_words, ibf_idx=i)
        b = ref.download_rows(0, f.bin_size, f.bin_words, ibf_idx=i)
        assert np.array_equal(a, b), f"IBF {i}"
        some = some or bool(a.any())
    assert some
    # a path that leaves its IBF is refused before anything is launched
    bad = paths.copy()
    bad[0, 0]["first_bin"] = hb.ibfs[int(bad[0, 0]["ibf"])].bins
    with pytest.raises(hip.GanonHipError):
        one.emplace_path(sets, bad)
    one.free()
    ref.free()


# ------------------------------------------------------------------------------------------------------------ the written index
CASES = [("genomes", 64, 0, 0.05, 0), ("genomes", 8, 3, 0.001, 0), ("genomes", 4, 0, 0.001, 42000),
         ("short200", 64, 3, 0.001, 0), ("short200", 8, 0, 0.05, 1000), ("short200", 4, 3, 0.05, 0)]


@pytest.mark.parametrize("which,tmax,s,max_fp,min_length", CASES)
def test_index_against_the_oracle(hip, request, tmp_path, which, tmax, s, max_fp, min_length):
    inp = request.getfixturevalue(which)
    out = str(tmp_path / "db.hibf")
    build(inp, out, tmax, s, max_fp, min_length)
    m, hb, depth = check_file(out, inp, tmax, s, max_fp, min_length)
    names, _ = inp.sets(min_length)
    if min_length:
        assert 0 < len(names) < len(inp.order), "the case is meant to lose some targets to --min-length, not all"
    levels = max(depth) + 1
    assert levels == (1 if len(names) <= tmax else levels) and levels <= hc.levels_for(len(names), tmax)
    if which == "genomes" and not min_length:
        assert levels == {64: 1, 8: 2, 4: 3}[tmax]  # 25 user bins: one IBF, two levels, three levels
    again = str(tmp_path / "db2.hibf")
    if (which, tmax) in (("genomes", 8), ("short200", 4)):  # two builds of one input: the same bytes
        build(inp, again, tmax, s, max_fp, min_length)
        assert open(out, "rb").read() == open(again, "rb").read()


def cut_reads(inp, min_length, rng, per_target=3, n_random=40):
    """150 bp reads from every target that has a user bin, plus random ones: [(id, sequence, source | None)]"""
    names, _ = inp.sets(min_length)
    reads = []
    for t in names:
        pool = [s for s in inp.seqs[t] if len(s) >= max(min_length, 150)]
        for j in range(per_target if pool else 0):
            s = pool[int(rng.integers(0, len(pool)))]
            a = int(rng.integers(0, len(s) - 150 + 1))
            reads.append((f"r{len(reads)}", s[a:a + 150], t))
    for _ in range(n_random):
        reads.append((f"r{len(reads)}", gu.random_seq(rng, 150).decode(), None))
    return reads


@pytest.mark.parametrize("which,tmax,s,max_fp", [("genomes", 8, 0, 0.05), ("short200", 4, 3, 0.001)])
def test_no_false_negatives_and_the_classify_side_agrees(hip, request, tmp_path, which, tmax, s, max_fp):
    inp = request.getfixturevalue(which)
    out = str(tmp_path / "db.hibf")
    build(inp, out, tmax, s, max_fp)
    m, hb, _ = check_file(out, inp, tmax, s, max_fp, 0)
    names, sets = inp.sets(0)
    reads = cut_reads(inp, 0, np.random.default_rng(tmax))
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
    # the same through the ABI: dense per-user-bin counts of the device == the oracle's bulk_count on the oracle.Hibf of the file
    from ganon_amd import ibf_file
    flt = hip.HipFilter.hibf([(m.payload(out, i).reshape(-1), b, r, hf) for i, (b, r, hf, _) in enumerate(m.ibfs)], m.next_ibf_id, m.bin_to_user,
                             len(names))
    seqs = [seq.encode() for _, seq, _ in reads]
    bases, off1, _ = gu.pack_reads(seqs)
    st = hip.HipStream(flt, len(seqs), bases.size)
    rel_cutoff = 0.25
    st.submit(bases, off1, None, K, W, rel_cutoff)
    nh, status, _, _ = st.fetch()
    dense = st.dense_counts(0, len(seqs), len(names))
    user = {t: u for u, t in enumerate(names)}
    for i, (rid, seq, source) in enumerate(reads):
        hh = hashes_of(seq)
        assert status[i] == 0 and nh[i] == len(hh)
        exp = hb.bulk_count(hh, oracle.threshold_cutoff(len(hh), rel_cutoff))
        assert np.array_equal(dense[i], exp), rid
        if source is not None:
            # (a user bin split over several bins adds its bins' counts up: a sibling bin may hold a hash again as a false positive,
            # which is why the reported count is capped at the read's hashes, GanonClassify.cpp:561-564)
            assert dense[i][user[source]] >= len(hh)
    st.destroy()
    flt.free()


def test_targets_without_a_long_enough_sequence(hip, tmp_path):
    rng = np.random.default_rng(77)
    seqs = {f"L{i}": gu.random_seq(rng, 3000 + 500 * i).decode() for i in range(6)}
    seqs["short one"] = gu.random_seq(rng, 120).decode()
    order = ["L0", "L1", "short one", "L2", "L3", "L4", "L5"]
    files = {}
    for t in order:
        files[t] = str(tmp_path / f"{t.replace(' ', '_')}.fasta")
        gf.write_fasta(files[t], [(t.replace(" ", "_"), seqs[t])])
    with_short, without = str(tmp_path / "with.tsv"), str(tmp_path / "without.tsv")
    open(with_short, "w").write("".join(f"{files[t]}\t{t}\n" for t in order))
    open(without, "w").write("".join(f"{files[t]}\t{t}\n" for t in order if t != "short one"))
    a, b, c = str(tmp_path / "a.hibf"), str(tmp_path / "b.hibf"), str(tmp_path / "c.hibf")
    build(with_short, a, 4, min_length=150)
    build(without, b, 4, min_length=150)
    build(with_short, c, 4)
    from ganon_amd import ibf_file
    assert ibf_file.read_hibf_meta(a).names == [t for t in order if t != "short one"]
    assert open(a, "rb").read() == open(b, "rb").read(), "the others unchanged"
    assert ibf_file.read_hibf_meta(c).names == order
    # every target so: what the flat path says and returns
    flat = subprocess.run([BIN_BUILD, "-i", with_short, "-o", str(tmp_path / "x.ibf"), "-k", str(K), "-w", str(W), "--min-length", "100000"],
                          capture_output=True, text=True)
    hier = subprocess.run([BIN_BUILD, "-i", with_short, "-o", str(tmp_path / "x.hibf"), "-k", str(K), "-w", str(W), "--min-length", "100000", "--hibf",
                           "--tmax", "4"], capture_output=True, text=True)
    assert flat.returncode == 1 and "No valid sequences to build" in flat.stderr
    assert (hier.returncode, hier.stderr) == (flat.returncode, flat.stderr)
    assert not os.path.exists(str(tmp_path / "x.hibf"))
