"""gn_filter_extend_path on the GPU: every word of every IBF after the call against a numpy restatement of include/ganon_hip.h
(presence with rows_of, rank with cumsum, bin with searchsorted on the cumulative quotas, the ORs), the two guarantees -- every hash is
found on its whole path, no absent hash is dealt twice -- the refusals with the matrix unchanged, and one set that crosses the 32 M
round boundary, checked on the device."""
import ctypes as C
import time

import numpy as np
import pytest

import ganon_fixtures as gf
from test_build_hibf_gpu import hip, paths_of  # noqa: F401  (hip is a fixture)
from test_build_update_gpu import one_ibf, storage_only
from test_build_verify_gpu import NONE, contained, rows_of

pytestmark = pytest.mark.gpu

U64 = np.uint64
SIZES = (1, 63, 64, 65, 511, 512, 513, 4097)  # slot, item and multi-item boundaries


# ------------------------------------------------------------------------------------------------------------ the restatement
def or_into(mat, h, v, bins):
    """hash v[i] into bin bins[i] of one IBF's matrix [rows, words]"""
    bins = np.broadcast_to(np.asarray(bins, dtype=np.int64), v.shape)
    for i in range(h):
        np.bitwise_or.at(mat, (rows_of(v, i, mat.shape[0]).astype(np.int64), bins >> 6), U64(1) << (bins & 63).astype(U64))


def extend_ref(mats, h, sets, paths, quotas):
    """-> (the matrices after the call, per set the absent mask, per set the leaf bin of every absent hash); presence is taken against
    `mats` as they are, whatever the sets before this one set"""
    out = [m.copy() for m in mats]
    absent, where = [], []
    for s, v in enumerate(sets):
        e = paths[s, 0]
        if e["n_bins"] == 0 or len(v) == 0:
            absent.append(np.zeros(len(v), bool)), where.append(np.zeros(0, np.int64))
            continue
        a = ~contained(mats, h, v, e)
        cum = np.cumsum(np.asarray(quotas[s], dtype=np.int64))
        assert cum[-1] == np.count_nonzero(a), "the test's own quotas"
        b = int(e["first_bin"]) + np.searchsorted(cum, np.arange(np.count_nonzero(a)), side="right")
        or_into(out[int(e["ibf"])], h, v[a], b)
        for d in range(1, paths.shape[1]):
            if paths[s, d]["n_bins"] == 0:
                break
            or_into(out[int(paths[s, d]["ibf"])], h, v, int(paths[s, d]["first_bin"]))
        absent.append(a), where.append(b)
    return out, absent, where


def popcount64(a):
    return np.unpackbits(np.ascontiguousarray(a).view(np.uint8).reshape(len(a), 8), axis=1).sum(axis=1, dtype=np.int64)


def bins_holding(mat, h, v, first, n):
    """per hash: the number of bins of the run first .. first + n - 1 in which all h rows have the bin's bit"""
    total = np.zeros(len(v), np.int64)
    for w in range(first >> 6, ((first + n - 1) >> 6) + 1):
        lo, hi = max(first, w * 64), min(first + n, w * 64 + 64)
        a = np.full(len(v), ((1 << (hi - lo)) - 1) << (lo - w * 64), dtype=U64)
        for i in range(h):
            a &= mat[rows_of(v, i, mat.shape[0]), w]
        total += popcount64(a)
    return total


def deal(style, a, n):
    """quotas of n bins that sum to a"""
    q = np.zeros(n, np.int64)
    if style == "each" and a <= n:   # one hash per bin
        q[:a] = 1
    elif style == "one":             # all in one bin
        q[n // 2] = a
    elif style == "zeros" and n > 1:  # every other bin takes nothing
        take = np.arange(1, n, 2)
        q[take] = a // len(take)
        q[take[: a % len(take)]] += 1
    else:
        q[:] = a // n
        q[: a % n] += 1
    assert q.sum() == a
    return q


def pools(rng, size):
    """(base, extension), ascending, `size` each, size // 2 of them shared"""
    pool = np.unique(rng.integers(0, 1 << 40, size=3 * size + 16, dtype=U64))
    assert len(pool) >= 2 * size
    pool = rng.permutation(pool)
    k = size // 2
    return np.sort(pool[:size]), np.sort(np.concatenate([pool[:k], pool[size:2 * size - k]]))


def download(flt, shapes):
    return [flt.download_rows(0, rows, (bins + 63) >> 6, ibf_idx=i) for i, (bins, rows) in enumerate(shapes)]


def check_call(hip, flt, shapes, h, sets, paths, quotas_of):
    """one call against the restatement; quotas_of(s, absent count, bins) -> quotas.  Returns (before, after, absent masks)"""
    from ganon_amd import hip as H
    before = download(flt, shapes)
    counts = [int(np.count_nonzero(~contained(before, h, v, paths[s, 0]))) if len(v) and paths[s, 0]["n_bins"] else 0 for s, v in enumerate(sets)]
    quotas = [quotas_of(s, counts[s], int(paths[s, 0]["n_bins"])) for s in range(len(sets))]
    exp, absent, where = extend_ref(before, h, sets, paths, quotas)
    flt.extend_path(sets, paths, quotas)
    after = download(flt, shapes)
    for i, (a, b) in enumerate(zip(after, exp)):
        assert np.array_equal(a, b), f"IBF {i}: {np.count_nonzero(a != b)} words differ, the first at {np.argwhere(a != b)[0].tolist()}"
    # the two guarantees
    found, lost, first = flt.probe_path(sets, paths)
    assert found.tolist() == [len(v) for v in sets] and not lost.any() and (first == U64(NONE)).all(), "every hash on its whole path"
    for s, v in enumerate(sets):
        if not absent[s].any():
            continue
        e = paths[s, 0]
        got = bins_holding(after[int(e["ibf"])], h, v[absent[s]], int(e["first_bin"]), int(e["n_bins"]))
        ref = bins_holding(exp[int(e["ibf"])], h, v[absent[s]], int(e["first_bin"]), int(e["n_bins"]))
        assert (got >= 1).all() and (got[ref == 1] == 1).all(), f"set {s}: an absent hash dealt to no bin or to two"
    assert isinstance(paths, np.ndarray) and paths.dtype == H.PATH_DTYPE
    return before, after, absent


# ------------------------------------------------------------------------------------------------------------ runs, sizes, hash functions
BINS, ROWS = 200, 20011
RUNS = [(5, 1), (3, 4), (60, 9), (10, 130), (190, 10)]  # one bin; inside a word; straddling a word; three words; ending on the last bin


@pytest.mark.parametrize("h", [2, 3, 4, 5])
def test_runs_sizes_and_quotas(hip, h):
    from ganon_amd import hip as H
    styles = ("even", "zeros", "one", "each")
    overlap = each = False
    for first, n in RUNS:
        flt = one_ibf(hip, BINS, ROWS, h)
        rng = np.random.default_rng(first * 1000 + n * 10 + h)
        for k, size in enumerate(SIZES):
            base, ext = pools(rng, size)
            p = np.zeros((1, 1), dtype=H.PATH_DTYPE)
            p[0, 0] = (0, first, n, 0, max(1, (size + n - 1) // n))
            flt.emplace_path([base], p)
            style = styles[(k + first) % 4]
            _, _, absent = check_call(hip, flt, [(BINS, ROWS)], h, [ext], p, lambda s, a, nb: deal(style, a, nb))
            overlap = overlap or (0 < np.count_nonzero(absent[0]) < size)
            each = each or (style == "each" and 1 < np.count_nonzero(absent[0]) <= n)
            assert np.count_nonzero(absent[0]) <= size - size // 2, "what the base shares with the extension is present"
        flt.free()
    assert overlap, "no call had both present and absent hashes"
    assert each, "no call dealt one hash to each of several bins"


# ------------------------------------------------------------------------------------------------------------ a tree, six sets in one call
def test_six_sets_in_a_tree_of_three_levels(hip):
    n_ub, h = 40, 3
    rng = np.random.default_rng(406)
    hb = gf.random_hibf(n_ub, 8, 3, seed=n_ub + 8, density=0.0, hash_funs=h, rows=(3000, 9000))
    base = [np.unique(rng.integers(0, 1 << 40, size=600, dtype=U64)) for _ in range(n_ub)]
    paths, where, _ = paths_of(hb, [len(x) for x in base])
    assert paths.shape[1] == 3
    used = (paths["n_bins"] != 0).sum(axis=1)
    by_leaf = {}
    for u in range(n_ub):
        by_leaf.setdefault(where[u][0], []).append(u)
    pair = next(us for us in by_leaf.values() if len(us) >= 2)[:2]                                     # two in the same leaf IBF
    rest = [u for u in range(n_ub) if u not in pair]
    short = next(u for u in rest if used[u] != used[pair[0]])                                          # a path of another length
    deep = [u for u in rest if u != short and used[u] >= 2][:3]                                        # under a merged bin
    chosen = pair + [short] + deep
    assert len(chosen) == 6 and len({int(used[u]) for u in chosen}) >= 2, "paths of different lengths in one call"
    whole, nothing, empty = deep[0], deep[1], deep[2]
    # the pre-state: every user bin along its path -- but `whole` only into its leaf run, so that the merged bins above lack it
    pre = paths.copy()
    pre[whole, 1:] = np.zeros(paths.shape[1] - 1, dtype=paths.dtype)
    shapes = [(None, f.bins, f.bin_size, f.hash_funs) for f in hb.ibfs]
    flt = hip.HipFilter.hibf(shapes, hb.next_ibf_id, hb.bin_to_user, n_ub)
    flt.emplace_path(base, pre)
    ext = {}
    for u in chosen:
        fresh = np.unique(rng.integers(1 << 40, 1 << 41, size=700, dtype=U64))
        ext[u] = np.sort(np.concatenate([base[u][::2], fresh]))
    ext[whole] = base[whole][1::3]                                                                      # wholly present
    ext[nothing] = np.unique(rng.integers(1 << 41, 1 << 42, size=1100, dtype=U64))                      # nothing shared
    ext[empty] = np.zeros(0, U64)
    sets, p = [ext[u] for u in chosen], np.ascontiguousarray(paths[chosen])
    sizes = [(f.bins, f.bin_size) for f in hb.ibfs]
    before, after, absent = check_call(hip, flt, sizes, h, sets, p, lambda s, a, nb: deal(("even", "zeros", "one")[s % 3], a, nb))
    k = chosen.index(whole)
    leaf, above = int(p[k, 0]["ibf"]), int(p[k, 1]["ibf"])
    assert not absent[k].any(), "a subset of what the run holds is present"
    first, n = int(p[k, 0]["first_bin"]), int(p[k, 0]["n_bins"])
    col = lambda m, b: (m[:, b >> 6] >> U64(b & 63)) & U64(1)
    assert all(np.array_equal(col(before[leaf], b), col(after[leaf], b)) for b in range(first, first + n)), "a present hash sets no leaf bit"
    assert not np.array_equal(before[above], after[above]), "... and is ORed into the merged bin above"
    assert np.count_nonzero(absent[chosen.index(nothing)]) > 0.7 * len(ext[nothing]), "nothing of this set was there (false positives aside)"
    flt.free()


# ------------------------------------------------------------------------------------------------------------ refusals
def test_refusals_leave_the_matrix_as_it_is(hip):
    from ganon_amd import hip as H
    h = 3
    rng = np.random.default_rng(5)
    flt = one_ibf(hip, BINS, ROWS, h)
    base, ext = pools(rng, 900)
    p = np.zeros((1, 1), dtype=H.PATH_DTYPE)
    p[0, 0] = (0, 3, 4, 0, 225)
    flt.emplace_path([base], p)
    before = download(flt, [(BINS, ROWS)])[0]
    a = int(np.count_nonzero(~contained([before], h, ext, p[0, 0])))
    good = deal("even", a, 4)

    def refused(sets, paths, quotas, *words, on=flt):
        with pytest.raises(hip.GanonHipError) as e:
            on.extend_path(sets, paths, quotas)
        for w in words:
            assert w in str(e.value), str(e.value)
        assert np.array_equal(download(flt, [(BINS, ROWS)])[0], before), "a refused call wrote"

    refused([ext], p, [good + np.array([0, 1, 0, 0])], "set 0", str(a + 1), f"{a} of")            # the quotas do not sum to the absent count
    refused([ext], p, [good - np.array([0, 0, 1, 0])], "set 0", str(a - 1), f"{a} of")
    refused([ext], p, [np.append(good, 0)], "5 quotas", "4 bins")                                   # a quota list of the wrong length
    refused([ext], p, [good[:3]], "3 quotas")
    refused([ext[::-1].copy()], p, [good], "ascending")                                             # a descending set
    refused([np.repeat(ext, 2)], p, [good], "ascending")                                            # ... and one that repeats
    out = p.copy()
    out[0, 0]["first_bin"] = BINS - 3                                                               # a bin out of range
    refused([ext], out, [good])
    out = p.copy()
    out[0, 0]["ibf"] = 1
    refused([ext], out, [good])
    flat = storage_only(hip, BINS, ROWS, h)                                                         # a flat filter
    refused([ext], p, [good], "HIBF", on=flat)
    flat.free()
    L = H.load_library()
    off, doff = np.array([0, len(ext)], U64), np.array([0, 4], U64)
    quota = good.astype(U64)
    full = [flt._h, H._p(ext), H._p(off), 1, p.ctypes.data_as(C.c_void_p), 1, H._p(doff), H._p(quota)]
    for null in (0, 1, 2, 4, 6, 7):                                                                 # null arguments
        args = list(full)
        args[null] = None
        assert L.gn_filter_extend_path(*args) == -22, f"argument {null} null"
    args = list(full)
    args[5] = 0
    assert L.gn_filter_extend_path(*args) == -22, "depth 0"
    assert np.array_equal(download(flt, [(BINS, ROWS)])[0], before)
    assert L.gn_filter_extend_path(flt._h, None, None, 0, None, 1, None, None) == 0, "no set at all is legal"
    flt.extend_path([ext], p, [good])                                                               # and the call that is in order goes through
    assert not np.array_equal(download(flt, [(BINS, ROWS)])[0], before)
    flt.free()


# ------------------------------------------------------------------------------------------------------------ across a round boundary
def test_one_set_across_the_round_boundary(hip):
    """2^25 + 777 hashes are two rounds of the staging buffer: an empty run of 5 bins, checked on the device alone"""
    from ganon_amd import hip as H
    n, h, rows, bins = (1 << 25) + 777, 2, 50_000_017, 8
    v = np.arange(n, dtype=U64) * U64(32771) + U64(5)  # ascending without a sort: below 2^41
    q = np.array([n // 4, 0, n // 8, n // 2, 0], np.int64)
    q[4] = n - q.sum()
    cum = np.concatenate([[0], np.cumsum(q)])
    flt = one_ibf(hip, bins, rows, h)
    p = np.zeros((1, 1), dtype=H.PATH_DTYPE)
    p[0, 0] = (0, 2, 5, 0, 1)
    t0 = time.perf_counter()
    flt.extend_path([v], p, [q])
    print(f"gn_filter_extend_path, {n} hashes into an empty run of 5 bins, {rows} rows, h = {h}: {time.perf_counter() - t0:.3f} s")
    found, _, first = flt.probe_path([v], p, with_lost_at=False)
    assert int(found[0]) == n and first[0] == U64(NONE)
    own = np.zeros((5, 1), dtype=H.PATH_DTYPE)
    for j in range(5):
        own[j, 0] = (0, 2 + j, 1, 0, 1)
    found, _, first = flt.probe_path([v[cum[j]:cum[j + 1]] for j in range(5)], own, with_lost_at=False)
    assert found.tolist() == q.tolist() and (first == U64(NONE)).all(), "each quota's slice is in its own bin"
    pop = flt.bin_popcounts(bins)
    assert not pop[:2].any() and not pop[7:].any() and (pop[2:7] <= h * q).all() and (pop[2:7][q > 0] > 0).all(), pop.tolist()
    assert pop[3] == 0 and int(pop[2:7].sum()) > 0.7 * h * n, "a bin with quota 0 stays empty; h bits a hash, collisions aside"
    flt.free()


# ------------------------------------------------------------------------------------------------------------ the command
import math  # noqa: E402
import os  # noqa: E402
import subprocess  # noqa: E402

import cli_util as cu  # noqa: E402
import gpu_util as gu  # noqa: E402
import hibf_checks as hc  # noqa: E402
from test_build_cpu import BIN_BUILD  # noqa: E402
from test_build_extend_cpu import plan_extend as plan_restated  # noqa: E402
from test_build_hibf_gpu import Inputs, build, hashes_of  # noqa: E402
from test_build_update_gpu import all_ok, column_sums  # noqa: E402

MEMBERS = 6
LENGTHS = (10000, 12000, 14000, 30000, 36000, 40000, 12000, 30000)  # the ancestors; families 6 and 7 are the new targets.  The three small
# ones together stay below the largest, so that a merged bin over them does not set its IBF's rows and has room
_HASHES = {}


def hashes_cached(seq):
    if seq not in _HASHES:
        _HASHES[seq] = hashes_of(seq)
    return _HASHES[seq]


class FamilyInputs(Inputs):
    def sets(self, min_length):
        """as Inputs.sets, every sequence hashed once for the whole module"""
        assert min_length == 0
        return list(self.order), [np.unique(np.concatenate([hashes_cached(x) for x in self.seqs[t]])) for t in self.order]



@pytest.fixture(scope="module")
def families(tmp_path_factory):
    """8 families of 6 members, written the way families36 writes them (an ancestor, a member = the ancestor with every base
    substituted with probability 0.01 and a random 0 .. 10 % cut from its end), but the TARGET is the family: {family: [(file, sequence)]}"""
    d = tmp_path_factory.mktemp("hibf_extend_families")
    rng = np.random.default_rng(86)
    out = {}
    for f, length in enumerate(LENGTHS):
        ancestor = np.frombuffer(gu.random_seq(rng, length), dtype=np.uint8)
        for i in range(MEMBERS):
            seq = ancestor.copy()
            for at in np.nonzero(rng.random(len(seq)) < 0.01)[0]:
                seq[at] = [c for c in b"ACGT" if c != seq[at]][int(rng.integers(0, 3))]
            seq = seq[:len(seq) - int(rng.random() * 0.1 * len(seq))].tobytes().decode()
            path = str(d / f"F{f}m{i}.fasta")
            gf.write_fasta(path, [(f"F{f}m{i}", seq)])
            out.setdefault(f"F{f}", []).append((path, seq))
    return out


def inputs(families, members, path, order=None):
    """an input file of the given members {family: [member index]} and the Inputs that describes it"""
    order = list(order if order is not None else members)
    with open(path, "w") as o:
        for fam in order:
            for i in members[fam]:
                o.write(f"{families[fam][i][0]}\t{fam}\n")
    return FamilyInputs(path, order, {fam: [families[fam][i][1] for i in members[fam]] for fam in order})


def union(families, fam, idx):
    return np.unique(np.concatenate([hashes_cached(families[fam][i][1]) for i in idx]))


def extend(old, tsv, out, expect=0, flag=("--extend",)):
    p = subprocess.run([BIN_BUILD, "--hibf", "--update", old, "-i", tsv, "-o", out, "-t", "2", "--verbose"] + list(flag), capture_output=True, text=True, timeout=300)
    assert p.returncode == expect, (p.returncode, p.stdout[-2000:], p.stderr[-2000:])
    if expect:
        return p
    lines = p.stdout.splitlines()
    assert lines[0].startswith("index\t") and lines[-1].startswith("result\tok\t")
    assert all(w in p.stderr for w in (" - seconds: hash ", " load ", " count ", " plan ", " copy ", " emplace ", " write "))
    rep = dict(targets={}, extended={}, run=[], merged=[], result=lines[-1])
    for ln in lines[1:-1]:
        f = ln.split("\t")
        path = lambda s: [tuple(int(x) for x in e.split(":")) for e in s.split(" ")]
        if f[0] == "target":
            rep["targets"][f[1]] = dict(user_bin=int(f[2]), n=int(f[3]), leaf=int(f[4]), first=int(f[5]), bins=int(f[6]), path=path(f[8]))
        elif f[0] == "extended":
            assert len(f) == 10, ln
            rep["extended"][f[1]] = dict(user_bin=int(f[2]), n=int(f[3]), present=int(f[4]), inserted=int(f[5]), leaf=int(f[6]), first=int(f[7]), bins=int(f[8]), path=path(f[9]))
        elif f[0] == "run":
            rep["run"].append((int(f[1]), int(f[2]), int(f[3]), int(f[4]), float(f[5]), int(f[6])))
        elif f[0] == "merged":
            rep["merged"].append((int(f[1]), int(f[2]), int(f[3]), float(f[4]), int(f[5])))
        else:
            assert f[0] == "ibf" or ln.startswith("#"), ln
    return rep


def old_paths(meta):
    """user bin -> [(ibf, first, n_bins)] leaf first, from the file's tables"""
    bins = [f[0] for f in meta.ibfs]
    _, _, _, where, parent = hc.check_tree(bins, [np.asarray(a) for a in meta.next_ibf_id], [np.asarray(a) for a in meta.bin_to_user], len(meta.names), max(bins), max_levels=64)
    out = {}
    for u, (i, first, n) in where.items():
        out[u], at = [(i, first, n)], i
        while at != 0:
            at, b = parent[at]
            out[u].append((at, b, 1))
    return out


def as_paths(entries, depth):
    from ganon_amd import hip as H
    p = np.zeros((len(entries), depth), dtype=H.PATH_DTYPE)
    for s, es in enumerate(entries):
        for d, (i, first, n) in enumerate(es):
            p[s, d] = (i, first, n, 0, 1)
    return p


def restated(old, ext_sets):
    """the plan restated on the old file: -> (accepted names in order, their quotas, lost_at, paths); a family with a bin over its bound
    is left out and the plan made again"""
    from ganon_amd import ibf_file
    a = ibf_file.read_hibf_meta(old)
    h, rows = a.ibfs[0][2], [f[1] for f in a.ibfs]
    mats = [a.payload(old, i) for i in range(len(a.ibfs))]
    pop = [[int(x) for x in column_sums(m, f[0])] for m, f in zip(mats, a.ibfs)]
    paths = old_paths(a)
    depth = max(len(p) for p in paths.values())
    names = [t for t in ext_sets if t in a.names]
    lost = {}
    for t in names:
        u = a.names.index(t)
        p = as_paths([paths[u]], depth)
        lost[t] = [int(np.count_nonzero(~contained(mats, h, ext_sets[t], p[0, d]))) for d in range(len(paths[u]))]
    while True:
        ext = [(a.names.index(t), len(ext_sets[t]), lost[t]) for t in names]
        quotas, run_bins, merged, over, _ = plan_restated(paths, rows, h, a.fpr, pop, ext)
        if not over:
            return names, quotas, lost, paths, run_bins, merged
        names = [t for x, t in enumerate(names) if x not in {o[0] for o in over}]


def check_extended(old, new, rep, ext_sets, new_inp, plan):
    """checks 1 - 4: names and strings, every bit against the restatement along the REPORTED paths with the REPORTED quotas, the fills"""
    from ganon_amd import ibf_file
    a, b = ibf_file.read_hibf_meta(old), ibf_file.read_hibf_meta(new)
    accepted, quotas, lost, paths, run_bins, merged = plan
    new_names, new_sets = new_inp.sets(0) if new_inp else ([], [])
    n_old = len(a.names)
    assert b.names[:n_old] == a.names and b.names[n_old:] == new_names, "old names and ids stay, new ones follow in input order"
    assert b.bin_path[:n_old] == a.bin_path and b.user_bin_filenames[:n_old] == a.user_bin_filenames, "the file's strings, verbatim"
    assert list(rep["extended"]) == accepted and list(rep["targets"]) == new_names
    h = a.ibfs[0][2]
    depth = max(len(p) for p in paths.values())
    wide = []
    for i, ((bins_a, rows_a, _, _), (bins_b, rows_b, _, _)) in enumerate(zip(a.ibfs, b.ibfs)):
        assert rows_b == rows_a and bins_b >= bins_a
        m = np.zeros((rows_a, (bins_b + 63) >> 6), dtype=U64)
        m[:, :(bins_a + 63) >> 6] = a.payload(old, i)
        wide.append(m)
    dealt = {(i, bin_): q for i, bin_, q, _, _, _ in rep["run"]}
    entries, rq = [], []
    for x, t in enumerate(accepted):
        r = rep["extended"][t]
        u = a.names.index(t)
        assert r["user_bin"] == u and r["n"] == len(ext_sets[t]) and r["inserted"] == lost[t][0] and r["present"] == r["n"] - lost[t][0]
        assert [e[:2] for e in paths[u]] == r["path"][::-1] and (r["leaf"], r["first"], r["bins"]) == paths[u][0]
        rq.append([dealt[(r["leaf"], r["first"] + j)] for j in range(r["bins"])])
        assert rq[-1] == quotas[x], "the quotas of the restated plan"
        entries.append(paths[u])
    exp, _, _ = extend_ref(wide, h, [ext_sets[t] for t in accepted], as_paths(entries, depth), rq)
    for t, hs in zip(new_names, new_sets):  # as check_update of test_build_update_gpu.py
        r = rep["targets"][t]
        assert r["n"] == len(hs) and r["path"][-1] == (r["leaf"], r["first"])
        for d, (i, first) in enumerate(r["path"]):
            leaf = d == len(r["path"]) - 1
            bins = (first + np.arange(len(hs)) // -(-len(hs) // r["bins"])) if leaf else np.full(len(hs), first)
            or_into(exp[i], h, hs, bins)
    for i in range(len(a.ibfs)):
        assert np.array_equal(b.payload(new, i), exp[i]), f"IBF {i}"
    assert [(r[0], r[1], r[2], r[3]) for r in rep["run"]] == [(r[0], r[1], r[2], r[3]) for r in run_bins]
    for i, bin_, _, before, predicted, after in rep["run"]:
        assert after == int(column_sums(exp[i], b.ibfs[i][0])[bin_]) and after <= predicted + 3 * math.sqrt(a.ibfs[i][1]), (i, bin_, predicted, after)
    for i, bin_, before, predicted, after in rep["merged"]:
        assert after == int(column_sums(exp[i], b.ibfs[i][0])[bin_]) and after <= predicted + 3 * math.sqrt(a.ibfs[i][1]), (i, bin_, predicted, after)
    assert {(m[0], m[1]) for m in merged} <= {(m[0], m[1]) for m in rep["merged"]}, "the merged bins of extended paths are in the merged lines"
    assert f"{len(accepted)} user bin(s) extended, {len(new_names)} user bin(s) added" in rep["result"]
    return a, b


def classify_counts(index, all_members, tmp_path, seed):
    """check 6: two reads from EVERY member of every target: .all / .rep as the oracle backend's, every count = the read's minimisers"""
    rng = np.random.default_rng(seed)
    reads = []
    for fam, members in all_members.items():
        for _, seq in members:
            for _ in range(2):
                at = int(rng.integers(0, len(seq) - 150 + 1))
                reads.append((f"r{len(reads)}", seq[at:at + 150], fam))
    fq = str(tmp_path / "reads.fq")
    gf.write_fastq(fq, [(rid, seq) for rid, seq, _ in reads])
    outs = {}
    for tag, binary in (("hip", cu.BIN_HIP), ("oracle", cu.build_oracle_binary())):
        prefix = str(tmp_path / tag)
        cu.run(binary, ["--ibf", index, "--hibf", "--single-reads", fq, "-o", prefix, "--output-all", "--skip-lca", "--rel-cutoff", "1", "--rel-filter", "1", "--quiet"])
        outs[tag] = (open(prefix + ".all", "rb").read(), open(prefix + ".rep", "rb").read())
    assert outs["hip"] == outs["oracle"], ".all / .rep"
    found = {}
    for line in outs["hip"][0].decode().splitlines():
        rid, target, count = line.split("\t")
        found.setdefault(rid, {})[target] = int(count)
    for rid, seq, fam in reads:
        assert found.get(rid, {}).get(fam) == len(hashes_of(seq)), (rid, fam, found.get(rid), "a hash dealt twice inflates the count")


@pytest.mark.parametrize("tmax", [4, 64])
def test_extend_families(hip, families, tmp_path, tmax):
    """(a): six families built from four members each, extended with a fifth where the restated plan accepts it, two new families added in
    the same command; then the sixth members: an extension of an extension"""
    old_fams = [f"F{f}" for f in range(6)]
    base = inputs(families, {f: [0, 1, 2, 3] for f in old_fams}, str(tmp_path / "base.tsv"))
    files = [str(tmp_path / f"db{i}.hibf") for i in range(3)]
    build(base, files[0], tmax, 3, 0.05, extra=("--layout", "rule"))
    before = open(files[0], "rb").read()
    have = {f: [0, 1, 2, 3] for f in old_fams}
    for step, member in ((1, 4), (2, 5)):
        ext_sets = {f: union(families, f, [member]) for f in old_fams}
        plan = restated(files[step - 1], ext_sets)
        accepted = plan[0]
        print(f"tmax {tmax} step {step}: the restated plan accepts {accepted}")
        assert len(accepted) >= (3 if step == 1 else 1), "the fixture is meant to leave room for at least three extensions, and for one more after them"
        members = {f: [member] for f in accepted}
        if step == 1:
            members.update({"F6": list(range(MEMBERS)), "F7": list(range(MEMBERS))})
        inp = inputs(families, members, str(tmp_path / f"ext{step}.tsv"))
        rep = extend(files[step - 1], inp.tsv, files[step])
        new_inp = inputs(families, {f: members[f] for f in ("F6", "F7")}, str(tmp_path / "new.tsv")) if step == 1 else None
        a, b = check_extended(files[step - 1], files[step], rep, {f: ext_sets[f] for f in accepted}, new_inp, plan)
        assert open(files[0], "rb").read() == before, "the index given is left as it is"
        assert any(r["present"] > 0 and r["inserted"] > 0 for r in rep["extended"].values())
        if tmax == 4:
            assert any(len(r["path"]) > 1 for r in rep["extended"].values()), "an extended user bin under a merged bin"
        for f in members:
            have[f] = sorted(set(have.get(f, [])) | set(members[f]))
        everything = inputs(families, have, str(tmp_path / f"all{step}.tsv"), order=b.names)  # in the index's name order
        assert len(all_ok(files[step], everything, 0)) == len(b.names)
        classify_counts(files[step], {f: [families[f][i] for i in have[f]] for f in have}, tmp_path, tmax + step)


def test_extend_over_the_bound(hip, families, tmp_path):
    """the family that sets its IBF's rows gains an unrelated 40 kbp sequence: exit 1, the target and its bin named, no file"""
    from ganon_amd import ibf_file
    old_fams = [f"F{f}" for f in range(6)]
    base = inputs(families, {f: [0, 1, 2, 3] for f in old_fams}, str(tmp_path / "base.tsv"))
    old, new = str(tmp_path / "old.hibf"), str(tmp_path / "new.hibf")
    build(base, old, 64, 3, 0.05, extra=("--layout", "rule"))
    a = ibf_file.read_hibf_meta(old)
    paths = old_paths(a)
    names, sets = base.sets(0)
    sizing = [t for t, hs in zip(names, sets) if hc.run_bits(len(hs), paths[a.names.index(t)][0][2], a.fpr, a.ibfs[0][2]) == a.ibfs[paths[a.names.index(t)][0][0]][1]]
    assert sizing, "one user bin sets the rows of its IBF"
    fam = sizing[0]
    alien = str(tmp_path / "alien.fasta")
    gf.write_fasta(alien, [("alien", gu.random_seq(np.random.default_rng(40), 40000).decode())])
    tsv = str(tmp_path / "over.tsv")
    open(tsv, "w").write(f"{alien}\t{fam}\n")
    p = extend(old, tsv, new, expect=1)
    i, first, _ = paths[a.names.index(fam)][0]
    assert fam in p.stderr and f"IBF {i} bin {first}" in p.stderr and "leave it out or rebuild" in p.stderr and "nothing written" in p.stderr, p.stderr
    assert p.stdout == "" and not os.path.exists(new)
    # without --extend the same input gets the message it always got, and nothing is written
    p = extend(old, tsv, new, expect=1, flag=())
    assert "is already in the index (adding sequences to an existing user bin is not supported); nothing written" in p.stderr and fam in p.stderr
    assert p.stdout == "" and not os.path.exists(new)


def test_extend_a_hand_laid_index(hip, tmp_path):
    """(b): a tree of three levels laid out here, rows 1.5 x what hibf_run_bits asks, one user bin in a split run of 3 bins, filled with
    emplace_path and written with ibf_file.save_hibf; three of its user bins gain a mutated copy of their sequence"""
    from ganon_amd import hip as H, ibf_file
    from test_build_hibf_gpu import K, W
    rng = np.random.default_rng(33)
    fpr, h = 0.05, 3
    names = [f"H{u}" for u in range(5)]
    seqs, files = {}, {}
    for u, length in enumerate((9000, 24000, 7000, 12000, 8000)):
        base = np.frombuffer(gu.random_seq(rng, length), dtype=np.uint8)
        more = base.copy()
        for at in np.nonzero(rng.random(length) < 0.01)[0]:
            more[at] = [c for c in b"ACGT" if c != more[at]][int(rng.integers(0, 3))]
        seqs[names[u]] = [base.tobytes().decode(), more.tobytes().decode()]
        files[names[u]] = []
        for j, s in enumerate(seqs[names[u]]):
            files[names[u]].append((str(tmp_path / f"{names[u]}_{j}.fasta"), s))
            gf.write_fasta(files[names[u]][-1][0], [(f"{names[u]}_{j}", s)])
    sets = [hashes_cached(seqs[t][0]) for t in names]
    sets = [np.unique(x) for x in sets]
    n = [len(x) for x in sets]
    # IBF 0: H0, a merged bin over IBF 1.  IBF 1: H1 in a run of 3 bins, a merged bin over IBF 2, H2.  IBF 2: H3, H4.
    nx = [np.array([0, 1], np.int64), np.array([1, 1, 1, 2, 1], np.int64), np.array([2, 2], np.int64)]
    bu = [np.array([0, -1], np.int64), np.array([1, 1, 1, -1, 2], np.int64), np.array([3, 4], np.int64)]
    need = [max(hc.run_bits(n[0], 1, fpr, h), hc.run_bits(n[1] + n[2] + n[3] + n[4], 1, fpr, h)),
            max(hc.run_bits(n[1], 3, fpr, h), hc.run_bits(n[3] + n[4], 1, fpr, h), hc.run_bits(n[2], 1, fpr, h)),
            max(hc.run_bits(n[3], 1, fpr, h), hc.run_bits(n[4], 1, fpr, h))]
    rows = [int(1.5 * x) for x in need]
    shapes = [(2, rows[0], h), (5, rows[1], h), (2, rows[2], h)]
    flt = hip.HipFilter.hibf([(None, b, r, hf) for b, r, hf in shapes], nx, bu, 5)
    where = {0: [(0, 0, 1)], 1: [(1, 0, 3), (0, 1, 1)], 2: [(1, 4, 1), (0, 1, 1)], 3: [(2, 0, 1), (1, 3, 1), (0, 1, 1)], 4: [(2, 1, 1), (1, 3, 1), (0, 1, 1)]}
    p = np.zeros((5, 3), dtype=H.PATH_DTYPE)
    for u, es in where.items():
        for d, (i, first, nb) in enumerate(es):
            p[u, d] = (i, first, nb, 0, -(-n[u] // nb) if d == 0 else 1)
    flt.emplace_path(sets, p)
    old, new = str(tmp_path / "hand.hibf"), str(tmp_path / "hand_extended.hibf")
    ibf_file.save_hibf(old, flt, shapes, nx, bu, names, K, W, fpr)
    flt.free()
    before = open(old, "rb").read()
    chosen = ["H1", "H3", "H0"]
    ext_sets = {t: np.unique(hashes_cached(seqs[t][1])) for t in chosen}
    plan = restated(old, ext_sets)
    assert plan[0] == chosen, "rows at 1.5 x leave room for every extension"
    assert plan[3] == where, "the paths read from the file are the ones laid out"
    tsv = str(tmp_path / "ext.tsv")
    with open(tsv, "w") as o:
        for t in chosen:
            o.write(f"{files[t][1][0]}\t{t}\n")
    rep = extend(old, tsv, new)
    a, b = check_extended(old, new, rep, ext_sets, None, plan)
    assert open(old, "rb").read() == before, "the index given is left as it is"
    r = rep["extended"]
    assert r["H1"]["bins"] == 3 and len(r["H3"]["path"]) == 3 and len(r["H1"]["path"]) == 2, "a split run, and user bins under one and two merged bins"
    assert all(x["present"] > 0 and x["inserted"] > 0 for x in r.values())
    assert sum(q > 0 for i, bin_, q, *_ in rep["run"] if i == 1 and bin_ < 3) >= 2, "the split run's hashes go to more than one of its bins"
    have = {t: ([0, 1] if t in chosen else [0]) for t in names}
    with open(str(tmp_path / "all.tsv"), "w") as o:
        for t in names:
            for j in have[t]:
                o.write(f"{files[t][j][0]}\t{t}\n")
    everything = FamilyInputs(str(tmp_path / "all.tsv"), names, {t: [seqs[t][j] for j in have[t]] for t in names})
    assert len(all_ok(new, everything, 0)) == 5
    classify_counts(new, {t: [files[t][j] for j in have[t]] for t in names}, tmp_path, 33)


def test_extend_a_name_two_user_bins_hold(hip, tmp_path):
    """an index whose two user bins carry one name: the target is refused, nothing is written"""
    from ganon_amd import ibf_file
    from test_build_hibf_gpu import K, W
    flt = one_ibf(hip, 3, 20011, 3)
    old, new = str(tmp_path / "twice.hibf"), str(tmp_path / "new.hibf")
    ibf_file.save_hibf(old, flt, [(3, 20011, 3)], [np.zeros(3, np.int64)], [np.arange(3, dtype=np.int64)], ["D", "E", "D"], K, W, 0.05)
    flt.free()
    fasta, tsv = str(tmp_path / "d.fasta"), str(tmp_path / "d.tsv")
    gf.write_fasta(fasta, [("d", gu.random_seq(np.random.default_rng(2), 3000).decode())])
    open(tsv, "w").write(f"{fasta}\tD\n")
    p = extend(old, tsv, new, expect=1)
    assert "2 user bins of the index are named D" in p.stderr and "nothing written" in p.stderr, p.stderr
    assert p.stdout == "" and not os.path.exists(new)
