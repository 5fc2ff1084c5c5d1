"""`ganon-build --hibf --verify-index` in parts on the GPU: gn_filter_probe_path_window and gn_filter_probe_paths_shared_window on storage
filters of pieces, carried from part to part and closed as ganon_amd/host/hibf_verify_parts.hpp states it (restated here in numpy),
against the one-piece calls gn_filter_probe_path / gn_filter_probe_paths_shared on the whole filter and their numpy restatements; hand-made
filters that tell a carried answer from a per-slab one; the refusals; and the binary under budgets that cut the index by IBF and by rows:
the one-device report to the byte.  No expected value comes from the new calls."""
import ctypes as C
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from test_build_cpu import BIN_BUILD
from test_build_hibf_gpu import K, W, build, genomes, hip, short200  # noqa: F401  (fixtures among them)
from test_build_hibf_parts_cpu import parts_of, plan_rule
from test_build_hibf_parts_gpu import INPUTS, beside, budget_of, one_pass, tree
from test_build_verify_gpu import NONE, built, probe_path_ref, rows_of, shared_ref, swapped_tsv  # noqa: F401  (built: a fixture)

pytestmark = pytest.mark.gpu

U64 = np.uint64
ONES = U64(NONE)


# ------------------------------------------------------------------------------------------------------------ the carried state, restated
def words_of(n):
    return (n + 63) // 64


def valid_of(n):
    v = np.full(words_of(n), ONES, U64)
    if n % 64:
        v[-1] = U64((1 << (n % 64)) - 1)
    return v


def popcount(a):
    return int(np.unpackbits(np.ascontiguousarray(a, dtype=U64).view(np.uint8)).sum())


def bits_of(a, n):
    return np.unpackbits(np.ascontiguousarray(a, dtype=U64).view(np.uint8), bitorder="little")[:n].astype(bool)


def compact(paths, pieces, rows_total):
    """the units with an entry in one of the part's IBFs: (kept units, their paths cut down and renumbered, per kept entry the entry of the
    whole path it was, per kept entry whether its piece is a slab)"""
    local = {t: j for j, (t, _, _) in enumerate(pieces)}
    out, orig, slab, keep = [], [], [], []
    for u in range(paths.shape[0]):
        cut, og, sl = np.zeros(paths.shape[1], dtype=paths.dtype), [], []
        for d in range(paths.shape[1]):
            if paths[u, d]["n_bins"] == 0:
                break
            t = int(paths[u, d]["ibf"])
            if t in local:
                cut[len(og)] = paths[u, d]
                cut[len(og)]["ibf"] = local[t]
                og.append(d)
                sl.append(pieces[local[t]][2] != rows_total[t])
        if og:
            keep.append(u), out.append(cut), orig.append(og), slab.append(sl)
    return keep, (np.stack(out) if out else np.zeros((0, paths.shape[1]), dtype=paths.dtype)), orig, slab


def storage_of(hip, shapes, mats, pieces):  # noqa: F811
    """a storage filter of `pieces` (tree ibf, row_begin, n_rows) with those rows written, as the command loads a part"""
    flt = hip.HipFilter.hibf_storage([(shapes[t][0], n, shapes[t][2]) for t, _, n in pieces])
    for j, (t, a, n) in enumerate(pieces):
        flt.write_rows(0, np.ascontiguousarray(mats[t][a:a + n]), ibf_idx=j)
    return flt


class Carry:
    """alive, lost_at and the open planes of every unit, as hibf_verify_parts.hpp keeps them"""

    def __init__(self, sizes, depth):
        self.sizes = list(sizes)
        self.alive = [valid_of(n) for n in sizes]
        self.lost = np.zeros((len(sizes), depth), U64)
        self.planes = {}

    def take(self, u, alive):
        self.alive[u] &= alive

    def take_planes(self, u, d, planes):
        if (u, d) not in self.planes:
            self.planes[(u, d)] = np.full_like(planes, ONES)
        self.planes[(u, d)] &= planes

    def close_all(self):
        for (u, d), pl in self.planes.items():
            hit = np.bitwise_or.reduce(pl, axis=0)
            self.lost[u, d] += U64(popcount(valid_of(self.sizes[u]) & ~hit))
            self.alive[u] &= hit
        self.planes = {}

    def result(self):
        found = np.array([popcount(a & valid_of(n)) for a, n in zip(self.alive, self.sizes)], U64)
        first = np.full(len(self.sizes), ONES, U64)
        for u, (a, n) in enumerate(zip(self.alive, self.sizes)):
            dead = ~bits_of(a, n)
            if dead.any():
                first[u] = int(np.argmax(dead))
        return found, self.lost, first


def member_in_parts(hip, shapes, mats, sets, paths, parts, chunk=0):  # noqa: F811
    """(found, lost_at, first_lost) of sets along paths, from the windowed probe over `parts` (lists of pieces), carried and closed"""
    rows_total = [s[1] for s in shapes]
    st = Carry([len(s) for s in sets], paths.shape[1])
    for pieces in parts:
        keep, cut, orig, slab = compact(paths, pieces, rows_total)
        flt = storage_of(hip, shapes, mats, pieces)
        alive = [valid_of(len(sets[u])) for u in keep]
        lost = np.zeros((len(keep), paths.shape[1]), U64)
        planes = {(j, k): np.full((int(cut[j, k]["n_bins"]), words_of(len(sets[keep[j]]))), ONES, U64)
                  for j in range(len(keep)) for k in range(len(orig[j])) if slab[j][k]}
        flt.probe_path_window([sets[u] for u in keep], cut, [rows_total[t] for t, _, _ in pieces], [a for _, a, _ in pieces], alive, lost, planes, chunk)
        flt.free()
        for j, u in enumerate(keep):
            st.take(u, alive[j])
            for k, d in enumerate(orig[j]):
                if slab[j][k]:
                    assert lost[j, k] == 0, "lost_at is for whole pieces only"
                    st.take_planes(u, d, planes[(j, k)])
                else:
                    st.lost[u, d] += lost[j, k]
    st.close_all()
    return st.result()


def shared_in_parts(hip, shapes, mats, probes, paths, parts):  # noqa: F811
    """probes contained per path, from the windowed shared probe over `parts`"""
    rows_total = [s[1] for s in shapes]
    st = Carry([len(probes)] * paths.shape[0], paths.shape[1])
    nw = words_of(len(probes))
    for pieces in parts:
        keep, cut, orig, slab = compact(paths, pieces, rows_total)
        flt = storage_of(hip, shapes, mats, pieces)
        alive = np.tile(valid_of(len(probes)), (len(keep), 1))
        planes = {(j, k): np.full((int(cut[j, k]["n_bins"]), nw), ONES, U64) for j in range(len(keep)) for k in range(len(orig[j])) if slab[j][k]}
        flt.probe_paths_shared_window(probes, cut, [rows_total[t] for t, _, _ in pieces], [a for _, a, _ in pieces], alive, planes)
        flt.free()
        for j, u in enumerate(keep):
            st.take(u, alive[j])
            for k, d in enumerate(orig[j]):
                if slab[j][k]:
                    st.take_planes(u, d, planes[(j, k)])
    st.close_all()
    return st.result()[0]


def exercises_the_carry(shapes, sets, paths, parts):
    """at least two pieces, and at least one hash of an asked set with rows in two different pieces"""
    pieces = [(p, t, a, n) for p, pc in enumerate(parts) for t, a, n in pc]
    if len(pieces) < 2:
        return False
    for u, hs in enumerate(sets):
        if len(hs) == 0:
            continue
        hs, holds = hs[:64], []  # per piece: which of the set's first hashes have a row in it
        for d in range(paths.shape[1]):
            if paths[u, d]["n_bins"] == 0:
                break
            t = int(paths[u, d]["ibf"])
            rows = [rows_of(hs, i, shapes[t][1]) for i in range(shapes[t][2])]
            holds += [np.any([(r >= a) & (r < a + n) for r in rows], axis=0) for _, tt, a, n in pieces if tt == t]
        if holds and (np.sum(holds, axis=0) >= 2).any():
            return True
    return False


# ------------------------------------------------------------------------------------------------------------ whole trees
SHAPES = [(40, 8, 3), (10, 4, 4)]
SIZES = (0, 1, 63, 64, 65, 511, 512, 513, 1500, 20000)
_CASES = {}


def case(hip, n_ub, tmax, depth, h):  # noqa: F811
    """a tree of test_build_hibf_parts_gpu with sets to ask for (of every size in SIZES, part members and part strangers), probes, its rows
    intact and with bits cleared, and what the one-piece calls and their restatements say about both: made once, never changed"""
    key = (n_ub, tmax, depth, h)
    if key in _CASES:
        return _CASES[key]
    hb, sets, paths, where, parent, shapes, ref = tree(hip, n_ub, tmax, depth, h)
    rng = np.random.default_rng(n_ub + h)
    asked = []
    for u in range(n_ub):
        want = SIZES[u % len(SIZES)]
        pool = np.unique(np.concatenate([sets[u][:want - want // 8], rng.integers(0, 1 << 38, size=2 * want + 8, dtype=U64)]))
        asked.append(np.sort(rng.permutation(pool)[:want]) if want < len(pool) else pool[:want])
        assert len(asked[-1]) == want
    members = np.concatenate([s[:7] for s in sets])
    probes = rng.permutation(np.concatenate([rng.integers(0, 1 << 38, size=1000 - min(300, len(members)), dtype=U64), members[:300]]))
    assert len(probes) == 1000  # not a multiple of 64
    fp_paths = paths[np.arange(150) % n_ub]  # more than a wave of paths: paths repeat
    damaged = [m.copy() for m in ref]
    for m in damaged:
        m &= rng.integers(0, 1 << 63, size=m.shape, dtype=U64) | (rng.integers(0, 1 << 63, size=m.shape, dtype=U64) << U64(1))  # a quarter of the bits goes
        m[rng.integers(0, m.shape[0], size=5)] = 0  # and whole rows
    out = dict(shapes=shapes, paths=paths, asked=asked, probes=probes, fp_paths=fp_paths, where=where, mats={"intact": ref, "damaged": damaged}, want={})
    for state, mats in out["mats"].items():
        one = hip.HipFilter.hibf([(None,) + s for s in shapes], hb.next_ibf_id, hb.bin_to_user, n_ub)
        for i, m in enumerate(mats):
            one.write_rows(0, m, ibf_idx=i)
        member, shared = one.probe_path(asked, paths), one.probe_paths_shared(probes, fp_paths)
        one.free()
        exp = probe_path_ref(mats, h, asked, paths)
        assert all(np.array_equal(a, b) for a, b in zip(member, (exp[0], exp[1], exp[2]))), "the one-piece call and its restatement agree"
        assert np.array_equal(shared, shared_ref(mats, h, probes, fp_paths))
        out["want"][state] = (member, shared)
    sizes = np.array([len(a) for a in asked], U64)
    assert (out["want"]["intact"][0][0] < sizes).any() and out["want"]["intact"][0][0].any(), "strangers are lost, members are found"
    assert (out["want"]["damaged"][0][0] < out["want"]["intact"][0][0]).any() and (out["want"]["damaged"][1] < out["want"]["intact"][1]).any()
    _CASES[key] = out
    return out


def check_parts(hip, c, parts, chunk=0, fp=True):  # noqa: F811
    assert exercises_the_carry(c["shapes"], c["asked"], c["paths"], parts)
    covered = {}
    for pc in parts:
        for t, a, n in pc:
            covered[t] = covered.get(t, 0) + n
    assert covered == {t: s[1] for t, s in enumerate(c["shapes"])}, "every row of every IBF in exactly one piece"
    for state, mats in c["mats"].items():
        member, shared = c["want"][state]
        found, lost, first = member_in_parts(hip, c["shapes"], mats, c["asked"], c["paths"], parts, chunk)
        assert np.array_equal(found, member[0]), state
        assert np.array_equal(first, member[2]), state
        assert np.array_equal(lost, member[1]), state
        if fp:
            assert np.array_equal(shared_in_parts(hip, c["shapes"], mats, c["probes"], c["fp_paths"], parts), shared), state


@pytest.mark.parametrize("h", [1, 3, 5])
@pytest.mark.parametrize("n_ub,tmax,depth", SHAPES)
def test_every_ibf_whole_in_one_storage_filter(hip, n_ub, tmax, depth, h):  # noqa: F811
    c = case(hip, n_ub, tmax, depth, h)
    check_parts(hip, c, [[(t, 0, s[1]) for t, s in enumerate(c["shapes"])]])


@pytest.mark.parametrize("h", [1, 3, 5])
@pytest.mark.parametrize("n_ub,tmax,depth", SHAPES)
def test_every_ibf_alone_with_compacted_paths(hip, n_ub, tmax, depth, h):  # noqa: F811
    c = case(hip, n_ub, tmax, depth, h)
    check_parts(hip, c, [[(t, 0, s[1])] for t, s in enumerate(c["shapes"])])


@pytest.mark.parametrize("chunk", [0, 512, 700])
@pytest.mark.parametrize("h", [1, 3, 5])
@pytest.mark.parametrize("n_ub,tmax,depth", SHAPES)
def test_the_root_and_a_leaf_in_pieces(hip, n_ub, tmax, depth, h, chunk):  # noqa: F811
    c = case(hip, n_ub, tmax, depth, h)
    shapes = c["shapes"]
    leaf = c["where"][9][0]  # the IBF that holds the run of the user bin asked with 20 000 hashes
    if leaf == 0:
        leaf = max(i for i, _, _ in c["where"].values())
    for cut_ibf in (0, leaf):
        rows = shapes[cut_ibf][1]
        cuts = [0, 1, 7, 512, 999, 1000, rows // 2, rows - 1, rows]
        assert cuts == sorted(cuts)
        parts = [[(cut_ibf, a, b - a)] for a, b in zip(cuts, cuts[1:]) if b > a]
        parts.insert(3, [(t, 0, s[1]) for t, s in enumerate(shapes) if t != cut_ibf])  # the other IBFs whole, between two slabs
        check_parts(hip, c, parts, chunk, fp=chunk == 0)


# ------------------------------------------------------------------------------------------------------------ hand-made filters
ROWS0, ROWS1, H3 = 4001, 7001, 3
NX = [np.array([1], np.int64), np.full(192, 1, np.int64)]
BU = [np.array([-1], np.int64), np.arange(192, dtype=np.int64)]
HAND = [(1, ROWS0, H3), (192, ROWS1, H3)]  # (bins, rows, h): a root of one merged bin over an IBF of 192 bins


def hand_path(first, n):
    from ganon_amd import hip as H
    p = np.zeros((1, 2), dtype=H.PATH_DTYPE)
    p[0, 0] = (1, first, n, 0, 1)
    p[0, 1] = (0, 0, 1, 0, 1)
    return p


def hand_rows(v, ibf):
    return [int(rows_of(np.array([v], U64), i, HAND[ibf][1])[0]) for i in range(H3)]


def hand_hashes(n, seed):
    """hashes whose three rows in the leaf are distinct, so that the leaf can be cut between any two of them"""
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < n:
        v = int(rng.integers(1, 1 << 38))
        if len(set(hand_rows(v, 1))) == 3 and v not in out:
            out.append(v)
    return np.array(sorted(out), U64)


def set_bit(m, row, b):
    m[row, b >> 6] |= U64(1 << (b & 63))


def hand_mats(root_full=True):
    return [np.full((ROWS0, 1), U64(1) if root_full else U64(0), U64), np.zeros((ROWS1, 3), U64)]


def one_piece(hip, mats, sets, paths, probes=None):  # noqa: F811
    flt = hip.HipFilter.hibf([(None,) + s for s in HAND], NX, BU, 192)
    for i, m in enumerate(mats):
        flt.write_rows(0, m, ibf_idx=i)
    out = flt.probe_path(sets, paths) if probes is None else flt.probe_paths_shared(probes, paths)
    flt.free()
    return out


def cut_between(rows, k):
    """the leaf in k + 1 slabs, cut in front of the k largest of a hash's rows: every slab holds at least one of them when k = 2"""
    at = sorted(rows)[-k:]
    return [0] + at + [ROWS1]


def test_a_bin_per_slab_is_no_bin(hip):  # noqa: F811
    """a run of two bins; the hash's rows in slab A carry only bin b, those in slab B only bin b + 1: lost, and a probe of the false-positive
    pass is no false hit.  A per-slab OR would call both found."""
    v = hand_hashes(1, 1)
    b, rows = 70, hand_rows(int(v[0]), 1)
    mats = hand_mats()
    edges = cut_between(rows, 1)
    for r in rows:
        set_bit(mats[1], r, b if r < edges[1] else b + 1)
    assert any(r < edges[1] for r in rows) and any(r >= edges[1] for r in rows)
    paths = hand_path(b, 2)
    want = one_piece(hip, mats, [v], paths)
    assert want[0].tolist() == [0] and want[1].tolist() == [[1, 0]] and want[2].tolist() == [0], "the whole filter: lost in the leaf"
    parts = [[(0, 0, ROWS0)], [(1, edges[0], edges[1] - edges[0])], [(1, edges[1], edges[2] - edges[1])]]
    for pc in parts[1:]:  # each slab alone says yes
        assert member_in_parts(hip, HAND, mats, [v], paths, [[(0, 0, ROWS0)], pc, ])[0].tolist() == [1]
    got = member_in_parts(hip, HAND, mats, [v], paths, parts)
    assert all(np.array_equal(a, w) for a, w in zip(got, want))
    probes = np.concatenate([v, hand_hashes(70, 2)])  # the hash as probe 0 of 71
    assert one_piece(hip, mats, None, paths, probes).tolist() == [0]
    assert shared_in_parts(hip, HAND, mats, probes, paths, parts).tolist() == [0]
    for r in rows:  # ... and with bin b + 1 in every row it is found, in parts too
        set_bit(mats[1], r, b + 1)
    assert member_in_parts(hip, HAND, mats, [v], paths, parts)[0].tolist() == [1] == one_piece(hip, mats, [v], paths)[0].tolist()
    assert shared_in_parts(hip, HAND, mats, probes, paths, parts).tolist() == [1] == one_piece(hip, mats, None, paths, probes).tolist()


def test_a_run_over_a_word_boundary_cut_between_every_pair_of_rows(hip):  # noqa: F811
    """bins 60 .. 67; per hash a slab for each of its rows.  Found: the same bin in all three rows, in the first word or in the second.
    Lost: a bin in every row but never the same, bins just outside the run, a row without a bit."""
    vs = hand_hashes(6, 3)
    rows = [hand_rows(int(v), 1) for v in vs]
    mats = hand_mats()
    plan = [[61, 61, 61], [66, 66, 66], [61, 63, 66], [59, 59, 59], [68, 68, 68], [64, 64, None]]
    for rr, bins in zip(rows, plan):
        for r, b in zip(rr, bins):
            if b is not None:
                set_bit(mats[1], r, b)
    paths = hand_path(60, 8)
    want = one_piece(hip, mats, [vs], paths)
    assert want[0].tolist() == [2]
    for k in range(len(vs)):  # the cuts of every hash in turn
        edges = cut_between(rows[k], 2)
        parts = [[(1, a, b - a)] for a, b in zip(edges, edges[1:])] + [[(0, 0, ROWS0)]]
        assert len(parts) == 4 and len({sum(r >= e for e in edges) for r in rows[k]}) == 3, "each of the hash's rows in a slab of its own"
        got = member_in_parts(hip, HAND, mats, [vs], paths, parts)
        assert all(np.array_equal(a, w) for a, w in zip(got, want)), k
        assert np.array_equal(shared_in_parts(hip, HAND, mats, vs, paths, parts), one_piece(hip, mats, None, paths, vs))


def test_lost_twice_is_lost_once(hip):  # noqa: F811
    """hash 1 of three misses a row in two different slabs of the leaf: lost_at counts it once.  Hash 0 misses the root, whole in part 0, and
    a row in a slab of the leaf, a later part: found counts it once and first_lost is the smaller index."""
    vs = hand_hashes(3, 4)
    rows = [hand_rows(int(v), 1) for v in vs]
    assert len({r for rr in rows for r in rr}) == 9, "no two hashes share a row"
    mats = hand_mats()
    for rr in rows:
        for r in rr:
            set_bit(mats[1], r, 5)
    srt = sorted(rows[1])
    edges = [0, srt[1], srt[2], ROWS1]  # each row of hash 1 in a slab of its own
    mats[1][srt[0]] = 0
    mats[1][srt[2]] = 0
    mats[1][max(rows[0])] = 0
    for r in hand_rows(int(vs[0]), 0):
        mats[0][r] = 0
    paths = hand_path(5, 1)
    want = one_piece(hip, mats, [vs], paths)
    assert want[0].tolist() == [1] and want[1].tolist() == [[2, 1]] and want[2].tolist() == [0]
    parts = [[(0, 0, ROWS0)]] + [[(1, a, b - a)] for a, b in zip(edges, edges[1:])]
    for order in (parts, parts[::-1], parts[2:] + parts[:2]):
        got = member_in_parts(hip, HAND, mats, [vs], paths, order)
        assert all(np.array_equal(a, w) for a, w in zip(got, want)), (got, want)


def test_a_piece_no_row_falls_into_changes_nothing(hip):  # noqa: F811
    vs = hand_hashes(3, 5)
    used = sorted({r for v in vs for r in hand_rows(int(v), 1)})
    gaps = [(a + 1, b) for a, b in zip([-1] + used, used + [ROWS1]) if b - a > 1]
    a, b = max(gaps, key=lambda g: g[1] - g[0])
    mats = hand_mats()  # the leaf all zero: a row that did fall into the piece would clear its planes
    flt = storage_of(hip, HAND, mats, [(1, a, b - a)])
    p = hand_path(60, 8)
    p[0, 0]["ibf"], p[0, 1]["n_bins"] = 0, 0
    alive, lost, planes = [valid_of(3)], np.zeros((1, 2), U64), {(0, 0): np.full((8, 1), ONES, U64)}
    flt.probe_path_window([vs], p, [ROWS1], [a], alive, lost, planes)
    # (the bits behind the last hash are whatever the lanes without a hash answered: nobody reads them)
    assert alive[0].tolist() == [7] and not lost.any() and (planes[(0, 0)] & U64(7) == U64(7)).all()
    fp_alive, fp_planes = valid_of(3)[None, :].copy(), {(0, 0): np.full((8, 1), ONES, U64)}
    flt.probe_paths_shared_window(vs, p, [ROWS1], [a], fp_alive, fp_planes)
    assert fp_alive.tolist() == [[7]] and (fp_planes[(0, 0)] & U64(7) == U64(7)).all()
    flt.free()
    r = used[0]  # and a piece of the one row a hash does fall into says so, for that hash, in every bin
    left = 7 - sum(1 << k for k, v in enumerate(vs) if r in hand_rows(int(v), 1))
    assert left != 7
    flt = storage_of(hip, HAND, mats, [(1, r, 1)])
    planes, fp_planes = {(0, 0): np.full((8, 1), ONES, U64)}, {(0, 0): np.full((8, 1), ONES, U64)}
    flt.probe_path_window([vs], p, [ROWS1], [r], alive, lost, planes)
    flt.probe_paths_shared_window(vs, p, [ROWS1], [r], fp_alive, fp_planes)
    assert alive[0].tolist() == [7] and fp_alive.tolist() == [[7]] and not lost.any(), "an entry in a slab is answered into its planes alone"
    assert (planes[(0, 0)] & U64(7) == U64(left)).all() and (fp_planes[(0, 0)] & U64(7) == U64(left)).all()
    flt.free()


# ------------------------------------------------------------------------------------------------------------ refusals
def test_refusals_change_no_buffer(hip):  # noqa: F811
    H = hip.hip
    hs = np.sort(np.arange(1, 1001, dtype=U64) * U64(0x9E3779B97F4A7C15 % (1 << 38)))
    probes = hs[:100]
    flt = hip.HipFilter.hibf_storage([(70, 500, 3), (8, 300, 3)])
    flt.write_rows(0, np.full((500, 2), U64(0x5555555555555555)), ibf_idx=0)

    def path(*entries):
        p = np.zeros((1, 2), dtype=H.PATH_DTYPE)
        for d, e in enumerate(entries):
            p[0, d] = e
        return p

    good = path((1, 2, 4, 0, 250), (0, 69, 1, 0, 1))
    state = lambda: ([valid_of(1000)], np.full((1, 2), 7, U64), {(0, 0): np.full((4, 16), ONES, U64)},  # noqa: E731
                     valid_of(100)[None, :].copy(), {(0, 1): np.full((1, 2), ONES, U64)})
    cases = [("an IBF out of range", path((2, 0, 1, 0, 1)), [500, 300], [0, 0], -22),
             ("a bin out of range", path((1, 5, 4, 0, 250)), [500, 300], [0, 0], -22),
             ("a bin out of range above", path((1, 2, 4, 0, 250), (0, 70, 1, 0, 1)), [500, 300], [0, 0], -22),
             ("row_begin + rows > total_rows", good, [500, 300], [0, 1], -22),
             ("rows > total_rows", good, [499, 300], [0, 0], -22),
             ("total_rows of 2^32", good, [1 << 32, 300], [0, 0], -34),
             ("total_rows of 0", good, [500, 0], [0, 0], -34)]
    for what, p, total, begin, code in cases:
        alive, lost, planes, fp_alive, fp_planes = state()
        for call in (lambda: flt.probe_path_window([hs], p, total, begin, alive, lost, planes),
                     lambda: flt.probe_paths_shared_window(probes, p, total, begin, fp_alive, fp_planes)):
            with pytest.raises(hip.GanonHipError) as e:
                call()
            assert e.value.code == code, (what, str(e.value))
        for got, was in zip((alive, lost, planes, fp_alive, fp_planes), state()):
            assert str(got) == str(was), what
    # IBFs of unequal hash functions
    mixed = hip.HipFilter.hibf_storage([(70, 500, 3), (8, 300, 2)])
    alive, lost, planes, fp_alive, fp_planes = state()
    for call in (lambda: mixed.probe_path_window([hs], good, [500, 300], [0, 0], alive, lost, planes),
                 lambda: mixed.probe_paths_shared_window(probes, good, [500, 300], [0, 0], fp_alive, fp_planes)):
        with pytest.raises(hip.GanonHipError) as e:
            call()
        assert e.value.code == -22 and "hash functions" in str(e.value)
    mixed.free()
    # a flat filter is no HIBF
    flat = hip.HipFilter.ibf_storage(70, 500, 3)
    for call in (lambda: flat.probe_path_window([hs], path((0, 0, 1, 0, 1)), [500], [0], alive, lost[:, :2], None),
                 lambda: flat.probe_paths_shared_window(probes, path((0, 0, 1, 0, 1)), [500], [0], fp_alive, None)):
        with pytest.raises(hip.GanonHipError) as e:
            call()
        assert e.value.code == -22 and "HIBF" in str(e.value)
    flat.free()
    for got, was in zip((alive, lost, planes, fp_alive, fp_planes), state()):
        assert str(got) == str(was)
    # null arguments, through the library itself (planes may be null: every entry is then a whole piece)
    L = hip.load_library()
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    sizes, total, begin = np.array([len(hs)], U64), np.array([500, 300], U64), np.array([0, 0], U64)
    ptrs, aptrs = (C.c_void_p * 1)(hs.ctypes.data), (C.c_void_p * 1)(alive[0].ctypes.data)
    full = [flt._h, ptrs, vp(sizes), 1, vp(good), 2, vp(total), vp(begin), aptrs, None, vp(lost), 0]
    for k in (0, 1, 2, 4, 6, 7, 8, 10):
        args = list(full)
        args[k] = None
        assert L.gn_filter_probe_path_window(*args) == -22, k
    args = list(full)
    args[5] = 0  # no depth
    assert L.gn_filter_probe_path_window(*args) == -22
    full = [flt._h, vp(probes), len(probes), vp(good), 1, 2, vp(total), vp(begin), vp(fp_alive), None]
    for k in (0, 1, 3, 6, 7, 8):
        args = list(full)
        args[k] = None
        assert L.gn_filter_probe_paths_shared_window(*args) == -22, k
    for got, was in zip((alive, lost, planes, fp_alive, fp_planes), state()):
        assert str(got) == str(was)
    # nothing to do is legal and changes nothing; and the call that is not refused answers
    flt.probe_path_window([], np.zeros((0, 2), dtype=H.PATH_DTYPE), [500, 300], [0, 0], [], np.zeros((0, 2), U64))
    flt.probe_paths_shared_window(np.zeros(0, U64), good, [500, 300], [0, 0], np.zeros((1, 0), U64))
    flt.probe_path_window([hs], good, [500, 300], [0, 0], alive, lost, None)
    assert popcount(alive[0]) == 0 and lost.tolist() == [[7 + 1000, 7 + 1000]], "bins 2 .. 5 of an empty IBF, bin 69 of one with the even bins set"
    flt.free()


# ------------------------------------------------------------------------------------------------------------ the binary
def run_verify(index, tsv, extra=(), expect=0):
    p = subprocess.run([BIN_BUILD, "--hibf", "--verify-index", index, "-i", tsv, "-t", "2"] + list(extra), capture_output=True, text=True, timeout=300)
    assert p.returncode == expect, (p.returncode, p.stdout[-2000:], p.stderr[-2000:])
    return p


def ibfs_of(hip, index):  # noqa: F811
    """(rows, device bytes a row) per IBF of an index"""
    from ganon_amd import ibf_file
    L = hip.load_library()
    return [(rows, int(L.gn_hibf_row_stride_words((bins + 63) // 64)) * 8) for bins, rows, _, _ in ibf_file.read_hibf_meta(index).ibfs]


def parse_verbose(stderr):
    pieces, parts, end = {}, {}, None
    for ln in stderr.splitlines():
        m = re.fullmatch(r"part (\d+) device (\d+): ibf (\d+) rows \[(\d+), (\d+)\)", ln)
        if m:
            p, d, i, a, b = map(int, m.groups())
            pieces.setdefault(p, []).append((d, i, a, b - a))
        m = re.match(r"part (\d+) entry (\d+): (\d+) device bytes, (\d+) sets and (\d+) user bins probed, loaded in \S+ s, membership in \S+ s, fp in \S+ s$", ln)
        if m:
            p, e, by, n, u = map(int, m.groups())
            assert p not in parts
            parts[p] = (e, by, n, u)
        m = re.fullmatch(r"checked in (\d+) parts, (\d+) hash bytes uploaded \(one pass: (\d+)\)", ln)
        if m:
            assert end is None
            end = tuple(int(x) for x in m.groups())
    return pieces, parts, end


def check_parts_lines(stderr, ibfs, budget, n_entries):
    want = parts_of(plan_rule(ibfs, budget, n_entries), ibfs)
    pieces, parts, end = parse_verbose(stderr)
    assert sorted(pieces) == sorted(parts) == list(range(len(want))), (len(pieces), len(parts), len(want))
    for p, pc in enumerate(want):
        assert [x[1:] for x in pieces[p]] == pc, ("the part lines are those of the restated plan", p)
        e, by, n_sets, n_bins = parts[p]
        assert e == p % n_entries, "parts dealt round robin"
        assert by == sum(n * ibfs[i][1] for i, _, n in pc) <= budget, (p, by, budget)
        assert n_sets >= 1 and n_bins >= 1
    assert end[0] == len(want) and end[1] >= end[2] > 0, end
    assert re.search(r"^ - seconds: hash [0-9.e+-]+ load [0-9.e+-]+ membership [0-9.e+-]+ fp [0-9.e+-]+$", stderr, re.M), stderr
    return want


@pytest.mark.parametrize("kind", ["whole", "three", "two"])
@pytest.mark.parametrize("which", ["genomes", "short200"])
def test_budgets(hip, request, tmp_path_factory, which, kind):  # noqa: F811
    inp, one, ibfs, _ = one_pass(hip, request, tmp_path_factory, which)
    want_out = run_verify(one, inp.tsv).stdout
    assert want_out.splitlines()[-1].startswith("result\tok\t")
    budget = budget_of(ibfs, kind)
    p = run_verify(one, inp.tsv, extra=("--verbose", "--verify-memory", str(budget)))
    assert p.stdout == want_out, "the one-device report to the byte"
    want = check_parts_lines(p.stderr, ibfs, budget, 1)
    big = max(range(len(ibfs)), key=lambda i: ibfs[i][0] * ibfs[i][1])
    slabs = [pc for pc in want if pc[0][0] == big]
    if kind == "whole":
        assert len(want) > 1 and all(a == 0 and n == ibfs[i][0] for pc in want for i, a, n in pc), "every IBF whole, in several parts"
    else:
        assert len(slabs) == {"three": 3, "two": 2}[kind] and all(len(pc) == 1 for pc in slabs)


@pytest.mark.parametrize("entries", ["0,0", "0,0,0"])
def test_parts_dealt_to_a_list(hip, request, tmp_path_factory, entries):  # noqa: F811
    inp, one, ibfs, _ = one_pass(hip, request, tmp_path_factory, "short200")
    budget = budget_of(ibfs, "three")
    p = run_verify(one, inp.tsv, extra=("--verbose", "--verify-memory", str(budget), "--verify-devices", entries))
    assert p.stdout == run_verify(one, inp.tsv).stdout
    assert len(check_parts_lines(p.stderr, ibfs, budget, entries.count(",") + 1)) > 3


def every_ibf_cut(ibfs):
    """a budget under which every IBF of the index is cut into slabs: whatever is damaged lies in a slab"""
    budget = min((r - 1) * b for r, b in ibfs)
    want = parts_of(plan_rule(ibfs, budget, 1), ibfs)
    assert all(len(pc) == 1 and pc[0][2] < ibfs[pc[0][0]][0] for pc in want) and len(want) < 400
    return budget


def same_report(index, tsv, ibfs, expect):
    want = run_verify(index, tsv, expect=expect)
    got = run_verify(index, tsv, extra=("--verify-memory", str(every_ibf_cut(ibfs)), "--verify-devices", "0,0"), expect=expect)
    assert got.stdout == want.stdout
    return want.stdout


def test_swapped_targets(hip, built, tmp_path):  # noqa: F811
    inp, index = built("genomes", 8, 0, 0.05)
    names, _ = inp.sets(0)
    out = same_report(index, swapped_tsv(inp, str(tmp_path / "swapped.tsv"), names[0], names[-1]), ibfs_of(hip, index), 1)
    assert out.count("  first false negative: ") == 2 and "\nresult\tFAIL\t" in out and ", 2 failing" in out


def test_zeroed_root_row(hip, built, tmp_path):  # noqa: F811
    from ganon_amd import ibf_file
    inp, index = built("genomes", 8, 0, 0.05)
    names, sets = inp.sets(0)
    m = ibf_file.read_hibf_meta(index)
    bins, rows0, h, at = m.ibfs[0]
    Wd = (bins + 63) >> 6
    row = int(rows_of(sets[0][:1], 0, rows0)[0])
    data = bytearray(open(index, "rb").read())
    assert any(data[at + row * Wd * 8:at + (row + 1) * Wd * 8])
    data[at + row * Wd * 8:at + (row + 1) * Wd * 8] = bytes(Wd * 8)
    bad = str(tmp_path / "zeroed.hibf")
    open(bad, "wb").write(bytes(data))
    out = same_report(bad, inp.tsv, ibfs_of(hip, index), 1)
    assert f"{names[0]}\t" in out and "  first false negative: hash " + str(int(sets[0][0])) + " (index 0 " in out and ", ibf 0, " in out


def test_patched_fpr(hip, built, tmp_path):  # noqa: F811
    from ganon_amd import ibf_file
    inp, index = built("genomes", 8, 0, 0.05)
    m = ibf_file.read_hibf_meta(index)
    at = 30 + 8 + sum(8 + sum(8 + len(s.encode()) for s in lst) for lst in m.bin_path)
    data = bytearray(open(index, "rb").read())
    assert struct.unpack_from("<d", data, at)[0] == 0.05
    struct.pack_into("<d", data, at, 0.0001)
    bad = str(tmp_path / "fpr.hibf")
    open(bad, "wb").write(bytes(data))
    out = same_report(bad, inp.tsv, ibfs_of(hip, index), 0)
    assert "\tWARN fp\n" in out and "fpr=0.0001" in out


def test_unknown_target(hip, built, tmp_path):  # noqa: F811
    inp, index = built("genomes", 8, 0, 0.05)
    first = open(inp.tsv).readline().split("\t")[0]
    tsv = str(tmp_path / "more.tsv")
    open(tsv, "w").write(open(inp.tsv).read() + f"{first}\tnot in the index\n")
    out = same_report(index, tsv, ibfs_of(hip, index), 1)
    assert "not in the index\t-\t-\t" in out and "FAIL: no such user bin" in out


def test_one_part_is_the_one_device_check(hip, request, tmp_path_factory):  # noqa: F811
    inp, one, ibfs, _ = one_pass(hip, request, tmp_path_factory, "short200")
    outs = []
    for extra in ([], ["--verify-memory", str(sum(r * b for r, b in ibfs)), "--verify-devices", "0"]):
        p = run_verify(one, inp.tsv, extra=extra)
        assert "part " not in p.stderr and "hash bytes" not in p.stderr
        outs.append((p.stdout, re.sub(r"[0-9][0-9.e+:-]*", "#", p.stderr)))
    assert outs[0] == outs[1], "stdout and stderr as without the switches"


def test_a_budget_below_one_row_is_refused(hip, request, tmp_path_factory):  # noqa: F811
    inp, one, ibfs, _ = one_pass(hip, request, tmp_path_factory, "short200")
    widest = max(b for _, b in ibfs)
    p = run_verify(one, inp.tsv, extra=("--verify-memory", str(widest - 1)), expect=1)
    first = next(i for i, (_, b) in enumerate(ibfs) if b == widest)
    assert f"--verify-memory: IBF {first}: " in p.stderr and f"{widest} bytes" in p.stderr and "not one row fits" in p.stderr, p.stderr
    assert p.stdout == ""


def test_an_index_built_in_parts_verifies_in_parts(hip, request, tmp_path_factory):  # noqa: F811
    inp, one, ibfs, _ = one_pass(hip, request, tmp_path_factory, "short200")
    tmax, s, max_fp = INPUTS["short200"]
    budget = budget_of(ibfs, "three")
    out = beside(one, "verify_parts.hibf")
    build(inp, out, tmax, s, max_fp, extra=("--hibf-memory", str(budget), "--hibf-devices", "0,0"))
    p = run_verify(out, inp.tsv, extra=("--verbose", "--verify-memory", str(budget), "--verify-devices", "0,0"))
    assert p.stdout.splitlines()[-1].startswith("result\tok\t") and len(check_parts_lines(p.stderr, ibfs, budget, 2)) > 3
    os.remove(out)
