"""The merging gather (gn_gather_create_merged): per read the union of the parts' records in ascending translated id -- what puts the
subtree parts of an HIBF back together, whose user-bin ids interleave.  Checked against numpy over raw device buffers
(gn_gather_run_buffers, offsets of any origin) and over streams; the concatenating gather on the same inputs still gives part order."""
import ctypes as C

import numpy as np
import pytest

import gpu_util as gu
from ganon_amd.hip import MATCH_DTYPE as MATCH
from test_gpu_gather import K, W, _case, _parts

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    import ganon_amd
    ganon_amd.load_library()
    assert ganon_amd.device_count() >= 1, "no HIP device: the product path has no CPU fallback"
    return ganon_amd


def synthetic(k, seed, n_reads=300, universe=5000, empty_part=None, null_map_part=None):
    """-> (maps, per part (offsets, records)): every map strictly increasing, translated ids of the parts disjoint, every part's
    segment of a read ascending in local id.  Read 0: no match; 1: one part only; 2: six records; 3: more than 64 records in one
    part; 4: more than 200 in total; the others at random (most of them light, many empty)."""
    rng = np.random.default_rng(seed)
    owner = rng.integers(0, k, size=universe)
    if null_map_part is not None:  # a part without a map reports the caller's ids itself: it owns the lowest ids, local id = global id
        owner[owner == null_map_part] = (null_map_part + 1) % k
        owner[:universe // k] = null_map_part
    ids = [np.nonzero(owner == p)[0].astype(np.uint32) for p in range(k)]
    maps = [None if p == null_map_part else ids[p] for p in range(k)]
    parts = []
    live = [p for p in range(k) if p != empty_part]
    for p in range(k):
        counts = np.zeros(n_reads, dtype=np.int64)
        if p != empty_part:
            counts = np.where(rng.random(n_reads) < 0.5, rng.integers(0, 4, size=n_reads), 0)
            counts[0] = 0
            counts[1] = 3 if p == live[0] else 0
            counts[2] = 2 if p == live[0] else 4 if p == live[-1] else 0
            counts[3] = 90 if p == live[-1] else counts[3]
            counts[4] = 210 // len(live) + 5
        counts = np.minimum(counts, len(ids[p]))
        off = np.zeros(n_reads + 1, dtype=np.uint64)
        off[1:] = np.cumsum(counts)
        rec = np.zeros(int(off[-1]), dtype=MATCH)
        for r in range(n_reads):
            c = int(counts[r])
            if c:
                loc = np.sort(rng.choice(len(ids[p]), size=c, replace=False)).astype(np.uint32)
                seg = rec[int(off[r]):int(off[r + 1])]
                seg["read"] = r
                seg["target"] = ids[p][loc] if maps[p] is None else loc
                seg["count"] = rng.integers(1, 1 << 16, size=c)
        parts.append((off, rec))
    return maps, parts


def expected(maps, parts, lo, hi, merged):
    out, moff = [], [0]
    for r in range(lo, hi):
        segs = []
        for p, (off, rec) in enumerate(parts):
            seg = rec[int(off[r]):int(off[r + 1])].copy()
            if maps[p] is not None:
                seg["target"] = maps[p][seg["target"]]
            segs.append(seg)
        cat = np.concatenate(segs)
        if merged:
            cat = cat[np.argsort(cat["target"], kind="stable")]  # (stable: equal ids, lower part first)
        out.append(cat)
        moff.append(moff[-1] + len(cat))
    return np.array(moff, dtype=np.uint64), np.concatenate(out) if out else np.zeros(0, dtype=MATCH)


def run_buffers(hip, g, parts, lo, hi, origin):
    import torch
    offs, recs = [], []
    for off, rec in parts:
        # a slice of a longer offset array whose origin is not 0; the records of the slice's reads only
        o = off[lo:hi + 1].astype(np.int64) + origin
        offs.append(torch.from_numpy(o).cuda())
        chunk = np.ascontiguousarray(rec[int(off[lo]):int(off[hi])]).view(np.uint32).reshape(-1, 3).view(np.int32)
        recs.append(torch.from_numpy(chunk.copy()).cuda())
    torch.cuda.synchronize()
    g.run_buffers([t.data_ptr() for t in offs], [t.data_ptr() if t.numel() else 0 for t in recs], [t.shape[0] for t in recs], hi - lo)
    return g.fetch()


@pytest.mark.parametrize("k,empty_part,null_map_part", [(2, None, None), (3, None, 1), (8, None, None), (3, 0, None), (8, 7, 2)])
def test_merged_gather_of_raw_device_buffers_equals_numpy(hip, k, empty_part, null_map_part):
    maps, parts = synthetic(k, seed=10 * k + (empty_part or 0), empty_part=empty_part, null_map_part=null_map_part)
    n = len(parts[0][0]) - 1
    tot = sum(np.diff(off.astype(np.int64)) for off, _ in parts)
    assert tot[0] == 0 and 0 < tot[2] <= 6 and tot[4] > 200 and max(int(off[4]) - int(off[3]) for off, _ in parts) > 64
    assert sum(int(off[2]) != int(off[1]) for off, _ in parts) == 1  # read 1: matches in one part only
    if empty_part is not None:
        assert len(parts[empty_part][1]) == 0
    gm = hip.HipGather(0, maps, merged=True)
    gc = hip.HipGather(0, maps)
    for lo, hi, origin in ((0, n, 0), (0, n, 12345), (n // 3, 2 * n // 3, 0), (3, 5, 0), (7, 7, 0)):
        mo, m = run_buffers(hip, gm, parts, lo, hi, origin)
        emo, em = expected(maps, parts, lo, hi, True)
        assert np.array_equal(mo, emo) and np.array_equal(m, em), (lo, hi, origin)
        # the concatenating gather on the same inputs: part order, as before
        mo, m = run_buffers(hip, gc, parts, lo, hi, origin)
        cmo, cm = expected(maps, parts, lo, hi, False)
        assert np.array_equal(mo, cmo) and np.array_equal(m, cm), (lo, hi, origin)
        if hi - lo > 10:
            assert not np.array_equal(cm, em)  # (the ids interleave: the two orders differ)
    gm.destroy()
    gc.destroy()


def test_equal_ids_go_lower_part_first(hip):
    ids = np.arange(0, 300, dtype=np.uint32)
    maps = [ids, ids, None]
    parts = []
    for p, per_read in enumerate(([3, 100, 0], [3, 100, 2], [0, 100, 2])):
        off = np.zeros(4, dtype=np.uint64)
        off[1:] = np.cumsum(per_read)
        rec = np.zeros(int(off[-1]), dtype=MATCH)
        for r, c in enumerate(per_read):
            seg = rec[int(off[r]):int(off[r + 1])]
            seg["read"], seg["target"], seg["count"] = r, np.arange(c) * 2, 1000 * p + np.arange(c)
        parts.append((off, rec))
    g = hip.HipGather(0, maps, merged=True)
    mo, m = run_buffers(hip, g, parts, 0, 3, 0)
    emo, em = expected(maps, parts, 0, 3, True)
    assert np.array_equal(mo, emo) and np.array_equal(m, em)
    g.destroy()


@pytest.mark.parametrize("copy_path", [False, True])
def test_merged_gather_over_streams(hip, copy_path):
    # column parts of a flat IBF whose part-local target ids are mapped to ids that interleave between the parts: the merged result is
    # the whole filter's with the same relabelling, every read's matches sorted by the new id
    ibf, b2t, n_targets, seqs = _case(seed=3)
    bases, off1, _ = gu.pack_reads(seqs, None)
    full = hip.HipFilter.ibf(ibf.data, ibf.bins, ibf.bin_size, ibf.hash_funs, b2t, n_targets)
    st = hip.HipStream(full, len(seqs), bases.size)
    st.submit(bases, off1, None, K, W, 0.1)
    _, _, mo, m_full = st.fetch()
    if copy_path:
        gu.SW.on("gather_copy")
    for world in (2, 3):
        parts = _parts(hip, ibf, b2t, world)
        relabel = np.zeros(n_targets, dtype=np.uint32)
        maps = []
        for p, (_, sl) in enumerate(parts):
            maps.append((np.arange(len(sl.targets_global)) * world + p).astype(np.uint32))
            relabel[sl.targets_global] = maps[-1]
        exp = m_full.copy()
        exp["target"] = relabel[exp["target"]]
        for r in range(len(seqs)):
            seg = exp[int(mo[r]):int(mo[r + 1])]
            seg[:] = seg[np.argsort(seg["target"], kind="stable")]
        sts = [hip.HipStream(f, len(seqs), bases.size) for f, _ in parts]
        sts[0].submit(bases, off1, None, K, W, 0.1)
        for s in sts[1:]:
            s.classify_shared(sts[0], 0.1)
        g = hip.HipGather(0, maps, merged=True)
        g.run(sts)
        mo2, m2 = g.fetch()
        assert np.array_equal(mo2, mo) and np.array_equal(m2, exp) and not np.array_equal(exp["target"], relabel[m_full["target"]])
        assert (g.peer_bytes() > 0) == copy_path
        g.destroy()
        for s in sts:
            s.destroy()
        for f, _ in parts:
            f.free()
    st.destroy()
    full.free()


def test_merged_gather_refuses_what_it_cannot_do(hip):
    L = hip.load_library()
    h = C.c_void_p()
    assert L.gn_gather_create_merged(0, 65, None, None, C.byref(h)) != 0 and not h.value  # more than 64 parts
    assert L.gn_gather_create_merged(0, 0, None, None, C.byref(h)) != 0
    assert L.gn_gather_create_merged(0, 2, None, None, None) != 0  # null argument
    with pytest.raises(hip.GanonHipError):
        hip.HipGather(0, [None] * 65, merged=True)
    g = hip.HipGather(0, [None, None], merged=True)
    with pytest.raises(hip.GanonHipError):  # nothing gathered yet
        g.fetch()
    assert L.gn_gather_run_buffers(g._h, None, None, None, 2, 1) != 0  # null arguments
    assert L.gn_gather_run(g._h, None, 2) != 0
    g.destroy()
