"""The fast count kernel's two-row screen (gn_kernels.hip, "Screened flow"; switch `row_screen`) must not change a single match:
with the screen and with it ablated the offsets and the match records are identical, every third read also agrees with the oracle,
and bins built to pass the screen and miss (or just reach) the cutoff on the other rows are judged by their exact counts.  The byte
counter shows that the screen runs where the launch's table gives one, and only there.

What the byte counter is asked, and what not.  At cutoffs 0.75 and 0.9 a screened shape requests fewer bytes with the screen than
without, over all its batches.  Equality of the two is asserted where no read of the batch has a table entry: every batch of a shape
whose instance does not screen (`_screens`), and the 150 bp batch at cutoff 0.55, where the table gives nothing below n = 31.  The
mixed batch (its 600 bp reads, n ~ 70) and the paired batch (n ~ 35) do have entries at 0.55, so neither direction is asserted for
them there.  (8192, 2003, 4) has rows of 128 words in 16-byte lanes: that is the three-wave instance, which keeps the unscreened flow
(its screen would cost 48 bytes of scratch a lane), so this shape checks that the switch changes nothing there.  The same holds for
h = 5 and h = 3.  That the read with five adversaries really is aborted shows in the bytes of a launch of that read alone: the
unscreened flow's bytes and the screen's rows on top."""
import numpy as np
import pytest

import ganon_fixtures as gf
import gpu_util as gu
import oracle

pytestmark = pytest.mark.gpu

K, W = 19, 31
CUTOFFS = (0.55, 0.75, 0.9, 1.0)
N_GENOMES = 24


@pytest.fixture(scope="module")
def hip():
    import ganon_amd
    ganon_amd.load_library()
    assert ganon_amd.device_count() >= 1, "no HIP device: the product path has no CPU fallback"
    return ganon_amd


def _screens(bins, h):
    """does the instance this shape runs screen at all?  four hash functions; 8-byte lanes (odd words a row, or 64), or 16-byte
    lanes with rows of more than 128 words -- the three-wave build of 16-byte lanes keeps the unscreened flow"""
    words = (bins + 63) // 64
    return h == 4 and (words % 2 == 1 or words == 64 or words > 128)


def _mutated(rng, g, length, subs):
    p = int(rng.integers(0, len(g) - length))
    s = bytearray(g[p:p + length])
    for _ in range(subs):
        q = int(rng.integers(0, length))
        s[q] = b"ACGT"[(b"ACGT".index(s[q]) + 1 + int(rng.integers(0, 3))) % 4]
    return bytes(s)


def _set_bit(ibf, row, b, on):
    m = np.uint64(1) << np.uint64(b & 63)
    if on:
        ibf.data[row, b >> 6] |= m
    else:
        ibf.data[row, b >> 6] &= ~m


def _plant_adversary(ibf, hashes, b, full):
    """bin b gets its bit in rows 0 and 1 of every hash, and in all rows of exactly `full` of them (cleared in row 2 of the others);
    False when two of the read's rows coincide and spoil the count (the oracle decides)"""
    h = ibf.hash_funs
    for q, v in enumerate(hashes):
        for i in range(h):
            _set_bit(ibf, ibf.row(int(v), i), b, i < 2 or q < full)
    c = int(ibf.bulk_count(hashes)[b])
    c2 = sum(all((int(ibf.data[ibf.row(int(v), i), b >> 6]) >> (b & 63)) & 1 for i in range(2)) for v in hashes)
    return c == full and c2 == len(hashes)


def _workload(bins, rows, h, fill):
    rng = np.random.default_rng(bins * 7 + h * 3 + int(fill * 10))
    ibf = gf.random_ibf(bins, rows, h, fill, seed=bins + h)
    genomes = [gu.random_seq(rng, 1600) for _ in range(N_GENOMES)]
    gbins = [(gi * 611 + 5) % bins for gi in range(N_GENOMES)]
    for g, b in zip(genomes, gbins):
        ibf.emplace_many(np.unique(oracle.minimiser_hash(oracle.to_ranks(g), K, W)), b)
    reads = [_mutated(rng, genomes[i % N_GENOMES], 150, i % 8) if i % 5 else gu.random_seq(rng, 150) for i in range(420)]  # n ~ 17
    mixed = []
    for length, count in ((60, 60), (600, 60), (1100, 45)):  # n = 3..9, ~80, around the kernel's 127 (900 bp below it, 1100 bp above)
        for i in range(count):
            ln = length - 200 * (i & 1) if length == 1100 else length
            mixed.append(_mutated(rng, genomes[i % N_GENOMES], ln, i % 8) if i % 5 else gu.random_seq(rng, ln))
    pairs = ([], [])
    for i in range(150):
        g = genomes[i % N_GENOMES]
        for m in (0, 1):
            pairs[m].append(_mutated(rng, g, 150, i % 8) if i % 5 else gu.random_seq(rng, 150))
    # adversaries (h >= 4, cutoff 0.75): bins that hold no genome, inside the first column slice, which pass rows 0 and 1 of every
    # hash of a read; one misses the cutoff count by one on the other rows, the next reaches it exactly.  The last read gets five such
    # bins -- more than the finish follows, so its screen is aborted at any fill.
    expect = []  # (read, bin, count or None)
    if h >= 4:
        free = [b for b in range(7, min(bins, 4096), 97) if b not in gbins]
        plain = [i for i in range(420) if i % 5 == 0]  # random reads: no bin of their own
        for r in plain:
            hs = oracle.minimiser_hash(oracle.to_ranks(reads[r]), K, W)
            n = len(hs)
            T = oracle.threshold_cutoff(n, 0.75)
            if len(np.unique(hs)) != n or T < 3 or len(expect) >= 13:
                continue
            five = len(expect) >= 8
            want = [T - 1, T, T + 1, T - 1, T] if five else [T - 1, T]
            mine = [free.pop() for _ in want]
            if all(_plant_adversary(ibf, hs, b, c) for b, c in zip(mine, want)):
                expect += [(r, b, c if c >= T else None) for b, c in zip(mine, want)]
        assert len(expect) == 13, "four reads with two adversaries and one with five"
    return ibf, reads, mixed, pairs, expect


def _run(hip, flt, s1, s2, cutoff):
    bases, off1, off2 = gu.pack_reads(s1, s2)
    st = hip.HipStream(flt, len(s1), bases.size)
    st.submit(bases, off1, off2, K, W, cutoff)
    nh, status, mo, m = st.fetch()
    tm = st.timings()
    return st, nh, mo, m, tm


@pytest.mark.parametrize("bins,rows,h,fill", [(4096, 5003, 4, 0.5), (4096, 5003, 4, 0.2), (4096, 5003, 4, 0.8), (4160, 3001, 4, 0.5),
                                              (8192, 2003, 4, 0.5), (32768, 1201, 4, 0.5), (4096, 3001, 5, 0.5), (4096, 3001, 3, 0.5)])
def test_row_screen_is_exact(hip, bins, rows, h, fill):
    ibf, reads, mixed, pairs, expect = _workload(bins, rows, h, fill)
    flt = hip.HipFilter.ibf(ibf.data, bins, rows, h)
    b2t = np.arange(bins, dtype=np.uint32)
    for cutoff in CUTOFFS:
        total = total0 = 0  # bytes requested for all the shape's reads, with the screen and without
        for s1, s2 in ((reads, None), (mixed, None), pairs):
            gu.SW.on("row_screen")
            st0, nh0, mo0, m0, tm0 = _run(hip, flt, s1, s2, cutoff)
            gu.SW.off("row_screen")
            st, nh, mo, m, tm = _run(hip, flt, s1, s2, cutoff)
            ho, hs = st.fetch_hashes()
            gu.SW.on("early_exit")
            st2, _, mo2, m2, tm2 = _run(hip, flt, s1, s2, cutoff)
            gu.SW.off("early_exit")
            print(f"bins {bins} h {h} fill {fill} {'paired' if s2 else 'mixed' if s1 is mixed else 'single'} cutoff {cutoff}: algo {tm['algo_bytes']} "
                  f"fetched {tm['fetched_bytes']} without the screen {tm0['fetched_bytes']}")
            total += tm["fetched_bytes"]
            total0 += tm0["fetched_bytes"]
            assert np.array_equal(mo, mo0) and np.array_equal(m, m0), cutoff
            assert np.array_equal(mo, mo2) and np.array_equal(m, m2), cutoff
            assert tm2["fetched_bytes"] == tm2["algo_bytes"] == tm["algo_bytes"] == tm0["algo_bytes"]  # every row: no screen either
            if fill == 0.5 and (not _screens(bins, h) or (cutoff == 0.55 and s1 is reads)):
                assert tm["fetched_bytes"] == tm0["fetched_bytes"]  # (no table entry -- at 0.55 none below n = 31: the old flow)
            for i in sorted(set(range(0, len(s1), 3)) | ({r for r, _, _ in expect} if s1 is reads else set())):
                exp_m, _ = gu.oracle_matches(ibf, b2t, bins, hs[int(ho[i]):int(ho[i + 1])], cutoff)
                got = [(int(x["target"]), int(x["count"])) for x in m[int(mo[i]):int(mo[i + 1])]]
                assert got == exp_m, (cutoff, i, got[:3], exp_m[:3])
            if s1 is reads and cutoff == 0.75:
                for r, b, c in expect:
                    got = {int(x["target"]): int(x["count"]) for x in m[int(mo[r]):int(mo[r + 1])]}
                    assert got.get(b) == c, (r, b, c, got)
                if bins == 4096 and h == 4:  # one column slice of 64 words: the read with five adversaries alone in a launch
                    r5 = expect[-1][0]
                    n5 = int(nh[r5])
                    gu.SW.on("row_screen")
                    sa, _, _, _, tma = _run(hip, flt, [reads[r5]], None, cutoff)
                    gu.SW.off("row_screen")
                    sb, _, _, _, tmb = _run(hip, flt, [reads[r5]], None, cutoff)
                    extra = tmb["fetched_bytes"] - tma["fetched_bytes"]
                    print(f"  aborted read: n {n5}, {extra} bytes on top of the unscreened flow's {tma['fetched_bytes']}")
                    # five bins pass the survey, the finish follows four: the screen is aborted and the read runs the unscreened flow
                    # from hash 0, so it requested exactly that flow's bytes and its screen's 2 ds rows of 512 bytes on top
                    assert extra > 0 and extra % (2 * 512) == 0 and extra // (2 * 512) <= n5, (extra, n5)
                    sa.destroy()
                    sb.destroy()
            if s1 is mixed:  # the shortest reads; the longest on both sides of what the fast kernel takes
                assert 1 <= nh[:60].min() and nh[:60].max() <= 9 and nh[120:].min() <= 127 < nh[120:].max()
            for s in (st0, st, st2):
                s.destroy()
        if fill == 0.5 and _screens(bins, h) and cutoff in (0.75, 0.9):
            assert total < total0, "the screen saves rows"
    flt.free()
