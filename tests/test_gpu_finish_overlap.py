"""The fast count kernel between two units (gn_kernels.hip: the finish of one read, its epilogue, the next read's metadata, hashes,
row table and first rows).  What a unit reports and what it adds to the byte tally must not depend on the unit before or after it.

One batch runs every kind of unit next to every kind, in every order (a de Bruijn sequence over the kinds, twice, with other
reads the second time):
  exact   an error-free 150 bp cut of a genome: screened, its bin has c2 = ds, a finish without the probe
  subst   the same with substitutions: a finish that probes first
  random  dead at the screen's survey
  short   shorter than a window: no minimiser, the skip path
  long    1100 bp, more than 127 minimisers: deferred to the generic kernel, the skip path
  600bp   n = 70 .. 80: a finish of three passes of 32 hashes
  n15, n16, n17, n32, n33   cuts whose length gives exactly that many minimisers: the boundaries of the finish's passes (16 hashes a
          ballot, 32 a pass)
and a read with five adversary bins (they pass rows 0 and 1 of every hash: more survivors than the finish follows, so its screen
is aborted and the read runs the unscreened flow) first, in the middle and last.
At every cutoff the offsets and the records equal those of the run with `row_screen` ablated and of the run with `early_exit`
ablated, and every third read equals the oracle.  The batch reversed and under a seeded permutation requests the same bytes and
reports the same matches read by read.  Batches of one and of two reads have no next unit, and a next unit that is the last.  A
batch large enough for the launch to hand its units out on demand is compared with the two ablated runs and with itself reversed."""
import numpy as np
import pytest

import ganon_fixtures as gf
import gpu_util as gu
import oracle

pytestmark = pytest.mark.gpu

K, W = 19, 31
CUTOFFS = (0.55, 0.75, 0.9, 1.0)
N_GENOMES = 24
GENOME_LEN = 2400
KINDS = ("exact", "subst", "random", "short", "long", "600bp", "n15", "n16", "n17", "n32", "n33")
SHAPES = [(4096, 5003), (32768, 1201)]  # 8-byte lanes, one column slice; 16-byte lanes, rows of 512 words (the wide instance), four slices
H, FILL = 4, 0.5


@pytest.fixture(scope="module")
def hip():
    import ganon_amd
    ganon_amd.load_library()
    assert ganon_amd.device_count() >= 1, "no HIP device: the product path has no CPU fallback"
    return ganon_amd


def _n_of(seq):
    return len(oracle.minimiser_hash(oracle.to_ranks(seq), K, W))


def _cut_with(rng, g, n_want):
    """a cut of g with exactly n_want minimisers: a longer cut has as many or one more, so the length is found by bisection"""
    for _ in range(20):
        p = int(rng.integers(0, len(g) - 700))
        lo, hi = W, 700  # n(lo) = 1 <= n_want <= n(hi)
        if _n_of(g[p:p + hi]) < n_want:
            continue
        while lo < hi:
            mid = (lo + hi) // 2
            if _n_of(g[p:p + mid]) < n_want:
                lo = mid + 1
            else:
                hi = mid
        if _n_of(g[p:p + lo]) == n_want:
            return g[p:p + lo]
    raise AssertionError(f"no cut with {n_want} minimisers")


def _de_bruijn_pairs(k):
    """a cyclic sequence over range(k) in which every ordered pair, (a, a) included, is adjacent once; the first symbol is appended"""
    seq, a = [], [0] * (2 * k)

    def db(t, p):
        if t > 2:
            if 2 % p == 0:
                seq.extend(a[1:p + 1])
        else:
            a[t] = a[t - p]
            db(t + 1, p)
            for j in range(a[t - p] + 1, k):
                a[t] = j
                db(t + 1, t)

    db(1, 1)
    assert len(seq) == k * k
    return seq + seq[:1]


def _set_bit(ibf, row, b, on):
    m = np.uint64(1) << np.uint64(b & 63)
    if on:
        ibf.data[row, b >> 6] |= m
    else:
        ibf.data[row, b >> 6] &= ~m


def _plant_adversary(ibf, hashes, b, full):
    """bin b gets its bit in rows 0 and 1 of every hash and in all rows of exactly `full` of them; False when two of the read's rows
    coincide and spoil the count"""
    for q, v in enumerate(hashes):
        for i in range(ibf.hash_funs):
            _set_bit(ibf, ibf.row(int(v), i), b, i < 2 or q < full)
    c = int(ibf.bulk_count(hashes)[b])
    c2 = sum(all((int(ibf.data[ibf.row(int(v), i), b >> 6]) >> (b & 63)) & 1 for i in range(2)) for v in hashes)
    return c == full and c2 == len(hashes)


class _Workload:
    def __init__(self, bins, rows):
        rng = np.random.default_rng(bins * 5 + rows)
        self.bins, self.rows = bins, rows
        self.ibf = gf.random_ibf(bins, rows, H, FILL, seed=bins + 1)
        self.genomes = [gu.random_seq(rng, GENOME_LEN) for _ in range(N_GENOMES)]
        gbins = [(gi * 611 + 5) % bins for gi in range(N_GENOMES)]
        for g, b in zip(self.genomes, gbins):
            self.ibf.emplace_many(np.unique(oracle.minimiser_hash(oracle.to_ranks(g), K, W)), b)
        # the read with five adversaries: bins without a genome, in the first column slice, counts around the cutoff 0.75
        free = [b for b in range(7, 4096, 97) if b not in gbins]
        self.adversary = None
        while self.adversary is None:
            r = gu.random_seq(rng, 150)
            hs = oracle.minimiser_hash(oracle.to_ranks(r), K, W)
            T = oracle.threshold_cutoff(len(hs), 0.75)
            if len(np.unique(hs)) != len(hs) or T < 3:
                continue
            want = [T - 1, T, T + 1, T - 1, T]
            mine = [free.pop() for _ in want]
            if all(_plant_adversary(self.ibf, hs, b, c) for b, c in zip(mine, want)):
                self.adversary, self.adv_expect = r, [(b, c if c >= T else None) for b, c in zip(mine, want)]
        self.kinds = []
        body = []
        for rnd in range(2):
            for pos, kd in enumerate(_de_bruijn_pairs(len(KINDS))):
                body.append(self._read(rng, KINDS[kd], rnd * 7 + pos))
                self.kinds.append(KINDS[kd])
        mid = len(body) // 2
        self.reads = [self.adversary] + body[:mid] + [self.adversary] + body[mid:] + [self.adversary]
        self.kinds = ["adversary"] + self.kinds[:mid] + ["adversary"] + self.kinds[mid:] + ["adversary"]
        self.b2t = np.arange(bins, dtype=np.uint32)

    def _cut(self, rng, g, length):
        p = int(rng.integers(0, len(g) - length))
        return g[p:p + length]

    def _read(self, rng, kind, i):
        g = self.genomes[i % N_GENOMES]
        if kind == "exact":
            return self._cut(rng, g, 150)
        if kind == "subst":
            s = bytearray(self._cut(rng, g, 150))
            for _ in range(1 + i % 3):
                q = int(rng.integers(0, len(s)))
                s[q] = b"ACGT"[(b"ACGT".index(s[q]) + 1 + int(rng.integers(0, 3))) % 4]
            return bytes(s)
        if kind == "random":
            return gu.random_seq(rng, 150)
        if kind == "short":
            return gu.random_seq(rng, 12 + i % (W - 12))
        if kind == "long":
            return self._cut(rng, g, 1100)
        if kind == "600bp":
            return self._cut(rng, g, 600)
        return _cut_with(rng, g, int(kind[1:]))


_cache = {}


def _workload(bins, rows):
    if (bins, rows) not in _cache:
        _cache[(bins, rows)] = _Workload(bins, rows)
    return _cache[(bins, rows)]


def _run(hip, flt, reads, cutoff, ablate=None, hashes=False):
    bases, off1, _ = gu.pack_reads(reads)
    st = hip.HipStream(flt, len(reads), bases.size)
    if ablate:
        gu.SW.on(ablate)
    st.submit(bases, off1, None, K, W, cutoff)
    nh, status, mo, m = st.fetch()
    out = dict(nh=nh.copy(), mo=mo.copy(), m=m.copy(), fetched=st.timings()["fetched_bytes"])
    if hashes:
        ho, hs = st.fetch_hashes()
        out["ho"], out["hs"] = ho.copy(), hs.copy()
    if ablate:
        gu.SW.off(ablate)
    st.destroy()
    return out


def _per_read(r):
    """(target, count) of every record, read by read (the records' read numbers change with the order)"""
    tc = np.stack([r["m"]["target"].astype(np.int64), r["m"]["count"].astype(np.int64)], axis=1)
    return [tc[int(r["mo"][i]):int(r["mo"][i + 1])].tobytes() for i in range(len(r["mo"]) - 1)]


def _check_oracle(wl, r, cutoff, which):
    for i in which:
        exp_m, _ = gu.oracle_matches(wl.ibf, wl.b2t, wl.bins, r["hs"][int(r["ho"][i]):int(r["ho"][i + 1])], cutoff)
        got = [(int(x["target"]), int(x["count"])) for x in r["m"][int(r["mo"][i]):int(r["mo"][i + 1])]]
        assert got == exp_m, (cutoff, i, wl.kinds[i], got[:3], exp_m[:3])


@pytest.mark.parametrize("bins,rows", SHAPES)
def test_every_kind_of_next_unit(hip, bins, rows):
    wl = _workload(bins, rows)
    flt = hip.HipFilter.ibf(wl.ibf.data, bins, rows, H)
    for cutoff in CUTOFFS:
        r = _run(hip, flt, wl.reads, cutoff, hashes=True)
        r0 = _run(hip, flt, wl.reads, cutoff, ablate="row_screen")
        r2 = _run(hip, flt, wl.reads, cutoff, ablate="early_exit")
        print(f"bins {bins} cutoff {cutoff}: {len(wl.reads)} reads, fetched {r['fetched']}, without the screen {r0['fetched']}, every row {r2['fetched']}")
        for other in (r0, r2):
            assert np.array_equal(r["mo"], other["mo"]) and np.array_equal(r["m"], other["m"]), cutoff
        if cutoff == CUTOFFS[0]:  # the kinds are what their names say
            for i, kd in enumerate(wl.kinds):
                n = int(r["nh"][i])
                if kd[0] == "n":
                    assert n == int(kd[1:]), (i, kd, n)
                elif kd in ("short", "long", "600bp"):
                    assert (n == 0 if kd == "short" else n > 127 if kd == "long" else 65 <= n <= 96), (i, kd, n)
        adv = [i for i, kd in enumerate(wl.kinds) if kd == "adversary"]
        assert adv[0] == 0 and adv[-1] == len(wl.reads) - 1 and len(adv) == 3
        _check_oracle(wl, r, cutoff, sorted(set(range(0, len(wl.reads), 3)) | set(adv)))
        if cutoff == 0.75:
            for i in adv:
                got = {int(x["target"]): int(x["count"]) for x in r["m"][int(r["mo"][i]):int(r["mo"][i + 1])]}
                for b, c in wl.adv_expect:  # judged by their exact counts: a bin one below the cutoff count is not reported
                    assert got.get(b) == c, (i, b, c, got)
    flt.free()


@pytest.mark.parametrize("bins,rows", SHAPES)
def test_tally_does_not_depend_on_the_order(hip, bins, rows):
    wl = _workload(bins, rows)
    flt = hip.HipFilter.ibf(wl.ibf.data, bins, rows, H)
    n = len(wl.reads)
    orders = [np.arange(n)[::-1], np.random.default_rng(17).permutation(n)]
    for cutoff in CUTOFFS:
        r = _run(hip, flt, wl.reads, cutoff)
        mine = _per_read(r)
        for order in orders:
            o = _run(hip, flt, [wl.reads[int(i)] for i in order], cutoff)
            print(f"bins {bins} cutoff {cutoff}: fetched {r['fetched']}, reordered {o['fetched']}")
            theirs = _per_read(o)
            for pos, i in enumerate(order):
                assert theirs[pos] == mine[int(i)], (cutoff, pos, int(i), wl.kinds[int(i)])
            assert o["fetched"] == r["fetched"], cutoff
    flt.free()


@pytest.mark.parametrize("bins,rows", SHAPES)
def test_one_read_and_two(hip, bins, rows):
    wl = _workload(bins, rows)
    flt = hip.HipFilter.ibf(wl.ibf.data, bins, rows, H)
    first = {kd: wl.kinds.index(kd) for kd in KINDS}
    batches = [[first["exact"]], [first["subst"]], [first["random"]], [0], [first["exact"], first["subst"]], [first["random"], first["exact"]],
               [first["short"], first["exact"]], [first["exact"], first["long"]], [0, first["n33"]]]
    for cutoff in CUTOFFS:
        for b in batches:
            reads = [wl.reads[i] for i in b]
            r = _run(hip, flt, reads, cutoff, hashes=True)
            for ab in ("row_screen", "early_exit"):
                other = _run(hip, flt, reads, cutoff, ablate=ab)
                assert np.array_equal(r["mo"], other["mo"]) and np.array_equal(r["m"], other["m"]), (cutoff, b, ab)
            for pos in range(len(b)):
                exp_m, _ = gu.oracle_matches(wl.ibf, wl.b2t, wl.bins, r["hs"][int(r["ho"][pos]):int(r["ho"][pos + 1])], cutoff)
                got = [(int(x["target"]), int(x["count"])) for x in r["m"][int(r["mo"][pos]):int(r["mo"][pos + 1])]]
                assert got == exp_m, (cutoff, b, pos)
    flt.free()


def test_units_handed_out_on_demand(hip):
    """the launch hands units out from the cursor once it has 64 units a wave of its grid: 8 blocks of 4 waves a CU, 256 CUs and
    one unit a read on the small filter make that 524 288 reads.  512 reads of 150 bp (exact, with substitutions, random, the
    adversary) repeated 1100 times: 563 200."""
    bins, rows = SHAPES[0]
    wl = _workload(bins, rows)
    flt = hip.HipFilter.ibf(wl.ibf.data, bins, rows, H)
    pool = [r for r, kd in zip(wl.reads, wl.kinds) if len(r) == 150]
    rng = np.random.default_rng(3)
    base = [pool[int(i)] for i in rng.integers(0, len(pool), size=512)]
    reps = 1100
    n = len(base) * reps
    assert n >= 64 * 8 * 4 * 256

    def run(reads512, ablate=None):
        blob = np.frombuffer(b"".join(reads512), dtype=np.uint8)
        bases = np.tile(blob, reps)
        off = np.arange(n + 1, dtype=np.uint64) * np.uint64(150)
        st = hip.HipStream(flt, n, bases.size, n * 2)
        if ablate:
            gu.SW.on(ablate)
        st.submit(bases, off, None, K, W, 0.75)
        nh, status, mo, m = st.fetch()
        out = dict(mo=mo.copy(), m=m.copy(), fetched=st.timings()["fetched_bytes"])
        if ablate:
            gu.SW.off(ablate)
        st.destroy()
        return out

    r = run(base)
    assert len(r["m"]) > n // 4
    for ab in ("row_screen", "early_exit"):
        other = run(base, ab)
        assert np.array_equal(r["mo"], other["mo"]) and np.array_equal(r["m"], other["m"]), ab
    # reversed: read i of one run is read n - 1 - i of the other; a read's records are in ascending target order in both
    o = run(base[::-1])
    print(f"{n} reads: fetched {r['fetched']}, reversed {o['fetched']}")
    assert o["fetched"] == r["fetched"]
    cnt, cnt_o = np.diff(r["mo"].astype(np.int64)), np.diff(o["mo"].astype(np.int64))
    assert np.array_equal(cnt, cnt_o[::-1])
    rd_o = (n - 1) - np.repeat(np.arange(n, dtype=np.int64), cnt_o)
    back = np.lexsort((o["m"]["target"], rd_o))
    assert np.array_equal(o["m"]["target"][back], r["m"]["target"]) and np.array_equal(o["m"]["count"][back], r["m"]["count"])
    flt.free()
