"""The fast count kernel's flow over one flat IBF, restated over oracle.Ibf rows for tests/test_stray_probe_cpu.py and
tests/test_gpu_stray_probe.py: per unit (a read and a column slice of 64 or 128 words) which flow runs, which stages of the finish's
probe run for each bin the survey leaves (ganon_amd/csrc/gn_stray_probe.h), how many words they load, and what is reported -- and from
that the bytes a launch does not request (`algo_bytes - fetched_bytes` of the stream's timings), to the byte.

  screen_table   gn_screen_table.h in Python (the same recurrences in the same order; the CPU test holds it against the header)
  unit           one unit: the screened flow with a probe of F kept hashes (F = 0: the one-stage probe the switch `stray_masks`
                 restores), or the unscreened flow with its exact exit and narrow mode where the table gives no screen or the survey
                 leaves more than four bins
  batch          all units of a batch of reads -> (bytes not requested, per-read reports, tallies by stage)
"""
import functools

import numpy as np

import oracle

NMAX = 127
NARROW_MAX = 4
PROBE_HASHES = 4
H = 4


@functools.lru_cache(maxsize=None)
def _tails(p):
    t = [[0.0] * (NMAX + 2) for _ in range(NMAX + 1)]
    prev = None
    for d in range(NMAX + 1):
        cur = [0.0] * (NMAX + 2)
        if d == 0:
            cur[0] = 1.0
        else:
            for k in range(d + 1):
                cur[k] = (1.0 - p) * (prev[k] if k < d else 0.0) + p * (prev[k - 1] if k else 0.0)
        for k in range(d, -1, -1):
            t[d][k] = t[d][k + 1] + cur[k]
        prev = cur
    return t


@functools.lru_cache(maxsize=None)
def screen_table(rel_cutoff, hash_funs, unit_bins):
    """ds[n] for n = 0 .. 127"""
    ds = [0] * (NMAX + 1)
    if hash_funs != 4 or unit_bins == 0:
        return ds
    two, every = _tails(0.25), _tails(0.0625)
    row_lines = unit_bins / 1024.0 if unit_bins > 1024 else 1.0
    for n in range(1, NMAX + 1):
        T = oracle.threshold_cutoff(n, rel_cutoff)
        if T < 2 or T > n:
            continue
        its = n
        c = 2 * (n - T + 1)
        if c + 2 <= n:
            d = c - 1
            while d <= c + 2 and d + 1 < n:
                if d + T > n and float(unit_bins) * every[d][T - (n - d)] <= 0.5:
                    its = d + 1
                    break
                d += 1
        for d in range(n - T + 1, n + 1):
            surv = float(unit_bins) * two[d][T - (n - d)]
            if surv > 0.5:
                continue
            if 2.0 * d * row_lines + surv * 2.0 * d < float(its) * hash_funs * row_lines:
                ds[n] = d
            break
    return ds


def _unscreened(all4, n, T, wcol):
    """the flow without a screen (one hash an iteration): check points around the half-way bound, dead or narrow there -> bytes not requested"""
    chk1 = chk2 = None
    if T >= 2:
        c = max(2 * (n - T + 1), 1)
        if c + 2 <= n:
            chk1, chk2 = (c - 1 if c > 1 else c), c + 2
    cs = np.cumsum(all4, axis=0, dtype=np.int64)

    def surv(done, tval):
        return int((cs[done - 1] >= tval).sum())

    dead = narrow = drained = False
    fetched, nbins, it = n, 0, 0
    while it + 2 < n:
        if narrow:
            break
        done = it + 1
        if chk1 is not None and chk1 <= done <= chk2:
            left = surv(done, T - (n - done))
            if left == 0:
                dead, fetched = True, done + 1
                break
            if left <= NARROW_MAX and (done > chk1 or (done > 2 and surv(done, done - 1) == left)):
                narrow, drained, fetched, nbins = True, True, it + 2, left
                break
        done = it + 2
        if chk1 is not None and chk1 <= done <= chk2:
            left = surv(done, T - (n - done))
            if left == 0:
                dead, fetched = True, done + 1
                break
            if left <= NARROW_MAX:
                narrow, nbins = True, left
        it += 2
    if narrow and not drained and not dead:
        fetched = it + 1
    if not (dead or narrow):
        return 0
    got = min(fetched, n)
    return (n - got) * H * wcol * 8 - nbins * (n - got) * H * 128


def new_tally():
    return dict(unscreened=0, dead=0, aborted=0, finish=0, clean=0, drop1=0, drop2=0, full=0, stage1_words=0, stage2_words=0, trace=[])


def unit_pre(bits):
    """what every cutoff and every F of a unit share: all four rows per hash, the exact counts, rows 0 AND 1 per hash"""
    all4 = bits.all(axis=1)
    return all4, all4.sum(axis=0), bits[:, 0] & bits[:, 1]


def unit(bits, n, T, ds, wcol, F, tally, at=None, pre=None):
    """bits: bool [n, 4, wcol * 64], the unit's bits of the read's rows -> (bytes not requested, {bin of the slice: count});
    tally["trace"] gets (at, bin of the slice, 'clean' | 'drop1' | 'drop2' | 'full', m, e) for every bin a finish looks at"""
    all4, c4, r01_all = pre if pre is not None else unit_pre(bits)
    reports = {int(b): int(c4[b]) for b in np.nonzero(c4 >= T)[0]}
    if ds == 0:
        tally["unscreened"] += 1
        return _unscreened(all4, n, T, wcol), reports
    r01 = r01_all[:ds]
    c2 = r01.sum(axis=0)
    left = np.nonzero(c2 >= T - (n - ds))[0]
    if len(left) == 0:
        tally["dead"] += 1
        assert not reports, "a bin the survey drops cannot reach T"
        return (n * H - 2 * ds) * wcol * 8, {}
    if len(left) > NARROW_MAX:
        tally["aborted"] += 1
        return _unscreened(all4, n, T, wcol) - 2 * ds * wcol * 8, reports
    tally["finish"] += 1
    loads, out = 0, {}
    for b in (int(x) for x in left):
        r23 = bits[:ds, 2, b] & bits[:ds, 3, b]
        hit = r01[:, b]
        if int(c2[b]) == ds:  # an error-free read's bin: rows 0 and 1 of the screened hashes need no second look
            stage, m, e = "clean", 0, 0
            loads += n * H - 2 * ds
        else:
            fp = min(F, ds)
            m = int(hit[:fp].sum())
            e = int((hit[:fp] & r23[:fp]).sum())
            loads += 2 * m
            tally["stage1_words"] += 2 * m
            if e + (int(c2[b]) - m) + (n - ds) < T:
                stage = "drop1"
            else:
                loads += 2 * (ds - fp)
                tally["stage2_words"] += 2 * (ds - fp)
                if e + int(r23[fp:].sum()) + (n - ds) < T:
                    stage = "drop2"
                else:
                    stage = "full"
                    loads += n * H
        tally[stage] += 1
        tally["trace"].append((at, b, stage, m, e))
        if stage in ("clean", "full") and int(c4[b]) >= T:
            out[b] = int(c4[b])
    assert out == reports, "the finish is exact"
    return (n * H - 2 * ds) * wcol * 8 - loads * 128, out


def batch(ibf, hashes_per_read, cutoffs, lane_words, Fs=(PROBE_HASHES, 0), screen=True):
    """hashes_per_read: the minimiser hashes of each read (those with none, or more than 127, request nothing the fast kernel
    tallies); lane_words: 1 (8-byte lanes, slices of 64 words) or 2 (16-byte lanes, 128 words).  For every cutoff and every F
    -> skipped[(cutoff, F)] bytes not requested, tally[(cutoff, F)], reports[cutoff] = [[(bin, count)] a read]"""
    assert ibf.hash_funs == H
    W = ibf.bin_words
    sw = 64 * lane_words
    tables = {c: (screen_table(c, H, min(W, sw) * 64) if screen else [0] * (NMAX + 1)) for c in cutoffs}
    skipped = {(c, F): 0 for c in cutoffs for F in Fs}
    tally = {(c, F): new_tally() for c in cutoffs for F in Fs}
    reports = {c: [] for c in cutoffs}
    for r, hs in enumerate(hashes_per_read):
        n = len(hs)
        if n == 0 or n > NMAX:
            for c in cutoffs:
                reports[c].append(None)
            continue
        rows = ibf.data[[[ibf.row(int(v), i) for i in range(H)] for v in hs]]  # [n, 4, W]
        got = {c: [] for c in cutoffs}
        for w0 in range(0, W, sw):
            wcol = min(sw, W - w0)
            bits = np.unpackbits(np.ascontiguousarray(rows[:, :, w0:w0 + wcol]).view(np.uint8), axis=2, bitorder="little").astype(bool)
            pre = unit_pre(bits)
            for c in cutoffs:
                T = oracle.threshold_cutoff(n, c)
                ds = tables[c][n] if T >= 2 else 0
                if ds > n or ds + T <= n:
                    ds = 0
                for F in Fs:
                    s, rep = unit(bits, n, T, ds, wcol, F, tally[(c, F)], at=(r, w0), pre=pre)
                    skipped[(c, F)] += s
                got[c] += [(w0 * 64 + b, cnt) for b, cnt in sorted(rep.items())]
        for c in cutoffs:
            reports[c].append(got[c])
    return skipped, tally, reports


def unit_params(n, cutoff, unit_bins):
    """(T, ds) of a read of n minimisers in a launch whose units hold unit_bins bins"""
    T = oracle.threshold_cutoff(n, cutoff)
    ds = screen_table(cutoff, H, unit_bins)[n] if T >= 2 and n <= NMAX else 0
    return T, (0 if ds > n or ds + T <= n else ds)
