"""The screen-only fast count kernel (gn_kernels.hip, gn_ibf_count_fast_kernel_lean) and the launch over the units it leaves,
against the single launch of the screening instance that the switch `lean_screen` restores.  The two must agree in everything a
caller sees: minimiser counts, status, match offsets and match records in the same per-read order -- and in every byte they
request, launch by launch: a unit the new kernel leaves runs the unscreened flow from hash 0, which requests what the screening
instance requests for it (an aborted screen's rows on top, tallied by the kernel that ran the screen).  The byte equality is
what catches a unit deferred that should not be, or one that runs twice.  Both also equal the run with `row_screen` ablated, the
run with `early_exit` ablated, and the oracle on every third read.

Shapes: one column slice (4096 bins) at fills 0.2, 0.5 and 0.8 -- at 0.8 most screens are aborted; 4160 bins (65 words: two
slices a read, the second one word wide, so units are left to the list per slice); 6144 bins (96 words); a filter of all ones
(every unit is left, every bin reports) and one of all zeros.  Reads: those of test_gpu_row_screen.py (planted, random, 2 and 5
stray bins at T - 1, T, T + 1; lengths with n = 3 .. 9, ~80, around 127 and beyond; pairs) plus lengths with n = 0, 1, 2, ...
and around n = 31."""
import functools

import numpy as np
import pytest

import ganon_fixtures as gf
import gpu_util as gu
from test_gpu_row_screen import K, W, _workload

pytestmark = pytest.mark.gpu

CUTOFFS = (0.55, 0.75, 0.9)
SHAPES = [(4096, 5003, 0.5), (4096, 5003, 0.2), (4096, 5003, 0.8), (4160, 3001, 0.5), (6144, 3001, 0.5)]


@pytest.fixture(scope="module")
def hip():
    import ganon_amd
    ganon_amd.load_library()
    assert ganon_amd.device_count() >= 1, "no HIP device: the product path has no CPU fallback"
    return ganon_amd


def _lean(bins):
    """does the screen-only kernel run for this shape?  8-byte lanes: an odd number of words a row, or 64 (rows of 96 words take
    16-byte lanes and the three-wave instance, which does not screen: nothing may change there either)"""
    words = (bins + 63) // 64
    return words % 2 == 1 or words == 64


def _short_reads(rng):
    """lengths below the window (n = 0), at it (n = 1), just above (n = 1, 2, ...) and around n = 31"""
    lengths = [20, 30, 31, 32, 33, 36, 40, 44, 50, 57, 64, 70, 77, 85, 93, 100] + list(range(255, 300, 5))
    return [gu.random_seq(rng, ln) for ln in lengths]


@functools.lru_cache(maxsize=None)
def _shape(bins, rows, fill):
    ibf, reads, mixed, pairs, expect = _workload(bins, rows, 4, fill)
    mixed = mixed + _short_reads(np.random.default_rng(bins + rows))
    return ibf, reads, mixed, pairs, expect


def _run(hip, flt, s1, s2, cutoff, ablate=(), pf=None, repeat=1):
    """one stream, the batch `repeat` times on it; what the last one gave"""
    for name in ablate:
        gu.SW.on(name)
    try:
        bases, off1, off2 = gu.pack_reads(s1, s2)
        st = hip.HipStream(flt, len(s1), max(bases.size, 1))
        if pf is not None:
            st.set_postfilter(rel_filter=pf)
        for _ in range(repeat):
            st.submit(bases, off1, off2, K, W, cutoff)
            nh, status, mo, m = st.fetch()
        out = dict(nh=nh, status=status, mo=mo, m=m, tm=st.timings(), deferred=st.screen_deferred())
        if pf is not None:
            out["pf"] = st.fetch_postfilter()
        else:
            out["hashes"] = st.fetch_hashes()
        st.destroy()
        return out
    finally:
        for name in ablate:
            gu.SW.off(name)


def _same(a, b, what):
    assert np.array_equal(a["nh"], b["nh"]) and np.array_equal(a["status"], b["status"]), what
    assert np.array_equal(a["mo"], b["mo"]), what
    assert np.array_equal(a["m"], b["m"]), what  # (records compared field by field, in the order they lie in)


def _same_bytes(a, b, what):
    assert a["tm"]["algo_bytes"] == b["tm"]["algo_bytes"], what
    assert a["tm"]["fetched_bytes"] == b["tm"]["fetched_bytes"], (what, a["tm"]["fetched_bytes"], b["tm"]["fetched_bytes"])


def _per_read(r):
    return [r["m"][int(r["mo"][i]):int(r["mo"][i + 1])][["target", "count"]].tolist() for i in range(len(r["nh"]))]


@pytest.mark.parametrize("cutoff", CUTOFFS)
@pytest.mark.parametrize("bins,rows,fill", SHAPES)
def test_lean_screen_changes_nothing(hip, bins, rows, fill, cutoff):
    ibf, reads, mixed, pairs, expect = _shape(bins, rows, fill)
    flt = hip.HipFilter.ibf(ibf.data, bins, rows, 4)
    b2t = np.arange(bins, dtype=np.uint32)
    wpr = ((bins + 63) // 64 + 63) // 64  # (column slices a read at 8-byte lanes)
    for name, (s1, s2) in (("single", (reads, None)), ("mixed", (mixed, None)), ("paired", pairs)):
        new = _run(hip, flt, s1, s2, cutoff)
        old = _run(hip, flt, s1, s2, cutoff, ablate=("lean_screen",))
        what = (bins, fill, cutoff, name)
        print(f"{what}: units {len(s1) * wpr} left to the list {new['deferred']}, fetched {new['tm']['fetched_bytes']} of {new['tm']['algo_bytes']}")
        _same(new, old, what)
        _same_bytes(new, old, what)
        assert old["deferred"] == 0 and new["deferred"] <= len(s1) * wpr and (_lean(bins) or new["deferred"] == 0)
        _same(new, _run(hip, flt, s1, s2, cutoff, ablate=("row_screen",)), what)
        _same(new, _run(hip, flt, s1, s2, cutoff, ablate=("early_exit",)), what)
        ho, hs = new["hashes"]
        got = _per_read(new)
        for i in sorted(set(range(0, len(s1), 3)) | ({r for r, _, _ in expect} if s1 is reads else set())):
            exp_m, _ = gu.oracle_matches(ibf, b2t, bins, hs[int(ho[i]):int(ho[i + 1])], cutoff)
            assert [tuple(x) for x in got[i]] == exp_m, (what, i)
        if s1 is reads and cutoff == 0.75:
            for r, b, c in expect:  # the stray bins at T - 1 (no match), T and T + 1 (their exact counts)
                assert dict(tuple(x) for x in got[r]).get(b) == c, (what, r, b, c)
            if fill == 0.5 and _lean(bins):
                assert 0 < new["deferred"] < len(s1) * wpr // 2, "the screen-only kernel takes most units of this batch"
        if s1 is mixed:
            nh = new["nh"]
            assert {0, 1} <= set(nh.tolist()) and len(set(nh[nh < 10].tolist())) >= 5 and (nh > 127).any() and ((nh > 64) & (nh <= 127)).any()
    flt.free()


@pytest.mark.parametrize("bins,rows,fill", [(4096, 5003, 0.5), (4096, 5003, 0.8), (4160, 3001, 0.5)])
def test_same_batch_twice_reversed_and_small_launches(hip, bins, rows, fill):
    ibf, reads, mixed, pairs, expect = _shape(bins, rows, fill)
    flt = hip.HipFilter.ibf(ibf.data, bins, rows, 4)
    cutoff = 0.75
    batch = reads[:200] + mixed
    once = _run(hip, flt, batch, None, cutoff)
    old = _run(hip, flt, batch, None, cutoff, ablate=("lean_screen",))
    _same(once, old, "once")
    # twice on one stream: the list's counter starts from zero again
    twice = _run(hip, flt, batch, None, cutoff, repeat=2)
    _same(once, twice, "twice")
    _same_bytes(once, twice, "twice")
    assert once["deferred"] == twice["deferred"]
    # the same reads in reversed order: the same matches read by read
    rev = _run(hip, flt, batch[::-1], None, cutoff)
    assert _per_read(rev)[::-1] == _per_read(once)
    _same_bytes(once, rev, "reversed")
    # a launch of one read and of two: a read with a screen, a short one without, the read with five stray bins (its screen is aborted)
    r5 = expect[-1][0]
    per = _per_read(_run(hip, flt, reads, None, cutoff, ablate=("lean_screen",)))
    for idx in ([1], [r5], [r5, 1], [1, 2]):
        sub = [reads[i] for i in idx]
        a = _run(hip, flt, sub, None, cutoff)
        b = _run(hip, flt, sub, None, cutoff, ablate=("lean_screen",))
        _same(a, b, idx)
        _same_bytes(a, b, idx)
        assert _per_read(a) == [per[i] for i in idx]
    short = [mixed[0], mixed[-25]]
    _same(_run(hip, flt, short, None, cutoff), _run(hip, flt, short, None, cutoff, ablate=("lean_screen",)), "short")
    flt.free()


@pytest.mark.parametrize("cutoff", (0.75, 0.9))
@pytest.mark.parametrize("bins,rows,fill", [(4096, 5003, 0.5), (4096, 5003, 0.8), (4160, 3001, 0.5)])
def test_with_a_postfilter(hip, bins, rows, fill, cutoff):
    ibf, reads, mixed, pairs, _ = _shape(bins, rows, fill)
    flt = hip.HipFilter.ibf(ibf.data, bins, rows, 4)
    for s1, s2 in ((reads, None), (mixed, None), pairs):
        for rel in (0.0, 0.5):
            a = _run(hip, flt, s1, s2, cutoff, pf=rel)
            b = _run(hip, flt, s1, s2, cutoff, pf=rel, ablate=("lean_screen",))
            _same(a, b, (cutoff, rel))
            _same_bytes(a, b, (cutoff, rel))
            assert np.array_equal(a["pf"][0], b["pf"][0]) and a["pf"][1:] == b["pf"][1:], (cutoff, rel, a["pf"][1:], b["pf"][1:])
    flt.free()


@pytest.mark.parametrize("cutoff", CUTOFFS)
@pytest.mark.parametrize("ones", (True, False))
def test_all_ones_and_all_zeros(hip, ones, cutoff):
    bins, rows = 4096, 1009
    ibf = gf.random_ibf(bins, rows, 4, 0.5, seed=11)
    ibf.data[:] = np.uint64(0xFFFFFFFFFFFFFFFF) if ones else np.uint64(0)
    rng = np.random.default_rng(5)
    batch = [gu.random_seq(rng, 150) for _ in range(48)] + _short_reads(rng) + [gu.random_seq(rng, ln) for ln in (600, 900, 1100)]
    flt = hip.HipFilter.ibf(ibf.data, bins, rows, 4)
    new = _run(hip, flt, batch, None, cutoff)
    old = _run(hip, flt, batch, None, cutoff, ablate=("lean_screen",))
    _same(new, old, (ones, cutoff))
    _same_bytes(new, old, (ones, cutoff))
    _same(new, _run(hip, flt, batch, None, cutoff, ablate=("row_screen",)), (ones, cutoff))
    nh = new["nh"]
    fast = int(((nh >= 1) & (nh <= 127)).sum())  # units the fast kernels take (one slice a read)
    per = _per_read(new)
    for i, n in enumerate(nh.tolist()):
        want = [(b, n) for b in range(bins)] if ones and n else []
        assert per[i] == want, (ones, cutoff, i, n)
    screens = cutoff >= 0.75  # (at 0.55 the table gives nothing below n = 31, and above it only with a cutoff count of two and more)
    if ones:
        # every bin passes every survey: every unit is left to the list (where no n of the launch has a table entry, the kernel does not run)
        assert new["deferred"] == fast if screens else new["deferred"] in (0, fast)
    else:
        assert new["deferred"] < fast if screens else new["deferred"] <= fast, "a screened unit of an empty filter ends dead at its survey"
    flt.free()
