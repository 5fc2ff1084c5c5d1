"""The stream kernels of the fast count path: the same kernels with non-temporal row loads, which a flat filter of four hash functions
takes from `stream_rows_min_bytes` of row storage on (gn_row_policy.h; 2 GiB by default, so the test sets 0 on its small filters).  A
cache policy changes no value: with the threshold at 0 everything a caller sees -- hashes, status, offsets, match records -- and every
byte a launch requests equal the run with the switch `stream_rows` (plain loads everywhere) and the oracle.

Shapes (those of test_gpu_stray_probe.py, Bernoulli(0.5) rows): 4096 bins (the screen-only kernel and its list launch), 4160 bins (two
column slices a read, the second one word wide), 32768 bins (16-byte lanes, wide rows: the wide instances).  Reads: the batches of
test_gpu_stray_probe.py -- the reads of test_gpu_row_screen.py plus that file's adversary reads.  Cutoffs: 0.2 (no screen in the
launch's table: the instance without a screen, every read), 0.75 and 1.0.  `lean_screen` ablated runs the screening instance
<4,1,true,false,true> as a stream kernel.  The instances without a screen have no stream twin (they measured slower with one,
gn_row_policy.h): at cutoff 0.2 every shape launches plain kernels whatever the threshold, and the comparison still holds."""
import numpy as np
import pytest

import ganon_fixtures as gf
import gpu_util as gu
from test_gpu_lean_screen import _per_read, _same, _same_bytes
from test_gpu_row_screen import K, W
from test_gpu_stray_probe import SHAPES, _shape

pytestmark = pytest.mark.gpu

CUTOFFS = (0.2, 0.75, 1.0)
assert SHAPES == [(4096, 5003), (4160, 3001), (32768, 1201)]


@pytest.fixture(scope="module")
def hip():
    import ganon_amd
    ganon_amd.load_library()
    assert ganon_amd.device_count() >= 1, "no HIP device: the product path has no CPU fallback"
    return ganon_amd


def _run(hip, flt, seqs, cutoff, ablate=(), repeat=1):
    """one stream, the batch `repeat` times on it; what the last one gave, and which row loads its launches took"""
    for name in ablate:
        gu.SW.on(name)
    try:
        bases, off1, off2 = gu.pack_reads(seqs, None)
        st = hip.HipStream(flt, len(seqs), max(bases.size, 1))
        for _ in range(repeat):
            st.submit(bases, off1, off2, K, W, cutoff)
            nh, status, mo, m = st.fetch()
        out = dict(nh=nh, status=status, mo=mo, m=m, tm=st.timings(), hashes=st.fetch_hashes(), streamed=st.rows_streamed())
        st.destroy()
        return out
    finally:
        for name in ablate:
            gu.SW.off(name)


def _same_all(a, b, what):
    _same(a, b, what)
    _same_bytes(a, b, what)
    assert np.array_equal(a["hashes"][0], b["hashes"][0]) and np.array_equal(a["hashes"][1], b["hashes"][1]), what


def _filter(hip, sh, bins, rows, threshold=0):
    flt = hip.HipFilter.ibf(sh["ibf"].data, bins, rows, 4)
    if threshold is not None:
        flt.set_stream_rows_min_bytes(threshold)
    return flt


@pytest.mark.parametrize("cutoff", CUTOFFS)
@pytest.mark.parametrize("bins,rows", SHAPES)
def test_stream_rows_change_nothing(hip, bins, rows, cutoff):
    sh = _shape(bins, rows)
    ibf, batch = sh["ibf"], sh["batch"]
    flt = _filter(hip, sh, bins, rows)
    b2t = np.arange(bins, dtype=np.uint32)
    new = _run(hip, flt, batch, cutoff)
    old = _run(hip, flt, batch, cutoff, ablate=("stream_rows",))
    streams = cutoff != 0.2  # (a launch without a screen has no stream instance)
    assert new["streamed"] == streams and not old["streamed"]
    print(f"bins {bins} cutoff {cutoff}: fetched {new['tm']['fetched_bytes']} of {new['tm']['algo_bytes']}, plain {old['tm']['fetched_bytes']}")
    _same_all(new, old, (bins, cutoff))
    ho, hs = new["hashes"]
    got = _per_read(new)
    for i in sorted(set(range(0, len(batch), 3)) | set(sh["engineered"])):
        assert np.array_equal(hs[int(ho[i]):int(ho[i + 1])], sh["hashes"][i]), i
        exp_m, _ = gu.oracle_matches(ibf, b2t, bins, sh["hashes"][i], cutoff)
        assert [tuple(x) for x in got[i]] == exp_m, (bins, cutoff, i)
    # the screening instance as a stream kernel: one launch, no list (8-byte lanes: <4,1,true,false,true>; the wide shape has no
    # screen-only kernel, there the switch changes nothing)
    lean_new = _run(hip, flt, batch, cutoff, ablate=("lean_screen",))
    lean_old = _run(hip, flt, batch, cutoff, ablate=("lean_screen", "stream_rows"))
    assert lean_new["streamed"] == streams and not lean_old["streamed"]
    _same_all(lean_new, lean_old, (bins, cutoff, "lean_screen"))
    _same_all(lean_new, new, (bins, cutoff, "lean_screen against the default"))
    flt.free()


@pytest.mark.parametrize("bins,rows", SHAPES)
def test_twice_reversed_and_small_launches(hip, bins, rows):
    sh = _shape(bins, rows)
    batch, cutoff = sh["batch"], 0.75
    flt = _filter(hip, sh, bins, rows)
    once = _run(hip, flt, batch, cutoff)
    plain = _run(hip, flt, batch, cutoff, ablate=("stream_rows",))
    assert once["streamed"] and not plain["streamed"]
    twice = _run(hip, flt, batch, cutoff, repeat=2)
    assert twice["streamed"]
    _same_all(once, twice, "twice")
    rev = _run(hip, flt, batch[::-1], cutoff)
    assert rev["streamed"] and _per_read(rev)[::-1] == _per_read(once)
    _same_bytes(once, rev, "reversed")
    # launches of one read and of two: a plain read, an adversary read (its finish probes, or its screen is aborted)
    per = _per_read(plain)
    adv = sh["engineered"][0]
    for idx in ([1], [adv], [adv, 1], [1, 2]):
        sub = [batch[i] for i in idx]
        a = _run(hip, flt, sub, cutoff)
        b = _run(hip, flt, sub, cutoff, ablate=("stream_rows",))
        assert a["streamed"] and not b["streamed"]
        _same_all(a, b, idx)
        assert _per_read(a) == [per[i] for i in idx]
    flt.free()


def test_launch_rule(hip):
    bins, rows = SHAPES[0]
    sh = _shape(bins, rows)
    batch = sh["batch"][:64]
    # the default threshold: these filters are megabytes, far below it
    flt = _filter(hip, sh, bins, rows, threshold=None)
    assert not _run(hip, flt, batch, 0.75)["streamed"]
    assert not _run(hip, flt, batch, 0.2)["streamed"]
    flt.set_stream_rows_min_bytes(0)
    assert _run(hip, flt, batch, 0.75)["streamed"]
    assert not _run(hip, flt, batch, 0.2)["streamed"], "no screen: no stream instance"
    assert not _run(hip, flt, batch, 0.75, ablate=("row_screen",))["streamed"]
    assert not _run(hip, flt, batch, 0.75, ablate=("stream_rows",))["streamed"]
    assert _run(hip, flt, batch, 0.75)["streamed"], "the switch is off again"
    # exactly at the row storage, and one byte above it
    flt.set_stream_rows_min_bytes(rows * (bins // 64) * 8)
    assert _run(hip, flt, batch, 0.75)["streamed"]
    flt.set_stream_rows_min_bytes(rows * (bins // 64) * 8 + 1)
    assert not _run(hip, flt, batch, 0.75)["streamed"]
    # every row fetched (no early exit): the instance has no stream twin
    flt.set_stream_rows_min_bytes(0)
    assert not _run(hip, flt, batch, 0.75, ablate=("early_exit",))["streamed"]
    flt.free()
    # other numbers of hash functions have no stream instance
    ibf3 = gf.random_ibf(bins, 1009, 3, 0.5, seed=3)
    flt3 = hip.HipFilter.ibf(ibf3.data, bins, 1009, 3)
    flt3.set_stream_rows_min_bytes(0)
    assert not _run(hip, flt3, batch, 0.75)["streamed"]
    flt3.free()
    # an HIBF: no launch of it takes a stream kernel
    hb = gf.random_hibf(60, 32, 2, seed=4, density=0.3, hash_funs=4)
    hflt = hip.HipFilter.hibf(*gf.hibf_upload_args(hb))
    hflt.set_stream_rows_min_bytes(0)
    assert not _run(hip, hflt, batch, 0.75)["streamed"]
    hflt.free()
