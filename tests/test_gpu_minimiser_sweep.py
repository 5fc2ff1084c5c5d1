"""The minimiser kernels against the oracle in every cell of their dispatch (tests/minimiser_cases.py): path A in all 16
window widths with the float and the integer minimum, paths B and D at their boundaries, path C through the reads above
640 bases inside every A and B shape -- single reads, pairs, read ranges, and the shapes the library refuses.
Every read is compared, hash for hash; tests/test_minimiser_reference_cpu.py shows that the oracle is right on these
inputs and that the inputs separate the usual wrong kernels from a right one."""
import functools

import numpy as np
import pytest

import ganon_fixtures as gf
import gpu_util as gu
import minimiser_cases as mc

pytestmark = pytest.mark.gpu

MAX_READS, MAX_BASES = 1024, 1 << 20
IDS = [s.id for s in mc.SHAPES]


@pytest.fixture(scope="module")
def hip():
    import ganon_amd
    ganon_amd.load_library()
    assert ganon_amd.device_count() >= 1, "no HIP device: the product path has no CPU fallback"
    return ganon_amd


@pytest.fixture(scope="module")
def streams(hip):
    """one tiny filter; one stream for the single-read sets and one for the paired sets, kept over all shapes"""
    ibf = gf.random_ibf(64, 257, 3, 0.3, 1)
    flt = hip.HipFilter.ibf(ibf.data, ibf.bins, ibf.bin_size, ibf.hash_funs)
    sts = {kind: hip.HipStream(flt, MAX_READS, MAX_BASES) for kind in ("single", "paired")}
    yield sts
    for st in sts.values():
        st.destroy()
    flt.free()


def _reads(kind, k, w):
    return (mc.single_reads(k, w), None) if kind == "single" else mc.paired_reads(k, w)


@functools.lru_cache(maxsize=None)
def _expected(kind, k, w):
    """[(status, hashes)] per read from the oracle -- computed once per read set and shared, never written to"""
    s1, s2 = _reads(kind, k, w)
    return gu.oracle_hashes(s1, s2, k, w)


def _run(streams, kind, k, w, classify=False):
    s1, s2 = _reads(kind, k, w)
    st = streams[kind]
    st.upload(*gu.pack_reads(s1, s2))
    return _hash(st, k, w, classify)


def _hash(st, k, w, classify):
    """-> (n_hashes, status, hash_off, hashes).  gn_stream_classify is the product path (minimiser kernels on the side stream,
    ranges) and the one after which the ABI hands out status; gn_stream_minimisers is the builder's entry, on the main
    stream: after it the tap alone is readable, so n_hashes is taken from its offsets and status is None."""
    if classify:
        st.classify(k, w, 0.5)
        nh, status = st.fetch_read_info()
        ho, hs = st.fetch_hashes()
        return nh, status, ho, hs
    st.minimisers(k, w)
    ho, hs = st.fetch_hashes()
    return np.diff(ho).astype(np.uint32), None, ho, hs


def _assert_oracle(res, kind, k, w):
    nh, status, ho, hs = res
    s1, s2 = _reads(kind, k, w)
    exp = _expected(kind, k, w)
    assert len(nh) == len(exp) == len(ho) - 1
    for i, (es, eh) in enumerate(exp):
        where = (kind, i, len(s1[i]), len(s2[i]) if s2 else None)
        assert status is None or status[i] == es, where
        assert nh[i] == len(eh), where + (int(nh[i]), len(eh))
        assert np.array_equal(hs[int(ho[i]):int(ho[i + 1])], eh), where
    ok = np.array([es == 0 for es, _ in exp])
    assert int(ho[-1]) == int(nh[ok].sum()) == len(hs) == sum(len(eh) for _, eh in exp)
    assert status is None or len(status) == len(exp)


def _assert_same(a, b):
    for x, y in zip(a, b):
        assert (x is None and y is None) or np.array_equal(x, y)


@pytest.mark.parametrize("shape", mc.SHAPES, ids=IDS)
def test_sweep(streams, shape):
    for kind in ("single", "paired"):
        for classify in (False, True):
            _assert_oracle(_run(streams, kind, shape.k, shape.w, classify), kind, shape.k, shape.w)


@pytest.mark.parametrize("kind", ["single", "paired"])
@pytest.mark.parametrize("shape", mc.RANGE_SHAPES, ids=[s.id for s in mc.RANGE_SHAPES])
def test_read_ranges(streams, shape, kind):
    # chunk=100 hashes the batch in ranges of 100 reads (read_begin > 0, ranges that start inside a wave, a deferred list
    # per range); chunk=0 is one range
    k, w = shape.k, shape.w
    gu.SW.on("chunk=100")
    cut = _run(streams, kind, k, w, classify=True)
    gu.SW.on("chunk=0")
    whole = _run(streams, kind, k, w, classify=True)
    _assert_same(cut, whole)
    _assert_oracle(cut, kind, k, w)
    _assert_oracle(whole, kind, k, w)


def test_refused_shapes(hip, streams):
    first = mc.SHAPES[0]
    st = streams["single"]
    _assert_oracle(_run(streams, "single", first.k, first.w), "single", first.k, first.w)
    for k, w, code in ((0, 5, -22), (33, 40, -22), (20, 19, -22), (0, 0, -22),       # GN_EINVAL
                       (1, 449, -34), (32, 480, -34)):                               # GN_ERANGE: K = 449
        for call in (lambda: st.minimisers(k, w), lambda: st.classify(k, w, 0.5)):
            with pytest.raises(hip.GanonHipError) as e:
                call()
            assert e.value.code == code, (k, w, e.value.code)
            # the stream is as usable as before: the same reads, a valid shape
            _assert_oracle(_hash(st, first.k, first.w, classify=True), "single", first.k, first.w)
    _assert_oracle(_run(streams, "single", 1, 448), "single", 1, 448)    # K = 448 itself is served


def test_no_state_survives_a_batch(streams):
    # the first shape, then batches that leave a long deferred list, a work hint taken from it (classify records it) and
    # no list at all (path D), then the first shape again on the same stream: a left-over deferred counter, stale staged
    # emissions or a grid sized by a stale hint would change it
    first, last = mc.SHAPES[0], mc.SHAPES[-1]
    for kind in ("single", "paired"):
        before = _run(streams, kind, first.k, first.w, classify=True)
        _assert_oracle(before, kind, first.k, first.w)
        _assert_oracle(_run(streams, kind, 19, 83, classify=True), kind, 19, 83)
        _assert_oracle(_run(streams, kind, 20, 35, classify=True), kind, 20, 35)
        _assert_oracle(_run(streams, kind, last.k, last.w), kind, last.k, last.w)
        again = _run(streams, kind, first.k, first.w, classify=True)
        _assert_same(before, again)
        _assert_oracle(again, kind, first.k, first.w)
