"""Wrapped, multi-record FASTA tokenised on the device (csrc/gn_genome.hip: gn_stream_upload_genome_text / _genome_index / _genome_records)
against a restatement of the host reader's record rules (host/seq_io.cpp, SeqReader::next's FASTA branch) and the oracle's minimisers.
Every text is at most 64 KiB."""
import numpy as np
import pytest

import oracle

pytestmark = pytest.mark.gpu

SHAPES = [(19, 31, 512), (4, 4, 64)]  # (k, w, stride)
LETTERS = b"ABCDGHKMNRSTUVWY"
LEGAL = set(LETTERS + LETTERS.lower())
IGNORED = set(b" \t\n\v\f\r0123456789")
BAD_LETTER, NO_HEADER = 1, 2
TILE = 4096


@pytest.fixture(scope="module")
def hip():
    import ganon_amd
    ganon_amd.load_library()
    assert ganon_amd.device_count() >= 1, "no HIP device: the product path has no CPU fallback"
    return ganon_amd


@pytest.fixture(scope="module")
def flt(hip):
    f = hip.HipFilter.ibf(np.zeros((10, 1), dtype=np.uint64), 64, 10, 2)
    yield f
    f.free()


@pytest.fixture(scope="module")
def stream(hip, flt):
    st = hip.HipStream(flt, 4096, 1 << 17)
    yield st
    st.destroy()


def parse(text: bytes, continues=False):
    """the record rules: -> (status, bad_at, [(offset of the header, letters)])"""
    recs = [[0, bytearray()]] if continues else []
    at = 0
    for raw in text.split(b"\n"):
        line = raw[:-1] if raw.endswith(b"\r") else raw
        if line[:1] in (b">", b";"):
            recs.append([at, bytearray()])
        elif not recs:
            if line:
                return NO_HEADER, None, []
        else:
            for j, c in enumerate(raw):
                if c in IGNORED:
                    continue
                if c not in LEGAL:
                    return BAD_LETTER, at + j, []
                recs[-1][1].append(c)
        at += len(raw) + 1
    return 0, None, [(a, bytes(s)) for a, s in recs]


def state_of(n, w, min_length):
    return 1 if n < min_length else 2 if n < w else 0


def pieces_of(n, w, stride):
    return (n - w) // stride + 1 if n >= w else 0


def hashes_of(seqs, k, w):
    sets = [oracle.minimiser_hash(oracle.to_ranks(s), k, w) for s in seqs if len(s) >= w]
    return np.unique(np.concatenate(sets)) if sets else np.zeros(0, np.uint64)


def device_set(st, k, w, n_pieces):
    if n_pieces == 0:
        return np.zeros(0, np.uint64)
    st.minimisers(k, w)
    return st.distinct_hashes().copy()


def check(st, text, k, w, stride, min_length=0):
    assert len(text) <= 65536
    status, bad_at, recs = parse(text)
    st.upload_genome_text(text, w, stride, min_length)
    ix = st.genome_index()
    assert ix["status"] == status, ix
    if status:
        if bad_at is not None:
            assert ix["bad_at"] == bad_at
        return ix
    rec_at, rec_letters, rec_state = st.genome_records()
    assert ix["n_records"] == len(recs) and ix["parsed_bytes"] == len(text) and ix["open_letters"] == 0
    assert rec_at.tolist() == [a for a, _ in recs]
    assert rec_letters.tolist() == [len(s) for _, s in recs]
    states = [state_of(len(s), w, min_length) for _, s in recs]
    assert rec_state.tolist() == states
    kept = [s for (_, s), e in zip(recs, states) if e == 0]
    assert ix["n_pieces"] == sum(pieces_of(len(s), w, stride) for s in kept)
    got = device_set(st, k, w, ix["n_pieces"])
    assert np.array_equal(got, hashes_of(kept, k, w))
    return ix


def dna(rng, n, alphabet=b"ACGT"):
    return bytes(rng.choice(np.frombuffer(alphabet, np.uint8), n).tobytes())


def wrap(seq, width, eol=b"\n"):
    if isinstance(width, int):
        return b"".join(seq[i:i + width] + eol for i in range(0, len(seq), width))
    out, i, j = [], 0, 0
    while i < len(seq):  # ragged: the widths in turn
        out.append(seq[i:i + width[j % len(width)]] + eol)
        i += width[j % len(width)]
        j += 1
    return b"".join(out)


def formatting_cases(w):
    rng = np.random.default_rng(11)
    a, b, c = dna(rng, 700), dna(rng, 333), dna(rng, 1201)
    yield "width1", b">a\n" + wrap(a, 1) + b">b\n" + wrap(b, 1)
    yield "width60", b">a\n" + wrap(a, 60) + b">b\n" + wrap(b, 60) + b">c\n" + wrap(c, 60)
    yield "width70", b">a x y\n" + wrap(a, 70) + b">b\n" + wrap(c, 70)
    yield "ragged", b">a\n" + wrap(a, (7, 1, 80, 2, 61)) + b">b\n" + wrap(c, (3, 200, 5))
    yield "crlf", b">a\r\n" + wrap(a, 60, b"\r\n") + b">b\r\n" + wrap(b, 70, b"\r\n")
    yield "blank_lines", b"\n\r\n\n>a\n" + wrap(a[:300], 60) + b"\n\n" + wrap(a[300:], 60) + b"\r\n>b\n\n" + wrap(b, 60) + b"\n"
    yield "spaces_digits", b">a\n" + b"".join(b"%9d " % (i + 1) + a[i:i + 10] + b" " + a[i + 10:i + 20] + b"\t\v\f\n" for i in range(0, 700, 20)) + b">b\n" + wrap(b, 60)
    yield "lower_iupac", b">a\n" + wrap(dna(rng, 900, LETTERS + LETTERS.lower()), 60) + b">b\n" + wrap(a.lower(), 70)
    yield "semicolon_header", b";a comment header\n" + wrap(a, 60) + b">b\n" + wrap(b, 60) + b";c\n" + wrap(c, 60)
    yield "header_with_letters", b">ACGT>ACGT ACGTACGTACGTACGTACGTACGTACGTACGT >>\n" + wrap(a, 60) + b">;>GATTACA!*\n" + wrap(b, 60)
    yield "no_trailing_newline", b">a\n" + wrap(a, 60) + b">b\n" + wrap(b, 60)[:-1]
    yield "empty_records", b">a\n>b\n" + wrap(a, 60) + b">c\n>d\n\n>e\n" + wrap(b, 60) + b">f\n"
    yield "header_only", b">a"
    yield "empty_text", b""


@pytest.mark.parametrize("k,w,stride", SHAPES)
def test_line_widths_and_formatting(stream, k, w, stride):
    for name, text in formatting_cases(w):
        try:
            check(stream, text, k, w, stride)
        except AssertionError as e:
            raise AssertionError(f"case {name}: {e}") from e


@pytest.mark.parametrize("k,w,stride", SHAPES)
def test_record_lengths(stream, k, w, stride):
    rng = np.random.default_rng(5)
    lengths = [k - 1, k, w - 1, w, w + 1, stride + w - 2, stride + w - 1, stride + w, 2 * stride + w - 1, 2 * stride + w]
    text = b"".join(b">r%d\n" % n + wrap(dna(rng, n), 60) for n in lengths)
    check(stream, text, k, w, stride)
    for n in lengths:  # ... and each alone, at the end of a text without a newline
        check(stream, b">r\n" + wrap(dna(rng, n), 70)[:-1], k, w, stride)


@pytest.mark.parametrize("k,w,stride", SHAPES)
def test_tile_boundaries(stream, k, w, stride):
    rng = np.random.default_rng(3)
    a, b = dna(rng, 6000), dna(rng, 3000)
    head = b">a\n" + wrap(a, 60)
    cut = head[:TILE - 1]  # ends somewhere in a line
    # the '\n' is the last byte of tile 0 and '>' the first byte of tile 1
    text = cut + b"\n>b\n" + wrap(b, 60)
    assert text[TILE - 1:TILE + 1] == b"\n>"
    check(stream, text, k, w, stride)
    # '\n' first byte of tile 1 (the header begins one byte later)
    check(stream, cut + b"A\n>b\n" + wrap(b, 60), k, w, stride)
    # a header line that straddles the boundary, full of letters
    text = head[:TILE - 40] + b"\n>" + b"ACGT" * 30 + b"\n" + wrap(b, 60)
    assert text.index(b"\n>") < TILE < text.index(b"\n", TILE - 38)
    check(stream, text, k, w, stride)
    # a header line longer than a tile (two whole tiles lie inside it), then a record; and one as the text's last line
    text = b">a\n" + wrap(a[:500], 60) + b">" + b"GATTACA " * 1300 + b"\n" + wrap(b, 60)
    check(stream, text, k, w, stride)
    check(stream, text + b">" + b"ACGT" * 2500, k, w, stride)
    # a single sequence line of 10 000 letters, with and without a header line behind it
    long = dna(rng, 10000)
    check(stream, b">a\n" + long + b"\n", k, w, stride)
    check(stream, b">a\n" + long + b"\n>b\n" + wrap(b, 70), k, w, stride)
    # a text of exactly one tile, and one byte more
    check(stream, (b">a\n" + wrap(a, 60))[:TILE - 1] + b"\n", k, w, stride)
    check(stream, (b">a\n" + wrap(a, 60))[:TILE] + b"\n", k, w, stride)


@pytest.mark.parametrize("k,w,stride", SHAPES)
def test_errors(stream, k, w, stride):
    rng = np.random.default_rng(2)
    a, b = dna(rng, 5000), dna(rng, 900)
    good = b">a\n" + wrap(a, 60) + b">b\n" + wrap(b, 60)
    for bad_byte in (b"!", b"E", b">", b";", b"\x00", b"\xc1", b"-", b"*"):
        for at in (len(good) - 100, 4100, 7):
            assert good[at] != 10 and good[at - 1] != 10 and at > 3  # inside a sequence line, not its first byte
            text = good[:at] + bad_byte + good[at + 1:]
            ix = check(stream, text, k, w, stride)
            assert ix["status"] == BAD_LETTER and ix["bad_at"] == at
    # two illegal bytes: the first is reported
    text = good[:200] + b"?" + good[201:6000] + b"?" + good[6001:]
    assert check(stream, text, k, w, stride)["bad_at"] == 200
    # the same bytes in a header line are no error
    ix = check(stream, b">a!E>;\x01\xc1-*\n" + wrap(a, 60) + b">b ! \n" + wrap(b, 60), k, w, stride)
    assert ix["status"] == 0 and ix["n_records"] == 2
    # a first line that is no header
    for text in (wrap(a[:100], 60) + good, b"\n\n x\n" + good, b" \n" + good, b"\r\r\n" + good, b"ACGT", b"\n\r"  b"\r"):
        assert check(stream, text, k, w, stride)["status"] == NO_HEADER
    assert check(stream, b"\n\r\n\r", k, w, stride)["status"] == 0  # blank lines alone are an empty text


@pytest.mark.parametrize("k,w,stride", SHAPES)
def test_min_length_filters(stream, k, w, stride):
    rng = np.random.default_rng(8)
    lengths = [10, 2000, 499, 500, 501, 30, 0, 1500]
    text = b"".join(b">r%d\n" % n + wrap(dna(rng, n), 70) for n in lengths)
    check(stream, text, k, w, stride, min_length=500)
    _, _, state = stream.genome_records()
    assert state.tolist() == [1, 0, 1, 0, 0, 1, 1, 0]
    check(stream, text, k, w, stride, min_length=3000)
    assert stream.genome_records()[2].tolist() == [1] * 8


@pytest.mark.parametrize("k,w,stride", SHAPES)
def test_chunked_record(stream, k, w, stride):
    """a 40 kb record fed as texts cut at newlines: the union of the sets is the whole record's set"""
    rng = np.random.default_rng(13)
    seq = dna(rng, 40000)
    body = wrap(seq, (70, 70, 70, 1, 2, 70, 61))
    text = b">long one\n" + body + b">next\n" + wrap(seq[:300], 60)
    whole = hashes_of([seq, seq[:300]], k, w)
    nl = [i + 1 for i in range(len(text)) if text[i:i + 1] == b"\n" and i + 1 < len(text) - 400]
    # the second cut lies fewer than w - 1 letters behind the first (the 1- and 2-letter lines): the tail is carried twice
    first = next(i for i, p in enumerate(nl) if p > 13000 and nl[i + 1] - p == 2)
    for cuts in ([nl[first], nl[first + 1]], [nl[first], nl[first + 2], nl[len(nl) // 2]], [nl[1], nl[-1]], [nl[0], nl[1]]):
        parts = [text[a:b] for a, b in zip([0] + cuts, cuts + [len(text)])]
        sets, letters = [], 0
        for i, part in enumerate(parts):
            last = i == len(parts) - 1
            stream.upload_genome_text(part, w, stride, 0, continues=i > 0, open_end=not last)
            ix = stream.genome_index()
            rec_at, rec_letters, rec_state = stream.genome_records()
            letters += sum(c in LEGAL for c in part[part.index(b"\n") + 1 if i == 0 else 0:]) if not last else 0
            assert ix["status"] == 0 and ix["parsed_bytes"] == len(part)
            if not last:
                assert ix["open_letters"] == letters and ix["n_records"] == 1 and rec_state.tolist() == [3] and rec_letters.tolist() == [letters]
            else:
                assert ix["open_letters"] == 0 and rec_state.tolist() == [0, 0] and rec_letters.tolist() == [40000, 300]
                assert rec_at.tolist() == [0, part.index(b">next")]
            sets.append(device_set(stream, k, w, ix["n_pieces"]))
        assert np.array_equal(np.unique(np.concatenate(sets)), whole), cuts
    # a text that continues nothing after one that was left open starts afresh
    stream.upload_genome_text(text[:nl[5]], w, stride, 0, open_end=True)
    assert stream.genome_index()["open_letters"] > 0
    check(stream, text, k, w, stride)


@pytest.mark.parametrize("k,w,stride", SHAPES)
def test_capacity_takes_a_prefix(hip, flt, k, w, stride):
    rng = np.random.default_rng(21)
    seqs = [dna(rng, int(n)) for n in rng.integers(w, 4 * stride, 24)]
    text = b"".join(b">r%d\n" % i + wrap(s, 60) for i, s in enumerate(seqs))
    starts = [text.index(b">r%d\n" % i) for i in range(len(seqs))] + [len(text)]
    small = hip.HipStream(flt, 8, 1 << 16)
    try:
        at, r, sets = 0, 0, []
        while at < len(text):
            small.upload_genome_text(text[at:], w, stride)
            ix = small.genome_index()
            take, pieces = 0, 0
            while r + take < len(seqs) and pieces + pieces_of(len(seqs[r + take]), w, stride) <= 8:
                pieces += pieces_of(len(seqs[r + take]), w, stride)
                take += 1
            assert 0 < take < len(seqs)
            assert ix["status"] == 0 and ix["n_records"] == take and ix["n_pieces"] == pieces and ix["parsed_bytes"] == starts[r + take] - at
            assert small.genome_records()[1].tolist() == [len(s) for s in seqs[r:r + take]]
            sets.append(device_set(small, k, w, ix["n_pieces"]))
            at, r = starts[r + take], r + take
        assert np.array_equal(np.unique(np.concatenate(sets)), hashes_of(seqs, k, w))
        # a first record that alone is too large
        small.upload_genome_text(b">big\n" + wrap(dna(rng, 9 * stride + w), 60), w, stride)
        with pytest.raises(hip.GanonHipError):
            small.genome_index()
    finally:
        small.destroy()
