"""`ganon-build --hibf --hibf-hash-sets packed|spilled` on the GPU: the packed path insert against gn_filter_emplace_path and the oracle
(every IBF whole, every IBF alone, the root and a leaf in pieces), its refusals; the union of packed runs against gn_hashes_union and the
restated format; the sketches of packed runs against those of the raw sets; and the binary: the file of a packed or spilled build is byte
for byte the raw build's, in one pass, in parts, over a device list and under every layout."""
import ctypes as C
import filecmp
import os
import re

import numpy as np
import pytest

import cli_util as cu
import ganon_fixtures as gf
import oracle
from test_build_hibf_gpu import build, check_file, cut_reads, genomes, hip, short200  # noqa: F401  (fixtures among them)
from test_build_hibf_parts_gpu import INPUTS, SHAPES, beside, budget_of, check_parts, compact, one_pass, tree
from test_build_packed_cpu import BLOCK_BYTES, ITEM_BYTES, M64, encode

pytestmark = pytest.mark.gpu

U64 = np.uint64
GN_EINVAL, GN_EOVERFLOW = -22, -75
_PACKED = {}


def pack(hip, files):  # noqa: F811
    """a run of files' sets through the restated format -> (blocks, payload) as the library takes a packed run"""
    blocks, payload = encode(files)
    return np.array(blocks, dtype=hip.hip.PACKED_BLOCK_DTYPE).reshape(len(blocks)), np.array(payload, dtype=U64)


def packed_tree(hip, key, sets):  # noqa: F811
    """the sets of a tree as packed runs, made once per shape: set 2 (20 000 hashes) as two files behind each other, 700 + the rest, so that
    a short block lies in the middle of its run; the run's hashes are the set's, in its order"""
    if key not in _PACKED:
        _PACKED[key] = [pack(hip, [s[:700], s[700:]] if u == 2 else ([s] if len(s) else [])) for u, s in enumerate(sets)]
        assert [int(c) for c in _PACKED[key][2][0]["cnt"][:3]] == [512, 188, 512]
    return _PACKED[key]


def fill_packed(hip, shapes, runs, paths, pieces, chunk=0):  # noqa: F811
    """fill_pieces of the parts test through the packed insert"""
    flt = hip.HipFilter.hibf_storage([(shapes[t][0], n, shapes[t][2]) for t, _, n in pieces])
    keep, cut = compact(paths, [t for t, _, _ in pieces])
    flt.emplace_path_packed_window([runs[u] for u in keep], cut, [shapes[t][1] for t, _, _ in pieces], [a for _, a, _ in pieces], chunk)
    got = [flt.download_rows(0, n, (shapes[t][0] + 63) // 64, ibf_idx=j) for j, (t, _, n) in enumerate(pieces)]
    flt.free()
    return got


# ------------------------------------------------------------------------------------------------------------ the ABI: the insert
@pytest.mark.parametrize("h", [1, 3, 5])
@pytest.mark.parametrize("n_ub,tmax,depth", SHAPES)
def test_every_ibf_whole_and_every_ibf_alone(hip, n_ub, tmax, depth, h):  # noqa: F811
    hb, sets, paths, where, parent, shapes, ref = tree(hip, n_ub, tmax, depth, h)
    runs = packed_tree(hip, (n_ub, tmax, depth, h), sets)
    got = fill_packed(hip, shapes, runs, paths, [(t, 0, r) for t, (_, r, _) in enumerate(shapes)])
    for t in range(len(shapes)):
        assert np.array_equal(got[t], ref[t]), f"IBF {t}, every IBF whole: the bits gn_filter_emplace_path sets"
    for t, (_, r, _) in enumerate(shapes):
        assert np.array_equal(fill_packed(hip, shapes, runs, paths, [(t, 0, r)])[0], ref[t]), f"IBF {t} alone"


@pytest.mark.parametrize("chunk", [0, 700])
@pytest.mark.parametrize("h", [1, 3, 5])
@pytest.mark.parametrize("n_ub,tmax,depth", SHAPES)
def test_the_root_and_a_leaf_in_pieces(hip, n_ub, tmax, depth, h, chunk):  # noqa: F811
    hb, sets, paths, where, parent, shapes, ref = tree(hip, n_ub, tmax, depth, h)
    runs = packed_tree(hip, (n_ub, tmax, depth, h), sets)
    rows0 = shapes[0][1]
    cuts = [0, 1, 7, 512, 999, 1000, rows0 // 2, rows0 - 1, rows0]
    assert cuts == sorted(cuts)
    root = [fill_packed(hip, shapes, runs, paths, [(0, a, b - a)], chunk)[0] for a, b in zip(cuts, cuts[1:])]
    assert np.array_equal(np.concatenate(root), ref[0]), "the pieces behind each other are the root"
    leaf = where[2][0]  # the IBF that holds the 20 000-hash set's run
    if leaf == 0:
        leaf = max(i for i, _, _ in where.values())
    half = shapes[leaf][1] // 2 + 1
    other = next(t for t in range(1, len(shapes)) if t != leaf)
    a0, a1 = fill_packed(hip, shapes, runs, paths, [(0, 512, 487), (leaf, 0, half)], chunk)
    b0, b1 = fill_packed(hip, shapes, runs, paths, sorted([(other, 0, shapes[other][1]), (leaf, half, shapes[leaf][1] - half)]), chunk)
    if other > leaf:
        b0, b1 = b1, b0
    assert np.array_equal(a0, ref[0][512:999]) and np.array_equal(b0, ref[other])
    assert np.array_equal(np.concatenate([a1, b1]), ref[leaf]), "the leaf's halves"


def test_against_the_oracle(hip):  # noqa: F811
    hb, sets, paths, where, parent, shapes, ref = tree(hip, 10, 4, 4, 3)
    runs = packed_tree(hip, (10, 4, 4, 3), sets)
    refs = [oracle.Ibf(b, r, h) for b, r, h in shapes]
    for u, hs in enumerate(sets):
        if len(hs) == 0:
            continue
        i, first, n = where[u]
        refs[i].emplace_many(hs, (first + np.arange(len(hs)) // ((len(hs) + n - 1) // n)).astype(np.uint32))
        at = i
        while at != 0:
            at, b = parent[at]
            refs[at].emplace_many(hs, np.full(len(hs), b, dtype=np.uint32))
    got = fill_packed(hip, shapes, runs, paths, [(t, 0, r) for t, (_, r, _) in enumerate(shapes)])
    for t in range(len(shapes)):
        assert np.array_equal(got[t], refs[t].data), f"IBF {t}"


def test_deltas_of_64_bits(hip):  # noqa: F811
    """values up to 2^64 - 1 whose deltas take all 64 bits, among 1000 others over all 64 bits: against the raw windowed insert and the oracle"""
    H = hip.hip
    rng = np.random.default_rng(64)
    wide = np.array([0, 1 << 63, M64], dtype=U64)
    many = np.unique(np.concatenate([rng.integers(0, 1 << 64, size=1000, dtype=U64, endpoint=False), np.array([M64], dtype=U64)]))
    paths = np.zeros((2, 2), dtype=H.PATH_DTYPE)
    paths[0, 0], paths[0, 1] = (1, 0, 3, 0, 1), (0, 69, 1, 0, 1)
    paths[1, 0], paths[1, 1] = (1, 3, 5, 0, (len(many) + 4) // 5), (0, 68, 1, 0, 1)
    runs = [pack(hip, [wide]), pack(hip, [many])]
    assert int(runs[0][0]["width"][0]) == 64 and int(many[-1]) == M64
    shapes, got = [(70, 500, 3), (8, 300, 3)], []
    for packed in (False, True):
        flt = hip.HipFilter.hibf_storage(shapes)
        if packed:
            flt.emplace_path_packed_window(runs, paths, [500, 300], [0, 0])
        else:
            flt.emplace_path_window([wide, many], paths, [500, 300], [0, 0])
        got.append([flt.download_rows(0, 500, 2, ibf_idx=0), flt.download_rows(0, 300, 1, ibf_idx=1)])
        flt.free()
    refs = [oracle.Ibf(b, r, h) for b, r, h in shapes]
    refs[1].emplace_many(wide, np.arange(3, dtype=np.uint32))
    refs[1].emplace_many(many, (3 + np.arange(len(many)) // ((len(many) + 4) // 5)).astype(np.uint32))
    refs[0].emplace_many(wide, np.full(3, 69, dtype=np.uint32))
    refs[0].emplace_many(many, np.full(len(many), 68, dtype=np.uint32))
    for j in range(2):
        assert np.array_equal(got[1][j], got[0][j]) and np.array_equal(got[1][j], refs[j].data), f"IBF {j}"


def test_a_piece_no_row_falls_into_stays_zero(hip):  # noqa: F811
    hs = np.array([3, 1 << 20, (1 << 37) + 5], dtype=U64)
    whole = oracle.Ibf(70, 1000, 1)
    whole.emplace_many(hs, np.full(3, 69, dtype=np.uint32))
    used = np.nonzero(whole.data.any(axis=1))[0]
    assert 1 <= len(used) <= 3
    gaps = [(a + 1, b) for a, b in zip([-1] + used.tolist(), used.tolist() + [1000]) if b - a > 1]
    a, b = max(gaps, key=lambda g: g[1] - g[0])
    paths = np.zeros((1, 1), dtype=hip.hip.PATH_DTYPE)
    paths[0, 0] = (0, 69, 1, 0, 1)
    run = pack(hip, [hs])
    flt = hip.HipFilter.hibf_storage([(70, b - a, 1)])
    flt.emplace_path_packed_window([run], paths, [1000], [a])
    assert not flt.download_rows(0, b - a, 2).any()
    flt.free()
    r = int(used[0])  # and a piece of one row that a hash does fall into
    flt = hip.HipFilter.hibf_storage([(70, 1, 1)])
    flt.emplace_path_packed_window([run], paths, [1000], [r])
    assert np.array_equal(flt.download_rows(0, 1, 2), whole.data[r:r + 1])
    flt.free()


def test_refusals_write_nothing(hip):  # noqa: F811
    H = hip.hip
    hs = np.arange(1, 1001, dtype=U64) * U64(0x9E3779B97F4A7C15 % (1 << 38))
    hs.sort()
    run = pack(hip, [hs])
    flt = hip.HipFilter.hibf_storage([(70, 500, 3), (8, 300, 3)])
    untouched = lambda: not flt.download_rows(0, 500, 2, ibf_idx=0).any() and not flt.download_rows(0, 300, 1, ibf_idx=1).any()  # noqa: E731

    def path(*entries):
        p = np.zeros((1, 2), dtype=H.PATH_DTYPE)
        for d, e in enumerate(entries):
            p[0, d] = e
        return p

    good = path((1, 2, 4, 0, 250), (0, 69, 1, 0, 1))
    cases = [("an IBF out of range", path((2, 0, 1, 0, 1)), [500, 300], [0, 0]),
             ("a bin out of range", path((1, 5, 4, 0, 250)), [500, 300], [0, 0]),
             ("a bin out of range above", path((1, 2, 4, 0, 250), (0, 70, 1, 0, 1)), [500, 300], [0, 0]),
             ("hashes that do not fit the run", path((1, 2, 4, 0, 249)), [500, 300], [0, 0]),
             ("no hashes a bin", path((1, 2, 4, 0, 0)), [500, 300], [0, 0]),
             ("row_begin + rows > total_rows", good, [500, 300], [0, 1]),
             ("rows > total_rows", good, [499, 300], [0, 0]),
             ("total_rows of 2^32", good, [1 << 32, 300], [0, 0]),
             ("total_rows of 0", good, [500, 0], [0, 0])]
    for what, p, total, begin in cases:
        with pytest.raises(hip.GanonHipError):
            flt.emplace_path_packed_window([run], p, total, begin)
        assert untouched(), what
    # bad blocks: the second block of the run is spoilt, the first is good
    for what, field, value in (("cnt 0", "cnt", 0), ("cnt 513", "cnt", 513), ("width 65", "width", 65)):
        blocks = run[0].copy()
        blocks[field][1] = value
        with pytest.raises(hip.GanonHipError) as e:
            flt.emplace_path_packed_window([(blocks, run[1])], good, [500, 300], [0, 0])
        assert e.value.code == GN_EINVAL and untouched(), what
    with pytest.raises(hip.GanonHipError) as e:
        flt.emplace_path_packed_window([(run[0], None)], good, [500, 300], [0, 0])
    assert e.value.code == GN_EINVAL and untouched(), "payload words without a payload"
    # null arguments, through the library itself
    L = hip.load_library()
    bptr, wptr = (C.c_void_p * 1)(run[0].ctypes.data), (C.c_void_p * 1)(run[1].ctypes.data)
    n_blocks, total, begin = np.array([len(run[0])], U64), np.array([500, 300], U64), np.array([0, 0], U64)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    full = [flt._h, bptr, vp(n_blocks), wptr, 1, vp(good), 2, vp(total), vp(begin), 0]
    for k in (0, 1, 2, 3, 5, 7, 8):
        args = list(full)
        args[k] = None
        assert L.gn_filter_emplace_path_packed_window(*args) != 0, k
    args = list(full)
    args[6] = 0  # no depth
    assert L.gn_filter_emplace_path_packed_window(*args) != 0
    assert untouched()
    # a flat filter is no HIBF
    flat = hip.HipFilter.ibf_storage(70, 500, 3)
    with pytest.raises(hip.GanonHipError):
        flat.emplace_path_packed_window([run], path((0, 0, 1, 0, 1)), [500], [0])
    assert not flat.download_rows(0, 500, 2).any()
    flat.free()
    # and the call that is not refused writes what the raw insert writes
    flt.emplace_path_packed_window([run], good, [500, 300], [0, 0])
    raw = hip.HipFilter.hibf_storage([(70, 500, 3), (8, 300, 3)])
    raw.emplace_path_window([hs], good, [500, 300], [0, 0])
    for j, (n, w) in enumerate(((500, 2), (300, 1))):
        assert flt.download_rows(0, n, w, ibf_idx=j).any() and np.array_equal(flt.download_rows(0, n, w, ibf_idx=j), raw.download_rows(0, n, w, ibf_idx=j))
    flt.free(), raw.free()


# ------------------------------------------------------------------------------------------------------------ the ABI: the union
def union_inputs():
    rng = np.random.default_rng(41)
    a = np.unique(rng.integers(0, 1 << 38, size=3000, dtype=U64))
    b = np.unique(rng.integers(0, 1 << 38, size=1300, dtype=U64))
    c = np.unique(rng.integers(0, 1 << 64, size=513, dtype=U64, endpoint=False))
    return a, b, c


@pytest.mark.parametrize("case", ["one run", "duplicates", "an empty run", "unsorted blocks across a run", "all 64 bits"])
def test_union_equals_the_raw_union_packed(hip, case):  # noqa: F811
    H = hip.hip
    a, b, c = union_inputs()
    runs = {"one run": [[a]], "duplicates": [[a], [a[100:900]], [b], [np.sort(np.concatenate([b[:50], a[:7]]))]], "an empty run": [[a], [], [b]],
            "unsorted blocks across a run": [[b[600:], a, b[:600]], [a[::2]]],  # a target's files as the one run they are: no order among them
            "all 64 bits": [[c], [np.array([0, 1 << 63, M64], dtype=U64)], [a[:5]]]}[case]
    flat = [np.concatenate([np.asarray(v, dtype=U64) for v in files]) if files else np.zeros(0, U64) for files in runs]
    want = H.hashes_union([np.sort(x) for x in flat])
    assert np.array_equal(want, np.unique(np.concatenate(flat)))
    blocks, payload = pack(hip, [want])
    packed = [pack(hip, files) for files in runs]
    n, got_blocks, got_words = H.packed_union(packed)
    assert n == len(want) and np.array_equal(got_blocks, blocks) and np.array_equal(got_words, payload), "word for word the encoding of the raw union"
    assert H.packed_union(packed, size_only=True) == (len(want), len(blocks), len(payload))
    with pytest.raises(hip.GanonHipError) as e:  # a buffer too small: the sizes, and nothing written
        H.packed_union(packed, cap_blocks=len(blocks) - 1)
    assert e.value.code == GN_EOVERFLOW and e.value.sizes == (len(want), len(blocks), len(payload)) and not e.value.written
    if len(payload):
        with pytest.raises(hip.GanonHipError) as e:
            H.packed_union(packed, cap_words=len(payload) - 1)
        assert e.value.code == GN_EOVERFLOW and e.value.sizes == (len(want), len(blocks), len(payload)) and not e.value.written


def test_union_refusals_and_nothing_to_unite(hip):  # noqa: F811
    H = hip.hip
    a, _, _ = union_inputs()
    run = pack(hip, [a])
    assert H.packed_union([])[0] == 0 and H.packed_union([pack(hip, [])], size_only=True) == (0, 0, 0)
    for what, field, value in (("cnt 0", "cnt", 0), ("cnt 513", "cnt", 513), ("width 65", "width", 65)):
        blocks = run[0].copy()
        blocks[field][1] = value
        with pytest.raises(hip.GanonHipError) as e:
            H.packed_union([(blocks, run[1])])
        assert e.value.code == GN_EINVAL, what
    with pytest.raises(hip.GanonHipError) as e:
        H.packed_union([(run[0], None)])
    assert e.value.code == GN_EINVAL, "payload words without a payload"
    L = hip.load_library()
    n = C.c_uint64(0)
    assert L.gn_packed_union(0, None, None, None, 1, None, 0, None, 0, C.byref(n), C.byref(n), C.byref(n)) == GN_EINVAL
    assert L.gn_packed_union(0, None, None, None, 0, None, 0, None, 0, None, C.byref(n), C.byref(n)) == GN_EINVAL


# ------------------------------------------------------------------------------------------------------------ the ABI: the sketches
def tiled(hip, n, step):  # noqa: F811
    """the set {0, step, 2 * step, ...} of n hashes and its packed form without a Python loop over the hashes: every full block has the
    deltas of the first, so the restated format's encoding of one block is tiled, and the tail is encoded on its own"""
    v = np.arange(n, dtype=U64) * U64(step)
    full = n // 512
    (_, _, _, width), = encode([v[:512]])[0]
    one = np.array(encode([v[:512]])[1], dtype=U64)
    blocks = np.zeros(full + (1 if n % 512 else 0), dtype=hip.hip.PACKED_BLOCK_DTYPE)
    blocks["first"][:full], blocks["word_at"][:full] = v[:full * 512:512], np.arange(full, dtype=U64) * U64(len(one))
    blocks["cnt"][:full], blocks["width"][:full] = 512, width
    payload = np.tile(one, full)
    if n % 512:
        (first, _, cnt, w), = encode([v[full * 512:]])[0]
        blocks[full] = (first, len(payload), cnt, w)
        payload = np.concatenate([payload, np.array(encode([v[full * 512:]])[1], dtype=U64)])
    return v, (blocks, payload)


def test_sketches_equal_those_of_the_raw_sets(hip):  # noqa: F811
    H = hip.hip
    rng = np.random.default_rng(51)
    sets = [np.zeros(0, U64), np.array([12345], dtype=U64), np.unique(rng.integers(0, 1 << 38, size=600, dtype=U64))[:512],
            np.unique(rng.integers(0, 1 << 64, size=600, dtype=U64, endpoint=False))[:513], np.unique(rng.integers(0, 1 << 38, size=20000, dtype=U64))]
    assert [len(s) for s in sets[:4]] == [0, 1, 512, 513] and len(sets[4]) > 8192 + 512, "a set over one sketch chunk"
    runs = [pack(hip, [s] if len(s) else []) for s in sets]
    runs[4] = pack(hip, [sets[4][:700], sets[4][700:]])  # (a short block in the middle)
    big, big_run = tiled(hip, (8 << 20) + 1000, 3)      # a set over one round of 8 Mi hashes, cut by the round's end
    sets.append(big), runs.append(big_run)
    sets.append(sets[2]), runs.append(runs[2])          # (and a small set behind the cut one)
    raw, packed = H.HipSketches(sets), H.HipSketches.from_packed(runs)
    a, b = raw.download(), packed.download()
    assert a.shape == b.shape == (len(sets), H.SKETCH_M) and a.tobytes() == b.tobytes(), np.nonzero((a != b).any(axis=1))[0]
    assert not b[0].any() and b[1].any() and np.array_equal(b[2], b[6])
    order = np.array([4, 2, 6, 0, 3, 5, 1], dtype=np.uint32)
    assert np.array_equal(raw.union_table(order, 4), packed.union_table(order, 4))
    raw.free(), packed.free()
    with pytest.raises(hip.GanonHipError) as e:
        blocks = runs[4][0].copy()
        blocks["cnt"][1] = 0
        H.HipSketches.from_packed([(blocks, runs[4][1])])
    assert e.value.code == GN_EINVAL


# ------------------------------------------------------------------------------------------------------------ the binary
_FIGURES = {}


def figures(inp, which):
    """what the `hibf hash sets:` line and a pass over packed sets have to say, from the restated encoding of the united sets: (hashes, bytes
    held, bytes a pass uploads, targets of several files)"""
    if which not in _FIGURES:
        enc = [encode([s]) for s in inp.sets(0)[1]]
        n_blocks, n_words = sum(len(b) for b, _ in enc), sum(len(w) for _, w in enc)
        files = {}
        for ln in open(inp.tsv):
            f, t = ln.rstrip("\n").split("\t")
            files[t] = files.get(t, 0) + 1
        _FIGURES[which] = (sum(len(s) for s in inp.sets(0)[1]), 8 * n_words + BLOCK_BYTES * n_blocks, 8 * n_words + ITEM_BYTES * n_blocks,
                           sum(1 for t in inp.sets(0)[0] if files[t] > 1))
    return _FIGURES[which]


def no_spill(folder):
    return not [f for f in os.listdir(folder) if ".hashsets." in f]


def sets_line(stderr):
    got = re.findall(r"^hibf hash sets: (\d+) hashes held (\w+) in (\d+) bytes, (\d+) targets united$", stderr, re.M)
    assert len(got) == 1, stderr
    return (int(got[0][0]), got[0][1], int(got[0][2]), int(got[0][3]))


@pytest.mark.parametrize("mode", ["packed", "spilled"])
@pytest.mark.parametrize("which", ["genomes", "short200"])
def test_one_pass_and_parts_write_the_raw_builds_file(hip, request, tmp_path_factory, which, mode):  # noqa: F811
    inp, one, ibfs, _ = one_pass(hip, request, tmp_path_factory, which)
    tmax, s, max_fp = INPUTS[which]
    hashes, held, pass_bytes, united = figures(inp, which)
    if which == "short200":
        assert united == 23
    out = beside(one, f"{mode}.hibf")
    p = build(inp, out, tmax, s, max_fp, extra=("--verbose", "--hibf-hash-sets", mode))
    assert filecmp.cmp(out, one, shallow=False), "byte for byte the raw build's file"
    assert sets_line(p.stderr) == (hashes, mode, held, united)
    assert f"filled in 1 part, {pass_bytes} hash bytes uploaded" in p.stderr and f"--hibf-hash-sets    {mode}" in p.stderr
    assert no_spill(os.path.dirname(one))
    if mode == "spilled":
        check_file(out, inp, tmax, s, max_fp, 0)
    for kind in ("three", "two"):
        budget = budget_of(ibfs, kind)
        out = beside(one, f"{mode}_{kind}.hibf")
        p = build(inp, out, tmax, s, max_fp, extra=("--verbose", "--hibf-memory", str(budget), "--hibf-hash-sets", mode))
        check_parts(p.stderr, ibfs, budget, 1, pass_bytes)
        assert filecmp.cmp(out, one, shallow=False), kind
        assert sets_line(p.stderr) == (hashes, mode, held, united) and no_spill(os.path.dirname(one))


@pytest.mark.parametrize("mode", ["packed", "spilled"])
def test_parts_dealt_to_a_list(hip, request, tmp_path_factory, mode):  # noqa: F811
    inp, one, ibfs, _ = one_pass(hip, request, tmp_path_factory, "short200")
    tmax, s, max_fp = INPUTS["short200"]
    budget = budget_of(ibfs, "three")
    out = beside(one, f"{mode}_list.hibf")
    p = build(inp, out, tmax, s, max_fp, extra=("--verbose", "--hibf-memory", str(budget), "--hibf-devices", "0,0", "--hibf-hash-sets", mode))
    want = check_parts(p.stderr, ibfs, budget, 2, figures(inp, "short200")[2])
    assert len(want) > 3 and filecmp.cmp(out, one, shallow=False) and no_spill(os.path.dirname(one))


@pytest.mark.parametrize("layout", ["sketch", "similarity"])
@pytest.mark.parametrize("which", ["genomes", "short200"])
def test_layouts(hip, request, tmp_path_factory, which, layout):  # noqa: F811
    inp, one, _, _ = one_pass(hip, request, tmp_path_factory, which)
    tmax, s, max_fp = INPUTS[which]
    raw = beside(one, f"raw_{layout}.hibf")
    build(inp, raw, tmax, s, max_fp, extra=("--layout", layout))
    for mode in ("packed", "spilled"):
        out = beside(one, f"{mode}_{layout}.hibf")
        build(inp, out, tmax, s, max_fp, extra=("--layout", layout, "--hibf-hash-sets", mode))
        assert filecmp.cmp(out, raw, shallow=False), (mode, "the same sketches, the same tree, the same file")
    assert no_spill(os.path.dirname(one))


def test_raw_is_the_command_of_before(hip, request, tmp_path_factory):  # noqa: F811
    inp, one, _, _ = one_pass(hip, request, tmp_path_factory, "short200")
    tmax, s, max_fp = INPUTS["short200"]
    errs = []
    for tag, extra in (("before", ()), ("raw", ("--hibf-hash-sets", "raw"))):
        out = beside(one, f"said_{tag}.hibf")
        p = build(inp, out, tmax, s, max_fp, extra=("--verbose",) + extra)
        assert filecmp.cmp(out, one, shallow=False) and p.stdout == ""
        errs.append(re.sub(r"[0-9][0-9.e+:-]*", "#", p.stderr.replace(out, "OUT").replace("--hibf-hash-sets    raw\n", "")))
    assert errs[0] == errs[1] and "hibf hash sets:" not in errs[0]


def test_a_failing_spilled_run_leaves_no_file(hip, request, tmp_path_factory, tmp_path):  # noqa: F811
    inp, one, _, _ = one_pass(hip, request, tmp_path_factory, "short200")
    tmax, s, max_fp = INPUTS["short200"]
    plain = str(tmp_path / "plain")
    open(plain, "w").write("no folder\n")
    out = str(tmp_path / "none.hibf")
    p = build(inp, out, tmax, s, max_fp, extra=("--hibf-hash-sets", "spilled", "--tmp-output-folder", plain), expect=1)
    assert "cannot create" in p.stderr and not os.path.exists(out)
    assert sorted(os.listdir(str(tmp_path))) == ["plain"] and no_spill(str(tmp_path)) and no_spill(os.path.dirname(one))


def test_classify_on_the_file_built_from_packed_sets(hip, request, tmp_path_factory, tmp_path):  # noqa: F811
    inp, one, ibfs, _ = one_pass(hip, request, tmp_path_factory, "short200")
    tmax, s, max_fp = INPUTS["short200"]
    out = beside(one, "packed_classify.hibf")
    build(inp, out, tmax, s, max_fp, extra=("--hibf-hash-sets", "packed"))
    assert filecmp.cmp(out, one, shallow=False)
    fq = str(tmp_path / "reads.fq")
    gf.write_fastq(fq, [(rid, seq) for rid, seq, _ in cut_reads(inp, 0, np.random.default_rng(8), per_target=1, n_random=20)])
    outs = []
    for tag, index in (("packed", out), ("raw", one)):
        prefix = str(tmp_path / tag)
        cu.run(cu.BIN_HIP, ["--ibf", index, "--hibf", "--single-reads", fq, "-o", prefix, "--output-all", "--skip-lca", "--rel-cutoff", "1", "--rel-filter", "1",
                            "--quiet"])
        outs.append((open(prefix + ".all", "rb").read(), open(prefix + ".rep", "rb").read()))
    assert outs[0] == outs[1] and outs[0][0]
