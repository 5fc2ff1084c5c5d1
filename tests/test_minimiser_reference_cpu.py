"""The reference side of the minimiser sweep, on the CPU: the oracle's minimiser_hash equals a brute force written from the
definition on every shape and read of tests/minimiser_cases.py, and those read sets can tell a subtly wrong kernel from
a right one (conditions on the inputs, checked here so that the GPU sweep's "equal to the oracle" means something)."""
import numpy as np
import pytest

import minimiser_cases as mc
import oracle

# seqan3::dna4 assign_char, byte by byte: rows of 16, 0x40 = "@ABCDEFGHIJKLMNO", 0x50 = "PQRSTUVWXYZ[\]^_", the lower-case
# rows the same.  C Y S B -> 1, G K -> 2, T U -> 3, every other byte (the IUPAC codes that start with A included) -> 0.
DNA4_RANK = "".join([
    "0000000000000000", "0000000000000000", "0000000000000000", "0000000000000000",
    "0011000200020000", "0001330001000000", "0011000200020000", "0001330001000000",
    "0000000000000000", "0000000000000000", "0000000000000000", "0000000000000000",
    "0000000000000000", "0000000000000000", "0000000000000000", "0000000000000000"])

IDS = [s.id for s in mc.SHAPES]


def test_shape_list_covers_the_dispatch():
    assert len(mc.SHAPES) == len({(s.k, s.w) for s in mc.SHAPES}) == 50
    for s in mc.SHAPES:
        assert s.path == mc.dispatch_path(s.k, s.w) and 1 <= s.k <= 32 and 1 <= s.K <= 448
    for k in (20, 21):    # every instantiation of path A in its float and its integer form
        assert {s.K for s in mc.SHAPES if s.k == k and s.path in ("A", "Ai")} == set(range(1, 17))
    assert {s.path for s in mc.SHAPES if s.k == 20} == {"A"} and {s.path for s in mc.SHAPES if s.k == 21} == {"Ai"}
    assert [(s.k, s.w, s.path) for s in mc.RANGE_SHAPES] == [(21, 28, "Ai"), (25, 40, "B"), (19, 84, "D")]


def test_rank_tables_agree_on_every_byte():
    lit = np.array([int(c) for c in DNA4_RANK], dtype=np.uint8)
    assert len(lit) == 256
    assert np.array_equal(oracle.rank_lut(), lit)
    assert np.array_equal(mc.dna4_rank_table(), lit)


def test_brute_force_on_a_documented_example():
    # the sequence of seqan3's minimiser_hash documentation (tests/test_oracle_kat.py pins the oracle on the reference's vectors)
    r = mc.to_ranks(b"ACGTCGACGTTTAG")
    assert np.array_equal(mc.brute_minimisers(r, 4, 8), oracle.minimiser_hash(r, 4, 8))
    assert len(mc.brute_minimisers(r, 4, 15)) == 0 and len(mc.brute_minimisers(r, 4, 14)) == 1


def _streams(k, w, seq, **variant):
    return mc.brute_minimisers(mc.to_ranks(seq), k, w, **variant)


@pytest.mark.parametrize("shape", mc.SHAPES, ids=IDS)
def test_oracle_equals_brute_force(shape):
    k, w = shape.k, shape.w
    s1, s2 = mc.paired_reads(k, w)
    for name, seqs in (("single", mc.single_reads(k, w)), ("mate1", s1), ("mate2", s2)):
        for i, s in enumerate(seqs):
            got = oracle.minimiser_hash(oracle.to_ranks(s), k, w)
            exp = _streams(k, w, s)
            assert np.array_equal(got, exp), (name, i, len(s))
            assert len(exp) == 0 if len(s) < w else 1 <= len(exp) <= len(s) - w + 1


@pytest.mark.parametrize("shape", mc.SHAPES, ids=IDS)
def test_read_sets_discriminate(shape):
    k, w, K = shape.k, shape.w, shape.K
    single = mc.single_reads(k, w)
    s1, s2 = mc.paired_reads(k, w)
    assert len(single) % 64 and len(s1) % 64 and len(s1) == len(s2)
    assert 550 <= len(single) <= 650 and 230 <= len(s1) <= 290

    # a wave-aligned block of one length, one at the limit, one with a lane below w and a lane of one window
    U = mc.uniform_len(k, w)
    assert {len(s) for s in single[0:64]} == {U} and {len(s) for s in single[64:128]} == {mc.LPR_MAX_LEN}
    assert sorted({len(s) for s in single[128:192]}) == sorted({w - 1, w, U})
    assert {(len(a), len(b)) for a, b in zip(s1[:64], s2[:64])} == {(U, U)}

    # deferred and not, single and paired; a pair deferred by its second mate alone and one by its first alone
    assert any(mc.deferred(len(s)) for s in single) and any(w <= len(s) <= mc.LPR_MAX_LEN for s in single)
    pl = [(len(a), len(b)) for a, b in zip(s1, s2)]
    assert any(w <= a <= 640 < b for a, b in pl) and any(w <= b <= 640 < a for a, b in pl)
    assert any(a < w <= b for a, b in pl) and any(b < w <= a for a, b in pl) and (640, 640) in pl

    # each wrong variant changes at least one read the lane-per-read kernels take and one they defer
    variants = mc.WRONG_VARIANTS if K > 1 else ("drop_repeats",)
    pools = {"single": single, "mate2": s2}
    for var in variants:
        for pname, pool in pools.items():
            for long_read in (False, True):
                hit = False
                for s in pool:
                    if len(s) < w or (len(s) > mc.LPR_MAX_LEN) != long_read:
                        continue
                    if not np.array_equal(_streams(k, w, s), _streams(k, w, s, **{var: True})):
                        hit = True
                        break
                assert hit, (var, pname, "> 640" if long_read else "<= 640")

    # path A: both sides of the staging limit, single reads and each mate of non-deferred pairs
    if shape.path in ("A", "Ai"):
        n_single = [len(_streams(k, w, s)) for s in single if w <= len(s) <= mc.LPR_MAX_LEN]
        assert max(n_single) > mc.LPRK_STAGE and min(n_single) <= mc.LPRK_STAGE
        both = [(len(_streams(k, w, a)), len(_streams(k, w, b))) for a, b in zip(s1, s2)
                if w <= len(a) <= mc.LPR_MAX_LEN and w <= len(b) <= mc.LPR_MAX_LEN]
        assert any(a > mc.LPRK_STAGE and b > mc.LPRK_STAGE for a, b in both)
        assert any(a <= mc.LPRK_STAGE and b <= mc.LPRK_STAGE for a, b in both)
        assert any(a > mc.LPRK_STAGE >= b for a, b in both) and any(b > mc.LPRK_STAGE >= a for a, b in both)
        if K == 1:
            assert mc.LPRK_STAGE in n_single and mc.LPRK_STAGE + 1 in n_single
            assert (mc.LPRK_STAGE, mc.LPRK_STAGE + 1) in both and (mc.LPRK_STAGE + 1, mc.LPRK_STAGE) in both
