"""Shapes, read sets and a definitional reference for the minimiser sweep (test_minimiser_reference_cpu.py checks the
oracle and the inputs here, test_gpu_minimiser_sweep.py runs them through the library).  Everything is deterministic.

The device has four implementations behind one dispatch (gn_capi.hip gn_run_minimisers_range, gn_minimiser_lpr.hip
gn_launch_minimiser_lpr), K = w - k + 1 k-mers per window:
  A  gn_minimiser_lprk_kernel<KW, FMIN>   K <= 16 and k <= 24, both mates <= 640 bases (FMIN for k <= 20)
  B  gn_minimiser_lpr_kernel              K <= 65 otherwise, both mates <= 640 bases
  C  gn_mate_minimisers_fast              K <= 65, a mate > 640 bases (the list A or B deferred)
  D  gn_mate_minimisers                   K = 66..448, every read
"""
from __future__ import annotations

import functools
from typing import List, NamedTuple, Tuple

import numpy as np

LPR_MAX_LEN = 640   # a read with a longer mate leaves the lane-per-read kernels (A, B) for the wave-per-read one (C)
LPRK_STAGE = 24     # path A stages this many emissions per mate in LDS and stores further ones directly
SEED = 0x8F3F73B5CF1C9ADE


class Shape(NamedTuple):
    k: int
    w: int
    path: str   # the implementation reads of at most LPR_MAX_LEN bases must reach: "A" (k <= 20), "Ai" (integer minimum), "B", "D"

    @property
    def K(self) -> int:
        return self.w - self.k + 1

    @property
    def id(self) -> str:
        return f"{self.path}-k{self.k}-w{self.w}"


def dispatch_path(k: int, w: int) -> str:
    """the dispatch as the library's sources state it"""
    K = w - k + 1
    if K <= 16 and k <= 24:
        return "A" if k <= 20 else "Ai"
    return "B" if K <= 65 else "D"


def _shapes() -> List[Shape]:
    kw = [(k, k + KW - 1) for k in (20, 21) for KW in range(1, 17)]            # every instantiation, float and integer minimum
    kw += [(k, k + KW - 1) for k in (24, 1) for KW in (1, 8, 16)]              # the ends of path A's k range
    kw += [(25, 25), (25, 40), (19, 35), (19, 82), (19, 83), (32, 32), (32, 33), (32, 96)]   # B: k > 24, K = 17, 64, 65, k = 32
    kw += [(19, 84), (8, 136), (32, 479), (1, 448)]                            # D: K = 66, 129, 448
    return [Shape(k, w, dispatch_path(k, w)) for k, w in kw]


SHAPES = _shapes()
# one shape each from A-integer, B and D for the read-range (chunked) runs
RANGE_SHAPES = [s for s in SHAPES if (s.k, s.w) in ((21, 28), (25, 40), (19, 84))]


def dna4_rank_table() -> np.ndarray:
    """seqan3::dna4 assign_char for every byte: ACGT, U as T, the IUPAC codes as their first letter, either case; else A"""
    t = np.zeros(256, dtype=np.uint8)
    for letters, rank in (("CYSB", 1), ("GK", 2), ("TU", 3)):
        for c in letters:
            t[ord(c)] = t[ord(c.lower())] = rank
    return t


_RANKS = dna4_rank_table()


def to_ranks(seq: bytes) -> np.ndarray:
    return _RANKS[np.frombuffer(seq, dtype=np.uint8)]


def canonical_values(ranks: np.ndarray, k: int) -> np.ndarray:
    """min(fwd ^ seed, rc ^ seed) of every k-mer: fwd reads the ranks as base-4 digits, first base highest; rc reads the
    complements (3 - rank) with the LAST base highest; seed = SEED >> (64 - 2k)"""
    r = np.asarray(ranks, dtype=np.uint64)
    M = len(r) - k + 1
    fwd = np.zeros(M, dtype=np.uint64)
    rc = np.zeros(M, dtype=np.uint64)
    for j in range(k):
        d = r[j:j + M]
        fwd |= d << np.uint64(2 * (k - 1 - j))
        rc |= (np.uint64(3) - d) << np.uint64(2 * j)
    seed = np.uint64(SEED >> (64 - 2 * k))
    return np.minimum(fwd ^ seed, rc ^ seed)


def brute_minimisers(ranks: np.ndarray, k: int, w: int, leftmost_tie: bool = False, entering_le: bool = False,
                     drop_repeats: bool = False) -> np.ndarray:
    """seqan3::views::minimiser_hash from its definition, O(L * K): the first window emits its rightmost minimum; on each
    slide, if the remembered position has left the window, the window's rightmost minimum is recomputed and emitted,
    else the entering value is emitted (and remembered) if it is strictly smaller.
    The three switches are WRONG variants (leftmost minimum on ties / entering value emitted when equal too / an emission
    equal to the one before it dropped); they exist to prove that a read set tells them apart."""
    L = len(ranks)
    if L < w:
        return np.zeros(0, dtype=np.uint64)
    K = w - k + 1
    v = canonical_values(ranks, k)
    win = np.lib.stride_tricks.sliding_window_view(v, K)           # [windows, K]
    if leftmost_tie:
        arg = np.argmin(win, axis=1)
    else:
        arg = K - 1 - np.argmin(win[:, ::-1], axis=1)
    wpos = (arg + np.arange(len(win))).tolist()                    # absolute position of every window's minimum
    vl = v.tolist()
    pos = wpos[0]
    m = vl[pos]
    out = [m]
    for j in range(1, len(wpos)):
        e = vl[j + K - 1]
        if pos < j:
            pos = wpos[j]
            m = vl[pos]
            out.append(m)
        elif e < m or (entering_le and e == m):
            pos, m = j + K - 1, e
            out.append(m)
    if drop_repeats:
        out = [x for i, x in enumerate(out) if i == 0 or x != out[i - 1]]
    return np.array(out, dtype=np.uint64)


WRONG_VARIANTS = ("leftmost_tie", "entering_le", "drop_repeats")


def deferred(len1: int, len2: int = 0) -> bool:
    """the read leaves paths A / B for path C (for a D shape it only names the length class)"""
    return len1 > LPR_MAX_LEN or len2 > LPR_MAX_LEN


def _rand(rng, n: int, alphabet: bytes = b"ACGT") -> bytes:
    return bytes(np.frombuffer(alphabet, dtype=np.uint8)[rng.integers(0, len(alphabet), size=n)])


def _periodic(unit: bytes, n: int) -> bytes:
    return (unit * (n // len(unit) + 1))[:n]


def _repeat_maker(rng, k: int, w: int, n: int) -> bytes:
    """A read of period K whose smallest k-mer value sits near the start of the first window: that minimiser leaves after
    a few slides and the same VALUE comes back as the next window's minimum, so a repeated emission exists within a few
    windows -- `A...` needs K slides for one, which reads of at most LPR_MAX_LEN bases do not have when w + K > 640."""
    K = w - k + 1
    best = None
    for unit in (_rand(rng, K), b"C" + b"A" * (K - 1), b"A" + b"C" * (K - 1)):
        v = canonical_values(to_ranks(_periodic(unit, K + k - 1)), k)       # one period of values
        at = np.nonzero(v == v.min())[0]
        for a in at.tolist():                                               # rotate occurrence a to the front
            q = int(((at - a) % K).max())                                   # then the window's rightmost minimum is at q
            if best is None or q < best[0]:
                best = (q, unit[a:] + unit[:a])
    return _periodic(best[1], n)


def _tie_makers(rng, k: int, w: int, n: int) -> List[bytes]:
    return [b"A" * n, b"T" * n, _periodic(b"AC", n), _periodic(b"ACGT", n), _rand(rng, n, b"AG"), _repeat_maker(rng, k, w, n)]


def uniform_len(k: int, w: int) -> int:
    return min(LPR_MAX_LEN, max(150, w + (w - k + 1) + 5))


@functools.lru_cache(maxsize=None)
def single_reads(k: int, w: int) -> Tuple[bytes, ...]:
    rng = np.random.default_rng(100_000 + 1000 * k + w)
    K = w - k + 1
    U = uniform_len(k, w)
    seqs = [_rand(rng, U) for _ in range(64)]                   # a whole wave inside its reads: the unpredicated blocks
    seqs += [_rand(rng, LPR_MAX_LEN) for _ in range(64)]        # the longest reads the lane-per-read kernels take
    blk = [_rand(rng, U) for _ in range(64)]                    # one lane too short, one of exactly one window
    blk[17], blk[41] = _rand(rng, max(w - 1, 0)), _rand(rng, w)
    seqs += blk
    for n in (0, 1, k - 1, k, w - 1, w, w + 1, w + K - 1, w + K, 2 * w, 639, 640, 641, 1000, 5000):
        seqs.append(_rand(rng, n))
    if K == 1:
        seqs += [_rand(rng, k + LPRK_STAGE - 1), _rand(rng, k + LPRK_STAGE)]   # exactly 24 and 25 emissions
    tie = w + 3 * K + 7
    seqs += _tie_makers(rng, k, w, min(LPR_MAX_LEN, tie))
    seqs += _tie_makers(rng, k, w, tie + LPR_MAX_LEN)
    seqs.append(_rand(rng, 300, b"ACGTNRYKMSWBDHVUacgtnrykmswbdhvu"))
    every = bytes(range(256))
    seqs += [every * 2, every[::-1] * 3]                        # every byte value, below and above LPR_MAX_LEN
    seqs += [bytes(rng.integers(0, 256, size=n, dtype=np.uint8)) for n in (w, 150, 333, 640, 641, 1500)]
    seqs += [_rand(rng, int(rng.integers(0, 701))) for _ in range(370)]
    if len(seqs) % 64 == 0:
        seqs.append(_rand(rng, U))
    return tuple(seqs)


@functools.lru_cache(maxsize=None)
def paired_reads(k: int, w: int) -> Tuple[Tuple[bytes, ...], Tuple[bytes, ...]]:
    rng = np.random.default_rng(200_000 + 1000 * k + w)
    K = w - k + 1
    U = uniform_len(k, w)
    lens = [(U, U)] * 64                                        # a uniform wave in both mates
    lens += [(w - 1, U), (w - 1, 641), (0, U), (k - 1, w)]      # mate 1 < w: skipped whatever mate 2 is
    lens += [(U, w - 1), (U, 0), (641, w - 1), (w, k - 1)]      # mate 2 < w: it contributes nothing
    lens += [(100, 641), (641, 100), (max(100, w), 641), (641, max(100, w)), (640, 1000), (2000, 640)]   # deferred by one mate alone
    lens += [(640, 640)] * 6 + [(640, U), (U, 640), (639, 640)]   # both at the limit: more than LPRK_STAGE emissions each on path A
    lens += [(w, w), (w + 5, w + 5), (w + 1, w + K), (640, w + 5), (w + 5, 640)]   # few emissions in both mates, in one
    if K == 1:
        lens += [(k + LPRK_STAGE - 1, k + LPRK_STAGE), (k + LPRK_STAGE, k + LPRK_STAGE - 1)]
    s1 = [_rand(rng, max(a, 0)) for a, _ in lens]
    s2 = [_rand(rng, max(b, 0)) for _, b in lens]
    tie = w + 3 * K + 7
    for n in (min(LPR_MAX_LEN, tie), tie + LPR_MAX_LEN):        # tie makers in mate 2
        t = _tie_makers(rng, k, w, n)
        s2 += t
        s1 += [_rand(rng, U) for _ in t]
    every = bytes(range(256))
    s1 += [_rand(rng, U), every * 2]
    s2 += [every * 2, bytes(rng.integers(0, 256, size=641, dtype=np.uint8))]
    for _ in range(150):
        s1.append(_rand(rng, int(rng.integers(0, 701))))
        s2.append(_rand(rng, int(rng.integers(0, 701))))
    if len(s1) % 64 == 0:
        s1.append(_rand(rng, U))
        s2.append(_rand(rng, U))
    return tuple(s1), tuple(s2)
