"""Helpers of the subtree-partition tests: the plan of ganon_amd/host/hibf_partition.hpp restated in Python (units, costs, an exact
optimum by dynamic programming, the part-local trees), the fixtures with permuted user-bin ids, and reads cut from planted sequences."""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

import ganon_fixtures as gf
import oracle


def stride_words(w: int) -> int:
    """gn_hibf_row_stride_words: rows of an HIBF's IBFs are padded to whole 128-byte lines on the device"""
    if w >= 16:
        return (w + 15) & ~15
    p = 1
    while p < w:
        p <<= 1
    return p


def ibf_bytes(h: oracle.Hibf, i: int) -> int:
    f = h.ibfs[i]
    return f.bin_size * stride_words((f.bins + 63) >> 6) * 8


def units_of(h: oracle.Hibf) -> List[Tuple[int, int, List[int]]]:
    """(bin_lo, bin_hi, IBFs below) per maximal inseparable piece of the root: a (split) user bin's run, or one merged bin"""
    b2u, nxt = h.bin_to_user, h.next_ibf_id
    B, out, b = h.ibfs[0].bins, [], 0
    while b < B:
        u = int(b2u[0][b])
        if u >= 0:
            e = b + 1
            while e < B and int(b2u[0][e]) == u:
                e += 1
            out.append((b, e, []))
            b = e
            continue
        below, todo = [], [int(nxt[0][b])]
        while todo:
            i = todo.pop()
            below.append(i)
            todo += [int(nxt[i][t]) for t in range(h.ibfs[i].bins) if int(b2u[i][t]) < 0]
        out.append((b, b + 1, sorted(below)))
        b += 1
    return out


def cost_matrix(h: oracle.Hibf, units) -> np.ndarray:
    """C[a, b] = device bytes of a part of units [a, b) (b > a): its subtrees + words [bin_lo // 64, ceil(bin_hi / 64)) of the root"""
    U = len(units)
    pre = np.zeros(U + 1, dtype=np.int64)
    pre[1:] = np.cumsum([sum(ibf_bytes(h, i) for i in u[2]) for u in units])
    wl = np.array([u[0] >> 6 for u in units], dtype=np.int64)
    wh = np.array([(u[1] + 63) >> 6 for u in units], dtype=np.int64)
    C = np.full((U + 1, U + 1), np.iinfo(np.int64).max, dtype=np.int64)
    rows = h.ibfs[0].bin_size
    for a in range(U):
        w = wh[a:] - wl[a]
        C[a, a + 1:] = pre[a + 1:] - pre[a] + rows * 8 * np.array([stride_words(int(x)) for x in w], dtype=np.int64)
    return C


def optimum(C: np.ndarray, budgets: Sequence[int]) -> Optional[int]:
    """the smallest possible largest part when contiguous unit ranges go to the budgets in order (a budget may stay empty), each part
    within its budget; None when nothing fits.  Exact: dynamic programming over (budget, units placed)."""
    U = C.shape[0] - 1
    INF = np.iinfo(np.int64).max
    best = np.full(U + 1, INF, dtype=np.int64)
    best[0] = 0
    for bud in budgets:
        ok = np.where(C <= bud, C, INF)  # [i, j]
        cand = np.maximum(best[:, None], ok)  # part [i, j) on this budget after best[i]
        best = np.minimum(best, cand.min(axis=0))
    return None if best[U] == INF else int(best[U])


def build_part(h: oracle.Hibf, units, a: int, b: int) -> dict:
    """the tree of a part that owns units [a, b): local numbering, absent bins (-1 / -1) in the root's boundary words"""
    b2u, nxt = h.bin_to_user, h.next_ibf_id
    B = h.ibfs[0].bins
    bin_lo, bin_hi = units[a][0], units[b - 1][1]
    wl, wh = bin_lo >> 6, (bin_hi + 63) >> 6
    ibf_global = [0] + sorted(i for u in units[a:b] for i in u[2])
    users = set()
    for g in ibf_global:
        span = range(bin_lo, bin_hi) if g == 0 else range(h.ibfs[g].bins)
        users |= {int(b2u[g][t]) for t in span if int(b2u[g][t]) >= 0}
    user_global = sorted(users)
    ul = {u: i for i, u in enumerate(user_global)}
    il = {g: i for i, g in enumerate(ibf_global)}
    shapes, nx_l, bu_l = [], [], []
    for g in ibf_global:
        f = h.ibfs[g]
        if g == 0:
            first, last = wl * 64, min(B, wh * 64)
            nx, bu = [-1] * (last - first), [-1] * (last - first)
            for t in range(bin_lo, bin_hi):
                u = int(b2u[0][t])
                bu[t - first] = ul[u] if u >= 0 else -1
                nx[t - first] = 0 if u >= 0 else il[int(nxt[0][t])]
            shapes.append((last - first, f.bin_size, f.hash_funs))
        else:
            nx, bu = [], []
            for t in range(f.bins):
                u = int(b2u[g][t])
                bu.append(ul[u] if u >= 0 else -1)
                nx.append(il[g] if u >= 0 else il[int(nxt[g][t])])
            shapes.append((f.bins, f.bin_size, f.hash_funs))
        nx_l.append(nx)
        bu_l.append(bu)
    return dict(bin_lo=bin_lo, bin_hi=bin_hi, word_lo=wl, word_hi=wh, ibf_global=ibf_global, user_global=user_global, shapes=shapes,
                next_ibf_id=nx_l, bin_to_user=bu_l)


def permuted(h: oracle.Hibf, seed: int) -> Tuple[oracle.Hibf, np.ndarray]:
    """the same tree with its user-bin ids permuted (the fixture numbers them subtree by subtree; a real layout sorts user bins by
    size, so every subtree holds ids from all over the range); -> (tree, perm) with new id = perm[old id]"""
    perm = np.random.default_rng(seed).permutation(h.n_user_bins).astype(np.int64)
    b2u = [np.where(a >= 0, perm[np.maximum(a, 0)], a) for a in h.bin_to_user]
    return oracle.Hibf(h.ibfs, h.next_ibf_id, b2u, h.n_user_bins), perm


def interleaves(parts: Sequence[dict]) -> bool:
    """some part's global user-bin ids lie between another's: a concatenation of the parts' results would not be sorted"""
    for i, p in enumerate(parts):
        for q in parts[i + 1:]:
            if p["user_global"] and q["user_global"] and min(q["user_global"]) < max(p["user_global"]) and min(p["user_global"]) < max(q["user_global"]):
                return True
    return False


K, W = 19, 31


def revcomp(s):
    """reverse complement of a read (bytes or str): the mate of a pair that hits what the read hits"""
    return s[::-1].translate(bytes.maketrans(b"ACGT", b"TGCA") if isinstance(s, bytes) else str.maketrans("ACGT", "TGCA"))


def planted_fixture(n_user_bins: int, tmax: int, seed: int, hash_funs: int = 3, n_planted: int = 60, n_random: int = 30, read_len: int = 120, density: float = 0.3):
    """-> (tree with permuted ids, read strings, sequence per user bin): user bins with sequences of their own emplaced along their
    paths, reads cut from some of them -- one from every user bin that is split over three bins of the root -- plus random reads"""
    rng = np.random.default_rng(seed)
    seqs0 = {ub: bytes(rng.choice(list(b"ACGT"), size=400).astype(np.uint8)) for ub in range(n_user_bins)}
    uh = {ub: np.unique(oracle.minimiser_hash(oracle.to_ranks(s), K, W)) for ub, s in seqs0.items()}
    h0 = gf.random_hibf(n_user_bins, tmax, 3, seed=seed, density=density, hash_funs=hash_funs, rows=(300, 900), user_hashes=uh)
    h, perm = permuted(h0, seed + 1)
    seqs = {int(perm[ub]): s for ub, s in seqs0.items()}
    want = [int(rng.integers(0, n_user_bins)) for _ in range(n_planted)]
    want += [int(h.bin_to_user[0][u[0]]) for u in units_of(h) if u[1] - u[0] == 3 and not u[2]]
    reads = []
    for ub in want:
        at = int(rng.integers(0, 400 - read_len))
        reads.append(seqs[ub][at:at + read_len].decode())
    for _ in range(n_random):
        reads.append(bytes(rng.choice(list(b"ACGT"), size=read_len).astype(np.uint8)).decode())
    return h, reads, seqs


def even_cuts(C: np.ndarray, k: int) -> List[int]:
    """unit cuts of the optimal k-part split with unlimited budgets (restated plan, left-packed like the product's)"""
    U = C.shape[0] - 1
    bound = optimum(C, [np.iinfo(np.int64).max - 1] * k)
    cuts, at = [0], 0
    for _ in range(k):
        j = at
        while j < U and C[at, j + 1] <= bound:
            j += 1
        at = j
        cuts.append(at)
    assert at == U
    return cuts
