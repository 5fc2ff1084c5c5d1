"""What a reader of a `ganon-build --hibf` index may rely on, checked on the tables of the tree (next_ibf_id, bin_to_user) and
not on a restated layout rule; and the sizing rule of the IBFs restated in Python."""
import math
from typing import List, Sequence, Tuple

import numpy as np

from oracle import build_params as bp


def levels_for(n: int, tmax: int) -> int:
    """the smallest L >= 1 with tmax ** L >= n (integers)"""
    L, p = 1, tmax
    while p < n:
        p *= tmax
        L += 1
    return L


def run_bits(hashes: int, splits: int, max_fp: float, hash_funs: int) -> int:
    """rows a run of `splits` bins holding `hashes` distinct hashes needs: the textbook size for the share of one bin at the rate
    one bin may have so that the user bin as a whole stays at max_fp (the per-bin rate as split_correction writes it)"""
    share = (hashes + splits - 1) // splits
    per_bin = 1.0 - math.exp(math.log(1.0 - max_fp) / splits)
    return bp.bin_size3(per_bin, share, hash_funs)


def check_tree(bins: Sequence[int], next_ibf_id: Sequence[np.ndarray], bin_to_user: Sequence[np.ndarray], n_user: int, tmax: int, max_levels=None):
    """-> (runs per IBF as (first, n_bins, user | -1, child | -1), depth per IBF, user bins below every IBF, run of every user bin
    as (ibf, first, n_bins), (parent IBF, bin there) of every IBF but the root).  Asserts every invariant of the layout; max_levels
    replaces the depth bound of `ganon-build --hibf` for trees of another origin."""
    n_ibf = len(bins)
    assert len(next_ibf_id) == n_ibf and len(bin_to_user) == n_ibf
    runs: List[List[Tuple[int, int, int, int]]] = []
    where = {}
    parent = {}
    for i in range(n_ibf):
        B = int(bins[i])
        assert 1 <= B <= tmax, (i, B, tmax)
        nx, bu = np.asarray(next_ibf_id[i]), np.asarray(bin_to_user[i])
        assert len(nx) == B and len(bu) == B, (i, B, len(nx), len(bu))
        rs = []
        b = 0
        while b < B:
            u = int(bu[b])
            assert -1 <= u < n_user, (i, b, u)
            if u < 0:  # merged exactly when it has a child
                c = int(nx[b])
                assert 0 < c < n_ibf and c != i, (i, b, c)
                assert c not in parent, ("two merged bins lead to IBF", c)
                parent[c] = (i, b)
                rs.append((b, 1, -1, c))
                b += 1
            else:
                e = b
                while e < B and int(bu[e]) == u:
                    assert int(nx[e]) == i, (i, e, int(nx[e]))
                    e += 1
                assert u not in where, ("user bin in two runs", u, where.get(u), (i, b))
                where[u] = (i, b, e - b)
                rs.append((b, e - b, u, -1))
                b = e
        runs.append(rs)
    assert sorted(where) == list(range(n_user)), "a user bin has no run"
    assert sorted(parent) == list(range(1, n_ibf)), "an IBF is not reached, or IBF 0 has a parent"
    depth = [0] * n_ibf
    for i in range(1, n_ibf):  # every chain of parents ends at IBF 0 without a cycle
        at, steps = i, 0
        while at != 0:
            at = parent[at][0]
            steps += 1
            assert steps <= n_ibf, "cycle in next_ibf_id"
        depth[i] = steps
    bound = levels_for(n_user, tmax) if max_levels is None else max_levels
    assert max(depth) + 1 <= bound, (max(depth) + 1, bound)
    below = [[] for _ in range(n_ibf)]
    for u, (i, _, _) in where.items():
        at = i
        below[at].append(u)
        while at != 0:
            at = parent[at][0]
            below[at].append(u)
    return runs, depth, below, where, parent
