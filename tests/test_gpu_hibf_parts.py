"""An HIBF cut into subtree parts at the C ABI: every part an HIBF of its own with absent bins in the root's boundary words
(gn_filter_upload_hibf), rows streamed with word_lo, one batch classified through all parts (gn_stream_classify_shared) and the
parts' results merged (gn_gather_create_merged) -- against gn_fetch_batch of the whole HIBF on the same device and oracle.Hibf."""
import numpy as np
import pytest

import ganon_fixtures as gf
import gpu_util as gu
import hibf_partition_checks as hp
import oracle

pytestmark = pytest.mark.gpu

K, W = hp.K, hp.W


@pytest.fixture(scope="module")
def hip():
    import ganon_amd
    ganon_amd.load_library()
    assert ganon_amd.device_count() >= 1, "no HIP device: the product path has no CPU fallback"
    return ganon_amd


class Case:
    """a fixture, its whole-filter result per (rel_cutoff, paired) -- computed once, shared and left unchanged"""

    def __init__(self, hip, n_user_bins, tmax, seed):
        self.h, reads, _ = hp.planted_fixture(n_user_bins, tmax, seed)
        self.seqs = [r.encode() for r in reads]
        self.units = hp.units_of(self.h)
        self.C = hp.cost_matrix(self.h, self.units)
        self.full = hip.HipFilter.hibf(*gf.hibf_upload_args(self.h))
        self.whole = {}

    def batch(self, paired):
        return gu.pack_reads(self.seqs, [hp.revcomp(s) for s in self.seqs] if paired else None)

    def reference(self, hip, rel_cutoff, paired):
        key = (rel_cutoff, paired)
        if key not in self.whole:
            bases, o1, o2 = self.batch(paired)
            st = hip.HipStream(self.full, len(self.seqs), bases.size)
            st.submit(bases, o1, o2, K, W, rel_cutoff)
            nh, status, mo, m = st.fetch()
            ho, hs = st.fetch_hashes()
            # ... and the oracle's: counting_agent_type::bulk_count + select_matches(THIBF)
            exp = []
            for i in range(len(self.seqs)):
                hh = hs[int(ho[i]):int(ho[i + 1])]
                if status[i] != 0 or len(hh) == 0:
                    continue
                cnt = self.h.bulk_count(hh, oracle.threshold_cutoff(len(hh), rel_cutoff))
                exp += [(i, int(u), int(min(c, len(hh)))) for u, c in enumerate(cnt) if c > 0]
            assert [(int(x["read"]), int(x["target"]), int(x["count"])) for x in m] == exp and len(exp) > 50
            st.destroy()
            mo.setflags(write=False)
            m.setflags(write=False)
            self.whole[key] = (mo, m)
        return self.whole[key]


@pytest.fixture(scope="module")
def wide(hip):
    c = Case(hip, 600, 192, seed=7)
    assert (c.h.ibfs[0].bins + 63) // 64 == 3  # a root of three words
    return c


@pytest.fixture(scope="module")
def narrow(hip):
    c = Case(hip, 200, 64, seed=9)
    assert c.h.ibfs[0].bins <= 64  # a root of one word: every part holds it whole, with absent bins
    return c


def upload_parts(hip, c, cuts):
    """-> [(filter, part)]: rows streamed in -- an IBF's rows to the part that owns it, the root's to every part with its word_lo"""
    out = []
    for a, b in zip(cuts, cuts[1:]):
        p = hp.build_part(c.h, c.units, a, b)
        flt = hip.HipFilter.hibf([(None, bins, rows, hf) for bins, rows, hf in p["shapes"]], p["next_ibf_id"], p["bin_to_user"],
                                 max(len(p["user_global"]), 1))
        for local, g in enumerate(p["ibf_global"]):
            flt.write_rows(0, c.h.ibfs[g].data, p["word_lo"] if g == 0 else 0, ibf_idx=local)
        flt.finalize()
        out.append((flt, p))
    return out


def cut_sets(c):
    """unit cuts for 2, 3 and 5 parts: the restated plan's, one on a word boundary of the root, and one right behind a user bin that
    is split over three root bins"""
    U = len(c.units)
    sets = [hp.even_cuts(c.C, k) for k in (2, 3, 5)]
    sets = [[x for i, x in enumerate(s) if i == 0 or x != s[i - 1]] for s in sets]  # (parts the plan left empty)
    on_word = [i for i, u in enumerate(c.units) if 0 < i and u[0] % 64 == 0]
    if on_word:
        sets.append([0, on_word[0], U])
    split3 = [i for i, u in enumerate(c.units) if u[1] - u[0] == 3 and not u[2] and 0 < i < U - 1]
    assert split3, "the fixture has no user bin split over three root bins"
    sets.append([0, split3[0], split3[0] + 1, U])  # cuts on both sides of it
    return sets, split3[0]


@pytest.mark.parametrize("paired", [False, True])
@pytest.mark.parametrize("rel_cutoff", [0.1, 0.6])
@pytest.mark.parametrize("which", ["wide", "narrow"])
def test_parts_merged_equal_the_whole_hibf_and_the_oracle(hip, request, which, rel_cutoff, paired):
    c = request.getfixturevalue(which)
    mo, m = c.reference(hip, rel_cutoff, paired)
    bases, o1, o2 = c.batch(paired)
    sets, split3 = cut_sets(c)
    if which == "wide":
        inside = [any(c.units[x][0] % 64 for x in s[1:-1]) for s in sets]
        on = [any(c.units[x][0] % 64 == 0 for x in s[1:-1]) for s in sets]
        assert any(inside) and any(on)  # cuts inside a word and on a word boundary
    interleaved = False
    for cuts in sets:
        parts = upload_parts(hip, c, cuts)
        interleaved |= hp.interleaves([p for _, p in parts])
        sts = [hip.HipStream(f, len(c.seqs), bases.size) for f, _ in parts]
        sts[0].submit(bases, o1, o2, K, W, rel_cutoff)
        for s in sts[1:]:
            s.classify_shared(sts[0], rel_cutoff)
        g = hip.HipGather(0, [np.array(p["user_global"], dtype=np.uint32) for _, p in parts], merged=True)
        g.run(sts)
        mo2, m2 = g.fetch()
        assert np.array_equal(mo2, mo) and np.array_equal(m2, m), cuts
        g.destroy()
        for s in sts:
            s.destroy()
        for f, _ in parts:
            f.free()
    assert interleaved  # (else a concatenation would be sorted already and the merge untested)
    # the user bin split over three root bins next to the cuts: reported, with its whole sum
    ub = int(c.h.bin_to_user[0][c.units[split3][0]])
    if rel_cutoff == 0.1:
        assert ub in set(int(t) for t in m["target"])


def test_absent_bins_are_cleared_and_owned_ones_untouched(hip, wide):
    c = wide
    inside = [i for i, u in enumerate(c.units) if 0 < i and u[0] % 64]
    cuts = [0, inside[len(inside) // 2], len(c.units)]
    root = c.h.ibfs[0]
    for flt, p in upload_parts(hip, c, cuts):
        words = p["word_hi"] - p["word_lo"]
        got = flt.download_rows(0, root.bin_size, words, ibf_idx=0)
        keep = np.zeros(words, dtype=np.uint64)
        for t in range(p["bin_lo"], p["bin_hi"]):
            keep[(t >> 6) - p["word_lo"]] |= np.uint64(1) << np.uint64(t & 63)
        src = root.data[:, p["word_lo"]:p["word_hi"]]
        assert np.array_equal(got, src & keep)
        assert (src & ~keep).any() and not np.array_equal(got, src)  # (the neighbour's bins did arrive with the rows)
        flt.free()


def test_absent_bins_were_refused_before_and_bad_tables_still_are(hip):
    # a bin that is neither a user bin nor leads to a child: absent (-1 / -1) is accepted, anything else stays an error
    f = hip.HipFilter.hibf([(None, 3, 64, 2)], [[0, -1, 0]], [[0, -1, 1]], 2)
    assert f.info()["n_targets"] == 2
    f.free()
    with pytest.raises(hip.GanonHipError):
        hip.HipFilter.hibf([(None, 3, 64, 2)], [[0, 5, 0]], [[0, -1, 1]], 2)
    with pytest.raises(hip.GanonHipError):
        hip.HipFilter.hibf([(None, 3, 64, 2)], [[0, 0, 0]], [[0, -1, 1]], 2)
