"""The staged probe of the fast count kernel's finish (gn_kernels.hip, gn_stray_probe.h; switch `stray_masks` restores the one-stage
probe) must change no result and request exactly the words its rule says.

Shapes: (4096 bins, 5003 rows) -- the screen-only kernel, one slice; (4160, 3001) -- two slices, the second one word wide;
(32768, 1201) -- 16-byte lanes, the wide screening instance.  Cutoffs 0.55, 0.75, 0.9, 1.0.  Reads: those of test_gpu_row_screen.py
and reads with adversary bins written into the filter at their rows (planned for cutoff 0.75; the stage each one ends in is read from
the restatement's trace, not assumed):
  (a) rows 0/1 hit only beyond the first four hashes: m = 0, stage 1 loads nothing, the bin falls in stage 2
  (b) m = 4 and all four pass stage 1, the bin falls in stage 2
  (c) rows 2 and 3 set for a first-four hash whose rows 0/1 miss: it must not count -- counted, the bin would pass stage 1
  (d) bins that pass both stages and end at exactly T - 1 (not reported) and at T
  (e) three and four surviving bins in one read: two in one word, the others in other lanes
  (f) the shortest reads the launch's table gives a screen at each cutoff, one with ds odd, and one with ds <= 4 where the table has one
  (g) an error-free read (its bin has c2 == ds) beside strays
Checks: hashes, status, offsets and records equal those of the runs with `stray_masks`, `lean_screen`, `row_screen` and `early_exit`
ablated; every third read and every engineered one equals the oracle; the bytes requested equal those of the `lean_screen`-ablated
run, and equal the restatement's tally (tests/stray_probe_model.py) to the byte -- as the `stray_masks`-ablated run equals the
restatement of the one-stage rule, strictly above the default where the restatement has strays; the batch reversed requests the same."""
import functools

import numpy as np
import pytest

import gpu_util as gu
import oracle
import stray_probe_model as model
from test_gpu_lean_screen import _per_read, _run, _same
from test_gpu_row_screen import K, N_GENOMES, W, _set_bit, _workload

pytestmark = pytest.mark.gpu

CUTOFFS = (0.55, 0.75, 0.9, 1.0)
SHAPES = [(4096, 5003), (4160, 3001), (32768, 1201)]
PLAN = 0.75  # the cutoff the adversaries are planned for


@pytest.fixture(scope="module")
def hip():
    import ganon_amd
    ganon_amd.load_library()
    assert ganon_amd.device_count() >= 1, "no HIP device: the product path has no CPU fallback"
    return ganon_amd


def _lane_words(bins):
    words = (bins + 63) // 64
    return 1 if words % 2 == 1 or words == 64 else 2


def _hashes(seq):
    return oracle.minimiser_hash(oracle.to_ranks(seq), K, W)


def _plant(ibf, hs, b, ds, r01, r23, beyond):
    """bin b: rows 0 and 1 of the screened hashes in r01, rows 2 and 3 of those in r23, every row of the hashes >= ds in `beyond`"""
    want = {}
    for q, v in enumerate(hs):
        for i in range(4):
            on = (q in beyond) if q >= ds else (q in r01 if i < 2 else q in r23)
            if want.setdefault(ibf.row(int(v), i), on) != on:
                return False  # two of the read's rows coincide and the pattern wants them apart: nothing is written
    for row, on in want.items():
        _set_bit(ibf, row, b, on)
    return True


def _patterns(n, T, ds):
    """kind -> (r01, r23, beyond, stage, m) for a read of (n, T, ds); None where the read has no room for the kind"""
    t, every = T - (n - ds), set(range(ds, n))
    out = {}
    if 4 + t <= ds and t + (n - ds) >= T:
        out["a"] = (set(range(4, 4 + t)), set(), set(), "drop2", 0)
    if t <= ds - 1 and ds >= 5 and 4 + (n - ds) < T <= n - 1:
        out["b"] = (set(range(ds - 1)), {0, 1, 2, 3}, set(), "drop2", 4)
    if t - 1 <= ds - 4 and t >= 1 and ds >= 5:
        out["c"] = ({0, 2, 3} | set(range(4, 4 + t - 1)), {1}, every, "drop1", 3)
    if 5 <= t <= ds - 1:
        out["d-"] = (set(range(ds - 1)), set(range(t - 1)) | {ds - 1}, every, "full", 4)
        out["d="] = (set(range(ds - 1)), set(range(t)), every, "full", 4)
    return out


def _read_of(rng, n_want):
    """a random read with exactly n_want minimisers"""
    for length in list(range(W + 5 * max(n_want - 2, 0), W + 10 * n_want + 40)) * 4:  # (about seven bases a minimiser)
        s = gu.random_seq(rng, length)
        hs = _hashes(s)
        if len(hs) == n_want and len(np.unique(hs)) == n_want:
            return s
    raise AssertionError(f"no read of {n_want} minimisers")


@functools.lru_cache(maxsize=None)
def _shape(bins, rows):
    ibf, reads, _, _, _ = _workload(bins, rows, 4, 0.5)
    lw = _lane_words(bins)
    unit_bins = min(ibf.bin_words, 64 * lw) * 64
    rng = np.random.default_rng(bins + 17)
    batch = list(reads if bins <= 8192 else reads[:160])
    taken = {(gi * 611 + 5) % bins for gi in range(N_GENOMES)} | set(range(7, min(bins, 4096), 97))
    free = [b for b in range(130, 3800, 37) if not {b, b + 1, b + 64 * lw, b + 128 * lw} & taken]
    if ibf.bin_words == 65:
        free = [4100, 4110] + free  # the second slice, one word wide
    planned = []  # (read, bin, kind, stage, m) at the cutoff PLAN

    def params(s):
        n = len(_hashes(s))
        return (n,) + model.unit_params(n, PLAN, unit_bins)

    def reaches_finish(hs, bins_, cutoff=PLAN):
        trace = model.batch(ibf, [hs], (cutoff,), lw, Fs=(model.PROBE_HASHES,))[1][(cutoff, model.PROBE_HASHES)]["trace"]
        return set(bins_) <= {at[1] * 64 + b for at, b, _, _, _ in trace}

    def engineer(seq, kinds, spread=False):
        """plants the kinds into free bins of the read; `spread`: the first two in one word, the next in the next lanes"""
        hs = _hashes(seq)
        n, T, ds = params(seq)
        pats = _patterns(n, T, ds)
        if ds == 0 or len(np.unique(hs)) != n or any(k not in pats for k in kinds):
            return False
        mine = [free[0], free[0] + 1, free[0] + 64 * lw, free[0] + 128 * lw][:len(kinds)] if spread else free[:len(kinds)]
        if not all(_plant(ibf, hs, b, ds, *pats[k][:3]) for b, k in zip(mine, kinds)):
            return False  # (what was written stays, and the bins are tried again: bits at rows of a read that is not in the batch)
        if not reaches_finish(hs, mine):
            return False  # (a stray of the filter's own beside them: more than four bins, the screen is aborted)
        del free[:1 if spread else len(kinds)]
        planned.extend((len(batch), b, k, pats[k][3], pats[k][4]) for b, k in zip(mine, kinds))
        batch.append(seq)
        return True

    for kinds, spread in ((("a",), False), (("b",), False), (("c",), False), (("d-", "d="), False), (("b", "c", "d="), True),
                          (("a", "b", "c", "d="), True)):
        for _ in range(600):
            if engineer(gu.random_seq(rng, 150), kinds, spread):
                break
        else:
            raise AssertionError(f"no read with room for {kinds}")
    # (g) strays in an error-free read's rows: the read is in the batch already
    for i in range(8, len(reads), 8):
        if i % 5 and i < len(batch):
            hs, (n, T, ds) = _hashes(reads[i]), params(reads[i])
            pats = _patterns(n, T, ds)
            if ds and len(np.unique(hs)) == n and "b" in pats and "c" in pats:
                before = len(planned)
                for k in ("b", "c"):
                    if _plant(ibf, hs, free[0], ds, *pats[k][:3]):
                        planned.append((i, free.pop(0), k, pats[k][3], pats[k][4]))
                if len(planned) > before and reaches_finish(hs, [p[1] for p in planned[before:]]):
                    clean_read = i
                    break
                del planned[before:]
    else:
        raise AssertionError("no error-free read to put strays beside")
    # (f) the shortest screened reads of each cutoff, with ds odd, with ds <= 4: a bin that passes the survey in each
    shortest = []  # (read, bin, cutoff)
    for c in CUTOFFS:
        table = [model.unit_params(n, c, unit_bins)[1] for n in range(model.NMAX + 1)]
        wanted = [[n for n in range(1, 100) if table[n]][:1], [n for n in range(1, 100) if table[n] % 2][:1], [n for n in range(1, 100) if 0 < table[n] <= 4][:1]]
        for n in sorted({w[0] for w in wanted if w}):
            T, ds = model.unit_params(n, c, unit_bins)
            c2 = ds - 1 if T - (n - ds) <= ds - 1 else ds
            b = free.pop(0)
            seq = _read_of(rng, n)
            while not (_plant(ibf, _hashes(seq), b, ds, set(range(c2)), {0}, set()) and reaches_finish(_hashes(seq), [b], c)):
                seq = _read_of(rng, n)
            shortest.append((len(batch), b, c))
            batch.append(seq)
    hashes = [_hashes(s) for s in batch]
    skipped, tally, reports = model.batch(ibf, hashes, CUTOFFS, lw)
    return dict(ibf=ibf, batch=batch, hashes=hashes, skipped=skipped, tally=tally, reports=reports, planned=planned, shortest=shortest,
                clean_read=clean_read, lw=lw, engineered=sorted({p[0] for p in planned} | {s[0] for s in shortest}))


@pytest.mark.parametrize("bins,rows", SHAPES)
def test_the_adversaries_end_where_planned(bins, rows):
    """(no GPU work: the restatement's trace of the planted bins at the cutoff they were planned for)"""
    sh = _shape(bins, rows)
    sw = 64 * sh["lw"] * 64
    trace = {(at[0], at[1] * 64 + b): (stage, m, e) for at, b, stage, m, e in sh["tally"][(PLAN, model.PROBE_HASHES)]["trace"]}
    for r, b, kind, stage, m in sh["planned"]:
        assert (r, b) in trace, (r, b, kind, "the bin reaches no finish")
        assert trace[(r, b)][:2] == (stage, m), (r, b, kind, trace[(r, b)])
        n = len(sh["hashes"][r])
        got = dict(sh["reports"][PLAN][r]).get(b)
        assert got == (oracle.threshold_cutoff(n, PLAN) if kind == "d=" else None), (r, b, kind, got)
    kinds = {k for _, _, k, _, _ in sh["planned"]}
    assert kinds == {"a", "b", "c", "d-", "d="}
    per_read = {}
    for r, b, _, _, _ in sh["planned"]:
        per_read.setdefault(r, []).append(b)
    assert sorted(len(v) for v in per_read.values())[-2:] == [3, 4], "reads with three and with four surviving bins"
    four = max(per_read.values(), key=len)
    assert four[0] // 64 == four[1] // 64 and len({b // sw for b in four}) == 1 and len({b // (64 * sh["lw"]) for b in four}) == 3
    # the error-free read: its own bin takes no probe, the strays beside it fall
    stages = sorted(s for (r, _), (s, _, _) in trace.items() if r == sh["clean_read"])
    assert "clean" in stages and set(stages) & {"drop1", "drop2"}, stages
    for r, b, c in sh["shortest"]:
        seen = {(at[0], at[1] * 64 + bb) for at, bb, _, _, _ in sh["tally"][(c, model.PROBE_HASHES)]["trace"]}
        assert (r, b) in seen, (r, b, c, "the shortest screened read's bin reaches the finish")
    if bins == 4160:
        assert any(b >= 4096 for _, b, _, _, _ in sh["planned"]), "a finish in the slice of one word"


@pytest.mark.parametrize("cutoff", CUTOFFS)
@pytest.mark.parametrize("bins,rows", SHAPES)
def test_staged_probe_changes_no_result_and_requests_what_the_rule_says(hip, bins, rows, cutoff):
    sh = _shape(bins, rows)
    ibf, batch = sh["ibf"], sh["batch"]
    flt = hip.HipFilter.ibf(ibf.data, bins, rows, 4)
    b2t = np.arange(bins, dtype=np.uint32)
    new = _run(hip, flt, batch, None, cutoff)
    runs = {name: _run(hip, flt, batch, None, cutoff, ablate=(name,)) for name in ("stray_masks", "lean_screen", "row_screen", "early_exit")}
    for name, old in runs.items():
        _same(new, old, (bins, cutoff, name))
        assert np.array_equal(new["hashes"][0], old["hashes"][0]) and np.array_equal(new["hashes"][1], old["hashes"][1]), name
    ho, hs = new["hashes"]
    got = _per_read(new)
    for i in sorted(set(range(0, len(batch), 3)) | set(sh["engineered"])):
        assert np.array_equal(hs[int(ho[i]):int(ho[i + 1])], sh["hashes"][i]), i
        exp_m, _ = gu.oracle_matches(ibf, b2t, bins, sh["hashes"][i], cutoff)
        assert [tuple(x) for x in got[i]] == exp_m, (bins, cutoff, i)
    for i, rep in enumerate(sh["reports"][cutoff]):
        assert [tuple(x) for x in got[i]] == rep, (bins, cutoff, i, "the restatement's reports")
    # bytes
    algo = new["tm"]["algo_bytes"]
    want_new, want_old = algo - sh["skipped"][(cutoff, model.PROBE_HASHES)], algo - sh["skipped"][(cutoff, 0)]
    t_new, t_old = sh["tally"][(cutoff, model.PROBE_HASHES)], sh["tally"][(cutoff, 0)]
    print(f"bins {bins} cutoff {cutoff}: algo {algo} fetched {new['tm']['fetched_bytes']} (restated {want_new}), one stage {runs['stray_masks']['tm']['fetched_bytes']} "
          f"(restated {want_old}); finishes {t_new['finish']} clean {t_new['clean']} drop1 {t_new['drop1']} drop2 {t_new['drop2']} full {t_new['full']}, "
          f"one stage: drop2 {t_old['drop2']} full {t_old['full']}")
    assert all(r["tm"]["algo_bytes"] == algo for r in runs.values())
    assert new["tm"]["fetched_bytes"] == runs["lean_screen"]["tm"]["fetched_bytes"]
    assert new["tm"]["fetched_bytes"] == want_new
    assert runs["stray_masks"]["tm"]["fetched_bytes"] == want_old
    # strays: bins probed at all (c2 != ds).  At cutoff 1.0 there are none -- T = n makes the survey's bound ds, so every bin it
    # leaves has c2 == ds -- and the two runs request the same.  At 0.75 and 0.9 the 150 bp reads are screened and some of their
    # strays fall in stage 1: strictly fewer bytes.  At 0.55 the table screens nothing below n = 31: the one probed bin of the batch is
    # that of the shortest screened read, planted with m = 4 hits of which one passes (2 m + 2 (ds - 4) = 2 ds words if it reaches
    # stage 2, 2 m if it falls before): fewer bytes exactly where the restatement says so.
    probed = t_new["drop1"] + t_new["drop2"] + t_new["full"]
    assert (probed == 0) == (cutoff == 1.0)
    if cutoff in (0.75, 0.9):
        assert t_new["drop1"] > 0, "the batch has strays that fall on their first hashes"
    if t_new["drop1"]:
        assert new["tm"]["fetched_bytes"] < runs["stray_masks"]["tm"]["fetched_bytes"]
    assert (want_new < want_old) == (new["tm"]["fetched_bytes"] < runs["stray_masks"]["tm"]["fetched_bytes"]) and want_new <= want_old
    rev = _run(hip, flt, batch[::-1], None, cutoff)
    assert _per_read(rev)[::-1] == got
    assert rev["tm"]["fetched_bytes"] == new["tm"]["fetched_bytes"] and rev["tm"]["algo_bytes"] == algo
    flt.free()
