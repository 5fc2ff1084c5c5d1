"""The count step's launch plan (ganon_amd/csrc/gn_count_plan.h) without a GPU: which kernels gn_run_count_range launches for a range
of reads, on what grid, with how much LDS, reading and writing which list, and the GnCountParams scalars the switches decide.

The header -- the very function the library calls -- runs in a stand-alone driver (tests/count_plan_driver.cpp) under AddressSanitizer
and UBSan, nothing preloaded: one case per stdin line, one plan per stdout line.  What a plan must be is written here from the launch
table (`_expect`), not by asking the header twice:

  an identity filter takes the fast family, then the generic kernel over the deferred reads
      ee = early exit on and gp_log2 == 6, wide = lw == 2 and W > 128,
      scr = h == 4 and ee and not row_screen and (lw == 1 or W > 128) and the screen table has an entry
      base = min(ceil(units / 4), n_cu * (8 if lw == 1 else 6)), units = (hi - lo) * wpr
      scr, lw 2               <4,2,1,1,1>, base blocks, LDS 16384 + 16384
      scr, lw 1, unit list    lean, min(ceil(units / 4), n_cu * 10) blocks, LDS 16384, out = units, grab; then <4,1,1,0,0> over the units,
                              max(1, min(base, list cap)) blocks, LDS 16384, no grab, never a stream kernel
      scr, lw 1               <4,1,1,0,1>, base blocks, LDS 16384 + 8192
      ee, wide                <h,2,1,1,0>;  ee: <h,lw,1,0,0>;  else <h,lw,0,0,0> (never a stream kernel): base blocks,
                              LDS 16384 for h <= 4, 24576 for h = 5
  a split-bin filter the split kernel, n_cu * max(split_bpc, 1) * 2 blocks at most, then the generic one over the deferred reads
  any other filter the generic kernel alone, n_cu * 16 blocks at most; long_reads appends the long kernel (128 blocks)
  a deferred list's grid follows the last batch's list when the range is the whole batch and that list's length is known."""
import json
import os
import subprocess

import pytest

from ganon_amd import build as B

HERE = os.path.dirname(os.path.abspath(__file__))
GIB = 1 << 30
# does gn_screen_table give some read a screen (h = 4; unit bins 4096 = 8-byte lanes, 8192 = 16-byte lanes)?  Held against the header's
# table itself in test_screen_table_facts; test_gpu_row_policy.py expects a plain, unscreened launch at 0.2.
SCREENS = {0.2: False, 0.75: True}
BASE = dict(is_hibf=0, identity=1, h=4, W=64, S=1 << 20, lw=1, wpr=1, gp_log2=6, rpb=4, block=256, lds_bytes=33000, split_lds_bytes=44000,
            n_cu=256, split_bpc=3, split_table=0, csr_identity=0, run_ok=0, uniform_nb=0, stream_rows_min_bytes=2 * GIB, unit_list=1,
            long_reads=0, prev_count_deferred="unknown", prev_unit_deferred="unknown", pf_on=0, pf_merge=0, pf_joint=0, pf_segmin=0,
            pf_segmin_cap=0, pf_rel_filter=0.0, lo=0, hi=100000, n_reads=100000, rel_cutoff=0.75, sw=())
SWITCHES = ("early_exit", "row_screen", "lean_screen", "stream_rows", "on_demand", "deferred_grids", "stray_masks", "cand_select", "split_kernel",
            "csr_identity", "uniform_select", "run_select", "const_nb", "max_first", "predrop", "fake_count")


def case(**kw):
    c = dict(BASE)
    c.update(kw)
    c["sw"] = tuple(c["sw"])
    return c


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("count_plan") / "count_plan_driver")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", exe, os.path.join(HERE, "count_plan_driver.cpp"), "-I", B.CSRC])
    return exe


def plans(driver, cases):
    text = "".join(" ".join(f"{k}={','.join(v) if k == 'sw' else v}" for k, v in c.items() if k != "sw" or v) + "\n" for c in cases)
    p = subprocess.run([driver], input=text, capture_output=True, text=True)
    assert p.returncode == 0 and p.stderr == "", (p.returncode, p.stdout[-300:], p.stderr[-3000:])  # (a sanitizer report ends the program with a status)
    out = [json.loads(line) for line in p.stdout.splitlines()]
    assert len(out) == len(cases)
    return out


def _ceil(a, b):
    return -(-a // b)


def _launch(family, blocks, lds, key=(0, 0, 0, 0, 0), stream=0, lin="none", lout="none", grab=0):
    return {"family": family, "key": list(key), "stream": int(stream), "blocks": blocks, "lds": lds, "in": lin, "out": lout, "grab": int(grab)}


def _expect(c):
    """the launches of a case, from the table in the module's docstring"""
    sw, n_cu, h, lw, W, lo, hi = set(c["sw"]), c["n_cu"], c["h"], c["lw"], c["W"], c["lo"], c["hi"]
    if "fake_count" in sw or hi <= lo:
        return [], False
    reads, units = hi - lo, (hi - lo) * c["wpr"]
    whole = lo == 0 and hi == c["n_reads"] and "deferred_grids" not in sw
    out, streamed = [], False
    split = not c["identity"] and c["split_table"] and "split_kernel" not in sw
    if c["identity"]:
        ee = "early_exit" not in sw and c["gp_log2"] == 6
        wide = lw == 2 and W > 128
        scr = h == 4 and ee and "row_screen" not in sw and (lw == 1 or W > 128) and SCREENS[c["rel_cutoff"]]
        # stream kernels: a flat filter of at least the threshold's row bytes, the screen-only kernel and the two instances that screen
        stream = scr and not c["is_hibf"] and "stream_rows" not in sw and c["S"] * W * 8 >= c["stream_rows_min_bytes"]
        base = min(_ceil(units, 4), n_cu * (8 if lw == 1 else 6))
        grab = "on_demand" not in sw
        lds = 24576 if h == 5 else 16384
        if scr and lw == 2:
            out.append(_launch("fast", base, 16384 + 16384, (4, 2, 1, 1, 1), stream, "none", "deferred", grab))
        elif scr and c["unit_list"] and "lean_screen" not in sw:
            out.append(_launch("lean", min(_ceil(units, 4), n_cu * 10), 16384, stream=stream, lout="units", grab=grab))
            cap = max(n_cu, c["prev_unit_deferred"] // 2 + 1) if whole and c["prev_unit_deferred"] != "unknown" else base
            out.append(_launch("fast", max(1, min(base, cap)), 16384, (4, 1, 1, 0, 0), 0, "units", "deferred", 0))
        elif scr:
            out.append(_launch("fast", base, 16384 + 8192, (4, 1, 1, 0, 1), stream, "none", "deferred", grab))
        elif ee and wide:
            out.append(_launch("fast", base, lds, (h, 2, 1, 1, 0), 0, "none", "deferred", grab))
        elif ee:
            out.append(_launch("fast", base, lds, (h, lw, 1, 0, 0), 0, "none", "deferred", grab))
        else:
            out.append(_launch("fast", base, lds, (h, lw, 0, 0, 0), 0, "none", "deferred", grab))
        streamed = bool(stream)
    elif split:
        out.append(_launch("split", min(_ceil(reads, c["rpb"]), n_cu * max(c["split_bpc"], 1) * 2), c["split_lds_bytes"], lout="deferred"))
    cap = n_cu * 16
    if (c["identity"] or split) and whole and c["prev_count_deferred"] != "unknown":
        cap = min(cap, max(n_cu, c["prev_count_deferred"] * 2))
    out.append(_launch("generic", min(_ceil(reads, c["rpb"]), cap), c["lds_bytes"], lin="deferred" if c["identity"] or split else "none"))
    if c["long_reads"]:
        out.append(_launch("long", 128, 0))
    return out, streamed


def _check(driver, cases):
    got = plans(driver, cases)
    for c, g in zip(cases, got):
        launches, streamed = _expect(c)
        assert g["launches"] == launches, (c, g["launches"], launches)
        assert g["streamed"] == int(streamed), c
        assert len(g["launches"]) <= 5
    return got


@pytest.mark.parametrize("bins", [4096, 8192])
def test_screen_table_facts(driver, bins):
    """what SCREENS says, from gn_screen_table.h itself: no read is screened at 0.2, some are at 0.75"""
    for cutoff, some in SCREENS.items():
        n = int(subprocess.run([driver, "screen", repr(cutoff), "4", str(bins)], capture_output=True, text=True, check=True).stdout)
        assert (n > 0) == some, (cutoff, bins, n)
    for h in (1, 2, 3, 5):
        assert int(subprocess.run([driver, "screen", "0.75", str(h), str(bins)], capture_output=True, text=True, check=True).stdout) == 0


@pytest.mark.parametrize("n_cu", [256, 8])
def test_fast_family_shapes(driver, n_cu):
    cases = [case(n_cu=n_cu, h=h, lw=lw, W=W, gp_log2=gp, rel_cutoff=cutoff, unit_list=ul)
             for h in (1, 2, 3, 4, 5) for lw in (1, 2) for W in (64, 128, 129, 512) for gp in (6, 5) for cutoff in (0.2, 0.75) for ul in (1, 0)]
    got = _check(driver, cases)
    kinds = {(g["launches"][0]["family"], tuple(g["launches"][0]["key"])) for g in got}
    assert {("lean", (0, 0, 0, 0, 0)), ("fast", (4, 1, 1, 0, 1)), ("fast", (4, 2, 1, 1, 1)), ("fast", (5, 2, 1, 1, 0)), ("fast", (3, 1, 0, 0, 0))} <= kinds
    for c, g in zip(cases, got):
        # the table the kernels get: filled for the shapes that can screen, whatever h and the cutoff make of it
        assert g["screen_filled"] == int(c["lw"] == 1 or c["W"] > 128), c
        if g["screen_filled"]:
            assert g["screen_unit_bins"] == min(c["W"], 64 * c["lw"]) * 64
        assert (g["n_screened"] > 0) == bool(g["screen_filled"] and c["h"] == 4 and SCREENS[c["rel_cutoff"]]), c


def test_switches_each_alone(driver):
    shapes = [dict(), dict(lw=2, W=512), dict(rel_cutoff=0.2), dict(S=1 << 23),  # (the last: 4 GiB of rows, past the stream threshold)
              dict(identity=0, split_table=1, csr_identity=1, run_ok=1, uniform_nb=2), dict(identity=0, split_table=1, csr_identity=1, run_ok=1),
              dict(identity=0), dict(prev_count_deferred=3, prev_unit_deferred=5), dict(pf_on=1, pf_segmin=1, pf_segmin_cap=1 << 20, pf_rel_filter=0.25)]
    cases = [case(sw=sw, **shape) for shape in shapes for sw in [()] + [(name,) for name in SWITCHES]]
    got = _check(driver, cases)
    for c, g in zip(cases, got):
        sw = set(c["sw"])
        if "fake_count" in sw:
            assert g["fake_count"] == 1 and g["launches"] == [] and g["clear"] == [] and g["predrop"] == 0
            continue
        assert g["fake_count"] == 0
        assert g["early_exit"] == int("early_exit" not in sw)
        assert g["probe_hashes"] == (0 if "stray_masks" in sw else 4)
        assert g["bin_nb2"] == int("cand_select" not in sw)
        assert g["max_first"] == int("max_first" not in sw)
        assert g["emit_probe"] == 0
        fast, split = bool(c["identity"]), bool(not c["identity"] and c["split_table"] and "split_kernel" not in sw)
        predrop = bool((fast or split) and c["pf_on"] and "predrop" not in sw)
        assert g["predrop"] == int(predrop) and g["pre_mode"] == int(predrop)
        clear = ["skipped"] + (["pre", "segmin"] if predrop else []) + (["deferred"] if fast or split else [])
        clear += ["unit_cursor"] if fast and "on_demand" not in sw else []
        clear += ["units_left"] if fast and "lean_screen" not in sw else []
        assert g["clear"] == clear, (c, g["clear"])
    # the switches that change the launches do: against the same shape with nothing switched
    by = {(i // (1 + len(SWITCHES)), c["sw"]): g for i, (c, g) in enumerate(zip(cases, got))}
    assert by[(0, ())]["launches"][0]["family"] == "lean" and by[(0, ("lean_screen",))]["launches"][0]["key"] == [4, 1, 1, 0, 1]
    assert by[(0, ("row_screen",))]["launches"][0]["key"] == [4, 1, 1, 0, 0] and by[(0, ("early_exit",))]["launches"][0]["key"] == [4, 1, 0, 0, 0]
    assert by[(1, ("row_screen",))]["launches"][0]["key"] == [4, 2, 1, 1, 0]
    assert by[(3, ())]["launches"][0]["stream"] == 1 and by[(3, ())]["streamed"] == 1 and by[(3, ("stream_rows",))]["streamed"] == 0
    assert by[(0, ())]["launches"][0]["grab"] == 1 and by[(0, ("on_demand",))]["launches"][0]["grab"] == 0
    assert by[(7, ())]["launches"][1]["blocks"] == 256 and by[(7, ("deferred_grids",))]["launches"][1]["blocks"] == 2048
    assert by[(7, ())]["launches"][2]["blocks"] == 256 and by[(7, ("deferred_grids",))]["launches"][2]["blocks"] == 4096
    assert [x["family"] for x in by[(4, ())]["launches"]] == ["split", "generic"] and [x["family"] for x in by[(4, ("split_kernel",))]["launches"]] == ["generic"]


def test_emit_probe_is_passed_on(driver):
    assert [g["emit_probe"] for g in plans(driver, [case(emit_probe=64), case(emit_probe=128)])] == [64, 128]


def test_stream_threshold(driver):
    rows = (1 << 23) * 64 * 8  # S * W * 8 bytes
    cases = [case(S=1 << 23, stream_rows_min_bytes=rows),       # exactly at the threshold
             case(S=1 << 23, stream_rows_min_bytes=rows - 1),   # one byte above it
             case(S=1 << 23, stream_rows_min_bytes=rows + 1),   # one byte below
             case(S=1 << 23, stream_rows_min_bytes=0, is_hibf=1),
             case(S=1 << 23, stream_rows_min_bytes=0, h=3),
             case(S=1 << 23, stream_rows_min_bytes=0, rel_cutoff=0.2),
             case(S=1 << 23, stream_rows_min_bytes=0, unit_list=0),
             case(S=1 << 20, lw=2, W=512, stream_rows_min_bytes=0),
             case(S=1 << 23, stream_rows_min_bytes=0, gp_log2=5)]
    got = _check(driver, cases)
    assert [g["streamed"] for g in got] == [1, 1, 0, 0, 0, 0, 1, 1, 0]
    assert [[x["stream"] for x in g["launches"]] for g in got[:2]] == [[1, 0, 0], [1, 0, 0]], "the screen-only kernel streams, the list launch never"
    assert got[6]["launches"][0]["key"] == [4, 1, 1, 0, 1] and got[7]["launches"][0]["key"] == [4, 2, 1, 1, 1]


def test_ranges_and_grids(driver):
    prevs = ["unknown", 0, 1, 10_000_000]
    cases = [case(n_cu=n_cu, prev_count_deferred=pc, prev_unit_deferred=pu, lo=lo, hi=hi, identity=ident, split_table=1 - ident)
             for n_cu in (256, 8) for pc in prevs for pu in prevs for lo, hi in ((0, 100000), (0, 50000), (50000, 100000)) for ident in (1, 0)]
    got = _check(driver, cases)
    for c, g in zip(cases, got):
        gen = g["launches"][-1]
        whole = (c["lo"], c["hi"]) == (0, 100000)
        if whole and c["prev_count_deferred"] in (0, 1):
            assert gen["blocks"] == c["n_cu"], "the cap floors at one block a CU"
        else:
            assert gen["blocks"] == c["n_cu"] * 16
        if c["identity"]:
            lst = g["launches"][1]
            assert lst["in"] == "units" and lst["blocks"] == (c["n_cu"] if whole and c["prev_unit_deferred"] in (0, 1) else c["n_cu"] * 8)
    # the list launch gets at least one block; an empty range gets no launch, and its counters are cleared as for any other
    one = plans(driver, [case(n_cu=0, lo=0, hi=1, n_reads=1), case(lo=7, hi=7), case(lo=0, hi=0, n_reads=0, long_reads=1)])
    assert [x["blocks"] for x in one[0]["launches"]] == [0, 1, 0]
    assert one[1]["launches"] == [] and one[1]["clear"] == ["deferred", "unit_cursor", "units_left"]
    assert one[2]["launches"] == [] and one[2]["clear"] == ["skipped", "deferred", "unit_cursor", "units_left", "long"]
    # ceil(units / 4): 1, 4 and 5 reads at one and four waves a read
    cases = [case(lo=0, hi=n, n_reads=n, wpr=wpr, long_reads=1) for n in (1, 4, 5) for wpr in (1, 4)]
    got = _check(driver, cases)
    assert [g["launches"][0]["blocks"] for g in got] == [1, 1, 1, 4, 2, 5]
    assert [g["launches"][2]["blocks"] for g in got] == [1, 1, 1, 1, 2, 2], "the generic kernel: four reads a block here"
    assert all(g["launches"][3] == _launch("long", 128, 0) and g["clear"][-1] == "long" for g in got)
    # a partial range (chunk=N) of a batch whose lists are known keeps the full grids
    part = plans(driver, [case(lo=0, hi=50000, prev_count_deferred=0, prev_unit_deferred=0), case(lo=50000, hi=100000, prev_count_deferred=0, prev_unit_deferred=0)])
    assert [[x["blocks"] for x in g["launches"]] for g in part] == [[2560, 2048, 4096]] * 2
    assert "skipped" in part[0]["clear"] and "skipped" not in part[1]["clear"], "the tally starts with the batch's first range"


# (csr_identity, run_ok, uniform_nb of the filter, switches) -> csr_identity, uniform_nb, run_select, const_nb of the launch
SCALARS = [((0, 0, 0, ()), (0, 0, 0, 0)), ((0, 1, 2, ()), (0, 0, 0, 0)),
           ((1, 0, 0, ()), (1, 0, 0, 0)), ((1, 1, 0, ()), (1, 0, 1, 4)), ((1, 1, 2, ()), (1, 2, 0, 2)), ((1, 0, 4, ()), (1, 4, 0, 4)),
           ((1, 1, 2, ("csr_identity",)), (0, 0, 0, 0)), ((1, 1, 2, ("uniform_select",)), (1, 0, 1, 4)), ((1, 0, 2, ("uniform_select",)), (1, 0, 0, 0)),
           ((1, 1, 0, ("run_select",)), (1, 0, 0, 0)), ((1, 1, 2, ("run_select",)), (1, 2, 0, 2)),
           ((1, 1, 2, ("const_nb",)), (1, 2, 0, 0)), ((1, 1, 0, ("const_nb",)), (1, 0, 1, 4)),
           ((1, 1, 2, ("uniform_select", "run_select")), (1, 0, 0, 0)), ((1, 1, 4, ("uniform_select", "const_nb")), (1, 0, 1, 4))]


def test_select_scalars(driver):
    cases = [case(identity=0, split_table=1, csr_identity=a, run_ok=b, uniform_nb=u, sw=sw) for (a, b, u, sw), _ in SCALARS]
    got = _check(driver, cases)
    assert [(g["csr_identity"], g["uniform_nb"], g["run_select"], g["const_nb"]) for g in got] == [want for _, want in SCALARS]


def test_predrop_and_pre_mode(driver):
    on = dict(pf_on=1, pf_segmin=1, pf_segmin_cap=100000, pf_rel_filter=0.5)
    cases = [case(), case(**on), case(**on, pf_joint=1),                                                   # 0 1 2
             case(**on, pf_merge=1), case(**dict(on, pf_segmin=0)), case(**dict(on, pf_rel_filter=1.0)),   # off: a merging level, no buffer, nothing to drop
             case(**dict(on, pf_rel_filter=-1.0)), case(**dict(on, pf_segmin_cap=99999)), case(**on, wpr=2),  # ... no filter, a buffer too small
             case(**on, identity=0), case(**on, identity=0, split_table=1), case(**on, identity=0, split_table=1, sw=("split_kernel",)),
             case(**on, lo=50000), case(**on, sw=("predrop",))]
    got = _check(driver, cases)
    assert [g["pre_mode"] for g in got] == [0, 1, 2, 0, 0, 0, 0, 0, 0, 0, 1, 0, 1, 0]
    assert [g["predrop"] for g in got] == [int(g["pre_mode"] != 0) for g in got]
    assert got[1]["clear"][:3] == ["skipped", "pre", "segmin"] and got[12]["clear"][0] == "segmin", "only a batch's first range clears the tally"
