// gn_count_plan.h -- which kernels the count step of a flat IBF launches for a range of reads, on what grid, with how much LDS, reading
// and writing which list; and the scalars of GnCountParams that the switches decide (host only: no HIP in here).
//
// gn_run_count_range (gn_capi.hip) fills a GnCountPlanIn from the filter, the stream and the switches, calls gn_count_plan, clears the
// counters the plan names and launches its records in order; the launchers (gn_kernels.hip, gn_split.hip) map a record to a template
// instance and decide nothing.  Every grid factor, LDS formula and launch condition of the count step is in this file, and
// tests/test_count_plan_cpu.py holds the plan against the table below without a GPU.
//
// An identity filter takes the fast family, then the generic kernel over the reads the fast kernels deferred (more than 127 minimisers):
//     ee   = early exit on && a wave is one hash group (gp_log2 == GN_FAST_EE_GP_LOG2)
//     wide = 16-byte lanes on rows of more than 128 words
//     scr  = four hash functions && ee && row_screen not ablated && (8-byte lanes || rows of more than 128 words)
//            && gn_screen_table gives some read a screen at this cutoff
//     base = min(ceil(units / 4), n_cu * (8 | 6 with 16-byte lanes)) blocks, units = reads * wpr, four units (waves) a block
//   scr, 16-byte lanes        <4,2,1,1,1>, base blocks, row table + match lists + hit masks
//   scr, 8-byte lanes, list   the screen-only kernel, min(ceil(units / 4), n_cu * 10) blocks, writes the unit list;
//                             then <4,1,1,0,0> over that list, max(1, min(base, list cap)) blocks, plain loads, no cursor
//   scr, 8-byte lanes         <4,1,1,0,1>, base blocks (no unit list on the stream, or lean_screen ablated)
//   ee, wide                  <h,2,1,1,0>, base blocks
//   ee                        <h,lw,1,0,0>, base blocks
//   otherwise                 <h,lw,0,0,0>, base blocks
// A split-bin filter (not identity, with the split kernel's table) takes the split kernel, then the generic one over what it deferred;
// any other filter the generic kernel over every read.  gn_set_long_reads appends the long-read kernel.
#pragma once
#include <algorithm>
#include <cstdint>

#include "gn_row_policy.h"
#include "gn_screen_table.h"
#include "gn_stray_probe.h"

#ifndef GN_WAVE
#define GN_WAVE 64
#endif
#define GN_FAST_LIST 512u // matches of a unit the fast kernel's epilogue lists in LDS before it writes them out (2 KiB a wave)
// EE launches only happen where "a wave is one hash group" (rows of 64 lanes and more); the screening instances take that as a
// compile-time fact, which spares them registers.  Kernel and plan both read it from here.
constexpr uint32_t GN_FAST_EE_GP_LOG2 = 6;
static_assert((1u << GN_FAST_EE_GP_LOG2) == GN_WAVE, "the EE instances of the fast kernel: one hash group a wave");

// persistent grids = a whole number of resident rounds, in blocks a CU
constexpr uint32_t GN_GENERIC_BLOCKS_PER_CU  = 16;
constexpr uint32_t GN_FAST_BLOCKS_PER_CU_LW1 = 8;  // the 8-byte-lane fast kernel holds 4 blocks a CU
constexpr uint32_t GN_FAST_BLOCKS_PER_CU_LW2 = 6;  // the 16-byte-lane one 3
constexpr uint32_t GN_LEAN_BLOCKS_PER_CU     = 10; // the screen-only kernel 5
constexpr uint32_t GN_FAST_WAVES             = 4;  // waves (= units in flight) of a fast-family block of 256 threads
#define GN_LONG_BLOCKS 128u // workgroups (and uint32 count slabs) of the long-read kernel

// LDS of a fast-kernel block, per wave: the row table (128 rows of 4 or 8 hash functions) + the epilogue's match list, and in the
// screening instances + the hit masks of the probe
constexpr uint64_t gn_fast_lds_bytes(uint32_t hash_funs, uint32_t lw, bool screens)
{
    return (uint64_t)GN_FAST_WAVES * (128u * (hash_funs <= 4 ? 4u : 8u) + GN_FAST_LIST + (screens ? GN_PROBE_HASHES * 2u * lw * GN_WAVE : 0u)) * 4u;
}
// ... of a screen-only block: the row table and the hit masks (four hash functions, 8-byte lanes)
constexpr uint64_t gn_lean_lds_bytes()
{
    return (uint64_t)GN_FAST_WAVES * (128u * 4u + GN_PROBE_HASHES * 2u * GN_WAVE) * 4u;
}

// the fields of GnSwitches (gn_internal.h) the count step reads
struct GnCountPlanSw
{
    bool     early_exit = false, row_screen = false, lean_screen = false, stream_rows = false, stray_masks = false, cand_select = false;
    bool     csr_identity = false, uniform_select = false, run_select = false, max_first = false, const_nb = false, split_kernel = false;
    bool     predrop = false, deferred_grids = false, on_demand = false, fake_count = false;
    uint32_t emit_probe = 0;
};

struct GnCountPlanIn
{
    // filter
    bool     is_hibf = false, identity = false;
    uint32_t h = 0;
    uint64_t W = 0, S = 0;
    uint32_t lw = 1, wpr = 1, gp_log2 = 0, rpb = 1, block = 256; // GnCountGeometry
    uint64_t lds_bytes = 0, split_lds_bytes = 0;                  // ... its LDS and gn_split_lds_bytes
    uint32_t n_cu = 0, split_bpc = 0;
    bool     split_table = false; // gn_filter::d_sl_nbr exists
    bool     csr_identity = false, run_ok = false;
    uint32_t uniform_nb = 0;
    uint64_t stream_rows_min_bytes = GN_STREAM_ROWS_MIN_BYTES;
    // stream
    bool     unit_list = false, long_reads = false;
    uint64_t prev_count_deferred = ~0ull, prev_unit_deferred = ~0ull; // ~0: unknown
    bool     pf_on = false, pf_merge = false, pf_joint = false, pf_segmin = false;
    uint64_t pf_segmin_cap = 0;
    double   pf_rel_filter = 0;
    // range [lo, hi) of a batch of n_reads
    uint32_t lo = 0, hi = 0, n_reads = 0;
    double   rel_cutoff = 0;
    GnCountPlanSw sw;
};

enum GnCountFamily : uint8_t { GN_COUNT_SPLIT, GN_COUNT_LEAN, GN_COUNT_FAST, GN_COUNT_GENERIC, GN_COUNT_LONG };
enum GnCountList : uint8_t { GN_LIST_NONE, GN_LIST_DEFERRED, GN_LIST_UNITS }; // reads left to the generic kernel | units the screen-only kernel left
// counters and buffers the executor clears before the launches (bits of GnCountPlan::clear)
enum GnCountClear : uint32_t
{
    GN_CLEAR_SKIPPED = 1, GN_CLEAR_PRE = 2, GN_CLEAR_SEGMIN = 4, GN_CLEAR_DEFERRED = 8, GN_CLEAR_UNIT_CURSOR = 16, GN_CLEAR_UNITS_LEFT = 32, GN_CLEAR_LONG = 64
};

struct GnCountLaunch
{
    GnCountFamily family = GN_COUNT_GENERIC;
    uint8_t       HF = 0, LW = 0;                          // the fast kernel's template key (family fast)
    bool          EE = false, WIDE = false, SCRN = false;
    bool          stream = false;                          // the stream twin (non-temporal row loads): families lean and fast
    uint32_t      blocks = 0;
    uint64_t      lds_bytes = 0;
    GnCountList   list_in = GN_LIST_NONE, list_out = GN_LIST_NONE; // (a launch that writes the unit list defers reads as well)
    bool          grab = false;                            // its waves take their later units from the unit cursor
};

constexpr uint32_t GN_COUNT_MAX_LAUNCHES = 5;
struct GnCountPlan
{
    uint32_t      n_launches = 0;
    GnCountLaunch launch[GN_COUNT_MAX_LAUNCHES];
    // GnCountParams
    uint32_t early_exit = 0, probe_hashes = 0, emit_probe = 0, csr_identity = 0, uniform_nb = 0, run_select = 0, max_first = 0, const_nb = 0, pre_mode = 0;
    bool     bin_nb2 = false;                  // the candidate-driven select's table is passed
    bool     screen_filled = false;            // `screen` is gn_screen_table for screen_unit_bins (else all zero)
    uint32_t screen_unit_bins = 0;
    uint8_t  screen[GN_SCREEN_NMAX + 1] = {};
    bool     predrop = false, fake_count = false, streamed = false;
    uint32_t clear = 0;
};

inline uint32_t gn_plan_grid(uint64_t work, uint64_t per_block, uint64_t cap)
{
    return (uint32_t)std::min<uint64_t>((work + per_block - 1) / per_block, cap);
}

// the generic kernel over every read of a range (one block per rpb reads, a persistent grid)
inline uint32_t gn_generic_grid(uint64_t reads, uint32_t rpb, uint32_t n_cu)
{
    return gn_plan_grid(reads, rpb, (uint64_t)n_cu * GN_GENERIC_BLOCKS_PER_CU);
}

inline void gn_count_plan(const GnCountPlanIn& in, GnCountPlan* out)
{
    GnCountPlan          pl;
    const GnCountPlanSw& sw = in.sw;
    pl.fake_count = sw.fake_count;
    if (sw.fake_count) // (every match is "written": nothing is counted, cleared or dropped ahead of a pre-pass)
    {
        *out = pl;
        return;
    }
    pl.early_exit   = sw.early_exit ? 0u : 1u;
    pl.probe_hashes = sw.stray_masks ? 0u : GN_PROBE_HASHES;
    pl.emit_probe   = sw.emit_probe;
    pl.bin_nb2      = !sw.cand_select;
    pl.csr_identity = in.csr_identity && !sw.csr_identity ? 1u : 0u;
    pl.uniform_nb   = pl.csr_identity && !sw.uniform_select ? in.uniform_nb : 0u;
    pl.run_select   = pl.csr_identity && in.run_ok && !pl.uniform_nb && !sw.run_select ? 1u : 0u;
    pl.max_first    = sw.max_first ? 0u : 1u;
    pl.const_nb     = pl.uniform_nb && !sw.const_nb ? pl.uniform_nb : (pl.run_select ? 4u : 0u);

    const bool fast = in.identity, split = !in.identity && in.split_table && !sw.split_kernel;
    // with a filter_matches pre-pass on the stream the fast and the split-bin kernel do not write matches the --rel-filter rule is bound to
    // drop (not for a merging level: there the minimum follows the entries that got in, which only the merge knows)
    pl.predrop  = (fast || split) && in.pf_on && !in.pf_merge && in.pf_segmin && in.pf_rel_filter >= 0.0 && in.pf_rel_filter < 1.0 &&
                 (uint64_t)in.hi * in.wpr <= in.pf_segmin_cap && !sw.predrop;
    pl.pre_mode = pl.predrop ? (in.pf_joint ? 2u : 1u) : 0u;

    const bool lean_list = fast && in.unit_list && !sw.lean_screen; // the stream has a unit list for the screen-only kernel
    if (in.lo == 0) // (a re-run after a match-buffer regrow starts the tallies again)
        pl.clear |= GN_CLEAR_SKIPPED | (pl.predrop ? GN_CLEAR_PRE : 0u);
    if (pl.predrop)
        pl.clear |= GN_CLEAR_SEGMIN;
    if (fast || split)
        pl.clear |= GN_CLEAR_DEFERRED;
    if (fast && !sw.on_demand)
        pl.clear |= GN_CLEAR_UNIT_CURSOR;
    if (lean_list)
        pl.clear |= GN_CLEAR_UNITS_LEFT;
    if (in.long_reads)
        pl.clear |= GN_CLEAR_LONG;

    // per launch: how many hashes a read of n minimisers is screened on with two of its rows (gn_screen_table.h; all zero = the flow
    // without a screen, which is also what "every row" needs)
    const bool ee   = pl.early_exit && in.gp_log2 == GN_FAST_EE_GP_LOG2; // the early exit only where a wave is one hash group (no cross-lane sums in its check)
    const bool wide = in.lw == 2 && in.W > 128;
    bool       scr  = false;
    if (fast && pl.early_exit && !sw.row_screen && (in.lw == 1 || in.W > 128))
    {
        pl.screen_filled    = true;
        pl.screen_unit_bins = (uint32_t)std::min<uint64_t>(in.W, 64u * in.lw) * 64u;
        gn_screen_table(in.rel_cutoff, in.h, pl.screen_unit_bins, pl.screen);
        for (uint8_t ds : pl.screen)
            scr = scr || ds != 0;
        scr = scr && ee && in.h == 4;
    }
    const bool whole = in.lo == 0 && in.hi == in.n_reads && !sw.deferred_grids; // a deferred list's grid may follow the last batch's list
    if (in.hi > in.lo)
    {
        const uint64_t reads = in.hi - in.lo, units = reads * in.wpr;
        auto           add = [&pl](GnCountFamily family, uint32_t blocks, uint64_t lds, GnCountList list_in, GnCountList list_out) -> GnCountLaunch& {
            GnCountLaunch& L = pl.launch[pl.n_launches++];
            L.family = family, L.blocks = blocks, L.lds_bytes = lds, L.list_in = list_in, L.list_out = list_out;
            return L;
        };
        if (split) // register counters + byte image for reads with <= 127 minimisers, the rest is deferred
            add(GN_COUNT_SPLIT, gn_plan_grid(reads, in.rpb, (uint64_t)in.n_cu * std::max(in.split_bpc, 1u) * 2u), in.split_lds_bytes, GN_LIST_NONE, GN_LIST_DEFERRED);
        if (fast)
        {
            GnRowPolicy pol; // (gn_row_policy.h: non-temporal row loads for a filter far past the caches)
            pol.flat       = !in.is_hibf;
            pol.plain_only = sw.stream_rows;
            pol.row_bytes  = in.S * in.W * 8ull;
            pol.min_bytes  = in.stream_rows_min_bytes;
            const bool     stream = gn_rows_stream(pol, in.h, in.lw, ee, wide, scr);
            const uint32_t base   = gn_plan_grid(units, GN_FAST_WAVES, (uint64_t)in.n_cu * (in.lw == 1 ? GN_FAST_BLOCKS_PER_CU_LW1 : GN_FAST_BLOCKS_PER_CU_LW2));
            const bool     lean   = scr && in.lw == 1 && lean_list;
            pl.streamed = stream;
            if (lean)
            {
                // the screen-only kernel, then the instance without a screen over the units it left: the list is usually short (reads
                // whose n has no table entry, aborted screens), so that grid follows the last batch's list (twice its length, four units a block)
                GnCountLaunch& L = add(GN_COUNT_LEAN, gn_plan_grid(units, GN_FAST_WAVES, (uint64_t)in.n_cu * GN_LEAN_BLOCKS_PER_CU), gn_lean_lds_bytes(), GN_LIST_NONE, GN_LIST_UNITS);
                L.stream = stream, L.grab = !sw.on_demand;
            }
            uint32_t blocks = base;
            if (lean && whole && in.prev_unit_deferred != ~0ull)
                blocks = (uint32_t)std::min<uint64_t>(blocks, std::max<uint64_t>(in.n_cu, in.prev_unit_deferred / 2 + 1));
            GnCountLaunch& L = add(GN_COUNT_FAST, lean ? std::max(blocks, 1u) : blocks, gn_fast_lds_bytes(in.h, in.lw, scr && !lean),
                                   lean ? GN_LIST_UNITS : GN_LIST_NONE, GN_LIST_DEFERRED);
            L.HF = (uint8_t)in.h, L.LW = (uint8_t)in.lw, L.EE = ee, L.WIDE = ee && wide, L.SCRN = scr && !lean;
            L.stream = stream && !lean; // (the list launch always loads plain)
            L.grab   = !lean && !sw.on_demand;
        }
        // the generic kernel: every read, or what the fast / split kernel deferred -- then a grid for twice the last batch's list (one block per read)
        uint32_t blocks = gn_generic_grid(reads, in.rpb, in.n_cu);
        if ((fast || split) && whole && in.prev_count_deferred != ~0ull)
            blocks = (uint32_t)std::min<uint64_t>(blocks, std::max<uint64_t>(in.n_cu, in.prev_count_deferred * 2));
        add(GN_COUNT_GENERIC, blocks, in.lds_bytes, fast || split ? GN_LIST_DEFERRED : GN_LIST_NONE, GN_LIST_NONE);
        if (in.long_reads) // reads the kernels above skipped as GN_READ_BIG: 32-bit counters, one workgroup each
            add(GN_COUNT_LONG, GN_LONG_BLOCKS, 0, GN_LIST_NONE, GN_LIST_NONE);
    }
    *out = pl;
}
