// gn_emplace_window.h -- the arithmetic of gn_filter_emplace_runs_window (gn_build.hip) that is not the hash itself: how the runs of a call
// are cut into staging chunks and wave items, which bin a hash of an item belongs to, and whether a row of the WHOLE filter lies in the
// window of rows a slab filter stands for (`ganon-build --device-memory` / `--device a,b`: a flat filter built in row slabs).
// No device call in here: the item builder is host code, the bin and the window test compile for the host and for the device, so that a
// CPU program (tests/build_slabs_driver.cpp) runs the very code the kernel runs.
// What can go wrong, and where it is handled:
//   a run longer than a chunk   its later pieces carry `begin`, the index of the piece's first hash in the RUN: the bin of a hash is
//                               first_bin + (begin + q) / per_bin whatever the chunking (gn_window_bin)
//   an empty run                has no item; the cursor steps over it
//   a row below the window      row - row_begin wraps to a value at or above n_rows (both below 2^32): one unsigned compare answers
//                               "inside" for both ends (gn_window_local)
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define GN_WIN_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define GN_WIN_HD inline
#endif

#define GN_WIN_PER_LANE 8u                    // hashes a lane holds in registers
#define GN_WIN_ITEM (64u * GN_WIN_PER_LANE)   // ... and a wave's item: 512 hashes
#define GN_WIN_CHUNK (1ull << 20)             // hashes of a staging chunk when the caller names none (measured: gn_build.hip)

// A wave's piece of work: `cnt` consecutive hashes of run `run`, the first of them hash number `begin` of the run and word `stage_at`
// of the staging chunk.
struct GnRunItem
{
    uint32_t run, cnt;
    uint64_t begin, stage_at;
};

// A run as the kernel reads it: 16 bytes, one scalar load.
struct GnRunDev
{
    uint64_t per_bin;
    uint32_t first_bin, reserved;
};

// the technical bin of hash number `index` of a run (the rule of gn_filter_emplace_split)
GN_WIN_HD uint32_t gn_window_bin(uint32_t first_bin, uint64_t index, uint64_t per_bin)
{
    return first_bin + (uint32_t)(index / per_bin);
}

// The same for hash begin + q of an item, q < GN_WIN_ITEM, without a 64-bit division per hash: bin0 = gn_window_bin(first_bin, begin,
// per_bin) and r0 = begin % per_bin are the item's, divided out once.  r0 + q is below per_bin + GN_WIN_ITEM: with per_bin >= GN_WIN_ITEM
// the hash is in bin0 or the one behind it, otherwise both operands are below 2^10.
GN_WIN_HD uint32_t gn_window_item_bin(uint32_t bin0, uint64_t r0, uint32_t q, uint64_t per_bin)
{
    const uint64_t t = r0 + q;
    return bin0 + (per_bin >= GN_WIN_ITEM ? (uint32_t)(t >= per_bin) : (uint32_t)t / (uint32_t)per_bin);
}

// Is row `row` of the whole filter inside the window [row_begin, row_begin + n_rows)?  *local: its row in the slab (valid when inside).
GN_WIN_HD bool gn_window_local(uint32_t row, uint32_t row_begin, uint32_t n_rows, uint32_t* local)
{
    *local = row - row_begin;
    return *local < n_rows;
}

#include <vector>

// where the next chunk starts: hash `at` of run `run`
struct GnRunCursor
{
    uint32_t run = 0;
    uint64_t at  = 0;
};

// The items of the next staging chunk: hashes from the cursor on, runs in order, at most cap_hashes hashes and at most cap_items items
// (cap_hashes >= 1, cap_items >= 1).  An item never mixes runs and never exceeds GN_WIN_ITEM.  Returns the hashes taken -- 0 when the
// cursor is behind the last run -- and leaves the cursor behind them.
inline uint64_t gn_window_next_chunk(const uint64_t* run_sizes, uint32_t n_runs, GnRunCursor& cur, uint64_t cap_hashes, uint64_t cap_items,
                                     std::vector<GnRunItem>& items)
{
    items.clear();
    uint64_t taken = 0;
    while (cur.run < n_runs && taken < cap_hashes && items.size() < cap_items)
    {
        const uint64_t left = run_sizes[cur.run] - cur.at;
        if (left == 0)
        {
            ++cur.run, cur.at = 0;
            continue;
        }
        uint64_t cnt = left < GN_WIN_ITEM ? left : GN_WIN_ITEM;
        if (cnt > cap_hashes - taken)
            cnt = cap_hashes - taken;
        items.push_back(GnRunItem{ cur.run, (uint32_t)cnt, cur.at, taken });
        taken += cnt;
        cur.at += cnt;
    }
    return taken;
}
