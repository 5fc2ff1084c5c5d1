// gn_path_window.h -- the arithmetic of gn_filter_emplace_path_window (gn_build_hibf.hip) that is not the hash itself: the path entry as
// the kernel reads it, which bin a hash of an item belongs to in an entry, and whether a row of the WHOLE IBF lies in the piece of rows the
// filter's IBF stands for (`ganon-build --hibf --hibf-memory` / `--hibf-devices`: a hierarchical filter built in parts).  The items, the
// staging chunks and the window test are those of the flat windowed insert (gn_emplace_window.h), with the sets of a call as its runs.
// No device call in here: everything compiles for the host and for the device, so that a CPU program
// (tests/build_hibf_parts_driver.cpp) runs the very code the kernel runs.
// What can go wrong, and where it is handled:
//   a single bin (n_bins == 1)  every hash of the set goes to first_bin: nothing is divided (a merged bin above the user bin)
//   a set longer than a chunk   its later items carry `begin`, the index in the SET: gn_path_window_start divides it out once per entry
//   a piece no row falls into   every window test fails; the piece stays as it was
#pragma once

#include "gn_emplace_window.h"

// One path entry as the kernel reads it: the geometry of the WHOLE IBF (S_total, shift) and the piece of it this filter holds, resolved
// on the host, so that a level costs one 48-byte scalar read.
struct GnPathWinDev
{
    uint64_t* rows;           // the piece: n_rows rows of Ws words
    uint64_t  S_total;        // rows of the whole IBF
    uint64_t  per_bin;        // hashes a bin of the run (n_bins > 1)
    uint32_t  Ws, shift;      // words from one row to the next; countl_zero(S_total)
    uint32_t  first_bin, n_bins; // n_bins == 0: the path ends above this entry
    uint32_t  row_begin, n_rows; // the piece is rows [row_begin, row_begin + n_rows) of the whole IBF
};

// The item's first bin in an entry and the index of its first hash inside that bin, divided out once per (item, entry): wave-uniform.
GN_WIN_HD void gn_path_window_start(uint32_t first_bin, uint32_t n_bins, uint64_t per_bin, uint64_t begin, uint32_t* bin0, uint64_t* r0)
{
    const uint64_t b0 = n_bins == 1 ? 0 : begin / per_bin;
    *bin0             = first_bin + (uint32_t)b0;
    *r0               = begin - b0 * per_bin;
}

// the bin of hash begin + q of the item, q < GN_WIN_ITEM (gn_window_item_bin: no 64-bit division per hash)
GN_WIN_HD uint32_t gn_path_window_bin(uint32_t bin0, uint64_t r0, uint32_t q, uint32_t n_bins, uint64_t per_bin)
{
    return n_bins == 1 ? bin0 : gn_window_item_bin(bin0, r0, q, per_bin);
}
