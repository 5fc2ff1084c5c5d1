// gn_stray_probe.h -- the staged probe of the fast count kernel's finish: when a bin the screen left is dropped (host and device).
//
// The screened flow (gn_kernels.hip, gn_screen_table.h) counts per bin c2 = the hashes q < ds whose rows 0 and 1 both have the
// bin's bit, and its survey keeps the bins with c2 + (n - ds) >= T.  A bin with c2 == ds is an error-free read's; any other is
// nearly always a stray, ahead on rows 0 and 1 by chance, with no slack left: c2 sits at or just above the bound.  Each of its hit
// hashes passes rows 2 and 3 with probability 1/4, so three or four of them settle it -- if the finish knows which hashes hit.  The
// screen keeps the hit masks of its first GN_PROBE_HASHES hashes (the AND of rows 0 and 1, as it is counted) for that:
//
//   stage 1   F' = min(F, ds); M = the bin's hit bits over q < F', m = popcount(M).  Rows 2 and 3 of exactly the hashes in M are
//             loaded (2 m words, one round trip): e = those with both bits = the bin's exact count over the first F' hashes.
//             The most the bin can still reach is e + (c2 - m) + (n - ds): below T it is dropped.
//   stage 2   rows 2 and 3 of the hashes F' <= q < ds (2 (ds - F') words): add = e + those with both bits, an upper bound of
//             the exact count over q < ds that is tighter by what stage 1 learnt.  add + (n - ds) < T: dropped.
//   else      every row of every hash is read from hash 0 (4 n words), as for a bin with c2 == ds beyond ds.
//
// Both tests are exact: a dropped bin cannot reach T whatever the words not read hold.  With F = 0 (switch stray_masks) stage 1
// loads nothing and never drops (the survey saw to c2 + (n - ds) >= T), and stage 2 is the one-stage probe of 2 ds words.
// Both finish sites of gn_kernels.hip call these; tests/test_stray_probe_cpu.py checks them by brute force.
#pragma once
#include <cstdint>

#ifndef GN_PROBE_HASHES
#define GN_PROBE_HASHES 4u // screened hashes whose hit masks are kept (model, lines a stray at n = 16 .. 19: 9.4 with 2, 7.0 with 4, 9.0 with 6, 11.9 with 8; 30 without)
#endif

#if defined(__HIPCC__) || defined(__CUDACC__)
#define GN_PROBE_HD __host__ __device__ inline
#else
#define GN_PROBE_HD inline
#endif

// F': the screened hashes stage 1 knows the hit bits of (F = 0: none, the one-stage probe)
GN_PROBE_HD uint32_t gn_probe_first(uint32_t F, uint32_t ds)
{
    return F < ds ? F : ds;
}

// after stage 1: e of the bin's m hit hashes below F' also have rows 2 and 3 (e <= m <= c2 <= ds <= n)
GN_PROBE_HD bool gn_probe_drop1(uint32_t n, uint32_t T, uint32_t ds, uint32_t c2, uint32_t m, uint32_t e)
{
    return e + (c2 - m) + (n - ds) < T;
}

// after stage 2: add = e + the hashes F' <= q < ds with the bit in rows 2 and 3
GN_PROBE_HD bool gn_probe_drop2(uint32_t n, uint32_t T, uint32_t ds, uint32_t add)
{
    return add + (n - ds) < T;
}
