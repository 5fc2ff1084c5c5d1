// gn_row_policy.h -- which cache policy the row loads of a fast count launch take (host only: no HIP in here).
//
// A filter far past the caches is read at random, every line once a wave: the 4 MiB L2 of an XCD and the 256 MiB Infinity Cache hold a
// few percent of it, and a plain load still allocates each line on its way through.  The stream kernels (gn_kernels.hip:
// gn_ibf_count_stream_kernel_lean, gn_ibf_count_stream_kernel<...>) are the fast count kernels with non-temporal row loads and nothing
// else changed.  Measured on a bare gather (scripts/calib_gather.hip, profiles/calib_gather_policy.json), 512-byte rows, plain -> nt:
// 32 MiB 8468 -> 7629 GB/s, 128 MiB 7606 -> 7077, 1 GiB 7137 -> 6796, 2 GiB 6740 -> 6771, 8 GiB 6143 -> 6634, 64 GiB 5970 -> 6151.
// A table the caches still serve part of loses with nt; from 2 GiB on it does not.
#pragma once
#include <cstdint>

// row storage from which a flat filter's launches take the stream kernels ($GANON_HIP_STREAM_ROWS_MIN_BYTES, gn_filter_set_stream_rows_min_bytes)
constexpr uint64_t GN_STREAM_ROWS_MIN_BYTES = 2ull << 30;

struct GnRowPolicy
{
    bool     flat       = false; // a flat IBF (no launch of an HIBF takes a stream kernel)
    bool     plain_only = false; // switch stream_rows: plain loads everywhere
    uint64_t row_bytes  = 0;     // the filter's row storage
    uint64_t min_bytes  = GN_STREAM_ROWS_MIN_BYTES;
};

// the fast kernel's instances that exist as stream kernels: the ones that screen -- four hash functions with the early exit, 8-byte lanes
// (the screen-only kernel, <4,1,true,false,true>) or 16-byte lanes on rows of more than 128 words (<4,2,true,true,true>).  The instances
// without a screen -- a launch at a low cutoff, the list launch -- keep plain loads: at --rel-cutoff 0.2 they ran slower with non-temporal
// row loads, 8-byte lanes on the 8 GiB benchmark filter by 1.6 % (129.3 - 129.5 against 131.0 - 131.7 Mreads/s), the wide one on the
// 128 GiB filter by 1.2 % (10.526 - 10.531 against 10.649 - 10.651): CHANGELOG.
static inline bool gn_stream_instance(uint32_t hash_funs, uint32_t lw, bool early_exit, bool wide, bool screens)
{
    return hash_funs == 4 && early_exit && screens && (lw == 1 ? !wide : (lw == 2 && wide));
}

static inline bool gn_rows_stream(const GnRowPolicy& pol, uint32_t hash_funs, uint32_t lw, bool early_exit, bool wide, bool screens)
{
    return pol.flat && !pol.plain_only && gn_stream_instance(hash_funs, lw, early_exit, wide, screens) && pol.row_bytes >= pol.min_bytes;
}
