// gn_packed_decode.h -- the one decode of a packed block (gn_packed_set.h) on the device: a wave takes a block, lane L its hashes
// 8L .. 8L + 7.  Called by the flat packed insert (gn_emplace_packed_window_kernel, gn_build.hip), by the packed path insert
// (gn_emplace_path_packed_window_kernel, gn_build_hibf.hip) and by the kernel that writes the hashes out for the sort of gn_packed_union
// and the staging buffer of gn_sketches_create_packed (gn_packed_decode_kernel, gn_build.hip): one 64-bit wave scan with its width-0 and
// width-64 edges, not three.  Device code only; the host's decoder is gn_packed_decode (gn_packed_set.h).
#pragma once

#include <hip/hip_runtime.h>

#include "gn_packed_set.h"

// The lane's hashes of a block of `cnt` hashes at `width` bits a delta whose payload starts at `words`: v[j] = hash 8 * lane + j for
// 8 * lane + j < cnt (what lies behind the block's last hash repeats it and is not to be used).  The lane extracts deltas 8L .. 8L + 7 --
// `width` bytes of the payload, adjacent lanes adjacent bytes; a delta past the block's last is not read -- and sums them; an inclusive
// scan of the lane sums across the wave, less the lane's own sum, plus `first` is hash 8L; the deltas lead from it to the seven behind
// it, in place.  All 64 lanes of the wave have to call it (the scan shuffles).
__device__ __forceinline__ void gn_packed_lane_hashes(const uint64_t* __restrict__ words, uint32_t cnt, uint32_t width, uint64_t first, uint32_t lane,
                                                      uint64_t (&v)[GN_WIN_PER_LANE])
{
    uint64_t sum = 0;
#pragma unroll
    for (uint32_t j = 0; j < GN_WIN_PER_LANE; ++j)
    {
        const uint32_t e = lane * GN_WIN_PER_LANE + j;
        v[j]             = e + 1 < cnt ? gn_packed_delta(words, e, width) : 0;
        sum += v[j];
    }
    uint64_t incl = sum;
#pragma unroll
    for (uint32_t o = 1; o < 64; o <<= 1)
    {
        const uint64_t below = __shfl_up(incl, o);
        if (lane >= o)
            incl += below;
    }
    uint64_t x = first + (incl - sum);
#pragma unroll
    for (uint32_t j = 0; j < GN_WIN_PER_LANE; ++j)
    {
        const uint64_t d = v[j];
        v[j]             = x;
        x += d;
    }
}
