// gn_build_row.h -- the row of a hash in an IBF, for the build-side kernels (gn_build.hip, gn_build_hibf.hip):
// seqan3::interleaved_bloom_filter hash seeds and hash_and_fit, as in gn_kernels.hip
#pragma once
#include "gn_internal.h"

static __constant__ uint64_t GN_BUILD_SEEDS[GN_IBF_MAX_HASH_FUNS] = GN_IBF_SEED_LIST;   // include/ganon_ibf_hash.h
__device__ __forceinline__ uint32_t gn_build_row(uint64_t v, uint32_t i, uint32_t shift, uint64_t S)
{
    uint64_t x = v * GN_BUILD_SEEDS[i];
    x ^= x >> shift;
    x *= GN_IBF_MULTIPLIER;
    return (uint32_t)__umul64hi(x, S);
}
