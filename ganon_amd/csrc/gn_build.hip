// gn_build.hip -- build-side device work behind the C ABI (the ganon-build half of the minimiser/IBF code):
//   gn_stream_distinct_hashes  the set of minimiser hashes of the sequences resident in a stream, sorted ascending
//                              (count_hashes' robin_hood::unordered_set per file, /root/reference/src/ganon-build/GanonBuild.cpp:184-249)
//   gn_filter_emplace_split    insert a target's hashes into its run of technical bins, equal shares per bin
//                              (create_bin_map_hash :619-653 + build :655-698: hash i of the target goes to bin
//                              first_bin + i / hashes_per_bin)
// HBM-bound integer work: a radix sort (hipCUB) over the hash array, a unique pass, an atomic-OR scatter.
#include "gn_internal.h"
#include <hipcub/hipcub.hpp>

#include "gn_build_row.h" // gn_build_row: seqan3::interleaved_bloom_filter's hash_and_fit

// hashes live in per-read slots (one slot per window, gn_slot_count_kernel); read r used the first nh[r] of them
__global__ void gn_pack_hashes_kernel(const uint64_t* __restrict__ hashes, const uint64_t* __restrict__ slot_off,
                                      const uint32_t* __restrict__ nh, uint32_t n_reads, uint64_t* __restrict__ out,
                                      unsigned long long* __restrict__ cursor)
{
    const uint32_t wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const uint32_t lane = threadIdx.x & 63u;
    if (wave >= n_reads)
        return;
    const uint32_t     c = nh[wave];
    const uint64_t     b = slot_off[wave];
    unsigned long long o = 0;
    if (lane == 0 && c)
        o = atomicAdd(cursor, (unsigned long long)c); // order is irrelevant: the array is sorted next
    o = ((unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(o >> 32)) << 32) |
        (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)o);
    for (uint32_t j = lane; j < c; j += 64)
        out[o + j] = hashes[b + j];
}

static int gn_build_reserve(gn_stream* s, uint64_t n)
{
    if (s->build.cap >= n)
        return GN_OK;
    // built aside and moved into the stream when it is whole: a failed allocation leaves the stream without the group
    GnBuildBufs b;
    b.d_ctr  = std::move(s->build.d_ctr); // (the counters do not grow)
    s->build = GnBuildBufs{};             // free before malloc
    const uint64_t cap = n + n / 8 + 1024;
    GN_HIP(b.d_build[0].alloc(cap));
    GN_HIP(b.d_build[1].alloc(cap));
    if (!b.d_ctr)
        GN_HIP(b.d_ctr.alloc(2));
    size_t x = 0, y = 0;
    hipcub::DeviceRadixSort::SortKeys(nullptr, x, b.d_build[0].get(), b.d_build[1].get(), (int)cap, 0, 64, s->st);
    hipcub::DeviceSelect::Unique(nullptr, y, b.d_build[1].get(), b.d_build[0].get(), b.d_ctr + 1, (int)cap, s->st);
    b.tmp_bytes = x > y ? x : y;
    GN_HIP(b.d_tmp.alloc(b.tmp_bytes));
    b.cap    = cap;
    s->build = std::move(b);
    return GN_OK;
}

extern "C" int gn_stream_distinct_hashes(gn_stream* s, uint64_t* out, uint64_t cap, uint64_t* n_distinct)
{
    if (!s || !n_distinct)
        return gn_fail(GN_EINVAL, "null argument");
    if (!s->hashed)
        return gn_fail(GN_EINVAL, "no minimisers computed on this stream");
    GN_HIP(hipSetDevice(s->device));
    *n_distinct = 0;
    const uint32_t n = s->n_reads;
    if (n == 0)
        return GN_OK;
    if (s->build_distinct != ~0ull) // asked before for these hashes (size query, then fetch): the sorted set is still there
    {
        *n_distinct = s->build_distinct;
        if (!out || s->build_distinct == 0)
            return GN_OK;
        if (cap < s->build_distinct)
            return gn_fail(GN_EOVERFLOW, "hash buffer too small: need %llu", (unsigned long long)s->build_distinct);
        GN_HIP(hipMemcpy(out, s->build.d_build[0], s->build_distinct * 8, hipMemcpyDeviceToHost));
        return GN_OK;
    }
    // every read's count is at most its window count, so the slot total bounds the packed size
    uint64_t slots = 0;
    GN_HIP(hipMemcpyAsync(&slots, s->d_slot_off + n, 8, hipMemcpyDeviceToHost, s->st));
    GN_HIP(hipStreamSynchronize(s->st));
    if (slots == 0)
    {
        s->build_distinct = 0;
        return GN_OK;
    }
    if (slots + slots / 8 + 1024 > 0x7FFFFFFFull) // (the sort / unique calls take their item count -- the reserved capacity -- as an int)
        return gn_fail(GN_ERANGE, "more than 1.9 * 10^9 minimiser windows in one batch");
    int rc = gn_build_reserve(s, slots);
    if (rc)
        return rc;
    GN_HIP(hipMemsetAsync(s->build.d_ctr, 0, 2 * sizeof(unsigned long long), s->st));
    hipLaunchKernelGGL(gn_pack_hashes_kernel, dim3((unsigned)(((uint64_t)n * 64 + 255) / 256)), dim3(256), 0, s->st, s->d_hashes,
                       s->d_slot_off, s->d_nh, n, s->build.d_build[0], s->build.d_ctr);
    GN_HIP(hipGetLastError());
    unsigned long long total = 0;
    GN_HIP(hipMemcpyAsync(&total, s->build.d_ctr, 8, hipMemcpyDeviceToHost, s->st));
    GN_HIP(hipStreamSynchronize(s->st));
    if (total == 0)
    {
        s->build_distinct = 0;
        return GN_OK;
    }
    size_t    tmp      = s->build.tmp_bytes;
    const int end_bit  = (int)(2 * s->k > 64 ? 64 : 2 * s->k); // values are below 4^k
    GN_HIP(hipcub::DeviceRadixSort::SortKeys(s->build.d_tmp, tmp, s->build.d_build[0].get(), s->build.d_build[1].get(), (int)total, 0, end_bit, s->st));
    tmp = s->build.tmp_bytes;
    GN_HIP(hipcub::DeviceSelect::Unique(s->build.d_tmp, tmp, s->build.d_build[1].get(), s->build.d_build[0].get(), s->build.d_ctr + 1, (int)total, s->st));
    unsigned long long nd = 0;
    GN_HIP(hipMemcpyAsync(&nd, s->build.d_ctr + 1, 8, hipMemcpyDeviceToHost, s->st));
    GN_HIP(hipStreamSynchronize(s->st));
    *n_distinct       = nd;
    s->build_distinct = nd;
    if (!out)
        return GN_OK;
    if (cap < nd)
        return gn_fail(GN_EOVERFLOW, "hash buffer too small: need %llu", nd);
    GN_HIP(hipMemcpy(out, s->build.d_build[0], nd * 8, hipMemcpyDeviceToHost));
    return GN_OK;
}

__global__ void gn_emplace_split_kernel(uint64_t* rows, uint64_t S, uint32_t W, uint32_t shift, uint32_t h,
                                        const uint64_t* __restrict__ hashes, uint64_t n, uint32_t first_bin, uint64_t per_bin,
                                        uint64_t index_base)
{
    const uint64_t idx = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n * h)
        return;
    const uint64_t q   = idx / h;
    const uint32_t i   = (uint32_t)(idx - q * h);
    const uint32_t bin = first_bin + (uint32_t)((index_base + q) / per_bin);
    const uint32_t row = gn_build_row(hashes[q], i, shift, S);
    atomicOr(reinterpret_cast<unsigned long long*>(rows + ((uint64_t)row * W + (bin >> 6))), 1ULL << (bin & 63));
}

extern "C" int gn_filter_emplace_split(gn_filter* f, const uint64_t* hashes, uint64_t n, uint32_t first_bin, uint64_t hashes_per_bin)
{
    if (!f || f->is_hibf)
        return gn_fail(GN_EINVAL, "gn_filter_emplace_split needs a flat IBF filter");
    if (n == 0)
        return GN_OK;
    if (!hashes || hashes_per_bin == 0)
        return gn_fail(GN_EINVAL, "bad argument");
    GnIbfHost& ib = f->ibf;
    if ((uint64_t)first_bin + (n - 1) / hashes_per_bin >= ib.B)
        return gn_fail(GN_EINVAL, "bins %u.. exceed the filter's %llu bins", first_bin, (unsigned long long)ib.B);
    GN_HIP(hipSetDevice(f->device));
    if (!f->load_st)
        GN_HIP(hipStreamCreateWithFlags(&f->load_st, hipStreamNonBlocking));
    // staged through a device buffer that stays with the filter (grown to the largest request so far), at most 32 M hashes
    // at a time
    const uint64_t step = n < (32ull << 20) ? n : (32ull << 20);
    GN_HIP(f->d_emplace_stage.reserve(step, step));
    for (uint64_t done = 0; done < n; done += step)
    {
        const uint64_t c = n - done < step ? n - done : step;
        GN_HIP(hipMemcpyAsync(f->d_emplace_stage, hashes + done, c * 8, hipMemcpyHostToDevice, f->load_st));
        const uint64_t total  = c * ib.h;
        const unsigned blocks = (unsigned)((total + 255) / 256);
        hipLaunchKernelGGL(gn_emplace_split_kernel, dim3(blocks), dim3(256), 0, f->load_st, ib.d_rows, ib.S, (uint32_t)ib.Ws, ib.shift,
                           ib.h, f->d_emplace_stage, c, first_bin, hashes_per_bin, done);
        GN_HIP(hipGetLastError());
        GN_HIP(hipStreamSynchronize(f->load_st)); // (the staging buffer is reused, and `hashes` may be pageable)
    }
    return GN_OK;
}

// ---- gn_filter_probe: the check of the reference's build test (tests/ganon-build/GanonBuild.test.cpp:53-98) on the device ------
// For every hash: in how many of the given technical bins are all h of its bits set?  hits = the sum over hashes (what the
// reference compares with hashes.size() after bulk_count: the target's bins' counts added up), missing = hashes that are in
// none of the bins (a false negative: the filter was not built from this sequence, or it is read with the wrong row / bin
// arithmetic), first = the smallest index of such a hash.  One lane per hash; h row words per (hash, bin) -- a few MB of
// gathered words per genome, nothing to tune.
__global__ void gn_probe_kernel(const uint64_t* __restrict__ rows, uint64_t S, uint32_t W, uint32_t shift, uint32_t h,
                                const uint64_t* __restrict__ hashes, uint64_t n, const uint32_t* __restrict__ bins, uint32_t n_bins,
                                uint64_t index_base, unsigned long long* __restrict__ out /* hits, missing, first */)
{
    const uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n)
        return;
    uint32_t row[5];
    for (uint32_t i = 0; i < h; ++i)
        row[i] = gn_build_row(hashes[q], i, shift, S);
    uint32_t found = 0;
    for (uint32_t b = 0; b < n_bins; ++b)
    {
        const uint32_t bin = bins[b];
        uint64_t       all = 1;
        for (uint32_t i = 0; i < h; ++i)
            all &= rows[(uint64_t)row[i] * W + (bin >> 6)] >> (bin & 63);
        found += (uint32_t)(all & 1);
    }
    if (found)
        atomicAdd(out, (unsigned long long)found);
    else
    {
        atomicAdd(out + 1, 1ull);
        atomicMin(out + 2, (unsigned long long)(index_base + q));
    }
}

extern "C" int gn_filter_probe(gn_filter* f, const uint64_t* hashes, uint64_t n, const uint32_t* bins, uint32_t n_bins, uint64_t* hits,
                               uint64_t* missing, uint64_t* first_missing)
{
    if (!f || f->is_hibf)
        return gn_fail(GN_EINVAL, "gn_filter_probe needs a flat IBF filter");
    if (!hits || !missing || !first_missing || (n && !hashes) || (n_bins && !bins))
        return gn_fail(GN_EINVAL, "gn_filter_probe: null argument");
    *hits = *missing = 0;
    *first_missing = ~0ull;
    if (n == 0)
        return GN_OK;
    GnIbfHost& ib = f->ibf;
    for (uint32_t b = 0; b < n_bins; ++b)
        if (bins[b] >= ib.B)
            return gn_fail(GN_EINVAL, "gn_filter_probe: bin %u of a filter with %llu bins", bins[b], (unsigned long long)ib.B);
    GN_HIP(hipSetDevice(f->device));
    if (!f->load_st)
        GN_HIP(hipStreamCreateWithFlags(&f->load_st, hipStreamNonBlocking));
    const uint64_t step = n < (32ull << 20) ? n : (32ull << 20);
    GN_HIP(f->d_emplace_stage.reserve(step, step));
    GnDev<uint32_t>           d_bins;
    GnDev<unsigned long long> d_out;
    unsigned long long        init[3] = { 0, 0, ~0ull };
    GN_HIP(d_bins.alloc(n_bins));
    GN_HIP(d_out.alloc(3));
    if (n_bins)
        GN_HIP(hipMemcpyAsync(d_bins, bins, (size_t)n_bins * 4, hipMemcpyHostToDevice, f->load_st));
    GN_HIP(hipMemcpyAsync(d_out, init, sizeof(init), hipMemcpyHostToDevice, f->load_st));
    for (uint64_t done = 0; done < n; done += step)
    {
        const uint64_t c = n - done < step ? n - done : step;
        GN_HIP(hipMemcpyAsync(f->d_emplace_stage, hashes + done, c * 8, hipMemcpyHostToDevice, f->load_st));
        hipLaunchKernelGGL(gn_probe_kernel, dim3((unsigned)((c + 255) / 256)), dim3(256), 0, f->load_st, ib.d_rows, ib.S, (uint32_t)ib.Ws, ib.shift,
                           ib.h, f->d_emplace_stage, c, d_bins, n_bins, done, d_out);
        GN_HIP(hipGetLastError());
        GN_HIP(hipStreamSynchronize(f->load_st)); // (the staging buffer is reused, and `hashes` may be pageable)
    }
    GN_HIP(hipMemcpy(init, d_out, sizeof(init), hipMemcpyDeviceToHost));
    *hits          = init[0];
    *missing       = init[1];
    *first_missing = init[2];
    return GN_OK;
}
