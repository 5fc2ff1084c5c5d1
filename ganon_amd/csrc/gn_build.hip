// gn_build.hip -- build-side device work behind the C ABI (the ganon-build half of the minimiser/IBF code):
//   gn_stream_distinct_hashes  the set of minimiser hashes of the sequences resident in a stream, sorted ascending
//                              (count_hashes' robin_hood::unordered_set per file, /root/reference/src/ganon-build/GanonBuild.cpp:184-249)
//   gn_filter_emplace_split    insert a target's hashes into its run of technical bins, equal shares per bin
//                              (create_bin_map_hash :619-653 + build :655-698: hash i of the target goes to bin
//                              first_bin + i / hashes_per_bin)
//   gn_stream_distinct_hashes_packed  that set packed where it lies, as blocks of deltas of fixed width (gn_packed_set.h)
//   gn_filter_emplace_runs_window  the same rule for many runs in one call, into a filter that stands for a window of the rows of a
//                              larger one: one launch per staging chunk, uploads under the kernels (a flat filter built in row slabs)
//   gn_filter_emplace_packed_window  its twin for packed runs: the staging moves payload words, the kernel decodes a block per wave
// HBM-bound integer work: a radix sort (hipCUB) over the hash array, a unique pass, an atomic-OR scatter.
#include "gn_internal.h"
#include <hipcub/hipcub.hpp>

#include "gn_build_row.h" // gn_build_row: seqan3::interleaved_bloom_filter's hash_and_fit
#include "gn_emplace_window.h"
#include "gn_packed_decode.h"
#include "gn_packed_set.h"
#include "gn_scan.h"

#include <algorithm>
#include <string.h>
#include <vector>

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
    s->pack_words = ~0ull; // (a new set: what gn_stream_distinct_hashes_packed made of the last one is stale)
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

// ---- gn_stream_distinct_hashes_packed: the sorted set, packed where it lies ------------------------------------------------------
// One wave per block of 512 hashes, twice: the first kernel finds the block's width and payload length, a scan over the lengths gives
// every block its place in the payload, the second kernel writes the deltas.  A lane holds 8 consecutive hashes and the last hash of
// the lane before it, so delta e = q - 1 leads to the lane's hash q.  No global atomics: a block's words are assembled in LDS (a delta
// may share a word with those of other lanes) and stored coalesced.
static_assert(sizeof(gn_packed_block) == sizeof(GnPackedBlock) && offsetof(gn_packed_block, word_at) == offsetof(GnPackedBlock, word_at) &&
                  offsetof(gn_packed_block, cnt) == offsetof(GnPackedBlock, cnt) && offsetof(gn_packed_block, width) == offsetof(GnPackedBlock, width),
              "gn_packed_block (ganon_hip.h) is GnPackedBlock (gn_packed_set.h)");

// the lane's deltas d[j] = v[q] - v[q - 1], q = 8 * lane + j, of a block of cnt hashes that starts at `v`; 0 where there is none
__device__ __forceinline__ void gn_pack_lane_deltas(const uint64_t* __restrict__ v, uint32_t cnt, uint32_t lane, uint64_t (&d)[GN_WIN_PER_LANE])
{
    const uint32_t q0   = lane * GN_WIN_PER_LANE;
    uint64_t       prev = q0 >= 1 && q0 - 1 < cnt ? v[q0 - 1] : 0;
#pragma unroll
    for (uint32_t j = 0; j < GN_WIN_PER_LANE; ++j)
    {
        const uint32_t q = q0 + j;
        const uint64_t x = q < cnt ? v[q] : 0;
        d[j]             = q >= 1 && q < cnt ? x - prev : 0;
        prev             = x;
    }
}

__global__ __launch_bounds__(256) void gn_pack_width_kernel(const uint64_t* __restrict__ v, uint64_t n, GnPackedBlock* __restrict__ blocks,
                                                            uint32_t* __restrict__ words, uint32_t n_blocks)
{
    const uint32_t b = (uint32_t)__builtin_amdgcn_readfirstlane((int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6));
    if (b >= n_blocks)
        return;
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t base = (uint64_t)b * GN_WIN_ITEM;
    const uint32_t cnt  = (uint32_t)(n - base < GN_WIN_ITEM ? n - base : GN_WIN_ITEM);
    uint64_t       d[GN_WIN_PER_LANE];
    gn_pack_lane_deltas(v + base, cnt, lane, d);
    uint64_t widest = 0; // (the OR of the deltas has the bit length of the largest)
#pragma unroll
    for (uint32_t j = 0; j < GN_WIN_PER_LANE; ++j)
        widest |= d[j];
#pragma unroll
    for (uint32_t o = 32; o >= 1; o >>= 1)
        widest |= __shfl_xor(widest, o);
    if (lane == 0)
    {
        const uint32_t width = gn_packed_bits(widest);
        blocks[b]            = GnPackedBlock{ v[base], 0, cnt, width };
        words[b]             = gn_packed_words(cnt, width);
        if (b == 0)
            words[n_blocks] = 0; // (the scan runs over one entry more: its last offset is the total)
    }
}

__global__ __launch_bounds__(256) void gn_pack_payload_kernel(const uint64_t* __restrict__ v, uint64_t n, GnPackedBlock* __restrict__ blocks,
                                                              const uint64_t* __restrict__ word_at, uint64_t* __restrict__ payload, uint32_t n_blocks)
{
    __shared__ unsigned long long lds[4][GN_WIN_ITEM];
    const uint32_t b    = (uint32_t)__builtin_amdgcn_readfirstlane((int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6));
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    const bool     live = b < n_blocks; // (every wave of the workgroup reaches both barriers)
    const uint64_t base = (uint64_t)b * GN_WIN_ITEM;
    const uint32_t cnt = live ? blocks[b].cnt : 0, width = live ? blocks[b].width : 0, n_words = live ? gn_packed_words(cnt, width) : 0;
    const uint64_t at = live ? word_at[b] : 0;
    for (uint32_t w = lane; w < n_words; w += 64)
        lds[wv][w] = 0;
    __syncthreads();
    if (live && width)
    {
        uint64_t d[GN_WIN_PER_LANE];
        gn_pack_lane_deltas(v + base, cnt, lane, d);
#pragma unroll
        for (uint32_t j = 0; j < GN_WIN_PER_LANE; ++j)
        {
            const uint32_t q = lane * GN_WIN_PER_LANE + j;
            if (q < 1 || q >= cnt)
                continue;
            const uint32_t bit = (q - 1) * width, w = bit >> 6, off = bit & 63u; // (gn_packed_put, with ORs that other lanes may share)
            atomicOr(&lds[wv][w], (unsigned long long)(d[j] << off));
            if (off + width > 64)
                atomicOr(&lds[wv][w + 1], (unsigned long long)(d[j] >> (64u - off)));
        }
    }
    __syncthreads();
    for (uint32_t w = lane; w < n_words; w += 64)
        payload[at + w] = lds[wv][w];
    if (live && lane == 0)
        blocks[b].word_at = at;
}

static int gn_pack_reserve(gn_stream* s, uint64_t n_blocks)
{
    if (s->pack.cap >= n_blocks)
        return GN_OK;
    GnPackBufs     b;
    const uint64_t cap = n_blocks + n_blocks / 8 + 64;
    s->pack            = GnPackBufs{}; // free before malloc
    GN_HIP(b.d_blocks.alloc(cap));
    GN_HIP(b.d_words.alloc(cap + 1));
    GN_HIP(b.d_off.alloc(cap + 1));
    GN_HIP(gn_scan_counts(nullptr, b.tmp_bytes, b.d_words.get(), b.d_off.get(), (int)(cap + 1), s->st));
    GN_HIP(b.d_tmp.alloc(b.tmp_bytes));
    b.cap   = cap;
    s->pack = std::move(b);
    return GN_OK;
}

extern "C" int gn_stream_distinct_hashes_packed(gn_stream* s, gn_packed_block* blocks, uint64_t cap_blocks, uint64_t* payload, uint64_t cap_words,
                                                uint64_t* n_distinct, uint64_t* n_blocks, uint64_t* n_words)
{
    if (!s || !n_distinct || !n_blocks || !n_words)
        return gn_fail(GN_EINVAL, "null argument");
    *n_distinct = *n_blocks = *n_words = 0;
    uint64_t nd = 0;
    int      rc = gn_stream_distinct_hashes(s, nullptr, 0, &nd); // (sorts and uniques, or finds the set of an earlier call)
    if (rc)
        return rc;
    *n_distinct = nd;
    if (nd == 0)
        return GN_OK;
    if (s->pack_words == ~0ull)
    {
        const uint64_t nb = gn_packed_max_blocks(nd); // (one set: every block but the last is full)
        rc                = gn_pack_reserve(s, nb);
        if (rc)
            return rc;
        const dim3 grid((unsigned)((nb + 3) / 4));
        hipLaunchKernelGGL(gn_pack_width_kernel, grid, dim3(256), 0, s->st, (const uint64_t*)s->build.d_build[0], nd, s->pack.d_blocks.get(),
                           s->pack.d_words.get(), (uint32_t)nb);
        GN_HIP(hipGetLastError());
        size_t tmp = s->pack.tmp_bytes;
        GN_HIP(gn_scan_counts(s->pack.d_tmp, tmp, s->pack.d_words.get(), s->pack.d_off.get(), (int)(nb + 1), s->st));
        // the payload takes the sort's second buffer: it holds nd hashes or more, a packed set fewer words than hashes
        hipLaunchKernelGGL(gn_pack_payload_kernel, grid, dim3(256), 0, s->st, (const uint64_t*)s->build.d_build[0], nd, s->pack.d_blocks.get(),
                           (const uint64_t*)s->pack.d_off, s->build.d_build[1].get(), (uint32_t)nb);
        GN_HIP(hipGetLastError());
        uint64_t total = 0;
        GN_HIP(hipMemcpyAsync(&total, s->pack.d_off + nb, 8, hipMemcpyDeviceToHost, s->st));
        GN_HIP(hipStreamSynchronize(s->st));
        s->pack_blocks = nb;
        s->pack_words  = total;
    }
    *n_blocks = s->pack_blocks;
    *n_words  = s->pack_words;
    if (!blocks && !payload)
        return GN_OK;
    if (!blocks || (!payload && s->pack_words))
        return gn_fail(GN_EINVAL, "null argument");
    if (cap_blocks < s->pack_blocks || cap_words < s->pack_words)
        return gn_fail(GN_EOVERFLOW, "packed buffers too small: need %llu blocks and %llu words", (unsigned long long)s->pack_blocks,
                       (unsigned long long)s->pack_words);
    GN_HIP(hipMemcpy(blocks, s->pack.d_blocks, s->pack_blocks * sizeof(GnPackedBlock), hipMemcpyDeviceToHost));
    if (s->pack_words)
        GN_HIP(hipMemcpy(payload, s->build.d_build[1], s->pack_words * 8, hipMemcpyDeviceToHost));
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

// ---- gn_filter_emplace_runs_window: many runs into a slab of rows ------------------------------------------------------------------
// The filter stands for rows [row_begin, row_begin + S) of a filter of total_rows rows (`ganon-build --device-memory`, `--device a,b`:
// build_slabs.cpp).  A hash's rows depend on the hash and on the WHOLE filter's row count alone, so every slab is filled from the same
// hash sets and takes the bits of the rows it holds.
typedef __attribute__((address_space(1))) unsigned long long GnGlobalWord;

// One wave per item, as gn_emplace_path_kernel (gn_build_hibf.hip): the item index goes through readfirstlane so that item and run are
// read with scalar loads into SGPRs; the lane's hashes are loaded first, from then on the wave only issues no-return atomic ORs.  The
// item's first bin is divided out once for the wave (gn_window_item_bin); a row outside the window costs its hash and one compare.
__global__ __launch_bounds__(256) void gn_emplace_window_kernel(uint64_t* rows, uint64_t S_total, uint32_t shift, uint32_t W, uint32_t h, uint32_t row_begin,
                                                                uint32_t n_rows, const uint64_t* __restrict__ stage, const GnRunItem* __restrict__ items,
                                                                uint32_t n_items, const GnRunDev* __restrict__ runs)
{
    const uint32_t item = (uint32_t)__builtin_amdgcn_readfirstlane((int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6));
    if (item >= n_items)
        return;
    const uint32_t  lane = threadIdx.x & 63u;
    const GnRunItem it   = items[item];
    const GnRunDev  run  = runs[it.run];
    uint64_t        v[GN_WIN_PER_LANE];
#pragma unroll
    for (uint32_t j = 0; j < GN_WIN_PER_LANE; ++j)
    {
        const uint32_t q = j * 64u + lane;
        v[j]             = q < it.cnt ? stage[it.stage_at + q] : 0;
    }
    const uint64_t b0   = it.begin / run.per_bin; // (wave-uniform: once per item)
    const uint64_t r0   = it.begin - b0 * run.per_bin;
    const uint32_t bin0 = run.first_bin + (uint32_t)b0;
#pragma unroll
    for (uint32_t j = 0; j < GN_WIN_PER_LANE; ++j)
    {
        const uint32_t q = j * 64u + lane;
        if (q >= it.cnt)
            continue;
        const uint32_t bin  = gn_window_item_bin(bin0, r0, q, run.per_bin);
        GnGlobalWord*  word = (GnGlobalWord*)rows + (bin >> 6);
        const uint64_t bit  = 1ULL << (bin & 63);
        for (uint32_t i = 0; i < h; ++i)
        {
            uint32_t local;
            if (gn_window_local(gn_build_row(v[j], i, shift, S_total), row_begin, n_rows, &local))
                (void)__hip_atomic_fetch_or(word + (uint64_t)local * W, bit, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

// Hashes of a staging chunk when the caller names none (GN_WIN_CHUNK, gn_emplace_window.h): 8 MiB, two of them page-locked and two on the
// device.  Page-locking is paid per call: one insert of 287 M hashes into a quarter of a filter's rows took 0.118 s with chunks of 4 Mi
// hashes, 0.080 s with 1 Mi, 0.098 s with 256 Ki and 0.155 s with 64 Ki (launches and waits take over).
namespace
{
struct GnWindowStage // everything a call holds; freed when the call returns
{
    GnStreamPair        streams;
    GnPinned<uint64_t>  h_stage[2];
    GnPinned<GnRunItem> h_items[2];
    GnDev<uint64_t>     d_stage[2];
    GnDev<GnRunItem>    d_items[2];
    GnDev<GnRunDev>     d_runs;
};
} // namespace

// Chunk c goes through buffer and stream c & 1: its hashes are gathered into the page-locked buffer, copied and inserted on that
// stream, while chunk c - 1 is still on the other one -- the upload of a chunk runs under the kernel of the one before.  A buffer is
// written again only after its stream has been waited for.
static int gn_runs_window_rounds(gn_filter* f, GnWindowStage& g, const uint64_t* const* runs, const uint64_t* run_sizes, uint32_t n_runs, uint64_t total_rows,
                                 uint64_t row_begin, uint64_t chunk, uint64_t cap_items)
{
    const GnIbfHost&       ib = f->ibf;
    std::vector<GnRunItem> items;
    GnRunCursor            cur;
    for (uint32_t c = 0;; ++c)
    {
        const uint32_t b = c & 1u;
        GN_HIP(hipStreamSynchronize(g.streams.st[b]));
        const uint64_t taken = gn_window_next_chunk(run_sizes, n_runs, cur, chunk, cap_items, items);
        if (taken == 0)
            return GN_OK;
        // (one thread gathers: with chunks of 4 Mi hashes four of them made a pass over a slab 5 % shorter, within the spread of the runs)
        for (const GnRunItem& it : items)
            memcpy(g.h_stage[b] + it.stage_at, runs[it.run] + it.begin, (size_t)it.cnt * 8);
        memcpy(g.h_items[b].get(), items.data(), items.size() * sizeof(GnRunItem));
        GN_HIP(hipMemcpyAsync(g.d_stage[b], g.h_stage[b], taken * 8, hipMemcpyHostToDevice, g.streams.st[b]));
        GN_HIP(hipMemcpyAsync(g.d_items[b], g.h_items[b], items.size() * sizeof(GnRunItem), hipMemcpyHostToDevice, g.streams.st[b]));
        const uint32_t n_items = (uint32_t)items.size();
        hipLaunchKernelGGL(gn_emplace_window_kernel, dim3((n_items + 3) / 4), dim3(256), 0, g.streams.st[b], ib.d_rows.get(), total_rows,
                           (uint32_t)__builtin_clzll(total_rows), (uint32_t)ib.Ws, ib.h, (uint32_t)row_begin, (uint32_t)ib.S, (const uint64_t*)g.d_stage[b],
                           (const GnRunItem*)g.d_items[b], n_items, (const GnRunDev*)g.d_runs);
        GN_HIP(hipGetLastError());
    }
}

extern "C" int gn_filter_emplace_runs_window(gn_filter* f, const uint64_t* const* runs, const uint64_t* run_sizes, const uint32_t* first_bin,
                                             const uint64_t* hashes_per_bin, uint32_t n_runs, uint64_t total_rows, uint64_t row_begin, uint64_t chunk_hashes)
{
    static const char* const who = "gn_filter_emplace_runs_window";
    if (!f || f->is_hibf)
        return gn_fail(GN_EINVAL, "%s needs a flat IBF filter", who);
    const GnIbfHost& ib = f->ibf;
    if (total_rows == 0 || total_rows > 0xFFFFFFFFull)
        return gn_fail(GN_ERANGE, "%s: a filter of %llu rows, 1 .. 2^32 - 1 are supported", who, (unsigned long long)total_rows);
    if (row_begin > total_rows || ib.S > total_rows - row_begin)
        return gn_fail(GN_EINVAL, "%s: rows %llu .. %llu of a filter of %llu rows", who, (unsigned long long)row_begin, (unsigned long long)(row_begin + ib.S),
                       (unsigned long long)total_rows);
    if (n_runs == 0)
        return GN_OK;
    if (!runs || !run_sizes || !first_bin || !hashes_per_bin)
        return gn_fail(GN_EINVAL, "%s: null argument", who);
    // every bin a hash can reach is checked before anything is launched (the local row is below S by the window test)
    std::vector<GnRunDev> dev(n_runs);
    uint64_t              total = 0;
    for (uint32_t r = 0; r < n_runs; ++r)
    {
        dev[r] = GnRunDev{ hashes_per_bin[r] ? hashes_per_bin[r] : 1, first_bin[r], 0 };
        if (run_sizes[r] == 0)
            continue;
        if (!runs[r] || hashes_per_bin[r] == 0)
            return gn_fail(GN_EINVAL, "%s: run %u: bad argument", who, r);
        if ((uint64_t)first_bin[r] + (run_sizes[r] - 1) / hashes_per_bin[r] >= ib.B)
            return gn_fail(GN_EINVAL, "%s: run %u: bins %u.. exceed the filter's %llu bins", who, r, first_bin[r], (unsigned long long)ib.B);
        total += run_sizes[r];
    }
    if (total == 0)
        return GN_OK;
    GN_HIP(hipSetDevice(f->device));
    const uint64_t chunk     = std::min<uint64_t>(chunk_hashes ? chunk_hashes : GN_WIN_CHUNK, total);
    const uint64_t cap_items = chunk / 64 + 16; // (a chunk of many short runs closes at this many items instead of at `chunk` hashes)
    GnWindowStage  g;
    for (int b = 0; b < 2; ++b)
    {
        GN_HIP(hipStreamCreateWithFlags(&g.streams.st[b], hipStreamNonBlocking));
        GN_HIP(g.h_stage[b].alloc(chunk));
        GN_HIP(g.h_items[b].alloc(cap_items));
        GN_HIP(g.d_stage[b].alloc(chunk));
        GN_HIP(g.d_items[b].alloc(cap_items));
    }
    GN_HIP(g.d_runs.upload(dev.data(), dev.size()));
    const int rc = gn_runs_window_rounds(f, g, runs, run_sizes, n_runs, total_rows, row_begin, chunk, cap_items);
    // (also after a failure: nothing of `g` is freed under a copy or a kernel that still uses it)
    const hipError_t e0 = hipStreamSynchronize(g.streams.st[0]), e1 = hipStreamSynchronize(g.streams.st[1]);
    if (rc != GN_OK)
        return rc;
    GN_HIP(e0);
    GN_HIP(e1);
    return GN_OK;
}

// ---- gn_filter_emplace_packed_window: packed runs into a slab of rows ----------------------------------------------------------------
// The twin of gn_filter_emplace_runs_window for runs packed as gn_packed_set.h says: the same filter, the same bins and rows, the same
// bits.  One wave per block.  Lane L unpacks deltas 8L .. 8L + 7 -- `width` bytes of the staged payload, adjacent lanes adjacent bytes --
// and sums them; an inclusive scan of the lane sums across the wave, less the lane's own sum, plus `first` is hash 8L, and the lane's
// deltas lead from it to hashes 8L + 1 .. 8L + 7.  From there it is gn_emplace_window_kernel with q = 8L + j.
__global__ __launch_bounds__(256) void gn_emplace_packed_window_kernel(uint64_t* rows, uint64_t S_total, uint32_t shift, uint32_t W, uint32_t h,
                                                                       uint32_t row_begin, uint32_t n_rows, const uint64_t* __restrict__ stage,
                                                                       const GnPackedItem* __restrict__ items, uint32_t n_items,
                                                                       const GnRunDev* __restrict__ runs)
{
    const uint32_t item = (uint32_t)__builtin_amdgcn_readfirstlane((int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6));
    if (item >= n_items)
        return;
    const uint32_t     lane = threadIdx.x & 63u;
    const GnPackedItem it   = items[item];
    const GnRunDev     run  = runs[it.run];
    uint64_t           v[GN_WIN_PER_LANE];
    gn_packed_lane_hashes(stage + it.stage_at, it.cnt, it.width, it.first, lane, v);
    const uint64_t b0   = it.begin / run.per_bin; // (wave-uniform: once per item)
    const uint64_t r0   = it.begin - b0 * run.per_bin;
    const uint32_t bin0 = run.first_bin + (uint32_t)b0;
#pragma unroll
    for (uint32_t j = 0; j < GN_WIN_PER_LANE; ++j)
    {
        const uint32_t q = lane * GN_WIN_PER_LANE + j;
        if (q >= it.cnt)
            continue;
        const uint32_t bin  = gn_window_item_bin(bin0, r0, q, run.per_bin);
        GnGlobalWord*  word = (GnGlobalWord*)rows + (bin >> 6);
        const uint64_t bit  = 1ULL << (bin & 63);
        for (uint32_t i = 0; i < h; ++i)
        {
            uint32_t local;
            if (gn_window_local(gn_build_row(v[j], i, shift, S_total), row_begin, n_rows, &local))
                (void)__hip_atomic_fetch_or(word + (uint64_t)local * W, bit, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

// ---- gn_packed_decode_kernel: packed blocks written out as hashes --------------------------------------------------------------------
// One wave per block: the hashes of item i go to out[items[i].begin ..), its payload lies at stage + items[i].stage_at.  What the sort of
// gn_packed_union and the fill kernel of gn_sketches_create_packed read: the link carries packed bytes, the hashes are born in HBM.
__global__ __launch_bounds__(256) void gn_packed_decode_kernel(const uint64_t* __restrict__ stage, const GnPackedItem* __restrict__ items, uint32_t n_items,
                                                               uint64_t* __restrict__ out)
{
    const uint32_t item = (uint32_t)__builtin_amdgcn_readfirstlane((int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6));
    if (item >= n_items)
        return;
    const uint32_t     lane = threadIdx.x & 63u;
    const GnPackedItem it   = items[item];
    uint64_t           v[GN_WIN_PER_LANE];
    gn_packed_lane_hashes(stage + it.stage_at, it.cnt, it.width, it.first, lane, v);
#pragma unroll
    for (uint32_t j = 0; j < GN_WIN_PER_LANE; ++j)
    {
        const uint32_t q = lane * GN_WIN_PER_LANE + j;
        if (q < it.cnt)
            out[it.begin + q] = v[j];
    }
}

hipError_t gn_packed_decode_launch(hipStream_t st, const uint64_t* stage, const GnPackedItem* items, uint32_t n_items, uint64_t* out)
{
    if (n_items == 0)
        return hipSuccess;
    hipLaunchKernelGGL(gn_packed_decode_kernel, dim3((n_items + 3) / 4), dim3(256), 0, st, stage, items, n_items, out);
    return hipGetLastError();
}

// one block of a packed run as every call that takes such runs checks it
bool gn_packed_block_ok(const GnPackedBlock& b, const uint64_t* payload)
{
    return b.cnt != 0 && b.cnt <= GN_WIN_ITEM && b.width <= 64 && (gn_packed_words(b.cnt, b.width) == 0 || payload);
}

// ---- gn_packed_union: the ascending union of packed runs, packed ---------------------------------------------------------------------
// Blocks and payload go up (a run's words from where they lie: neighbouring blocks' words are copied together), gn_packed_decode_kernel
// writes the hashes into the sort's input, radix sort and unique as gn_hashes_union, then the packer of gn_stream_distinct_hashes_packed
// on the unique hashes; blocks and payload come down.  The payload on the device takes the sort's second buffer both times: a packed set
// has fewer words than hashes, and the sort that overwrites it runs behind the decode.
extern "C" int gn_packed_union(int device, const gn_packed_block* const* blocks_abi, const uint64_t* n_blocks, const uint64_t* const* payload, uint32_t n_runs,
                               gn_packed_block* out_blocks, uint64_t cap_blocks, uint64_t* out_payload, uint64_t cap_words, uint64_t* n_union,
                               uint64_t* n_out_blocks, uint64_t* n_out_words)
{
    static const char* const    who    = "gn_packed_union";
    const GnPackedBlock* const* blocks = reinterpret_cast<const GnPackedBlock* const*>(blocks_abi);
    if (!n_union || !n_out_blocks || !n_out_words || (n_runs && (!blocks || !n_blocks || !payload)))
        return gn_fail(GN_EINVAL, "%s: null argument", who);
    *n_union = *n_out_blocks = *n_out_words = 0;
    uint64_t total = 0, in_blocks = 0, in_words = 0;
    for (uint32_t r = 0; r < n_runs; ++r)
    {
        if (n_blocks[r] && !blocks[r])
            return gn_fail(GN_EINVAL, "%s: run %u is null", who, r);
        for (uint64_t i = 0; i < n_blocks[r]; ++i)
        {
            const GnPackedBlock& b = blocks[r][i];
            if (!gn_packed_block_ok(b, payload[r]))
                return gn_fail(GN_EINVAL, "%s: run %u: block %llu of %u hashes at %u bits", who, r, (unsigned long long)i, b.cnt, b.width);
            total += b.cnt;
            in_words += gn_packed_words(b.cnt, b.width);
        }
        in_blocks += n_blocks[r];
    }
    if (total == 0)
        return GN_OK;
    if (total > 0x7FFFFFFFull) // (the sort / unique calls take their item count as an int)
        return gn_fail(GN_ERANGE, "%s: %llu hashes in one call, at most 2^31 - 1", who, (unsigned long long)total);
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || device < 0 || device >= n_dev)
        return gn_fail(GN_ENODEV, "%s: no HIP device %d", who, device);
    GN_HIP(hipSetDevice(device));
    std::vector<GnPackedItem> items; // (before the buffers it is copied into: they are freed, which waits for the device, first)
    items.reserve(in_blocks);
    GnDev<uint64_t>           d_a, d_b;
    GnDev<unsigned long long> d_n;
    GnDev<uint8_t>            d_tmp;
    GnDev<GnPackedItem>       d_items;
    GN_HIP(d_a.alloc(total));
    GN_HIP(d_b.alloc(total));
    GN_HIP(d_n.alloc(2));
    GN_HIP(d_items.alloc(in_blocks));
    size_t ta = 0, tb = 0, tc = 0;
    GN_HIP(hipcub::DeviceRadixSort::SortKeys(nullptr, ta, d_a.get(), d_b.get(), (int)total, 0, 64, nullptr));
    GN_HIP(hipcub::DeviceSelect::Unique(nullptr, tb, d_b.get(), d_a.get(), d_n.get(), (int)total, nullptr));
    GN_HIP(hipcub::DeviceReduce::Max(nullptr, tc, d_a.get(), d_n.get() + 1, (int)total, nullptr));
    const size_t tmp_bytes = std::max(ta, std::max(tb, tc));
    GN_HIP(d_tmp.alloc(tmp_bytes));
    // the payload: word `stage_at` of d_b is where a block's words go; blocks whose words follow each other in the run go up in one copy
    uint64_t at = 0, words = 0;
    for (uint32_t r = 0; r < n_runs; ++r)
    {
        uint64_t from = 0, len = 0; // the words of the run gathered for the next copy
        auto     flush = [&]() -> hipError_t {
            const hipError_t e = len ? hipMemcpy(d_b + (words - len), payload[r] + from, len * 8, hipMemcpyHostToDevice) : hipSuccess;
            len                = 0;
            return e;
        };
        for (uint64_t i = 0; i < n_blocks[r]; ++i)
        {
            const GnPackedBlock& b = blocks[r][i];
            const uint32_t       w = gn_packed_words(b.cnt, b.width);
            items.push_back(GnPackedItem{ r, b.cnt, b.width, 0, b.first, at, words, i });
            at += b.cnt;
            if (w == 0)
                continue;
            if (len && b.word_at != from + len)
                GN_HIP(flush());
            if (len == 0)
                from = b.word_at;
            len += w, words += w;
        }
        GN_HIP(flush());
    }
    GN_HIP(hipMemcpy(d_items, items.data(), items.size() * sizeof(GnPackedItem), hipMemcpyHostToDevice));
    GN_HIP(gn_packed_decode_launch(nullptr, d_b, d_items, (uint32_t)items.size(), d_a));
    size_t t = tmp_bytes;
    GN_HIP(hipcub::DeviceReduce::Max(d_tmp.get(), t, d_a.get(), d_n.get() + 1, (int)total, nullptr));
    unsigned long long top = 0, nu = 0;
    GN_HIP(hipMemcpy(&top, d_n + 1, sizeof(top), hipMemcpyDeviceToHost));
    int end_bit = 1;
    while (end_bit < 64 && (top >> end_bit))
        ++end_bit;
    t = tmp_bytes;
    GN_HIP(hipcub::DeviceRadixSort::SortKeys(d_tmp.get(), t, d_a.get(), d_b.get(), (int)total, 0, end_bit, nullptr));
    t = tmp_bytes;
    GN_HIP(hipcub::DeviceSelect::Unique(d_tmp.get(), t, d_b.get(), d_a.get(), d_n.get(), (int)total, nullptr));
    GN_HIP(hipMemcpy(&nu, d_n, sizeof(nu), hipMemcpyDeviceToHost));
    // the union lies in d_a: packed as gn_stream_distinct_hashes_packed packs a file's set
    const uint64_t       nb = gn_packed_max_blocks(nu);
    GnDev<GnPackedBlock> d_blocks;
    GnDev<uint32_t>      d_words;
    GnDev<uint64_t>      d_off;
    GN_HIP(d_blocks.alloc(nb));
    GN_HIP(d_words.alloc(nb + 1));
    GN_HIP(d_off.alloc(nb + 1));
    size_t ts = 0;
    GN_HIP(gn_scan_counts(nullptr, ts, d_words.get(), d_off.get(), (int)(nb + 1), nullptr));
    if (ts > tmp_bytes)
        GN_HIP(d_tmp.alloc(ts));
    const dim3 grid((unsigned)((nb + 3) / 4));
    hipLaunchKernelGGL(gn_pack_width_kernel, grid, dim3(256), 0, nullptr, (const uint64_t*)d_a, (uint64_t)nu, d_blocks.get(), d_words.get(), (uint32_t)nb);
    GN_HIP(hipGetLastError());
    GN_HIP(gn_scan_counts(d_tmp.get(), ts, d_words.get(), d_off.get(), (int)(nb + 1), nullptr));
    hipLaunchKernelGGL(gn_pack_payload_kernel, grid, dim3(256), 0, nullptr, (const uint64_t*)d_a, (uint64_t)nu, d_blocks.get(), (const uint64_t*)d_off, d_b.get(),
                       (uint32_t)nb);
    GN_HIP(hipGetLastError());
    uint64_t nw = 0;
    GN_HIP(hipMemcpy(&nw, d_off + nb, 8, hipMemcpyDeviceToHost));
    *n_union      = nu;
    *n_out_blocks = nb;
    *n_out_words  = nw;
    if (!out_blocks && !out_payload)
        return GN_OK;
    if (!out_blocks || (!out_payload && nw))
        return gn_fail(GN_EINVAL, "%s: null argument", who);
    if (cap_blocks < nb || cap_words < nw)
        return gn_fail(GN_EOVERFLOW, "%s: packed buffers too small: need %llu blocks and %llu words", who, (unsigned long long)nb, (unsigned long long)nw);
    GN_HIP(hipMemcpy(out_blocks, d_blocks, nb * sizeof(GnPackedBlock), hipMemcpyDeviceToHost));
    if (nw)
        GN_HIP(hipMemcpy(out_payload, d_b, nw * 8, hipMemcpyDeviceToHost));
    return GN_OK;
}

namespace
{
struct GnPackedStage // everything a call holds; freed when the call returns
{
    GnStreamPair           streams;
    GnPinned<uint64_t>     h_stage[2];
    GnPinned<GnPackedItem> h_items[2];
    GnDev<uint64_t>        d_stage[2];
    GnDev<GnPackedItem>    d_items[2];
    GnDev<GnRunDev>        d_runs;
};
} // namespace

// the rounds of gn_runs_window_rounds: what is gathered into the page-locked chunk is the payload of the chunk's blocks
static int gn_packed_window_rounds(gn_filter* f, GnPackedStage& g, const GnPackedBlock* const* blocks, const uint64_t* n_blocks, const uint64_t* const* payload,
                                   uint32_t n_runs, uint64_t total_rows, uint64_t row_begin, uint64_t chunk, uint64_t cap_items)
{
    const GnIbfHost&          ib = f->ibf;
    std::vector<GnPackedItem> items;
    GnPackedCursor            cur;
    for (uint32_t c = 0;; ++c)
    {
        const uint32_t b = c & 1u;
        GN_HIP(hipStreamSynchronize(g.streams.st[b]));
        uint64_t       words   = 0;
        const uint32_t n_items = (uint32_t)gn_packed_next_chunk(blocks, n_blocks, n_runs, cur, chunk, cap_items, items, &words);
        if (n_items == 0)
            return GN_OK;
        for (const GnPackedItem& it : items)
            if (const uint32_t w = gn_packed_words(it.cnt, it.width))
                memcpy(g.h_stage[b] + it.stage_at, payload[it.run] + blocks[it.run][it.block].word_at, (size_t)w * 8);
        memcpy(g.h_items[b].get(), items.data(), items.size() * sizeof(GnPackedItem));
        if (words)
            GN_HIP(hipMemcpyAsync(g.d_stage[b], g.h_stage[b], words * 8, hipMemcpyHostToDevice, g.streams.st[b]));
        GN_HIP(hipMemcpyAsync(g.d_items[b], g.h_items[b], items.size() * sizeof(GnPackedItem), hipMemcpyHostToDevice, g.streams.st[b]));
        hipLaunchKernelGGL(gn_emplace_packed_window_kernel, dim3((n_items + 3) / 4), dim3(256), 0, g.streams.st[b], ib.d_rows.get(), total_rows,
                           (uint32_t)__builtin_clzll(total_rows), (uint32_t)ib.Ws, ib.h, (uint32_t)row_begin, (uint32_t)ib.S, (const uint64_t*)g.d_stage[b],
                           (const GnPackedItem*)g.d_items[b], n_items, (const GnRunDev*)g.d_runs);
        GN_HIP(hipGetLastError());
    }
}

extern "C" int gn_filter_emplace_packed_window(gn_filter* f, const gn_packed_block* const* blocks_abi, const uint64_t* n_blocks, const uint64_t* const* payload,
                                               const uint32_t* first_bin, const uint64_t* hashes_per_bin, uint32_t n_runs, uint64_t total_rows, uint64_t row_begin,
                                               uint64_t chunk_words)
{
    static const char* const who = "gn_filter_emplace_packed_window";
    const GnPackedBlock* const* blocks = reinterpret_cast<const GnPackedBlock* const*>(blocks_abi);
    if (!f || f->is_hibf)
        return gn_fail(GN_EINVAL, "%s needs a flat IBF filter", who);
    const GnIbfHost& ib = f->ibf;
    if (total_rows == 0 || total_rows > 0xFFFFFFFFull)
        return gn_fail(GN_ERANGE, "%s: a filter of %llu rows, 1 .. 2^32 - 1 are supported", who, (unsigned long long)total_rows);
    if (row_begin > total_rows || ib.S > total_rows - row_begin)
        return gn_fail(GN_EINVAL, "%s: rows %llu .. %llu of a filter of %llu rows", who, (unsigned long long)row_begin, (unsigned long long)(row_begin + ib.S),
                       (unsigned long long)total_rows);
    if (n_runs == 0)
        return GN_OK;
    if (!blocks || !n_blocks || !payload || !first_bin || !hashes_per_bin)
        return gn_fail(GN_EINVAL, "%s: null argument", who);
    // every block is looked at and every bin a hash can reach is checked before anything is launched (the local row is below S by the
    // window test; a block's words are read only as far as cnt and width say)
    std::vector<GnRunDev> dev(n_runs);
    uint64_t              total = 0, words = 0;
    for (uint32_t r = 0; r < n_runs; ++r)
    {
        dev[r] = GnRunDev{ hashes_per_bin[r] ? hashes_per_bin[r] : 1, first_bin[r], 0 };
        if (n_blocks[r] == 0)
            continue;
        if (!blocks[r] || hashes_per_bin[r] == 0)
            return gn_fail(GN_EINVAL, "%s: run %u: bad argument", who, r);
        uint64_t size = 0;
        for (uint64_t i = 0; i < n_blocks[r]; ++i)
        {
            const GnPackedBlock& b = blocks[r][i];
            if (b.cnt == 0 || b.cnt > GN_WIN_ITEM || b.width > 64 || (gn_packed_words(b.cnt, b.width) && !payload[r]))
                return gn_fail(GN_EINVAL, "%s: run %u: block %llu of %u hashes at %u bits", who, r, (unsigned long long)i, b.cnt, b.width);
            size += b.cnt;
            words += gn_packed_words(b.cnt, b.width);
        }
        if ((uint64_t)first_bin[r] + (size - 1) / hashes_per_bin[r] >= ib.B)
            return gn_fail(GN_EINVAL, "%s: run %u: bins %u.. exceed the filter's %llu bins", who, r, first_bin[r], (unsigned long long)ib.B);
        total += n_blocks[r];
    }
    if (total == 0)
        return GN_OK;
    GN_HIP(hipSetDevice(f->device));
    // (a chunk holds any block: a cap below a block's most words is raised to it)
    const uint64_t chunk     = std::max<uint64_t>(std::min<uint64_t>(chunk_words ? chunk_words : GN_PACKED_CHUNK, words), GN_PACKED_MAX_WORDS);
    const uint64_t cap_items = std::min<uint64_t>(chunk / 16 + 16, total); // (a chunk of narrow blocks closes at this many items)
    GnPackedStage  g;
    for (int b = 0; b < 2; ++b)
    {
        GN_HIP(hipStreamCreateWithFlags(&g.streams.st[b], hipStreamNonBlocking));
        GN_HIP(g.h_stage[b].alloc(chunk));
        GN_HIP(g.h_items[b].alloc(cap_items));
        GN_HIP(g.d_stage[b].alloc(chunk));
        GN_HIP(g.d_items[b].alloc(cap_items));
    }
    GN_HIP(g.d_runs.upload(dev.data(), dev.size()));
    const int rc = gn_packed_window_rounds(f, g, blocks, n_blocks, payload, n_runs, total_rows, row_begin, chunk, cap_items);
    // (also after a failure: nothing of `g` is freed under a copy or a kernel that still uses it)
    const hipError_t e0 = hipStreamSynchronize(g.streams.st[0]), e1 = hipStreamSynchronize(g.streams.st[1]);
    if (rc != GN_OK)
        return rc;
    GN_HIP(e0);
    GN_HIP(e1);
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
