// gn_build_hibf.hip -- the device work of `ganon-build --hibf` behind the C ABI:
//   gn_hashes_union          the ascending union of several ascending hash sets and its size -- the cardinality of a merged bin
//                            (raptor estimates it from HyperLogLog sketches; here it is exact: concatenate, radix sort, unique,
//                            as gn_stream_distinct_hashes does for a file)
//   gn_filter_emplace_path   one launch inserts a batch of user bins along their whole root-to-leaf paths: a hash is read once
//                            and ORed into h rows of EVERY IBF on its path (the user bin's own run of bins in its leaf IBF, one
//                            merged bin in each IBF above).  Inserting every member's set into a merged bin sets the bits the
//                            union of the sets would: the unions are never materialised.
//   gn_filter_emplace_path_window  the same into a filter whose IBFs are pieces of rows of the tree's IBFs: a tree built in parts
//   gn_filter_emplace_path_packed_window  its twin for packed sets (gn_packed_set.h): payload words go up, a wave decodes a block in registers
//   gn_filter_bin_popcounts  set bits per technical bin of an IBF: how full each bin of an index is (towards `--update`)
//   gn_filter_copy_ibf       an IBF into one with more bins, device to device
//   gn_filter_copy_ibf_spans the same with runs of bins left out or moved (`--update --remove`)
//   gn_filter_fold_ibf       groups of bins of an IBF ORed into one bin each of another one: merged bins (`--update --fold`)
// No counterpart in the reference's own sources: `ganon build --filter-type hibf` runs `raptor build`
// (/root/reference/src/ganon/build_update.py:411-518).  HBM-bound integer work: depth * h atomic ORs per hash, each to a row
// of its own.
#include "gn_bin_spans.h"
#include "gn_fold_table.h"
#include "gn_build_row.h"
#include "gn_packed_decode.h"
#include "gn_path_window.h"
#include "gn_scan.h"
#include <hipcub/hipcub.hpp>
#include <cstring>
#include <vector>

extern "C" int gn_hashes_union(int device, const uint64_t* const* sets, const uint64_t* sizes, uint32_t n_sets, uint64_t* out, uint64_t cap,
                               uint64_t* n_union)
{
    if (!n_union || (n_sets && (!sets || !sizes)))
        return gn_fail(GN_EINVAL, "gn_hashes_union: null argument");
    *n_union       = 0;
    uint64_t total = 0;
    for (uint32_t i = 0; i < n_sets; ++i)
    {
        if (sizes[i] && !sets[i])
            return gn_fail(GN_EINVAL, "gn_hashes_union: set %u is null", i);
        total += sizes[i];
    }
    if (total == 0)
        return GN_OK;
    if (total > 0x7FFFFFFFull) // (the sort / unique calls take their item count as an int)
        return gn_fail(GN_ERANGE, "gn_hashes_union: %llu hashes in one call, at most 2^31 - 1", (unsigned long long)total);
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || device < 0 || device >= n_dev)
        return gn_fail(GN_ENODEV, "gn_hashes_union: no HIP device %d", device);
    GN_HIP(hipSetDevice(device));
    GnDev<uint64_t>           d_a, d_b;
    GnDev<unsigned long long> d_n;
    GnDev<uint8_t>            d_tmp;
    GN_HIP(d_a.alloc(total));
    GN_HIP(d_b.alloc(total));
    GN_HIP(d_n.alloc(1));
    size_t ta = 0, tb = 0;
    GN_HIP(hipcub::DeviceRadixSort::SortKeys(nullptr, ta, d_a.get(), d_b.get(), (int)total, 0, 64, nullptr));
    GN_HIP(hipcub::DeviceSelect::Unique(nullptr, tb, d_b.get(), d_a.get(), d_n.get(), (int)total, nullptr));
    const size_t tmp_bytes = ta > tb ? ta : tb;
    GN_HIP(d_tmp.alloc(tmp_bytes));
    uint64_t at = 0, top = 0;
    for (uint32_t i = 0; i < n_sets; ++i)
    {
        if (sizes[i] == 0)
            continue;
        GN_HIP(hipMemcpy(d_a + at, sets[i], sizes[i] * 8, hipMemcpyHostToDevice));
        at += sizes[i];
        top = std::max(top, sets[i][sizes[i] - 1]); // ascending sets: the last value is the largest
    }
    int end_bit = 1;
    while (end_bit < 64 && (top >> end_bit))
        ++end_bit;
    unsigned long long nu = total; // one ascending set is its own union
    if (n_sets != 1)
    {
        size_t t = tmp_bytes;
        GN_HIP(hipcub::DeviceRadixSort::SortKeys(d_tmp.get(), t, d_a.get(), d_b.get(), (int)total, 0, end_bit, nullptr));
        t = tmp_bytes;
        GN_HIP(hipcub::DeviceSelect::Unique(d_tmp.get(), t, d_b.get(), d_a.get(), d_n.get(), (int)total, nullptr));
        GN_HIP(hipMemcpy(&nu, d_n, sizeof(nu), hipMemcpyDeviceToHost));
    }
    if (out)
    {
        if (cap < nu)
        {
            *n_union = nu; // (the caller sizes its buffer from it)
            return gn_fail(GN_EOVERFLOW, "gn_hashes_union: hash buffer too small: need %llu", nu);
        }
        GN_HIP(hipMemcpy(out, d_a, nu * 8, hipMemcpyDeviceToHost));
    }
    *n_union = nu;
    return GN_OK;
}

// ---- gn_filter_emplace_path ---------------------------------------------------------------------------------------------------
// One path entry as the kernel reads it: the IBF's geometry resolved on the host, so that a level costs one 40-byte read.
struct GnPathDev
{
    uint64_t* rows;
    uint64_t  S, per_bin;
    uint32_t  Ws, shift, first_bin, n_bins; // n_bins == 0: the path ends above this entry
};
// A wave's piece of work: `cnt` consecutive hashes of set `seg`, the first of them hash number `begin` of the set and word
// `stage_at` of the staging buffer.
struct GnPathItem
{
    uint32_t seg, cnt;
    uint64_t begin, stage_at;
};

typedef __attribute__((address_space(1))) unsigned long long GnGlobalWord;

#define GN_PATH_PER_LANE 8u                       // hashes a lane holds in registers while it walks the path
#define GN_PATH_CHUNK (64u * GN_PATH_PER_LANE)    // ... and a wave's item

// One wave per item.  Item and path entries depend on the wave alone: the index goes through readfirstlane so that they are
// read with scalar loads into SGPRs (they wait on lgkmcnt, never behind the atomics on vmcnt).  The lane's hashes are loaded
// first; from then on the wave only issues no-return atomic ORs -- depth * h * GN_PATH_PER_LANE per lane -- and waits for nothing.
__global__ __launch_bounds__(256) void gn_emplace_path_kernel(const uint64_t* __restrict__ stage, const GnPathItem* __restrict__ items,
                                                              uint32_t n_items, const GnPathDev* __restrict__ paths, uint32_t depth,
                                                              uint32_t h)
{
    const uint32_t item = (uint32_t)__builtin_amdgcn_readfirstlane((int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6));
    if (item >= n_items)
        return;
    const uint32_t   lane = threadIdx.x & 63u;
    const GnPathItem it   = items[item];
    uint64_t         v[GN_PATH_PER_LANE];
#pragma unroll
    for (uint32_t j = 0; j < GN_PATH_PER_LANE; ++j)
    {
        const uint32_t q = j * 64u + lane;
        v[j]             = q < it.cnt ? stage[it.stage_at + q] : 0;
    }
    const GnPathDev* __restrict__ p = paths + (uint64_t)it.seg * depth;
    for (uint32_t d = 0; d < depth; ++d)
    {
        const GnPathDev e = p[d];
        if (e.n_bins == 0)
            break;
#pragma unroll
        for (uint32_t j = 0; j < GN_PATH_PER_LANE; ++j)
        {
            const uint32_t q = j * 64u + lane;
            if (q >= it.cnt)
                continue;
            const uint32_t bin  = e.first_bin + (e.n_bins == 1 ? 0u : (uint32_t)((it.begin + q) / e.per_bin));
            // (a pointer read from memory is generic to the compiler: say that it is global, or the ORs become flat_atomic and count
            // on lgkmcnt, where the next level's scalar loads wait)
            GnGlobalWord*  word = (GnGlobalWord*)e.rows + (bin >> 6);
            const uint64_t bit  = 1ULL << (bin & 63);
            for (uint32_t i = 0; i < h; ++i)
                (void)__hip_atomic_fetch_or(word + (uint64_t)gn_build_row(v[j], i, e.shift, e.S) * e.Ws, bit, __ATOMIC_RELAXED,
                                            __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

// ---- the host part the insert and the probes share ------------------------------------------------------------------------------
// One gn_path_entry against the filter, resolved for the kernels.  An insert deals hash i of a set of n to bin first_bin + i / hashes_per_bin,
// which is checked here too; a probe looks at every bin of the run and ignores hashes_per_bin.
static int gn_path_resolve(const char* who, const gn_filter* f, const gn_path_entry& e, uint32_t s, uint32_t d, bool dealt, uint64_t n, GnPathDev& o)
{
    if (e.ibf >= f->ibfs.size())
        return gn_fail(GN_EINVAL, "%s: set %u level %u: ibf %u of %zu", who, s, d, e.ibf, f->ibfs.size());
    const GnIbfHost& ib = f->ibfs[e.ibf];
    if ((uint64_t)e.first_bin + e.n_bins > ib.B)
        return gn_fail(GN_EINVAL, "%s: set %u level %u: bins %u..%llu of an IBF with %llu", who, s, d, e.first_bin,
                       (unsigned long long)e.first_bin + e.n_bins - 1, (unsigned long long)ib.B);
    if (dealt && e.n_bins > 1 && (e.hashes_per_bin == 0 || (n && (n - 1) / e.hashes_per_bin >= e.n_bins)))
        return gn_fail(GN_EINVAL, "%s: set %u level %u: %llu hashes at %llu a bin do not fit %u bins", who, s, d, (unsigned long long)n,
                       (unsigned long long)e.hashes_per_bin, e.n_bins);
    o = GnPathDev{ ib.d_rows, ib.S, dealt && e.n_bins > 1 ? e.hashes_per_bin : 1, (uint32_t)ib.Ws, ib.shift, e.first_bin, e.n_bins };
    return GN_OK;
}

// n_paths paths of `depth` entries each, resolved; an entry with n_bins == 0 ends its path (set_off == NULL: no sets, n = 0 for every path)
static int gn_paths_resolve(const char* who, const gn_filter* f, const uint64_t* set_off, uint32_t n_paths, const gn_path_entry* paths, uint32_t depth,
                            bool dealt, std::vector<GnPathDev>& dev)
{
    dev.assign((size_t)n_paths * depth, GnPathDev{ nullptr, 1, 1, 1, 0, 0, 0 });
    for (uint32_t s = 0; s < n_paths; ++s)
    {
        if (set_off && set_off[s + 1] < set_off[s])
            return gn_fail(GN_EINVAL, "%s: set offsets descend at set %u", who, s);
        const uint64_t n = set_off ? set_off[s + 1] - set_off[s] : 0;
        for (uint32_t d = 0; d < depth && paths[(size_t)s * depth + d].n_bins != 0; ++d)
            if (const int rc = gn_path_resolve(who, f, paths[(size_t)s * depth + d], s, d, dealt, n, dev[(size_t)s * depth + d]))
                return rc;
    }
    return GN_OK;
}

// hashes of a round of gn_path_rounds: all of them, at most 32 M
static inline uint64_t gn_path_step(uint64_t total) { return total < (32ull << 20) ? total : (32ull << 20); }

// Items gn_path_rounds cuts hashes [lo, hi) of the call into when they are one set: a set is cut at every round boundary (a multiple
// of `step`) and from there into items of GN_PATH_CHUNK.  Items are numbered through the call in the order they are launched: sets in
// order, rounds in order, so a set's items are consecutive.
static inline uint64_t gn_path_items_of(uint64_t lo, uint64_t hi, uint64_t step)
{
    uint64_t n = 0;
    while (lo < hi)
    {
        const uint64_t end = std::min(hi, (lo / step + 1) * step);
        n += (end - lo + GN_PATH_CHUNK - 1) / GN_PATH_CHUNK;
        lo = end;
    }
    return n;
}

// Argument checks, GnPathDev resolution, GnPathItem cutting and the staging upload of gn_filter_emplace_path and gn_filter_probe_path:
// every bin a hash can reach is checked before anything is launched (the row is below S by construction, gn_build_row); then
// launch(stage, items, n_items, paths) is called on f->load_st once per round of at most 32 M hashes, and waited for.
template <typename Launch>
static int gn_path_rounds(const char* who, gn_filter* f, const uint64_t* hashes, const uint64_t* set_off, uint32_t n_sets, const gn_path_entry* paths,
                          uint32_t depth, bool dealt, Launch launch)
{
    if (!set_off || !paths || depth == 0)
        return gn_fail(GN_EINVAL, "%s: null argument", who);
    const uint64_t total = set_off[n_sets];
    if (total && !hashes)
        return gn_fail(GN_EINVAL, "%s: null argument", who);
    std::vector<GnPathDev> dev;
    if (const int rc = gn_paths_resolve(who, f, set_off, n_sets, paths, depth, dealt, dev))
        return rc;
    if (total == 0)
        return GN_OK;
    GN_HIP(hipSetDevice(f->device));
    if (!f->load_st)
        GN_HIP(hipStreamCreateWithFlags(&f->load_st, hipStreamNonBlocking));
    // staged through the device buffer that stays with the filter, at most 32 M hashes at a time (as gn_filter_emplace_split)
    const uint64_t step = gn_path_step(total);
    GN_HIP(f->d_emplace_stage.reserve(step, step));
    const uint64_t          max_items = step / GN_PATH_CHUNK + n_sets + 2;
    std::vector<GnPathItem> items; // (before the buffers it is copied into: they are freed, which waits for the device, first)
    GnDev<GnPathDev>        d_paths;
    GnDev<GnPathItem>       d_items;
    GN_HIP(d_paths.alloc(dev.size()));
    GN_HIP(d_items.alloc(max_items));
    GN_HIP(hipMemcpyAsync(d_paths, dev.data(), dev.size() * sizeof(GnPathDev), hipMemcpyHostToDevice, f->load_st));
    uint32_t seg = 0;
    for (uint64_t done = 0; done < total; done += step)
    {
        const uint64_t c = total - done < step ? total - done : step;
        items.clear();
        while (seg < n_sets && set_off[seg + 1] <= done) // (sets that ended before this round, empty ones among them)
            ++seg;
        for (uint32_t s = seg; s < n_sets && set_off[s] < done + c; ++s)
        {
            const uint64_t lo = std::max(set_off[s], done), hi = std::min(set_off[s + 1], done + c);
            for (uint64_t a = lo; a < hi; a += GN_PATH_CHUNK)
                items.push_back(GnPathItem{ s, (uint32_t)std::min<uint64_t>(GN_PATH_CHUNK, hi - a), a - set_off[s], a - done });
        }
        if (items.size() > max_items) // (cannot happen: a round holds at most step / chunk full items and one short one per set)
            GN_HIP(hipErrorInvalidValue);
        GN_HIP(hipMemcpyAsync(f->d_emplace_stage, hashes + done, c * 8, hipMemcpyHostToDevice, f->load_st));
        GN_HIP(hipMemcpyAsync(d_items, items.data(), items.size() * sizeof(GnPathItem), hipMemcpyHostToDevice, f->load_st));
        GN_HIP(launch((const uint64_t*)f->d_emplace_stage, (const GnPathItem*)d_items, (uint32_t)items.size(), (const GnPathDev*)d_paths));
        GN_HIP(hipGetLastError());
        GN_HIP(hipStreamSynchronize(f->load_st)); // (the staging buffer and `items` are reused, and `hashes` may be pageable)
    }
    return GN_OK;
}

extern "C" int gn_filter_emplace_path(gn_filter* f, const uint64_t* hashes, const uint64_t* set_off, uint32_t n_sets, const gn_path_entry* paths,
                                      uint32_t depth)
{
    if (!f || !f->is_hibf)
        return gn_fail(GN_EINVAL, "gn_filter_emplace_path needs an HIBF filter");
    if (n_sets == 0)
        return GN_OK;
    return gn_path_rounds("gn_filter_emplace_path", f, hashes, set_off, n_sets, paths, depth, true,
                          [&](const uint64_t* stage, const GnPathItem* items, uint32_t n_items, const GnPathDev* d_paths) {
                              hipLaunchKernelGGL(gn_emplace_path_kernel, dim3((n_items + 3) / 4), dim3(256), 0, f->load_st, stage, items, n_items, d_paths,
                                                 depth, f->ibfs[0].h);
                              return hipSuccess;
                          });
}

// ---- gn_filter_emplace_path_window: the same insert into pieces of IBFs ------------------------------------------------------------
// IBF j of the filter stands for rows [row_begin[j], row_begin[j] + S_j) of an IBF of total_rows[j] rows (`ganon-build --hibf
// --hibf-memory`, `--hibf-devices`: build_hibf_parts.cpp).  A hash's rows in an IBF depend on the hash and on the WHOLE IBF's row count
// alone, so every piece is filled from the same hash sets and takes the bits of the rows it holds.
//
// One wave per item, as gn_emplace_path_kernel: item and path entries depend on the wave alone, the index goes through readfirstlane so
// that they are read with scalar loads.  The lane's 8 hashes are loaded first; from then on the wave only issues no-return atomic ORs and
// waits for nothing.  Per entry the item's first bin and the remainder are divided out once for the wave (gn_path_window_start): no
// 64-bit division per hash, which gn_emplace_path_kernel pays.  A row outside the piece costs its hash and one compare.
__global__ __launch_bounds__(256) void gn_emplace_path_window_kernel(const uint64_t* __restrict__ stage, const GnRunItem* __restrict__ items, uint32_t n_items,
                                                                     const GnPathWinDev* __restrict__ paths, uint32_t depth, uint32_t h)
{
    const uint32_t item = (uint32_t)__builtin_amdgcn_readfirstlane((int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6));
    if (item >= n_items)
        return;
    const uint32_t  lane = threadIdx.x & 63u;
    const GnRunItem it   = items[item];
    uint64_t        v[GN_WIN_PER_LANE];
#pragma unroll
    for (uint32_t j = 0; j < GN_WIN_PER_LANE; ++j)
    {
        const uint32_t q = j * 64u + lane;
        v[j]             = q < it.cnt ? stage[it.stage_at + q] : 0;
    }
    const GnPathWinDev* __restrict__ p = paths + (uint64_t)it.run * depth;
    for (uint32_t d = 0; d < depth; ++d)
    {
        const GnPathWinDev e = p[d];
        if (e.n_bins == 0)
            break;
        uint32_t bin0;
        uint64_t r0;
        gn_path_window_start(e.first_bin, e.n_bins, e.per_bin, it.begin, &bin0, &r0); // (wave-uniform: once per item and entry)
#pragma unroll
        for (uint32_t j = 0; j < GN_WIN_PER_LANE; ++j)
        {
            const uint32_t q = j * 64u + lane;
            if (q >= it.cnt)
                continue;
            const uint32_t bin  = gn_path_window_bin(bin0, r0, q, e.n_bins, e.per_bin);
            // (a pointer read from memory is generic to the compiler: say that it is global, as gn_emplace_path_kernel does)
            GnGlobalWord*  word = (GnGlobalWord*)e.rows + (bin >> 6);
            const uint64_t bit  = 1ULL << (bin & 63);
            for (uint32_t i = 0; i < h; ++i)
            {
                uint32_t local;
                if (gn_window_local(gn_build_row(v[j], i, e.shift, e.S_total), e.row_begin, e.n_rows, &local))
                    (void)__hip_atomic_fetch_or(word + (uint64_t)local * e.Ws, bit, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
    }
}

namespace
{
struct GnPathWindowStage // everything a call holds; freed when the call returns
{
    GnStreamPair        streams;
    GnPinned<uint64_t>  h_stage[2];
    GnPinned<GnRunItem> h_items[2];
    GnDev<uint64_t>     d_stage[2];
    GnDev<GnRunItem>    d_items[2];
    GnDev<GnPathWinDev> d_paths;
};
} // namespace

// Chunk c goes through buffer and stream c & 1, as gn_runs_window_rounds (gn_build.hip) sends it: gathered into the page-locked buffer,
// copied and inserted on that stream while chunk c - 1 is still on the other one.  A buffer is written again only after its stream has
// been waited for.
static int gn_path_window_rounds(GnPathWindowStage& g, const uint64_t* const* sets, const uint64_t* set_sizes, uint32_t n_sets, uint32_t depth, uint32_t h,
                                 uint64_t chunk, uint64_t cap_items)
{
    std::vector<GnRunItem> items;
    GnRunCursor            cur;
    for (uint32_t c = 0;; ++c)
    {
        const uint32_t b = c & 1u;
        GN_HIP(hipStreamSynchronize(g.streams.st[b]));
        const uint64_t taken = gn_window_next_chunk(set_sizes, n_sets, cur, chunk, cap_items, items);
        if (taken == 0)
            return GN_OK;
        for (const GnRunItem& it : items)
            memcpy(g.h_stage[b] + it.stage_at, sets[it.run] + it.begin, (size_t)it.cnt * 8);
        memcpy(g.h_items[b].get(), items.data(), items.size() * sizeof(GnRunItem));
        GN_HIP(hipMemcpyAsync(g.d_stage[b], g.h_stage[b], taken * 8, hipMemcpyHostToDevice, g.streams.st[b]));
        GN_HIP(hipMemcpyAsync(g.d_items[b], g.h_items[b], items.size() * sizeof(GnRunItem), hipMemcpyHostToDevice, g.streams.st[b]));
        const uint32_t n_items = (uint32_t)items.size();
        hipLaunchKernelGGL(gn_emplace_path_window_kernel, dim3((n_items + 3) / 4), dim3(256), 0, g.streams.st[b], (const uint64_t*)g.d_stage[b],
                           (const GnRunItem*)g.d_items[b], n_items, (const GnPathWinDev*)g.d_paths, depth, h);
        GN_HIP(hipGetLastError());
    }
}

extern "C" int gn_filter_emplace_path_window(gn_filter* f, const uint64_t* const* sets, const uint64_t* set_sizes, uint32_t n_sets, const gn_path_entry* paths,
                                             uint32_t depth, const uint64_t* total_rows, const uint64_t* row_begin, uint64_t chunk_hashes)
{
    static const char* const who = "gn_filter_emplace_path_window";
    if (!f || !f->is_hibf)
        return gn_fail(GN_EINVAL, "%s needs an HIBF filter", who);
    if (!total_rows || !row_begin)
        return gn_fail(GN_EINVAL, "%s: null argument", who);
    for (size_t j = 0; j < f->ibfs.size(); ++j)
    {
        if (total_rows[j] == 0 || total_rows[j] > 0xFFFFFFFFull)
            return gn_fail(GN_ERANGE, "%s: ibf %zu: an IBF of %llu rows, 1 .. 2^32 - 1 are supported", who, j, (unsigned long long)total_rows[j]);
        if (row_begin[j] > total_rows[j] || f->ibfs[j].S > total_rows[j] - row_begin[j])
            return gn_fail(GN_EINVAL, "%s: ibf %zu: rows %llu .. %llu of an IBF of %llu rows", who, j, (unsigned long long)row_begin[j],
                           (unsigned long long)(row_begin[j] + f->ibfs[j].S), (unsigned long long)total_rows[j]);
    }
    if (n_sets == 0)
        return GN_OK;
    if (!sets || !set_sizes || !paths || depth == 0)
        return gn_fail(GN_EINVAL, "%s: null argument", who);
    const uint32_t h = f->ibfs[0].h;
    // every bin a hash can reach is checked before anything is launched (the local row is below the piece's rows by the window test)
    std::vector<GnPathWinDev> dev((size_t)n_sets * depth, GnPathWinDev{ nullptr, 1, 1, 1, 0, 0, 0, 0, 0 });
    uint64_t                  total = 0;
    for (uint32_t s = 0; s < n_sets; ++s)
    {
        if (set_sizes[s] && !sets[s])
            return gn_fail(GN_EINVAL, "%s: set %u is null", who, s);
        total += set_sizes[s];
        for (uint32_t d = 0; d < depth && paths[(size_t)s * depth + d].n_bins != 0; ++d)
        {
            GnPathDev           o;
            const gn_path_entry& e = paths[(size_t)s * depth + d];
            if (const int rc = gn_path_resolve(who, f, e, s, d, true, set_sizes[s], o))
                return rc;
            const GnIbfHost& ib = f->ibfs[e.ibf];
            if (ib.h != h)
                return gn_fail(GN_EINVAL, "%s: ibf %u has %u hash functions, ibf 0 has %u", who, e.ibf, ib.h, h);
            dev[(size_t)s * depth + d] = GnPathWinDev{ o.rows, total_rows[e.ibf], o.per_bin, o.Ws, (uint32_t)__builtin_clzll(total_rows[e.ibf]),
                                                       o.first_bin, o.n_bins, (uint32_t)row_begin[e.ibf], (uint32_t)ib.S };
        }
    }
    if (total == 0)
        return GN_OK;
    GN_HIP(hipSetDevice(f->device));
    const uint64_t    chunk     = std::min<uint64_t>(chunk_hashes ? chunk_hashes : GN_WIN_CHUNK, total);
    const uint64_t    cap_items = chunk / 64 + 16; // (a chunk of many short sets closes at this many items instead of at `chunk` hashes)
    GnPathWindowStage g;
    for (int b = 0; b < 2; ++b)
    {
        GN_HIP(hipStreamCreateWithFlags(&g.streams.st[b], hipStreamNonBlocking));
        GN_HIP(g.h_stage[b].alloc(chunk));
        GN_HIP(g.h_items[b].alloc(cap_items));
        GN_HIP(g.d_stage[b].alloc(chunk));
        GN_HIP(g.d_items[b].alloc(cap_items));
    }
    GN_HIP(g.d_paths.upload(dev.data(), dev.size()));
    const int rc = gn_path_window_rounds(g, sets, set_sizes, n_sets, depth, h, chunk, cap_items);
    // (also after a failure: nothing of `g` is freed under a copy or a kernel that still uses it)
    const hipError_t e0 = hipStreamSynchronize(g.streams.st[0]), e1 = hipStreamSynchronize(g.streams.st[1]);
    if (rc != GN_OK)
        return rc;
    GN_HIP(e0);
    GN_HIP(e1);
    return GN_OK;
}

// ---- gn_filter_emplace_path_packed_window: the same insert from packed sets ----------------------------------------------------------
// The twin of gn_filter_emplace_path_window for sets packed as gn_packed_set.h says (`ganon-build --hibf --hibf-hash-sets packed|spilled`):
// the same filter, paths, pieces and bits.  One wave per block.  Lane L unpacks the block's hashes 8L .. 8L + 7 in registers
// (gn_packed_lane_hashes: the decode of the flat packed insert) -- they are never written to memory -- and from there it is the depth loop
// of gn_emplace_path_window_kernel with q = 8L + j and the item's `begin`, the index of the block's first hash in the SET.  Item and path
// entries are read with scalar loads; behind the decode the wave only issues no-return atomic ORs.
__global__ __launch_bounds__(256) void gn_emplace_path_packed_window_kernel(const uint64_t* __restrict__ stage, const GnPackedItem* __restrict__ items,
                                                                            uint32_t n_items, const GnPathWinDev* __restrict__ paths, uint32_t depth, uint32_t h)
{
    const uint32_t item = (uint32_t)__builtin_amdgcn_readfirstlane((int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6));
    if (item >= n_items)
        return;
    const uint32_t     lane = threadIdx.x & 63u;
    const GnPackedItem it   = items[item];
    uint64_t           v[GN_WIN_PER_LANE];
    gn_packed_lane_hashes(stage + it.stage_at, it.cnt, it.width, it.first, lane, v);
    const GnPathWinDev* __restrict__ p = paths + (uint64_t)it.run * depth;
    for (uint32_t d = 0; d < depth; ++d)
    {
        const GnPathWinDev e = p[d];
        if (e.n_bins == 0)
            break;
        uint32_t bin0;
        uint64_t r0;
        gn_path_window_start(e.first_bin, e.n_bins, e.per_bin, it.begin, &bin0, &r0); // (wave-uniform: once per item and entry)
#pragma unroll
        for (uint32_t j = 0; j < GN_WIN_PER_LANE; ++j)
        {
            const uint32_t q = lane * GN_WIN_PER_LANE + j;
            if (q >= it.cnt)
                continue;
            const uint32_t bin  = gn_path_window_bin(bin0, r0, q, e.n_bins, e.per_bin);
            // (a pointer read from memory is generic to the compiler: say that it is global, as gn_emplace_path_kernel does)
            GnGlobalWord*  word = (GnGlobalWord*)e.rows + (bin >> 6);
            const uint64_t bit  = 1ULL << (bin & 63);
            for (uint32_t i = 0; i < h; ++i)
            {
                uint32_t local;
                if (gn_window_local(gn_build_row(v[j], i, e.shift, e.S_total), e.row_begin, e.n_rows, &local))
                    (void)__hip_atomic_fetch_or(word + (uint64_t)local * e.Ws, bit, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
    }
}

namespace
{
struct GnPathPackedStage // everything a call holds; freed when the call returns
{
    GnStreamPair           streams;
    GnPinned<uint64_t>     h_stage[2];
    GnPinned<GnPackedItem> h_items[2];
    GnDev<uint64_t>        d_stage[2];
    GnDev<GnPackedItem>    d_items[2];
    GnDev<GnPathWinDev>    d_paths;
};
} // namespace

// the rounds of gn_packed_window_rounds (gn_build.hip) with the sets as runs: what is gathered into the page-locked chunk is the payload
// of the chunk's blocks; chunk c goes through buffer and stream c & 1, a buffer is written again only after its stream has been waited for
static int gn_path_packed_window_rounds(GnPathPackedStage& g, const GnPackedBlock* const* blocks, const uint64_t* n_blocks, const uint64_t* const* payload,
                                        uint32_t n_sets, uint32_t depth, uint32_t h, uint64_t chunk, uint64_t cap_items)
{
    std::vector<GnPackedItem> items;
    GnPackedCursor            cur;
    for (uint32_t c = 0;; ++c)
    {
        const uint32_t b = c & 1u;
        GN_HIP(hipStreamSynchronize(g.streams.st[b]));
        uint64_t       words   = 0;
        const uint32_t n_items = (uint32_t)gn_packed_next_chunk(blocks, n_blocks, n_sets, cur, chunk, cap_items, items, &words);
        if (n_items == 0)
            return GN_OK;
        for (const GnPackedItem& it : items)
            if (const uint32_t w = gn_packed_words(it.cnt, it.width))
                memcpy(g.h_stage[b] + it.stage_at, payload[it.run] + blocks[it.run][it.block].word_at, (size_t)w * 8);
        memcpy(g.h_items[b].get(), items.data(), items.size() * sizeof(GnPackedItem));
        if (words)
            GN_HIP(hipMemcpyAsync(g.d_stage[b], g.h_stage[b], words * 8, hipMemcpyHostToDevice, g.streams.st[b]));
        GN_HIP(hipMemcpyAsync(g.d_items[b], g.h_items[b], items.size() * sizeof(GnPackedItem), hipMemcpyHostToDevice, g.streams.st[b]));
        hipLaunchKernelGGL(gn_emplace_path_packed_window_kernel, dim3((n_items + 3) / 4), dim3(256), 0, g.streams.st[b], (const uint64_t*)g.d_stage[b],
                           (const GnPackedItem*)g.d_items[b], n_items, (const GnPathWinDev*)g.d_paths, depth, h);
        GN_HIP(hipGetLastError());
    }
}

extern "C" int gn_filter_emplace_path_packed_window(gn_filter* f, const gn_packed_block* const* blocks_abi, const uint64_t* n_blocks,
                                                    const uint64_t* const* payload, uint32_t n_sets, const gn_path_entry* paths, uint32_t depth,
                                                    const uint64_t* total_rows, const uint64_t* row_begin, uint64_t chunk_words)
{
    static const char* const    who    = "gn_filter_emplace_path_packed_window";
    const GnPackedBlock* const* blocks = reinterpret_cast<const GnPackedBlock* const*>(blocks_abi);
    if (!f || !f->is_hibf)
        return gn_fail(GN_EINVAL, "%s needs an HIBF filter", who);
    if (!total_rows || !row_begin)
        return gn_fail(GN_EINVAL, "%s: null argument", who);
    for (size_t j = 0; j < f->ibfs.size(); ++j)
    {
        if (total_rows[j] == 0 || total_rows[j] > 0xFFFFFFFFull)
            return gn_fail(GN_ERANGE, "%s: ibf %zu: an IBF of %llu rows, 1 .. 2^32 - 1 are supported", who, j, (unsigned long long)total_rows[j]);
        if (row_begin[j] > total_rows[j] || f->ibfs[j].S > total_rows[j] - row_begin[j])
            return gn_fail(GN_EINVAL, "%s: ibf %zu: rows %llu .. %llu of an IBF of %llu rows", who, j, (unsigned long long)row_begin[j],
                           (unsigned long long)(row_begin[j] + f->ibfs[j].S), (unsigned long long)total_rows[j]);
    }
    if (n_sets == 0)
        return GN_OK;
    if (!blocks || !n_blocks || !payload || !paths || depth == 0)
        return gn_fail(GN_EINVAL, "%s: null argument", who);
    const uint32_t h = f->ibfs[0].h;
    // every block is looked at and every bin a hash can reach is checked before anything is launched (the local row is below the piece's
    // rows by the window test; a block's words are read only as far as cnt and width say)
    std::vector<GnPathWinDev> dev((size_t)n_sets * depth, GnPathWinDev{ nullptr, 1, 1, 1, 0, 0, 0, 0, 0 });
    uint64_t                  total = 0, words = 0;
    for (uint32_t s = 0; s < n_sets; ++s)
    {
        if (n_blocks[s] && !blocks[s])
            return gn_fail(GN_EINVAL, "%s: set %u is null", who, s);
        uint64_t size = 0;
        for (uint64_t i = 0; i < n_blocks[s]; ++i)
        {
            const GnPackedBlock& b = blocks[s][i];
            if (!gn_packed_block_ok(b, payload[s]))
                return gn_fail(GN_EINVAL, "%s: set %u: block %llu of %u hashes at %u bits", who, s, (unsigned long long)i, b.cnt, b.width);
            size += b.cnt;
            words += gn_packed_words(b.cnt, b.width);
        }
        total += n_blocks[s];
        for (uint32_t d = 0; d < depth && paths[(size_t)s * depth + d].n_bins != 0; ++d)
        {
            GnPathDev            o;
            const gn_path_entry& e = paths[(size_t)s * depth + d];
            if (const int rc = gn_path_resolve(who, f, e, s, d, true, size, o))
                return rc;
            const GnIbfHost& ib = f->ibfs[e.ibf];
            if (ib.h != h)
                return gn_fail(GN_EINVAL, "%s: ibf %u has %u hash functions, ibf 0 has %u", who, e.ibf, ib.h, h);
            dev[(size_t)s * depth + d] = GnPathWinDev{ o.rows, total_rows[e.ibf], o.per_bin, o.Ws, (uint32_t)__builtin_clzll(total_rows[e.ibf]),
                                                       o.first_bin, o.n_bins, (uint32_t)row_begin[e.ibf], (uint32_t)ib.S };
        }
    }
    if (total == 0)
        return GN_OK;
    GN_HIP(hipSetDevice(f->device));
    // (a chunk holds any block: a cap below a block's most words is raised to it)
    const uint64_t    chunk     = std::max<uint64_t>(std::min<uint64_t>(chunk_words ? chunk_words : GN_PACKED_CHUNK, words), GN_PACKED_MAX_WORDS);
    const uint64_t    cap_items = std::min<uint64_t>(chunk / 16 + 16, total); // (a chunk of narrow blocks closes at this many items)
    GnPathPackedStage g;
    for (int b = 0; b < 2; ++b)
    {
        GN_HIP(hipStreamCreateWithFlags(&g.streams.st[b], hipStreamNonBlocking));
        GN_HIP(g.h_stage[b].alloc(chunk));
        GN_HIP(g.h_items[b].alloc(cap_items));
        GN_HIP(g.d_stage[b].alloc(chunk));
        GN_HIP(g.d_items[b].alloc(cap_items));
    }
    GN_HIP(g.d_paths.upload(dev.data(), dev.size()));
    const int rc = gn_path_packed_window_rounds(g, blocks, n_blocks, payload, n_sets, depth, h, chunk, cap_items);
    // (also after a failure: nothing of `g` is freed under a copy or a kernel that still uses it)
    const hipError_t e0 = hipStreamSynchronize(g.streams.st[0]), e1 = hipStreamSynchronize(g.streams.st[1]);
    if (rc != GN_OK)
        return rc;
    GN_HIP(e0);
    GN_HIP(e1);
    return GN_OK;
}

// ---- gn_filter_probe_path / gn_filter_probe_paths_shared: the insert read back ---------------------------------------------------
typedef const __attribute__((address_space(1))) unsigned long long GnGlobalConstWord;

// bits of word `w` of a row that belong to the run first_bin .. first_bin + n_bins - 1 (which reaches into that word)
__device__ __forceinline__ uint64_t gn_run_mask(uint32_t first_bin, uint32_t n_bins, uint32_t w)
{
    const uint64_t lo = max((uint64_t)first_bin, (uint64_t)w << 6), hi = min((uint64_t)first_bin + n_bins, ((uint64_t)w + 1) << 6);
    return (hi - lo >= 64u ? ~0ULL : (1ULL << (hi - lo)) - 1) << (lo & 63u);
}

// One wave per item, as the insert: item and path entries in SGPRs, 8 hashes a lane in registers.  Per entry and word of its run the
// H row words of all 8 hashes are loaded before any is looked at -- 8 * H independent loads in flight per lane, nothing to store -- then
// ANDed and masked to the run.  A lane without a hash in a slot probes hash 0 there (row 0 word w of the entry: inside the matrix)
// and its answer is not counted, so that no load sits behind a lane-dependent branch.  Counts leave the wave as one atomic each.
template <uint32_t H>
__global__ __launch_bounds__(256) void gn_probe_path_kernel(const uint64_t* __restrict__ stage, const GnPathItem* __restrict__ items, uint32_t n_items,
                                                            const GnPathDev* __restrict__ paths, uint32_t depth, unsigned long long* __restrict__ found,
                                                            unsigned long long* __restrict__ lost_at, unsigned long long* __restrict__ first_lost)
{
    const uint32_t item = (uint32_t)__builtin_amdgcn_readfirstlane((int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6));
    if (item >= n_items)
        return;
    const uint32_t   lane = threadIdx.x & 63u;
    const GnPathItem it   = items[item];
    uint64_t         v[GN_PATH_PER_LANE];
    uint32_t         valid = 0; // bit j: slot j holds a hash of the item
#pragma unroll
    for (uint32_t j = 0; j < GN_PATH_PER_LANE; ++j)
    {
        const uint32_t q = j * 64u + lane;
        v[j]             = q < it.cnt ? stage[it.stage_at + q] : 0;
        valid |= (q < it.cnt ? 1u : 0u) << j;
    }
    uint32_t alive = valid; // bit j: contained in every entry so far
    const GnPathDev* __restrict__ p = paths + (uint64_t)it.seg * depth;
    for (uint32_t d = 0; d < depth; ++d)
    {
        const GnPathDev e = p[d];
        if (e.n_bins == 0)
            break;
        if (!lost_at && __ballot(alive != 0) == 0) // (nobody asks at which level: a wave whose hashes are all lost already is done)
            break;
        GnGlobalConstWord* rows = (GnGlobalConstWord*)e.rows;
        const uint32_t     w1   = (e.first_bin + e.n_bins - 1) >> 6;
        uint32_t           hit  = 0;
        for (uint32_t w = e.first_bin >> 6; w <= w1; ++w)
        {
            const uint64_t mask = gn_run_mask(e.first_bin, e.n_bins, w);
            uint64_t       r[GN_PATH_PER_LANE][H];
#pragma unroll
            for (uint32_t j = 0; j < GN_PATH_PER_LANE; ++j)
#pragma unroll
                for (uint32_t i = 0; i < H; ++i)
                    r[j][i] = rows[(uint64_t)gn_build_row(v[j], i, e.shift, e.S) * e.Ws + w];
#pragma unroll
            for (uint32_t j = 0; j < GN_PATH_PER_LANE; ++j)
            {
                uint64_t a = r[j][0];
#pragma unroll
                for (uint32_t i = 1; i < H; ++i)
                    a &= r[j][i];
                hit |= ((a & mask) != 0 ? 1u : 0u) << j;
            }
        }
        alive &= hit;
        if (lost_at)
        {
            const uint32_t lost = valid & ~hit;
            uint32_t       n    = 0;
#pragma unroll
            for (uint32_t j = 0; j < GN_PATH_PER_LANE; ++j)
                n += (uint32_t)__popcll(__ballot((lost >> j) & 1u));
            if (n && lane == 0)
                atomicAdd(&lost_at[(uint64_t)it.seg * depth + d], (unsigned long long)n);
        }
    }
    uint32_t n = 0;
#pragma unroll
    for (uint32_t j = 0; j < GN_PATH_PER_LANE; ++j)
        n += (uint32_t)__popcll(__ballot((alive >> j) & 1u));
    if (n && lane == 0)
        atomicAdd(&found[it.seg], (unsigned long long)n);
    const uint32_t dead = valid & ~alive;
    if (__ballot(dead != 0) != 0)
    {
        // slot j of this lane is hash begin + j * 64 + lane of the set: the lowest dead slot is the lane's first
        unsigned long long m = dead ? it.begin + (uint64_t)(__ffs((int)dead) - 1) * 64u + lane : ~0ULL;
        for (int off = 32; off; off >>= 1)
        {
            const unsigned long long o = __shfl_xor(m, off);
            m                          = o < m ? o : m;
        }
        if (lane == 0)
            atomicMin(&first_lost[it.seg], m);
    }
}

template <uint32_t H>
static hipError_t gn_probe_path_launch(hipStream_t st, const uint64_t* stage, const GnPathItem* items, uint32_t n_items, const GnPathDev* paths, uint32_t depth,
                                       unsigned long long* found, unsigned long long* lost_at, unsigned long long* first_lost)
{
    hipLaunchKernelGGL(gn_probe_path_kernel<H>, dim3((n_items + 3) / 4), dim3(256), 0, st, stage, items, n_items, paths, depth, found, lost_at, first_lost);
    return hipSuccess;
}

extern "C" int gn_filter_probe_path(gn_filter* f, const uint64_t* hashes, const uint64_t* set_off, uint32_t n_sets, const gn_path_entry* paths,
                                    uint32_t depth, uint64_t* found, uint64_t* lost_at, uint64_t* first_lost)
{
    if (!f || !f->is_hibf)
        return gn_fail(GN_EINVAL, "gn_filter_probe_path needs an HIBF filter");
    if (n_sets == 0)
        return GN_OK;
    if (!found || !first_lost)
        return gn_fail(GN_EINVAL, "gn_filter_probe_path: null argument");
    const uint32_t h = f->ibfs[0].h;
    if (h < 1 || h > GN_IBF_MAX_HASH_FUNS)
        return gn_fail(GN_EINVAL, "gn_filter_probe_path: %u hash functions", h);
    GnDev<unsigned long long> d_found, d_lost, d_first;
    const size_t              n_lost = (size_t)n_sets * depth;
    const int                 rc     = gn_path_rounds(
        "gn_filter_probe_path", f, hashes, set_off, n_sets, paths, depth, false,
        [&](const uint64_t* stage, const GnPathItem* items, uint32_t n_items, const GnPathDev* d_paths) -> hipError_t {
            hipError_t e = hipSuccess;
            if (!d_found) // the first round: the counters, zero (first_lost: all ones), ordered before the kernel on the same stream
            {
                if ((e = d_found.alloc(n_sets)) != hipSuccess || (e = d_first.alloc(n_sets)) != hipSuccess || (lost_at && (e = d_lost.alloc(n_lost)) != hipSuccess))
                    return e;
                if ((e = hipMemsetAsync(d_found, 0, (size_t)n_sets * 8, f->load_st)) != hipSuccess ||
                    (e = hipMemsetAsync(d_first, 0xFF, (size_t)n_sets * 8, f->load_st)) != hipSuccess ||
                    (lost_at && (e = hipMemsetAsync(d_lost, 0, n_lost * 8, f->load_st)) != hipSuccess))
                    return e;
            }
            switch (h)
            {
            case 1: return gn_probe_path_launch<1>(f->load_st, stage, items, n_items, d_paths, depth, d_found, d_lost, d_first);
            case 2: return gn_probe_path_launch<2>(f->load_st, stage, items, n_items, d_paths, depth, d_found, d_lost, d_first);
            case 3: return gn_probe_path_launch<3>(f->load_st, stage, items, n_items, d_paths, depth, d_found, d_lost, d_first);
            case 4: return gn_probe_path_launch<4>(f->load_st, stage, items, n_items, d_paths, depth, d_found, d_lost, d_first);
            default: return gn_probe_path_launch<5>(f->load_st, stage, items, n_items, d_paths, depth, d_found, d_lost, d_first);
            }
        });
    if (rc != GN_OK)
        return rc;
    if (!d_found) // no hash in any set
    {
        std::fill(found, found + n_sets, 0);
        std::fill(first_lost, first_lost + n_sets, ~0ull);
        if (lost_at)
            std::fill(lost_at, lost_at + n_lost, 0);
        return GN_OK;
    }
    GN_HIP(hipMemcpy(found, d_found, (size_t)n_sets * 8, hipMemcpyDeviceToHost)); // (every round was waited for)
    GN_HIP(hipMemcpy(first_lost, d_first, (size_t)n_sets * 8, hipMemcpyDeviceToHost));
    if (lost_at)
        GN_HIP(hipMemcpy(lost_at, d_lost, n_lost * 8, hipMemcpyDeviceToHost));
    return GN_OK;
}

// A lane owns a path, a wave 64 paths and `chunks` chunks of 64 probes.  Per chunk the lane keeps a 64-bit mask of the probes still
// contained; the entries are walked from the root down (the root is the last used entry), so that most probes die where the lanes of
// a wave -- neighbours in (leaf ibf, first bin) order when the caller sorts -- read the same words of the same IBF.  The probe is read
// at a wave-uniform address.  found[] takes one atomic add per lane and wave: integers, so neither the order of the paths nor the
// cut of the probes into waves shows in the result.
template <uint32_t H>
__global__ __launch_bounds__(256) void gn_probe_shared_kernel(const uint64_t* __restrict__ probes, uint64_t n, const GnPathDev* __restrict__ paths,
                                                              uint32_t n_paths, uint32_t depth, uint32_t path_waves, uint32_t chunks,
                                                              unsigned long long* __restrict__ found)
{
    const uint32_t wave  = (uint32_t)__builtin_amdgcn_readfirstlane((int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6));
    const uint32_t group = wave % path_waves;
    const uint64_t c0    = (uint64_t)(wave / path_waves) * chunks;
    const uint32_t path  = group * 64u + (threadIdx.x & 63u);
    const bool     mine  = path < n_paths;
    const GnPathDev* __restrict__ p = paths + (uint64_t)(mine ? path : 0) * depth;
    uint32_t       total = 0;
    for (uint64_t c = c0; c < c0 + chunks && c * 64u < n; ++c)
    {
        const uint64_t* __restrict__ pr  = probes + c * 64u;
        const uint32_t               cnt = (uint32_t)min((uint64_t)64, n - c * 64u);
        uint64_t                     alive = !mine ? 0 : cnt == 64u ? ~0ULL : (1ULL << cnt) - 1;
        for (uint32_t d = depth; d-- > 0;)
        {
            const GnPathDev e    = p[d];
            const bool      used = e.n_bins != 0 && alive != 0;
            if (__ballot(used) == 0)
                continue;
            GnGlobalConstWord* rows = (GnGlobalConstWord*)e.rows;
            const uint32_t     w0 = e.first_bin >> 6, w1 = used ? (e.first_bin + e.n_bins - 1) >> 6 : w0;
            for (uint32_t q = 0; q < cnt; ++q)
            {
                const uint64_t v = pr[q];
                if (!used || !((alive >> q) & 1))
                    continue;
                bool hit = false;
                for (uint32_t w = w0; w <= w1 && !hit; ++w)
                {
                    uint64_t r[H];
#pragma unroll
                    for (uint32_t i = 0; i < H; ++i)
                        r[i] = rows[(uint64_t)gn_build_row(v, i, e.shift, e.S) * e.Ws + w];
                    uint64_t a = r[0];
#pragma unroll
                    for (uint32_t i = 1; i < H; ++i)
                        a &= r[i];
                    hit = (a & gn_run_mask(e.first_bin, e.n_bins, w)) != 0;
                }
                if (!hit)
                    alive &= ~(1ULL << q);
            }
        }
        total += (uint32_t)__popcll(alive);
    }
    if (mine && total)
        atomicAdd(&found[path], (unsigned long long)total);
}

extern "C" int gn_filter_probe_paths_shared(gn_filter* f, const uint64_t* probes, uint64_t n, const gn_path_entry* paths, uint32_t n_paths, uint32_t depth,
                                            uint64_t* found)
{
    if (!f || !f->is_hibf)
        return gn_fail(GN_EINVAL, "gn_filter_probe_paths_shared needs an HIBF filter");
    if (n_paths == 0)
        return GN_OK;
    if (!paths || !found || depth == 0 || (n && !probes))
        return gn_fail(GN_EINVAL, "gn_filter_probe_paths_shared: null argument");
    const uint32_t h = f->ibfs[0].h;
    if (h < 1 || h > GN_IBF_MAX_HASH_FUNS)
        return gn_fail(GN_EINVAL, "gn_filter_probe_paths_shared: %u hash functions", h);
    std::vector<GnPathDev> dev;
    if (const int rc = gn_paths_resolve("gn_filter_probe_paths_shared", f, nullptr, n_paths, paths, depth, false, dev))
        return rc;
    std::fill(found, found + n_paths, 0);
    if (n == 0)
        return GN_OK;
    GN_HIP(hipSetDevice(f->device));
    if (!f->load_st)
        GN_HIP(hipStreamCreateWithFlags(&f->load_st, hipStreamNonBlocking));
    GnDev<uint64_t>           d_probes;
    GnDev<GnPathDev>          d_paths;
    GnDev<unsigned long long> d_found;
    GN_HIP(d_probes.alloc(n));
    GN_HIP(d_paths.alloc(dev.size()));
    GN_HIP(d_found.alloc(n_paths));
    GN_HIP(hipMemcpyAsync(d_probes, probes, n * 8, hipMemcpyHostToDevice, f->load_st));
    GN_HIP(hipMemcpyAsync(d_paths, dev.data(), dev.size() * sizeof(GnPathDev), hipMemcpyHostToDevice, f->load_st));
    GN_HIP(hipMemsetAsync(d_found, 0, (size_t)n_paths * 8, f->load_st));
    // enough waves to fill the device whatever the number of paths: the probes are cut so that about 8192 waves come out
    const uint64_t n_chunks = (n + 63) / 64, path_waves = ((uint64_t)n_paths + 63) / 64;
    const uint64_t chunks   = std::max<uint64_t>(1, (n_chunks * path_waves + 8191) / 8192);
    const uint64_t waves    = path_waves * ((n_chunks + chunks - 1) / chunks);
    if (chunks > 0xFFFFFFFFull || (waves + 3) / 4 > 0x7FFFFFFFull)
        return gn_fail(GN_ERANGE, "gn_filter_probe_paths_shared: %llu probes against %u paths in one call", (unsigned long long)n, n_paths);
    const dim3 grid((uint32_t)((waves + 3) / 4)), block(256);
    switch (h)
    {
    case 1: hipLaunchKernelGGL(gn_probe_shared_kernel<1>, grid, block, 0, f->load_st, d_probes, n, d_paths, n_paths, depth, (uint32_t)path_waves, (uint32_t)chunks, d_found); break;
    case 2: hipLaunchKernelGGL(gn_probe_shared_kernel<2>, grid, block, 0, f->load_st, d_probes, n, d_paths, n_paths, depth, (uint32_t)path_waves, (uint32_t)chunks, d_found); break;
    case 3: hipLaunchKernelGGL(gn_probe_shared_kernel<3>, grid, block, 0, f->load_st, d_probes, n, d_paths, n_paths, depth, (uint32_t)path_waves, (uint32_t)chunks, d_found); break;
    case 4: hipLaunchKernelGGL(gn_probe_shared_kernel<4>, grid, block, 0, f->load_st, d_probes, n, d_paths, n_paths, depth, (uint32_t)path_waves, (uint32_t)chunks, d_found); break;
    default: hipLaunchKernelGGL(gn_probe_shared_kernel<5>, grid, block, 0, f->load_st, d_probes, n, d_paths, n_paths, depth, (uint32_t)path_waves, (uint32_t)chunks, d_found); break;
    }
    GN_HIP(hipGetLastError());
    GN_HIP(hipStreamSynchronize(f->load_st));
    GN_HIP(hipMemcpy(found, d_found, (size_t)n_paths * 8, hipMemcpyDeviceToHost));
    return GN_OK;
}

// ---- gn_filter_probe_path_window / gn_filter_probe_paths_shared_window: the probes on pieces of IBFs --------------------------------
// IBF j of the filter stands for rows [row_begin[j], row_begin[j] + S_j) of an IBF of total_rows[j] rows, as for the windowed insert
// (`ganon-build --hibf --verify-index --verify-memory / --verify-devices`: build_verify_parts.cpp).  A lookup cannot be cut as cheaply as
// an insert: a hash is in a run only if ONE bin has its bit in all h rows, and those rows may lie in different pieces.  So the answer of
// a piece that is a slab of its IBF is carried per bin: plane b of an entry says "every row of the hash seen so far has the bit of bin
// first_bin + b", and the caller closes the entry when the last slab is through (host/hibf_verify_parts.hpp).  An entry whose piece is
// the whole IBF needs no planes: its answer per hash is final.

// One path entry as the two kernels read it: the geometry of the WHOLE IBF and the piece of it this filter holds (48 bytes).
struct GnProbeWinDev
{
    uint64_t* rows;              // the piece: n_rows rows of Ws words
    uint64_t  S_total;           // rows of the whole IBF
    uint64_t  plane_at;          // gn_probe_shared_window_kernel: word of the entry's first plane in the planes buffer
    uint32_t  Ws, shift;         // words from one row to the next; countl_zero(S_total)
    uint32_t  first_bin, n_bins; // n_bins == 0: the path ends above this entry
    uint32_t  row_begin, n_rows; // the piece is rows [row_begin, row_begin + n_rows) of the whole IBF
    uint32_t  slab, reserved;    // slab != 0: answered per bin into planes
};

// One wave per item, as gn_probe_path_kernel: item and path entries in SGPRs, 8 hashes a lane in registers.  An item starts at a multiple
// of 512 hashes of its set (the host cuts them so), so slot j of the wave is word begin / 64 + j of every bitmap of the set and a ballot
// IS that word: the wave writes whole words that no other wave writes, to out + out_at[item] -- per used entry in order 8 words (bit l of
// word j: the hash in slot j of lane l is contained) for a whole piece, 8 * n_bins words (plane b at b * 8) for a slab -- and the host ANDs
// them into the caller's bitmaps.  Per entry and word of the run the row words of all 8 * H (hash, row) pairs are fetched before any is
// used.  A row outside the piece contributes all ones: its lane loads *ones_word, a word of all ones that is surely there -- the address
// is selected, not the value, so no flag has to outlive the loads and no load sits behind a lane-dependent branch.  A lane without a hash in a slot probes hash 0 there and the host masks its bit away.
template <uint32_t H>
__global__ __launch_bounds__(256) void gn_probe_path_window_kernel(const uint64_t* __restrict__ stage, const GnRunItem* __restrict__ items,
                                                                   const uint64_t* __restrict__ out_at, uint32_t n_items,
                                                                   const GnProbeWinDev* __restrict__ paths, uint32_t depth,
                                                                   const unsigned long long* __restrict__ ones_word, unsigned long long* __restrict__ out)
{
    const uint32_t item = (uint32_t)__builtin_amdgcn_readfirstlane((int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6));
    if (item >= n_items)
        return;
    const uint32_t  lane = threadIdx.x & 63u;
    const GnRunItem it   = items[item];
    uint64_t        v[GN_WIN_PER_LANE];
#pragma unroll
    for (uint32_t j = 0; j < GN_WIN_PER_LANE; ++j)
    {
        const uint32_t q = j * 64u + lane;
        v[j]             = q < it.cnt ? stage[it.stage_at + q] : 0;
    }
    const GnProbeWinDev* __restrict__ p = paths + (uint64_t)it.run * depth;
    unsigned long long* __restrict__ o  = out + out_at[item];
    for (uint32_t d = 0; d < depth; ++d)
    {
        const GnProbeWinDev e = p[d];
        if (e.n_bins == 0)
            break;
        GnGlobalConstWord* rows = (GnGlobalConstWord*)e.rows;
        const uint64_t     ones_at = ((uint64_t)ones_word - (uint64_t)e.rows) >> 3; // *ones_word as a word of `rows`, modulo 2^64
        const uint32_t     w1   = (e.first_bin + e.n_bins - 1) >> 6;
        uint32_t           hit  = 0;
        for (uint32_t w = e.first_bin >> 6; w <= w1; ++w)
        {
            uint64_t r[GN_WIN_PER_LANE][H];
#pragma unroll
            for (uint32_t j = 0; j < GN_WIN_PER_LANE; ++j)
#pragma unroll
                for (uint32_t i = 0; i < H; ++i)
                {
                    // gn_window_local in arithmetic, and the mask made opaque: 8 * H compares kept as lane masks until their selects
                    // would take 16 * H SGPRs, more than there are
                    const uint32_t local = gn_build_row(v[j], i, e.shift, e.S_total) - e.row_begin;
                    uint32_t       m     = 0u - (uint32_t)(((uint64_t)local - (uint64_t)e.n_rows) >> 63); // all ones: local < n_rows
                    asm("" : "+v"(m));
                    const uint64_t at = (uint64_t)local * e.Ws + w;
                    r[j][i]           = rows[ones_at + ((at - ones_at) & (uint64_t)(int64_t)(int32_t)m)];
                }
            uint64_t a[GN_WIN_PER_LANE];
#pragma unroll
            for (uint32_t j = 0; j < GN_WIN_PER_LANE; ++j)
            {
                a[j] = r[j][0];
#pragma unroll
                for (uint32_t i = 1; i < H; ++i)
                    a[j] &= r[j][i];
            }
            if (!e.slab)
            {
                const uint64_t mask = gn_run_mask(e.first_bin, e.n_bins, w);
#pragma unroll
                for (uint32_t j = 0; j < GN_WIN_PER_LANE; ++j)
                    hit |= ((a[j] & mask) != 0 ? 1u : 0u) << j;
                continue;
            }
            // a slab: one plane per bin of the run that lies in this word; lane j < 8 keeps ballot j, the eight leave as one 64-byte store
            const uint32_t b_lo = max(e.first_bin, w << 6), b_hi = min(e.first_bin + e.n_bins, (w + 1u) << 6);
            for (uint32_t b = b_lo; b < b_hi; ++b)
            {
                unsigned long long mine = 0;
#pragma unroll
                for (uint32_t j = 0; j < GN_WIN_PER_LANE; ++j)
                {
                    const unsigned long long bal = __ballot((a[j] >> (b & 63u)) & 1ull);
                    mine                         = lane == j ? bal : mine;
                }
                if (lane < GN_WIN_PER_LANE)
                    o[(uint64_t)(b - e.first_bin) * GN_WIN_PER_LANE + lane] = mine;
            }
        }
        if (!e.slab)
        {
            unsigned long long mine = 0;
#pragma unroll
            for (uint32_t j = 0; j < GN_WIN_PER_LANE; ++j)
            {
                const unsigned long long bal = __ballot((hit >> j) & 1u);
                mine                         = lane == j ? bal : mine;
            }
            if (lane < GN_WIN_PER_LANE)
                o[lane] = mine;
        }
        o += (uint64_t)(e.slab ? e.n_bins : 1u) * GN_WIN_PER_LANE;
    }
}

template <uint32_t H>
static void gn_probe_path_window_launch(hipStream_t st, const uint64_t* stage, const GnRunItem* items, const uint64_t* out_at, uint32_t n_items,
                                        const GnProbeWinDev* paths, uint32_t depth, const unsigned long long* ones, unsigned long long* out)
{
    hipLaunchKernelGGL(gn_probe_path_window_kernel<H>, dim3((n_items + 3) / 4), dim3(256), 0, st, stage, items, out_at, n_items, paths, depth, ones, out);
}

// What the two windowed probes check before anything is launched, with the codes of gn_filter_emplace_path_window: the windows, then
// every entry of every path -- the IBF and the bins in range, every IBF of h hash functions -- resolved into `dev`.  slab(s, d) says
// whether the caller gave planes for the entry.
template <typename Slab>
static int gn_probe_window_resolve(const char* who, const gn_filter* f, uint32_t n_paths, const gn_path_entry* paths, uint32_t depth, const uint64_t* total_rows,
                                   const uint64_t* row_begin, Slab slab, std::vector<GnProbeWinDev>& dev)
{
    for (size_t j = 0; j < f->ibfs.size(); ++j)
    {
        if (total_rows[j] == 0 || total_rows[j] > 0xFFFFFFFFull)
            return gn_fail(GN_ERANGE, "%s: ibf %zu: an IBF of %llu rows, 1 .. 2^32 - 1 are supported", who, j, (unsigned long long)total_rows[j]);
        if (row_begin[j] > total_rows[j] || f->ibfs[j].S > total_rows[j] - row_begin[j])
            return gn_fail(GN_EINVAL, "%s: ibf %zu: rows %llu .. %llu of an IBF of %llu rows", who, j, (unsigned long long)row_begin[j],
                           (unsigned long long)(row_begin[j] + f->ibfs[j].S), (unsigned long long)total_rows[j]);
    }
    const uint32_t h = f->ibfs[0].h;
    if (h < 1 || h > GN_IBF_MAX_HASH_FUNS)
        return gn_fail(GN_EINVAL, "%s: %u hash functions", who, h);
    dev.assign((size_t)n_paths * depth, GnProbeWinDev{ nullptr, 1, 0, 1, 0, 0, 0, 0, 0, 0, 0 });
    for (uint32_t s = 0; s < n_paths; ++s)
        for (uint32_t d = 0; d < depth && paths[(size_t)s * depth + d].n_bins != 0; ++d)
        {
            GnPathDev            o;
            const gn_path_entry& e = paths[(size_t)s * depth + d];
            if (const int rc = gn_path_resolve(who, f, e, s, d, false, 0, o))
                return rc;
            const GnIbfHost& ib = f->ibfs[e.ibf];
            if (ib.h != h)
                return gn_fail(GN_EINVAL, "%s: ibf %u has %u hash functions, ibf 0 has %u", who, e.ibf, ib.h, h);
            dev[(size_t)s * depth + d] = GnProbeWinDev{ o.rows, total_rows[e.ibf], 0, o.Ws, (uint32_t)__builtin_clzll(total_rows[e.ibf]), o.first_bin, o.n_bins,
                                                        (uint32_t)row_begin[e.ibf], (uint32_t)ib.S, slab(s, d) ? 1u : 0u, 0 };
        }
    return GN_OK;
}

namespace
{
struct GnProbeWindowStage // everything a call holds; freed when the call returns
{
    GnStreamPair                 streams;
    GnPinned<uint64_t>           h_stage[2], h_out_at[2], h_out[2];
    GnPinned<GnRunItem>          h_items[2];
    GnDev<uint64_t>              d_stage[2], d_out_at[2];
    GnDev<unsigned long long>    d_out[2];
    GnDev<GnRunItem>             d_items[2];
    GnDev<GnProbeWinDev>         d_paths;
    GnDev<unsigned long long>    d_ones; // one word of all ones: what a row outside its piece reads
    uint32_t                     n_items[2] = { 0, 0 };
};
} // namespace

extern "C" int gn_filter_probe_path_window(gn_filter* f, const uint64_t* const* sets, const uint64_t* set_sizes, uint32_t n_sets, const gn_path_entry* paths,
                                           uint32_t depth, const uint64_t* total_rows, const uint64_t* row_begin, uint64_t* const* alive,
                                           uint64_t* const* planes, uint64_t* lost_at, uint64_t chunk_hashes)
{
    static const char* const who = "gn_filter_probe_path_window";
    if (!f || !f->is_hibf)
        return gn_fail(GN_EINVAL, "%s needs an HIBF filter", who);
    if (!total_rows || !row_begin)
        return gn_fail(GN_EINVAL, "%s: null argument", who);
    if (n_sets && (!sets || !set_sizes || !paths || !alive || !lost_at || depth == 0))
        return gn_fail(GN_EINVAL, "%s: null argument", who);
    std::vector<GnProbeWinDev> dev;
    if (const int rc = gn_probe_window_resolve(who, f, n_sets, paths, depth, total_rows, row_begin,
                                               [&](uint32_t s, uint32_t d) { return planes && planes[(size_t)s * depth + d]; }, dev))
        return rc;
    if (n_sets == 0)
        return GN_OK;
    const uint32_t        h = f->ibfs[0].h;
    uint64_t              total = 0, widest = GN_WIN_PER_LANE;
    std::vector<uint64_t> item_words(n_sets, 0); // words an item of the set leaves in `out`
    for (uint32_t s = 0; s < n_sets; ++s)
    {
        if (set_sizes[s] && (!sets[s] || !alive[s]))
            return gn_fail(GN_EINVAL, "%s: set %u is null", who, s);
        total += set_sizes[s];
        for (uint32_t d = 0; d < depth && dev[(size_t)s * depth + d].n_bins != 0; ++d)
            item_words[s] += (uint64_t)(dev[(size_t)s * depth + d].slab ? dev[(size_t)s * depth + d].n_bins : 1u) * GN_WIN_PER_LANE;
        widest = std::max(widest, item_words[s]);
    }
    if (total == 0)
        return GN_OK;
    GN_HIP(hipSetDevice(f->device));
    // a chunk is a multiple of an item, and no item is cut by the end of a chunk (below): every item starts at a multiple of GN_WIN_ITEM
    // hashes of its set and owns whole words of the set's bitmaps
    uint64_t chunk = chunk_hashes ? chunk_hashes : GN_WIN_CHUNK;
    chunk          = std::min<uint64_t>((chunk + GN_WIN_ITEM - 1) / GN_WIN_ITEM * GN_WIN_ITEM, (total + GN_WIN_ITEM - 1) / GN_WIN_ITEM * GN_WIN_ITEM);
    const uint64_t cap_items = chunk / 64 + 16;
    const uint64_t cap_out   = std::max<uint64_t>(widest, chunk / 8); // words of answers a chunk may leave: one item's at least
    GnProbeWindowStage g;
    for (int b = 0; b < 2; ++b)
    {
        GN_HIP(hipStreamCreateWithFlags(&g.streams.st[b], hipStreamNonBlocking));
        GN_HIP(g.h_stage[b].alloc(chunk));
        GN_HIP(g.h_items[b].alloc(cap_items));
        GN_HIP(g.h_out_at[b].alloc(cap_items));
        GN_HIP(g.h_out[b].alloc(cap_out));
        GN_HIP(g.d_stage[b].alloc(chunk));
        GN_HIP(g.d_items[b].alloc(cap_items));
        GN_HIP(g.d_out_at[b].alloc(cap_items));
        GN_HIP(g.d_out[b].alloc(cap_out));
    }
    GN_HIP(g.d_paths.upload(dev.data(), dev.size()));
    const unsigned long long all_ones = ~0ull;
    GN_HIP(g.d_ones.upload(&all_ones, 1));
    // the answers of the chunk that went through buffer b, ANDed into the caller's bitmaps (its stream has been waited for)
    auto take = [&](uint32_t b) {
        for (uint32_t k = 0; k < g.n_items[b]; ++k)
        {
            const GnRunItem& it = g.h_items[b][k];
            const uint64_t*  o  = g.h_out[b] + g.h_out_at[b][k];
            const uint32_t   s = it.run, nw = (it.cnt + 63u) / 64u;
            const uint64_t   w0 = it.begin / 64, words = (set_sizes[s] + 63) / 64;
            for (uint32_t d = 0; d < depth && dev[(size_t)s * depth + d].n_bins != 0; ++d)
            {
                const GnProbeWinDev& e = dev[(size_t)s * depth + d];
                if (!e.slab)
                {
                    uint64_t lost = 0;
                    for (uint32_t j = 0; j < nw; ++j)
                    {
                        const uint32_t left  = it.cnt - j * 64u;
                        const uint64_t valid = left >= 64u ? ~0ull : (1ull << left) - 1;
                        lost += (uint64_t)__builtin_popcountll(valid & ~o[j]);
                        alive[s][w0 + j] &= o[j] | ~valid; // (bits behind the set's last hash stay as they are: zero)
                    }
                    lost_at[(size_t)s * depth + d] += lost;
                    o += GN_WIN_PER_LANE;
                    continue;
                }
                uint64_t* pl = planes[(size_t)s * depth + d];
                for (uint32_t bin = 0; bin < e.n_bins; ++bin, o += GN_WIN_PER_LANE)
                    for (uint32_t j = 0; j < nw; ++j)
                        pl[(uint64_t)bin * words + w0 + j] &= o[j];
            }
        }
        g.n_items[b] = 0;
    };
    std::vector<GnRunItem> items;
    GnRunCursor            cur;
    hipError_t             err = hipSuccess;
    for (uint32_t c = 0; err == hipSuccess; ++c)
    {
        const uint32_t b = c & 1u;
        if ((err = hipStreamSynchronize(g.streams.st[b])) != hipSuccess)
            break;
        take(b);
        uint64_t taken = gn_window_next_chunk(set_sizes, n_sets, cur, chunk, cap_items, items);
        if (taken == 0)
            break;
        // an item the end of the chunk has cut goes to the next chunk whole, and so do the items whose answers the buffer does not hold
        uint64_t words = 0;
        size_t   keep  = 0;
        for (; keep < items.size(); ++keep)
        {
            const GnRunItem& it = items[keep];
            if (it.cnt < GN_WIN_ITEM && it.begin + it.cnt < set_sizes[it.run])
                break;
            if (keep && words + item_words[it.run] > cap_out)
                break;
            g.h_out_at[b][keep] = words;
            words += item_words[it.run];
        }
        if (keep < items.size())
        {
            cur.run = items[keep].run, cur.at = items[keep].begin;
            taken = items[keep].stage_at;
            items.resize(keep);
        }
        for (const GnRunItem& it : items)
            memcpy(g.h_stage[b] + it.stage_at, sets[it.run] + it.begin, (size_t)it.cnt * 8);
        memcpy(g.h_items[b].get(), items.data(), items.size() * sizeof(GnRunItem));
        const uint32_t n_items = (uint32_t)items.size();
        hipStream_t    st = g.streams.st[b];
        if ((err = hipMemcpyAsync(g.d_stage[b], g.h_stage[b], taken * 8, hipMemcpyHostToDevice, st)) != hipSuccess ||
            (err = hipMemcpyAsync(g.d_items[b], g.h_items[b], n_items * sizeof(GnRunItem), hipMemcpyHostToDevice, st)) != hipSuccess ||
            (err = hipMemcpyAsync(g.d_out_at[b], g.h_out_at[b], n_items * sizeof(uint64_t), hipMemcpyHostToDevice, st)) != hipSuccess)
            break;
        const uint64_t*      d_stage = g.d_stage[b];
        const GnRunItem*     d_items = g.d_items[b];
        const uint64_t*      d_at    = g.d_out_at[b];
        const GnProbeWinDev* d_paths = g.d_paths;
        switch (h)
        {
        case 1: gn_probe_path_window_launch<1>(st, d_stage, d_items, d_at, n_items, d_paths, depth, g.d_ones, g.d_out[b]); break;
        case 2: gn_probe_path_window_launch<2>(st, d_stage, d_items, d_at, n_items, d_paths, depth, g.d_ones, g.d_out[b]); break;
        case 3: gn_probe_path_window_launch<3>(st, d_stage, d_items, d_at, n_items, d_paths, depth, g.d_ones, g.d_out[b]); break;
        case 4: gn_probe_path_window_launch<4>(st, d_stage, d_items, d_at, n_items, d_paths, depth, g.d_ones, g.d_out[b]); break;
        default: gn_probe_path_window_launch<5>(st, d_stage, d_items, d_at, n_items, d_paths, depth, g.d_ones, g.d_out[b]); break;
        }
        if ((err = hipGetLastError()) != hipSuccess || (words && (err = hipMemcpyAsync(g.h_out[b], g.d_out[b], words * 8, hipMemcpyDeviceToHost, st)) != hipSuccess))
            break;
        g.n_items[b] = n_items;
    }
    // (also after a failure: nothing of `g` is freed under a copy or a kernel that still uses it)
    const hipError_t e0 = hipStreamSynchronize(g.streams.st[0]), e1 = hipStreamSynchronize(g.streams.st[1]);
    GN_HIP(err);
    GN_HIP(e0);
    GN_HIP(e1);
    take(0), take(1);
    return GN_OK;
}

// The shape of gn_probe_shared_kernel: a lane owns a path, a wave 64 paths and `chunks` chunks of 64 probes; word c of the lane's `alive`
// bitmap is its mask of chunk c.  An entry in a whole piece clears the probes it does not hold from the mask, as there.  An entry in a slab
// ANDs per-bin masks into the lane's planes (plane b at plane_at + b * n_chunks): eight bins at a time in registers, so the rows of a probe
// are fetched once per eight bins of a word.  A row outside the piece contributes all ones.  No ballots, no atomics: the lane owns every
// word it writes.  A probe that an earlier entry or part has cleared from `alive` is not looked at again -- its planes then say nothing,
// and nobody asks them: the caller ANDs the closed planes into `alive`.
template <uint32_t H>
__global__ __launch_bounds__(256) void gn_probe_shared_window_kernel(const uint64_t* __restrict__ probes, uint64_t n, const GnProbeWinDev* __restrict__ paths,
                                                                     uint32_t n_paths, uint32_t depth, uint32_t path_waves, uint32_t chunks,
                                                                     unsigned long long* __restrict__ alive_words, unsigned long long* __restrict__ planes)
{
    const uint32_t wave     = (uint32_t)__builtin_amdgcn_readfirstlane((int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6));
    const uint32_t group    = wave % path_waves;
    const uint64_t c0       = (uint64_t)(wave / path_waves) * chunks;
    const uint64_t n_chunks = (n + 63) / 64;
    const uint32_t path     = group * 64u + (threadIdx.x & 63u);
    const bool     mine     = path < n_paths;
    const GnProbeWinDev* __restrict__ p = paths + (uint64_t)(mine ? path : 0) * depth;
    for (uint64_t c = c0; c < c0 + chunks && c < n_chunks; ++c)
    {
        const uint64_t* __restrict__ pr  = probes + c * 64u;
        const uint32_t               cnt = (uint32_t)min((uint64_t)64, n - c * 64u);
        uint64_t                     alive = mine ? alive_words[(uint64_t)path * n_chunks + c] : 0;
        for (uint32_t d = depth; d-- > 0;)
        {
            const GnProbeWinDev e    = p[d];
            const bool          used = e.n_bins != 0 && alive != 0;
            if (__ballot(used) == 0)
                continue;
            GnGlobalConstWord* rows = (GnGlobalConstWord*)e.rows;
            const uint32_t     w0 = e.first_bin >> 6, w1 = used ? (e.first_bin + e.n_bins - 1) >> 6 : w0;
            // the AND of the probe's rows inside the piece at word w
            auto rows_and = [&](uint64_t v, uint32_t w) {
                uint64_t a = ~0ULL;
#pragma unroll
                for (uint32_t i = 0; i < H; ++i)
                {
                    uint32_t   local;
                    const bool inside = gn_window_local(gn_build_row(v, i, e.shift, e.S_total), e.row_begin, e.n_rows, &local);
                    const uint64_t r  = rows[(uint64_t)(inside ? local : 0u) * e.Ws + w];
                    a &= inside ? r : ~0ULL;
                }
                return a;
            };
            if (!e.slab || !used)
            {
                for (uint32_t q = 0; q < cnt; ++q)
                {
                    const uint64_t v = pr[q];
                    if (!used || !((alive >> q) & 1))
                        continue;
                    bool hit = false;
                    for (uint32_t w = w0; w <= w1 && !hit; ++w)
                        hit = (rows_and(v, w) & gn_run_mask(e.first_bin, e.n_bins, w)) != 0;
                    if (!hit)
                        alive &= ~(1ULL << q);
                }
                continue;
            }
            unsigned long long* __restrict__ pl = planes + e.plane_at + c;
            for (uint32_t w = w0; w <= w1; ++w)
            {
                const uint32_t b_lo = max(e.first_bin, w << 6), b_hi = min(e.first_bin + e.n_bins, (w + 1u) << 6);
                for (uint32_t b0 = b_lo; b0 < b_hi; b0 += 8u)
                {
                    uint64_t m[8];
#pragma unroll
                    for (uint32_t t = 0; t < 8u; ++t)
                        m[t] = ~0ULL;
                    for (uint32_t q = 0; q < cnt; ++q)
                    {
                        const uint64_t v = pr[q];
                        if (!((alive >> q) & 1))
                            continue;
                        const uint64_t a = rows_and(v, w) >> (b0 & 63u);
#pragma unroll
                        for (uint32_t t = 0; t < 8u; ++t)
                            m[t] &= ~(((~a >> t) & 1ULL) << q);
                    }
#pragma unroll
                    for (uint32_t t = 0; t < 8u; ++t)
                        if (b0 + t < b_hi)
                            pl[(uint64_t)(b0 + t - e.first_bin) * n_chunks] &= m[t];
                }
            }
        }
        if (mine)
            alive_words[(uint64_t)path * n_chunks + c] = alive;
    }
}

extern "C" int gn_filter_probe_paths_shared_window(gn_filter* f, const uint64_t* probes, uint64_t n, const gn_path_entry* paths, uint32_t n_paths,
                                                   uint32_t depth, const uint64_t* total_rows, const uint64_t* row_begin, uint64_t* alive,
                                                   uint64_t* const* planes)
{
    static const char* const who = "gn_filter_probe_paths_shared_window";
    if (!f || !f->is_hibf)
        return gn_fail(GN_EINVAL, "%s needs an HIBF filter", who);
    if (!total_rows || !row_begin)
        return gn_fail(GN_EINVAL, "%s: null argument", who);
    if (n_paths && (!paths || depth == 0 || (n && (!probes || !alive))))
        return gn_fail(GN_EINVAL, "%s: null argument", who);
    std::vector<GnProbeWinDev> dev;
    if (const int rc = gn_probe_window_resolve(who, f, n_paths, paths, depth, total_rows, row_begin,
                                               [&](uint32_t s, uint32_t d) { return planes && planes[(size_t)s * depth + d]; }, dev))
        return rc;
    if (n_paths == 0 || n == 0)
        return GN_OK;
    const uint32_t h        = f->ibfs[0].h;
    const uint64_t n_chunks = (n + 63) / 64, path_waves = ((uint64_t)n_paths + 63) / 64;
    const uint64_t chunks   = std::max<uint64_t>(1, (n_chunks * path_waves + 8191) / 8192);
    const uint64_t waves    = path_waves * ((n_chunks + chunks - 1) / chunks);
    if (chunks > 0xFFFFFFFFull || (waves + 3) / 4 > 0x7FFFFFFFull)
        return gn_fail(GN_ERANGE, "%s: %llu probes against %u paths in one call", who, (unsigned long long)n, n_paths);
    // the planes of the call behind each other, in the order of the entries
    uint64_t plane_words = 0;
    for (GnProbeWinDev& e : dev)
        if (e.n_bins && e.slab)
            e.plane_at = plane_words, plane_words += (uint64_t)e.n_bins * n_chunks;
    std::vector<uint64_t> h_planes(plane_words);
    for (size_t k = 0; k < dev.size(); ++k)
        if (dev[k].n_bins && dev[k].slab)
            memcpy(h_planes.data() + dev[k].plane_at, planes[k], (size_t)dev[k].n_bins * n_chunks * 8);
    GN_HIP(hipSetDevice(f->device));
    if (!f->load_st)
        GN_HIP(hipStreamCreateWithFlags(&f->load_st, hipStreamNonBlocking));
    GnDev<uint64_t>           d_probes;
    GnDev<GnProbeWinDev>      d_paths;
    GnDev<unsigned long long> d_alive, d_planes;
    std::vector<uint64_t>     h_alive((size_t)n_paths * n_chunks);
    GN_HIP(d_probes.alloc(n));
    GN_HIP(d_paths.alloc(dev.size()));
    GN_HIP(d_alive.alloc(h_alive.size()));
    GN_HIP(d_planes.alloc(std::max<uint64_t>(plane_words, 1)));
    GN_HIP(hipMemcpyAsync(d_probes, probes, n * 8, hipMemcpyHostToDevice, f->load_st));
    GN_HIP(hipMemcpyAsync(d_paths, dev.data(), dev.size() * sizeof(GnProbeWinDev), hipMemcpyHostToDevice, f->load_st));
    GN_HIP(hipMemcpyAsync(d_alive, alive, h_alive.size() * 8, hipMemcpyHostToDevice, f->load_st));
    if (plane_words)
        GN_HIP(hipMemcpyAsync(d_planes, h_planes.data(), plane_words * 8, hipMemcpyHostToDevice, f->load_st));
    const dim3 grid((uint32_t)((waves + 3) / 4)), block(256);
    switch (h)
    {
    case 1: hipLaunchKernelGGL(gn_probe_shared_window_kernel<1>, grid, block, 0, f->load_st, d_probes, n, d_paths, n_paths, depth, (uint32_t)path_waves, (uint32_t)chunks, d_alive, d_planes); break;
    case 2: hipLaunchKernelGGL(gn_probe_shared_window_kernel<2>, grid, block, 0, f->load_st, d_probes, n, d_paths, n_paths, depth, (uint32_t)path_waves, (uint32_t)chunks, d_alive, d_planes); break;
    case 3: hipLaunchKernelGGL(gn_probe_shared_window_kernel<3>, grid, block, 0, f->load_st, d_probes, n, d_paths, n_paths, depth, (uint32_t)path_waves, (uint32_t)chunks, d_alive, d_planes); break;
    case 4: hipLaunchKernelGGL(gn_probe_shared_window_kernel<4>, grid, block, 0, f->load_st, d_probes, n, d_paths, n_paths, depth, (uint32_t)path_waves, (uint32_t)chunks, d_alive, d_planes); break;
    default: hipLaunchKernelGGL(gn_probe_shared_window_kernel<5>, grid, block, 0, f->load_st, d_probes, n, d_paths, n_paths, depth, (uint32_t)path_waves, (uint32_t)chunks, d_alive, d_planes); break;
    }
    GN_HIP(hipGetLastError());
    // into buffers of the call's own first: a copy that fails leaves the caller's as they were
    GN_HIP(hipMemcpyAsync(h_alive.data(), d_alive, h_alive.size() * 8, hipMemcpyDeviceToHost, f->load_st));
    if (plane_words)
        GN_HIP(hipMemcpyAsync(h_planes.data(), d_planes, plane_words * 8, hipMemcpyDeviceToHost, f->load_st));
    GN_HIP(hipStreamSynchronize(f->load_st));
    memcpy(alive, h_alive.data(), h_alive.size() * 8);
    for (size_t k = 0; k < dev.size(); ++k)
        if (dev[k].n_bins && dev[k].slab)
            memcpy(planes[k], h_planes.data() + dev[k].plane_at, (size_t)dev[k].n_bins * n_chunks * 8);
    return GN_OK;
}

// ---- gn_filter_extend_path: more hashes for user bins that are filled already ------------------------------------------------------
// Two sweeps over the items of the whole call, as gn_path_rounds cuts them; item g of the call is item g - item_base of its round.
// Sweep 1 is the probe restricted to entry 0 (the user bin's leaf run): per word of the run all 8 * H row words are loaded before any is
// looked at, ANDed and masked to the run.  Instead of a count the wave leaves its eight 64-bit ballots of "has a hash and the run does not
// hold it" -- flags[g * 8 + j], bit l = slot j of lane l -- and their population, counts[g].  Nothing is ORed before every round of sweep 1
// is through: sweep 2 reads the flags and never the filter, so that no wave's new bits turn another wave's absent hash into a present one.
template <uint32_t H>
__global__ __launch_bounds__(256) void gn_extend_mark_kernel(const uint64_t* __restrict__ stage, const GnPathItem* __restrict__ items, uint32_t n_items,
                                                             const GnPathDev* __restrict__ paths, uint32_t depth, uint64_t item_base,
                                                             unsigned long long* __restrict__ flags, uint32_t* __restrict__ counts)
{
    const uint32_t item = (uint32_t)__builtin_amdgcn_readfirstlane((int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6));
    if (item >= n_items)
        return;
    const uint32_t   lane = threadIdx.x & 63u;
    const GnPathItem it   = items[item];
    uint64_t         v[GN_PATH_PER_LANE];
    uint32_t         valid = 0; // bit j: slot j holds a hash of the item
#pragma unroll
    for (uint32_t j = 0; j < GN_PATH_PER_LANE; ++j)
    {
        const uint32_t q = j * 64u + lane;
        v[j]             = q < it.cnt ? stage[it.stage_at + q] : 0;
        valid |= (q < it.cnt ? 1u : 0u) << j;
    }
    const GnPathDev    e    = paths[(uint64_t)it.seg * depth]; // (n_bins >= 1: the host refuses a set with hashes and no leaf run)
    GnGlobalConstWord* rows = (GnGlobalConstWord*)e.rows;
    const uint32_t     w1   = (e.first_bin + e.n_bins - 1) >> 6;
    uint32_t           hit  = 0;
    for (uint32_t w = e.first_bin >> 6; w <= w1; ++w)
    {
        const uint64_t mask = gn_run_mask(e.first_bin, e.n_bins, w);
        uint64_t       r[GN_PATH_PER_LANE][H];
#pragma unroll
        for (uint32_t j = 0; j < GN_PATH_PER_LANE; ++j)
#pragma unroll
            for (uint32_t i = 0; i < H; ++i)
                r[j][i] = rows[(uint64_t)gn_build_row(v[j], i, e.shift, e.S) * e.Ws + w];
#pragma unroll
        for (uint32_t j = 0; j < GN_PATH_PER_LANE; ++j)
        {
            uint64_t a = r[j][0];
#pragma unroll
            for (uint32_t i = 1; i < H; ++i)
                a &= r[j][i];
            hit |= ((a & mask) != 0 ? 1u : 0u) << j;
        }
    }
    const uint32_t     absent = valid & ~hit;
    unsigned long long mine   = 0; // lane j < 8 keeps ballot j: the eight leave as one 64-byte store
    uint32_t           n      = 0;
#pragma unroll
    for (uint32_t j = 0; j < GN_PATH_PER_LANE; ++j)
    {
        const unsigned long long b = __ballot((absent >> j) & 1u);
        n += (uint32_t)__popcll(b);
        mine = lane == j ? b : mine;
    }
    const uint64_t g = item_base + item;
    if (lane < GN_PATH_PER_LANE)
        flags[g * GN_PATH_PER_LANE + lane] = mine;
    if (lane == 0)
        counts[g] = n;
}

// Sweep 2.  ranks[g] is the exclusive sum of counts[] over the call, so ranks[g] - ranks[set_first[seg]] is the rank within its set of the
// item's first absent hash; the absent hash in slot j of lane l follows the absent ones of the slots below and of the lanes below in its
// slot.  cum + cum_at[seg] is the set's running sum of quotas, n_bins + 1 entries from 0: rank r belongs to the bin j with
// cum[j] <= r < cum[j + 1].  The bins of the item's first and last absent hash are searched once for the wave (item, flags and table
// come through scalar loads); a lane searches, between those two, only when they differ.  Then every hash of the item, present or not,
// goes into the merged bins above, as gn_emplace_path_kernel puts it there.
__global__ __launch_bounds__(256) void gn_extend_insert_kernel(const uint64_t* __restrict__ stage, const GnPathItem* __restrict__ items, uint32_t n_items,
                                                               const GnPathDev* __restrict__ paths, uint32_t depth, uint32_t h, uint64_t item_base,
                                                               const unsigned long long* __restrict__ flags, const uint64_t* __restrict__ ranks,
                                                               const uint64_t* __restrict__ set_first, const uint64_t* __restrict__ cum,
                                                               const uint64_t* __restrict__ cum_at)
{
    const uint32_t item = (uint32_t)__builtin_amdgcn_readfirstlane((int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6));
    if (item >= n_items)
        return;
    const uint32_t   lane = threadIdx.x & 63u;
    const GnPathItem it   = items[item];
    uint64_t         v[GN_PATH_PER_LANE];
#pragma unroll
    for (uint32_t j = 0; j < GN_PATH_PER_LANE; ++j)
    {
        const uint32_t q = j * 64u + lane;
        v[j]             = q < it.cnt ? stage[it.stage_at + q] : 0;
    }
    const uint64_t     g = item_base + item;
    unsigned long long b[GN_PATH_PER_LANE];
    uint32_t           n_absent = 0;
#pragma unroll
    for (uint32_t j = 0; j < GN_PATH_PER_LANE; ++j)
    {
        b[j] = flags[g * GN_PATH_PER_LANE + j];
        n_absent += (uint32_t)__popcll(b[j]);
    }
    const GnPathDev* __restrict__ p = paths + (uint64_t)it.seg * depth;
    if (n_absent)
    {
        const GnPathDev e    = p[0];
        const uint64_t  base = ranks[g] - ranks[set_first[it.seg]];
        const uint64_t* __restrict__ c = cum + cum_at[it.seg] + 1; // c[j]: the quotas of bins 0 .. j of the run, summed
        // the first j of lo .. hi with c[j] > r, hi when there is none below it (j < hi <= n_bins - 1 is all that is read)
        auto bin_of = [&](uint64_t r, uint32_t lo, uint32_t hi) {
            while (lo < hi)
            {
                const uint32_t mid = (lo + hi) >> 1;
                if (c[mid] <= r)
                    lo = mid + 1;
                else
                    hi = mid;
            }
            return lo;
        };
        const uint32_t b_lo = bin_of(base, 0u, e.n_bins - 1u), b_hi = bin_of(base + n_absent - 1u, b_lo, e.n_bins - 1u);
        uint32_t       below = 0; // absent hashes of the item in the slots before this one
#pragma unroll
        for (uint32_t j = 0; j < GN_PATH_PER_LANE; ++j)
        {
            if ((b[j] >> lane) & 1ull)
            {
                const uint64_t rank = base + below + (uint32_t)__popcll(b[j] & ((1ull << lane) - 1ull));
                const uint32_t bin  = e.first_bin + (b_lo == b_hi ? b_lo : bin_of(rank, b_lo, b_hi));
                GnGlobalWord*  word = (GnGlobalWord*)e.rows + (bin >> 6);
                const uint64_t bit  = 1ULL << (bin & 63);
                for (uint32_t i = 0; i < h; ++i)
                    (void)__hip_atomic_fetch_or(word + (uint64_t)gn_build_row(v[j], i, e.shift, e.S) * e.Ws, bit, __ATOMIC_RELAXED,
                                                __HIP_MEMORY_SCOPE_AGENT);
            }
            below += (uint32_t)__popcll(b[j]);
        }
    }
    for (uint32_t d = 1; d < depth; ++d)
    {
        const GnPathDev e = p[d];
        if (e.n_bins == 0)
            break;
        GnGlobalWord*  word = (GnGlobalWord*)e.rows + (e.first_bin >> 6); // (n_bins == 1: checked on the host)
        const uint64_t bit  = 1ULL << (e.first_bin & 63);
#pragma unroll
        for (uint32_t j = 0; j < GN_PATH_PER_LANE; ++j)
        {
            if (j * 64u + lane >= it.cnt)
                continue;
            for (uint32_t i = 0; i < h; ++i)
                (void)__hip_atomic_fetch_or(word + (uint64_t)gn_build_row(v[j], i, e.shift, e.S) * e.Ws, bit, __ATOMIC_RELAXED,
                                            __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

template <uint32_t H>
static hipError_t gn_extend_mark_launch(hipStream_t st, const uint64_t* stage, const GnPathItem* items, uint32_t n_items, const GnPathDev* paths, uint32_t depth,
                                        uint64_t item_base, unsigned long long* flags, uint32_t* counts)
{
    hipLaunchKernelGGL(gn_extend_mark_kernel<H>, dim3((n_items + 3) / 4), dim3(256), 0, st, stage, items, n_items, paths, depth, item_base, flags, counts);
    return hipSuccess;
}

extern "C" int gn_filter_extend_path(gn_filter* f, const uint64_t* hashes, const uint64_t* set_off, uint32_t n_sets, const gn_path_entry* paths,
                                     uint32_t depth, const uint64_t* deal_off, const uint64_t* deal)
{
    static const char* const who = "gn_filter_extend_path";
    if (!f || !f->is_hibf)
        return gn_fail(GN_EINVAL, "gn_filter_extend_path needs an HIBF filter");
    if (n_sets == 0)
        return GN_OK;
    if (!set_off || !paths || !deal_off || depth == 0 || (set_off[n_sets] && !hashes))
        return gn_fail(GN_EINVAL, "%s: null argument", who);
    const uint32_t h = f->ibfs[0].h;
    if (h < 1 || h > GN_IBF_MAX_HASH_FUNS)
        return gn_fail(GN_EINVAL, "%s: %u hash functions", who, h);
    const uint64_t total = set_off[n_sets];
    // the host's checks: the shape of every path, one quota per bin of the leaf run, strictly ascending sets
    std::vector<uint64_t> quota(n_sets, 0); // a set's quotas summed; above `total` where the sum does not fit
    for (uint32_t s = 0; s < n_sets; ++s)
    {
        if (set_off[s + 1] < set_off[s] || set_off[s + 1] > total) // (the sets are read below: none may reach beyond the last offset)
            return gn_fail(GN_EINVAL, "%s: set offsets descend at set %u", who, s);
        const gn_path_entry* p = paths + (size_t)s * depth;
        if (deal_off[s + 1] < deal_off[s] || deal_off[s + 1] - deal_off[s] != p[0].n_bins)
            return gn_fail(GN_EINVAL, "%s: set %u: %llu quotas for a run of %u bins", who, s, (unsigned long long)(deal_off[s + 1] - deal_off[s]), p[0].n_bins);
        if (p[0].n_bins == 0 && set_off[s + 1] != set_off[s])
            return gn_fail(GN_EINVAL, "%s: set %u has hashes and no leaf run", who, s);
        if (p[0].n_bins && !deal)
            return gn_fail(GN_EINVAL, "%s: null argument", who);
        for (uint32_t d = 1; d < depth && p[d - 1].n_bins && p[d].n_bins; ++d)
            if (p[d].n_bins != 1)
                return gn_fail(GN_EINVAL, "%s: set %u level %u: a run of %u bins above the leaf", who, s, d, p[d].n_bins);
        for (uint64_t j = deal_off[s]; j < deal_off[s + 1]; ++j)
            quota[s] = deal[j] > total || quota[s] > total ? total + 1 : quota[s] + deal[j];
        for (uint64_t i = set_off[s] + 1; i < set_off[s + 1]; ++i)
            if (hashes[i] <= hashes[i - 1])
                return gn_fail(GN_EINVAL, "%s: set %u is not strictly ascending at hash %llu", who, s, (unsigned long long)(i - set_off[s]));
    }
    const uint64_t step = gn_path_step(total);
    std::vector<uint64_t> set_first(n_sets + 1, 0), cum, cum_at(n_sets);
    for (uint32_t s = 0; s < n_sets; ++s)
    {
        set_first[s + 1] = set_first[s] + (total ? gn_path_items_of(set_off[s], set_off[s + 1], step) : 0);
        cum_at[s]        = cum.size();
        cum.push_back(0);
        for (uint64_t j = deal_off[s]; j < deal_off[s + 1]; ++j)
            cum.push_back(cum.back() + std::min(deal[j], total + 1)); // (read by sweep 2 only when the sum is the absent count)
    }
    const uint64_t n_items = set_first[n_sets];
    if (n_items + 1 > 0x7FFFFFFFull) // (the scan takes its item count as an int)
        return gn_fail(GN_ERANGE, "%s: %llu hashes in one call", who, (unsigned long long)total);

    GnDev<unsigned long long> d_flags;
    GnDev<uint32_t>           d_counts;
    GnDev<uint64_t>           d_ranks, d_set_first, d_cum, d_cum_at;
    GnDev<uint8_t>            d_tmp;
    std::vector<uint64_t>     ranks(n_items + 1, 0);
    if (total)
    {
        GN_HIP(hipSetDevice(f->device));
        GN_HIP(d_flags.alloc(n_items * GN_PATH_PER_LANE));
        GN_HIP(d_counts.alloc(n_items + 1));
        GN_HIP(d_ranks.alloc(n_items + 1));
    }
    uint64_t at = 0; // items launched so far
    int      rc = gn_path_rounds(who, f, hashes, set_off, n_sets, paths, depth, false,
                                 [&](const uint64_t* stage, const GnPathItem* items, uint32_t n, const GnPathDev* d_paths) -> hipError_t {
                                     if (at + n > n_items)
                                         return hipErrorInvalidValue; // (cannot happen: gn_path_items_of counts what gn_path_rounds cuts)
                                     const uint64_t base = at;
                                     at += n;
                                     // (the entry behind the last item stays 0: its rank is the call's absent count)
                                     if (base == 0)
                                         if (const hipError_t e = hipMemsetAsync(d_counts, 0, (n_items + 1) * sizeof(uint32_t), f->load_st))
                                             return e;
                                     switch (h)
                                     {
                                     case 1: return gn_extend_mark_launch<1>(f->load_st, stage, items, n, d_paths, depth, base, d_flags, d_counts);
                                     case 2: return gn_extend_mark_launch<2>(f->load_st, stage, items, n, d_paths, depth, base, d_flags, d_counts);
                                     case 3: return gn_extend_mark_launch<3>(f->load_st, stage, items, n, d_paths, depth, base, d_flags, d_counts);
                                     case 4: return gn_extend_mark_launch<4>(f->load_st, stage, items, n, d_paths, depth, base, d_flags, d_counts);
                                     default: return gn_extend_mark_launch<5>(f->load_st, stage, items, n, d_paths, depth, base, d_flags, d_counts);
                                     }
                                 });
    if (rc != GN_OK)
        return rc;
    if (total)
    {
        if (at != n_items)
            GN_HIP(hipErrorInvalidValue);
        // between the sweeps: the items' ranks, and every set's absent count against its quotas (every round was waited for)
        size_t tmp_bytes = 0;
        GN_HIP(gn_scan_counts(nullptr, tmp_bytes, d_counts.get(), d_ranks.get(), (int)(n_items + 1), f->load_st));
        GN_HIP(d_tmp.alloc(tmp_bytes));
        GN_HIP(gn_scan_counts(d_tmp.get(), tmp_bytes, d_counts.get(), d_ranks.get(), (int)(n_items + 1), f->load_st));
        GN_HIP(hipMemcpyAsync(ranks.data(), d_ranks, (n_items + 1) * 8, hipMemcpyDeviceToHost, f->load_st));
        GN_HIP(hipStreamSynchronize(f->load_st));
    }
    for (uint32_t s = 0; s < n_sets; ++s)
    {
        const uint64_t absent = ranks[set_first[s + 1]] - ranks[set_first[s]];
        if (quota[s] != absent)
        {
            if (quota[s] > total)
                return gn_fail(GN_EINVAL, "%s: set %u: the quotas sum to more than the call's %llu hashes, %llu of the set's %llu are absent from its run; nothing written",
                               who, s, (unsigned long long)total, (unsigned long long)absent, (unsigned long long)(set_off[s + 1] - set_off[s]));
            return gn_fail(GN_EINVAL, "%s: set %u: the quotas sum to %llu, %llu of the set's %llu hashes are absent from its run; nothing written", who, s,
                           (unsigned long long)quota[s], (unsigned long long)absent, (unsigned long long)(set_off[s + 1] - set_off[s]));
        }
    }
    if (total == 0)
        return GN_OK;
    GN_HIP(d_set_first.upload(set_first.data(), set_first.size()));
    GN_HIP(d_cum.upload(cum.data(), cum.size()));
    GN_HIP(d_cum_at.upload(cum_at.data(), cum_at.size()));
    at = 0;
    rc = gn_path_rounds(who, f, hashes, set_off, n_sets, paths, depth, false,
                        [&](const uint64_t* stage, const GnPathItem* items, uint32_t n, const GnPathDev* d_paths) -> hipError_t {
                            if (at + n > n_items)
                                return hipErrorInvalidValue; // (cannot happen: the same cut as sweep 1)
                            const uint64_t base = at;
                            at += n;
                            hipLaunchKernelGGL(gn_extend_insert_kernel, dim3((n + 3) / 4), dim3(256), 0, f->load_st, stage, items, n, d_paths, depth, h, base,
                                               (const unsigned long long*)d_flags, (const uint64_t*)d_ranks, (const uint64_t*)d_set_first,
                                               (const uint64_t*)d_cum, (const uint64_t*)d_cum_at);
                            return hipSuccess;
                        });
    return rc;
}

// ---- gn_filter_bin_popcounts: how full is every technical bin? -------------------------------------------------------------------
// A .hibf does not record how many hashes went into a bin; the set bits of the bin's column are all there is (`ganon-build --hibf
// --update` decides from them where a new user bin still fits).  counts[b] = rows whose bit b is set: a column sum over the whole
// bit matrix, every word read once.
//
// A lane owns one 64-bit word column and walks a tile of rows; neighbouring lanes read neighbouring words:
//   rows of at most 64 words   the matrix is one flat array: the wave reads g = 64 / Ws whole rows (g * Ws contiguous words) per step,
//                              lane l owns column l % Ws.  Where 64 is a multiple of Ws every lane works; otherwise 64 % Ws lanes idle.
//   wider rows                 chunks of 64 word columns: lane l of chunk c owns column 64 c + l and reads one row per step.
// Both are one address rule: word (tile * T + j) * step + c0 + l for j = 0 .. T - 1, valid while below S * Ws.
// The 64 per-bit counters of a lane are not touched per word.  16 loads are issued, then the 16 words go through a carry-save adder
// tree (15 adders of 5 logic operations on 64 bits) into 8 vertical bit planes -- plane k holds bit k of every bit position's count --
// and after 240 words (<= 255, what 8 planes hold) the planes are added into 64 32-bit counters in registers, the plane bits of four
// bit positions gathered into the bytes of one register at a time.  The steps in which every lane has a word run without a
// predicate; what is left of a tile (fewer than 16 steps, the matrix's last one perhaps cut) is one predicated block.
// At the end of the tile lanes that own the same column add up (Ws a power of two) and every counter leaves as one 64-bit atomicAdd.
#define GN_POP_FLUSH 240u // words between two flushes of the planes: a multiple of 16, at most 255

struct GnPopParams
{
    const uint64_t* rows;
    uint64_t        n_words; // S * Ws
    uint64_t        step;    // words from one of a lane's words to its next
    uint64_t        tile;    // steps a wave walks (a multiple of GN_POP_FLUSH)
    uint64_t        whole_steps; // steps, from the matrix's first, in which every lane with a column has a word
    uint64_t        n_tiles;
    uint32_t        Ws, W, B;
    uint32_t        lanes;   // lanes of a wave that own a column (flat), 64 (chunks)
    uint32_t        chunked; // 0: flat, 1: chunks of 64 word columns
    uint32_t        fold;    // flat, Ws a power of two below 64: lanes l and l + Ws own the same column
};

// a value that is the same in every lane, moved to where the compiler knows it
__device__ __forceinline__ uint64_t gn_uniform64(uint64_t v)
{
    return (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v) |
           (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(v >> 32)) << 32;
}

#define GN_CSA(hi, lo, a, b, c)                \
    {                                          \
        const uint64_t u_ = (a) ^ (b);         \
        const uint64_t c_ = (c);               \
        hi                = ((a) & (b)) | (u_ & c_); \
        lo                = u_ ^ c_;           \
    }

// 8 words into the planes ones / twos / fours; the carry of weight 8 is returned
__device__ __forceinline__ uint64_t gn_pop_eight(const uint64_t (&x)[8], uint64_t& ones, uint64_t& twos, uint64_t& fours)
{
    uint64_t ta, tb, fa, fb, e;
    GN_CSA(ta, ones, ones, x[0], x[1]);
    GN_CSA(tb, ones, ones, x[2], x[3]);
    GN_CSA(fa, twos, twos, ta, tb);
    GN_CSA(ta, ones, ones, x[4], x[5]);
    GN_CSA(tb, ones, ones, x[6], x[7]);
    GN_CSA(fb, twos, twos, ta, tb);
    GN_CSA(e, fours, fours, fa, fb);
    return e;
}

// planes -> counters: for bit positions s, s + 8, s + 16, s + 24 of one 32-bit half, the 8 plane bits are gathered into one byte each
__device__ __forceinline__ void gn_pop_flush(uint64_t (&p)[8], uint32_t (&cnt)[64])
{
#pragma unroll
    for (uint32_t half = 0; half < 2; ++half)
    {
        uint32_t q[8];
#pragma unroll
        for (uint32_t k = 0; k < 8; ++k)
            q[k] = (uint32_t)(p[k] >> (32u * half));
#pragma unroll
        for (uint32_t s = 0; s < 8; ++s)
        {
            uint32_t v = 0;
#pragma unroll
            for (uint32_t k = 0; k < 8; ++k)
                v |= (k >= s ? q[k] << (k - s) : q[k] >> (s - k)) & (0x01010101u << k);
#pragma unroll
            for (uint32_t i = 0; i < 4; ++i)
                cnt[half * 32u + i * 8u + s] += (v >> (8u * i)) & 0xFFu;
        }
    }
#pragma unroll
    for (uint32_t k = 0; k < 8; ++k)
        p[k] = 0;
}

__global__ __launch_bounds__(256) void gn_bin_popcount_kernel(const GnPopParams P, unsigned long long* __restrict__ counts)
{
    // (tile and chunk are the same in every lane: through readfirstlane, so that everything derived from them is scalar arithmetic)
    const uint64_t tile = (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4u + (threadIdx.x >> 6)));
    const uint32_t c0   = blockIdx.y * 64u; // (0 unless chunked)
    if (tile >= P.n_tiles) // (the waves that fill up the last block)
        return;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t col  = P.chunked ? c0 + lane : lane % P.Ws;
    const bool     mine = P.chunked ? col < P.W : lane < P.lanes;
    // A load is a wave-uniform base (scalar arithmetic) plus the lane's own 32-bit byte offset, which never changes.  A lane without a
    // column reads what the wave's first lane reads (inside the matrix wherever that lane is) and drops its counters.
    // (there is no scalar 64-bit multiply: the products are made once, handed to the scalar unit, and only added to from there on)
    const uint64_t step0 = gn_uniform64(tile * P.tile);            // the tile's first step ...
    const uint64_t first = gn_uniform64(step0 * P.step + c0);      // ... and the wave's first word: below n_words, since the tile exists
    const uint64_t whole = P.whole_steps > step0 ? min(P.whole_steps - step0, P.tile) : 0; // steps of the tile every lane has a word in
    const uint32_t loff  = mine ? lane : 0u;
    const uint32_t boff  = loff * 8u;
    typedef const __attribute__((address_space(1))) char GnGlobalConstByte;
    GnGlobalConstByte* src = (GnGlobalConstByte*)P.rows;

    uint32_t cnt[64];
#pragma unroll
    for (uint32_t b = 0; b < 64; ++b)
        cnt[b] = 0;
    uint64_t p[8];
#pragma unroll
    for (uint32_t k = 0; k < 8; ++k)
        p[k] = 0;

    // 16 words through the adder tree: 15 adders, and a half adder per plane above for the carry of weight 16
    auto add16 = [&](const uint64_t (&xa)[8], const uint64_t (&xb)[8]) {
        const uint64_t ea = gn_pop_eight(xa, p[0], p[1], p[2]);
        const uint64_t eb = gn_pop_eight(xb, p[0], p[1], p[2]);
        uint64_t       carry;
        GN_CSA(carry, p[3], p[3], ea, eb);
#pragma unroll
        for (uint32_t k = 4; k < 8; ++k)
        {
            const uint64_t t = p[k] & carry;
            p[k] ^= carry;
            carry = t;
        }
    };

    uint64_t at    = first; // the wave's word of the next step
    uint32_t since = 0;     // words in the planes
    for (uint64_t j = 0; j + 16u <= whole; j += 16u)
    {
        uint64_t xa[8], xb[8];
#pragma unroll
        for (uint32_t i = 0; i < 8; ++i, at += P.step)
            xa[i] = *(GnGlobalConstWord*)(src + at * 8u + boff);
#pragma unroll
        for (uint32_t i = 0; i < 8; ++i, at += P.step)
            xb[i] = *(GnGlobalConstWord*)(src + at * 8u + boff);
        add16(xa, xb);
        since += 16u;
        if (since == GN_POP_FLUSH)
        {
            gn_pop_flush(p, cnt);
            since = 0;
        }
    }
    // What is left of the tile is less than 16 steps: up to 15 whole ones and the matrix's last, which may end inside the wave.  A step
    // outside reads the wave's first word and counts as zero; lim = the lanes' offsets that are inside (the same in every lane).
    const uint64_t done = whole & ~15ull;
    if (done < P.tile && at < P.n_words)
    {
        uint64_t x[16];
#pragma unroll
        for (uint32_t i = 0; i < 16; ++i, at += P.step)
        {
            const uint32_t lim = (done + i < P.tile && at < P.n_words) ? (uint32_t)min((uint64_t)64u, P.n_words - at) : 0u;
            const uint64_t v   = *(GnGlobalConstWord*)(src + (lim ? at : first) * 8u + (loff < lim ? boff : 0u));
            x[i]               = loff < lim ? v : 0;
        }
        uint64_t xa[8], xb[8];
#pragma unroll
        for (uint32_t i = 0; i < 8; ++i)
        {
            xa[i] = x[i];
            xb[i] = x[8 + i];
        }
        add16(xa, xb);
        since += 16u;
    }
    if (since)
        gn_pop_flush(p, cnt);

    if (P.fold)
        for (uint32_t off = 32; off >= P.Ws; off >>= 1)
#pragma unroll
            for (uint32_t b = 0; b < 64; ++b)
                cnt[b] += (uint32_t)__shfl_xor((int)cnt[b], (int)off);
    if (!mine || col >= P.W || (P.fold && lane >= P.Ws))
        return;
#pragma unroll
    for (uint32_t b = 0; b < 64; ++b)
    {
        const uint32_t bin = col * 64u + b;
        uint32_t       c;
        // (a copy the compiler cannot see through: otherwise every counter lives in the lower half of a register PAIR from the start,
        // the upper half kept free for the zero of this 64-bit operand -- 64 registers and a wave per SIMD)
        asm volatile("v_mov_b32 %0, %1" : "=&v"(c) : "v"(cnt[b]));
        if (bin < P.B && c)
            atomicAdd(&counts[bin], (unsigned long long)c);
    }
}

// IBF `ibf_idx` of a filter (0 of a flat one), or nullptr
static const GnIbfHost* gn_build_ibf(const gn_filter* f, uint32_t ibf_idx)
{
    if (f->is_hibf)
        return ibf_idx < f->ibfs.size() ? &f->ibfs[ibf_idx] : nullptr;
    return ibf_idx == 0 ? &f->ibf : nullptr;
}

extern "C" int gn_filter_bin_popcounts(const gn_filter* f, uint32_t ibf_idx, uint64_t* counts)
{
    if (!f || !counts)
        return gn_fail(GN_EINVAL, "gn_filter_bin_popcounts: null argument");
    const GnIbfHost* ib = gn_build_ibf(f, ibf_idx);
    if (!ib || !ib->d_rows)
        return gn_fail(GN_EINVAL, "gn_filter_bin_popcounts: ibf %u of %zu", ibf_idx, f->is_hibf ? f->ibfs.size() : (size_t)1);
    GnPopParams P{};
    P.rows    = ib->d_rows.get();
    P.n_words = ib->S * ib->Ws;
    P.Ws      = (uint32_t)ib->Ws;
    P.W       = (uint32_t)ib->W;
    P.B       = (uint32_t)ib->B;
    P.chunked = ib->Ws > 64 ? 1u : 0u;
    uint64_t steps, chunks = 1;
    if (P.chunked)
    {
        P.step  = ib->Ws;
        P.lanes = 64;
        steps   = ib->S;
        chunks  = (ib->W + 63) / 64;
        P.whole_steps = ib->S;
    }
    else
    {
        const uint64_t g = 64 / ib->Ws; // whole rows a wave reads per step
        P.step           = g * ib->Ws;
        P.lanes          = (uint32_t)P.step;
        P.fold           = (ib->Ws < 64 && (ib->Ws & (ib->Ws - 1)) == 0) ? 1u : 0u;
        steps            = (ib->S + g - 1) / g;
        P.whole_steps    = ib->S / g;
    }
    // about 8192 waves over the device, and tiles of at least 960 steps: a wave's 64 * Ws atomics then follow 60 KiB of reads or more
    const uint64_t per_chunk = std::max<uint64_t>(1, 8192 / chunks);
    uint64_t       tile      = std::max<uint64_t>(4 * GN_POP_FLUSH, (steps + per_chunk - 1) / per_chunk);
    tile                     = (tile + GN_POP_FLUSH - 1) / GN_POP_FLUSH * GN_POP_FLUSH;
    P.tile                   = tile;
    P.n_tiles                = (steps + tile - 1) / tile;
    if ((P.n_tiles + 3) / 4 > 0x7FFFFFFFull || chunks > 65535 || tile > (1ull << 25)) // (a 32-bit counter takes a tile of up to 64 lanes)
        return gn_fail(GN_ERANGE, "gn_filter_bin_popcounts: %llu rows of %llu words in one call", (unsigned long long)ib->S, (unsigned long long)ib->Ws);
    GN_HIP(hipSetDevice(f->device));
    GnDev<unsigned long long> d_counts;
    GN_HIP(d_counts.alloc(ib->B));
    GN_HIP(hipMemsetAsync(d_counts, 0, ib->B * 8, nullptr));
    hipLaunchKernelGGL(gn_bin_popcount_kernel, dim3((uint32_t)((P.n_tiles + 3) / 4), (uint32_t)chunks), dim3(256), 0, nullptr, P, d_counts.get());
    GN_HIP(hipGetLastError());
    GN_HIP(hipMemcpy(counts, d_counts, ib->B * 8, hipMemcpyDeviceToHost)); // (the null stream: after the kernel)
    return GN_OK;
}

// ---- gn_filter_copy_ibf: an IBF into one with more bins ----------------------------------------------------------------------------
// Row by row, device to device: words [0, W_src) of a row are the source's, the words from there to the destination's stride are zero.
// A thread moves V words (V = 2: 16 bytes, when both strides are even); it finds its row and word once and then steps by the grid.
template <uint32_t V>
__global__ __launch_bounds__(256) void gn_copy_ibf_kernel(uint64_t* __restrict__ dst, const uint64_t* __restrict__ src, uint64_t S, uint32_t Ws_dst,
                                                          uint32_t Ws_src, uint32_t W_src, uint64_t step_rows, uint32_t step_units)
{
    const uint32_t units = Ws_dst / V; // of V words, in a destination row
    const uint64_t gid   = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint64_t       r     = gid / units;
    uint32_t       u     = (uint32_t)(gid % units);
    for (; r < S; r += step_rows)
    {
        const uint32_t w = u * V;
        if (V == 2)
        {
            ulonglong2 v = make_ulonglong2(0, 0);
            if (w < W_src) // (w + 1 is below the source's even stride; the source's words beyond W_src are not trusted to be zero)
            {
                v = *reinterpret_cast<const ulonglong2*>(src + r * Ws_src + w);
                if (w + 1 >= W_src)
                    v.y = 0;
            }
            *reinterpret_cast<ulonglong2*>(dst + r * Ws_dst + w) = v;
        }
        else
            dst[r * Ws_dst + w] = w < W_src ? src[r * Ws_src + w] : 0;
        u += step_units;
        if (u >= units)
        {
            u -= units;
            ++r;
        }
    }
}

extern "C" int gn_filter_copy_ibf(gn_filter* dst, uint32_t dst_ibf, const gn_filter* src, uint32_t src_ibf)
{
    if (!dst || !src)
        return gn_fail(GN_EINVAL, "gn_filter_copy_ibf: null argument");
    if (!dst->is_hibf || !src->is_hibf)
        return gn_fail(GN_EINVAL, "gn_filter_copy_ibf needs two HIBF filters");
    if (dst->device != src->device)
        return gn_fail(GN_EINVAL, "gn_filter_copy_ibf: the filters are on devices %d and %d", dst->device, src->device);
    if (dst_ibf >= dst->ibfs.size() || src_ibf >= src->ibfs.size())
        return gn_fail(GN_EINVAL, "gn_filter_copy_ibf: ibf %u of %zu into ibf %u of %zu", src_ibf, src->ibfs.size(), dst_ibf, dst->ibfs.size());
    GnIbfHost&       d = dst->ibfs[dst_ibf];
    const GnIbfHost& s = src->ibfs[src_ibf];
    if (d.d_rows.get() == s.d_rows.get())
        return gn_fail(GN_EINVAL, "gn_filter_copy_ibf: an IBF onto itself");
    if (d.S != s.S || d.h != s.h)
        return gn_fail(GN_EINVAL, "gn_filter_copy_ibf: %llu rows and %u hash functions into %llu rows and %u", (unsigned long long)s.S, s.h,
                       (unsigned long long)d.S, d.h);
    if (d.W < s.W)
        return gn_fail(GN_EINVAL, "gn_filter_copy_ibf: rows of %llu words into rows of %llu", (unsigned long long)s.W, (unsigned long long)d.W);
    GN_HIP(hipSetDevice(dst->device));
    const bool     wide    = (d.Ws % 2 == 0) && (s.Ws % 2 == 0);
    const uint64_t units   = d.Ws / (wide ? 2 : 1);
    const uint64_t total   = d.S * units;
    const uint64_t blocks  = std::min<uint64_t>((total + 255) / 256, (uint64_t)dst->n_cu * 16);
    const uint64_t threads = blocks * 256;
    if (wide)
        hipLaunchKernelGGL(gn_copy_ibf_kernel<2>, dim3((uint32_t)blocks), dim3(256), 0, nullptr, d.d_rows.get(), s.d_rows.get(), d.S, (uint32_t)d.Ws,
                           (uint32_t)s.Ws, (uint32_t)s.W, threads / units, (uint32_t)(threads % units));
    else
        hipLaunchKernelGGL(gn_copy_ibf_kernel<1>, dim3((uint32_t)blocks), dim3(256), 0, nullptr, d.d_rows.get(), s.d_rows.get(), d.S, (uint32_t)d.Ws,
                           (uint32_t)s.Ws, (uint32_t)s.W, threads / units, (uint32_t)(threads % units));
    GN_HIP(hipGetLastError());
    GN_HIP(hipDeviceSynchronize());
    return GN_OK;
}

// ---- gn_filter_copy_ibf_spans: an IBF into another one, with bins left out -------------------------------------------------------------
// The copy above with the columns compacted on the way (`ganon-build --hibf --update --remove`): the spans are turned into a table of
// segments per destination word on the host (gn_bin_spans.h, where the arithmetic and its traps are described) and uploaded once.
// A thread owns V destination words of a row (V = 2: one 16-byte store, when the destination's stride is even) and keeps them for every
// row it walks, so that the segments of its words are read once: the first two of a word live in registers -- a word below a removed
// run has two, most words have one -- and only a word with more reads the rest from the table per row (L2-resident: the table is a few
// bytes per destination word).  The loads of a row are issued together, without a branch between the two words of a window.  A word is composed from all of its segments and stored once: no read-modify-write, no atomics, one
// writer per word whatever spans end in it.  Neighbouring lanes own neighbouring words:
//   rows of at least 256 units   blockIdx.x picks 256 units of the row, blockIdx.y the first row; the rows step by gridDim.y
//   narrower rows                a block covers 256 / units whole rows, which lie one behind the other: the flat array the popcount
//                                kernel reads; 256 % units threads idle (none for the power-of-two strides up to 16 words)
// A window is at most two neighbouring source words; its second word is on the line the first one fetched or on the next, so the source is
// read from HBM once, as by the plain copy.  Two destination words that are two whole neighbouring aligned source words -- every pair of
// an identity span -- are one 16-byte load.
struct GnSpanCopyParams
{
    uint64_t*        dst;
    const uint64_t*  src;
    const uint32_t*  seg_off;
    const GnSpanSeg* segs;
    uint64_t         S;
    uint32_t         Ws_dst, Ws_src;
    uint32_t         units; // of V words, in a destination row
    uint32_t         rpb;   // whole rows a block covers; 0: wide rows
};

template <uint32_t V>
__global__ __launch_bounds__(256) void gn_copy_ibf_spans_kernel(const GnSpanCopyParams P)
{
    uint32_t u;
    uint64_t r, step;
    if (P.rpb)
    {
        const uint32_t rr = threadIdx.x / P.units;
        if (rr >= P.rpb)
            return;
        u    = threadIdx.x % P.units;
        r    = (uint64_t)blockIdx.y * P.rpb + rr;
        step = (uint64_t)gridDim.y * P.rpb;
    }
    else
    {
        u = blockIdx.x * 256u + threadIdx.x;
        if (u >= P.units)
            return;
        r    = blockIdx.y;
        step = gridDim.y;
    }
    const uint32_t w0 = u * V; // (w0 + V <= Ws_dst: units = Ws_dst / V, exactly)
    uint32_t       first[V], n[V];
    GnSpanSeg      a[V], b[V];
#pragma unroll
    for (uint32_t v = 0; v < V; ++v)
    {
        first[v] = P.seg_off[w0 + v];
        n[v]     = P.seg_off[w0 + v + 1] - first[v];
        a[v] = b[v] = GnSpanSeg{ 0, 0, 0, 0, 0 };
        if (n[v] >= 1)
            a[v] = P.segs[first[v]];
        if (n[v] >= 2)
            b[v] = P.segs[first[v] + 1];
    }
    bool pair = false; // two whole source words, 16 bytes aligned in a source of even stride
    if (V == 2)
        pair = n[0] == 1 && n[V - 1] == 1 && gn_span_is_move(a[0]) && gn_span_is_move(a[V - 1]) && a[V - 1].src_word == a[0].src_word + 1u &&
               (a[0].src_word & 1u) == 0 && (P.Ws_src & 1u) == 0;
    for (; r < P.S; r += step)
    {
        const uint64_t* row = P.src + r * P.Ws_src; // (64-bit: row * stride passes 2^32 words in a large IBF)
        uint64_t        out[V];
        if (V == 2 && pair)
        {
            const ulonglong2 x = *reinterpret_cast<const ulonglong2*>(row + a[0].src_word);
            out[0] = x.x, out[V - 1] = x.y;
        }
        else
        {
            // every load of the row first, then the arithmetic: a word without a segment has a segment of 0 bits of word 0
            uint64_t alo[V], ahi[V], blo[V], bhi[V];
#pragma unroll
            for (uint32_t v = 0; v < V; ++v)
            {
                alo[v] = row[a[v].src_word];
                ahi[v] = row[a[v].src_word + gn_span_second(a[v])];
            }
#pragma unroll
            for (uint32_t v = 0; v < V; ++v)
            {
                blo[v] = bhi[v] = 0;
                if (n[v] >= 2)
                {
                    blo[v] = row[b[v].src_word];
                    bhi[v] = row[b[v].src_word + gn_span_second(b[v])];
                }
            }
#pragma unroll
            for (uint32_t v = 0; v < V; ++v)
            {
                uint64_t x = gn_span_bits(alo[v], ahi[v], a[v]) << a[v].dst_off | gn_span_bits(blo[v], bhi[v], b[v]) << b[v].dst_off;
                if (n[v] > 2)
                    x |= gn_span_compose(row, P.segs + first[v] + 2, n[v] - 2);
                out[v] = x;
            }
        }
        if (V == 2)
            *reinterpret_cast<ulonglong2*>(P.dst + r * P.Ws_dst + w0) = make_ulonglong2(out[0], out[V - 1]);
        else
            P.dst[r * P.Ws_dst + w0] = out[0];
    }
}

extern "C" int gn_filter_copy_ibf_spans(gn_filter* dst, uint32_t dst_ibf, const gn_filter* src, uint32_t src_ibf, const gn_bin_span* spans,
                                        uint32_t n_spans)
{
    if (!dst || !src || (n_spans && !spans))
        return gn_fail(GN_EINVAL, "gn_filter_copy_ibf_spans: null argument");
    if (!dst->is_hibf || !src->is_hibf)
        return gn_fail(GN_EINVAL, "gn_filter_copy_ibf_spans needs two HIBF filters");
    if (dst->device != src->device)
        return gn_fail(GN_EINVAL, "gn_filter_copy_ibf_spans: the filters are on devices %d and %d", dst->device, src->device);
    if (dst_ibf >= dst->ibfs.size() || src_ibf >= src->ibfs.size())
        return gn_fail(GN_EINVAL, "gn_filter_copy_ibf_spans: ibf %u of %zu into ibf %u of %zu", src_ibf, src->ibfs.size(), dst_ibf, dst->ibfs.size());
    GnIbfHost&       d = dst->ibfs[dst_ibf];
    const GnIbfHost& s = src->ibfs[src_ibf];
    if (!d.d_rows || !s.d_rows || d.d_rows.get() == s.d_rows.get())
        return gn_fail(GN_EINVAL, "gn_filter_copy_ibf_spans: an IBF onto itself");
    if (d.S != s.S || d.h != s.h)
        return gn_fail(GN_EINVAL, "gn_filter_copy_ibf_spans: %llu rows and %u hash functions into %llu rows and %u", (unsigned long long)s.S, s.h,
                       (unsigned long long)d.S, d.h);
    uint32_t    at  = 0;
    const char* why = gn_spans_check(spans, n_spans, s.B, d.B, &at);
    if (why)
        return gn_fail(GN_EINVAL, "gn_filter_copy_ibf_spans: span %u {source %u, destination %u, %u bins} of %u: %s (source %llu bins, destination %llu)", at,
                       spans[at].src_first, spans[at].dst_first, spans[at].n_bins, n_spans, why, (unsigned long long)s.B, (unsigned long long)d.B);
    if (d.Ws * 64 < d.B || s.W * 64 < s.B || s.Ws < s.W || d.Ws > 0xFFFFFFFFull || s.Ws > 0xFFFFFFFFull)
        return gn_fail(GN_EINVAL, "gn_filter_copy_ibf_spans: rows of %llu and %llu words for %llu and %llu bins", (unsigned long long)s.Ws, (unsigned long long)d.Ws,
                       (unsigned long long)s.B, (unsigned long long)d.B);
    if (d.S == 0)
        return GN_OK;
    std::vector<uint32_t>  seg_off;
    std::vector<GnSpanSeg> segs;
    gn_spans_table(spans, n_spans, d.Ws, seg_off, segs);
    GN_HIP(hipSetDevice(dst->device));
    GnDev<uint32_t>  d_off;
    GnDev<GnSpanSeg> d_segs;
    GN_HIP(d_off.upload(seg_off.data(), seg_off.size()));
    GN_HIP(d_segs.upload(segs.data(), segs.size()));
    GnSpanCopyParams P{};
    P.dst = d.d_rows.get(), P.src = s.d_rows.get(), P.seg_off = d_off.get(), P.segs = d_segs.get();
    P.S = d.S, P.Ws_dst = (uint32_t)d.Ws, P.Ws_src = (uint32_t)s.Ws;
    const bool two = d.Ws % 2 == 0;
    P.units        = (uint32_t)(d.Ws / (two ? 2 : 1));
    P.rpb          = P.units < 256 ? 256 / P.units : 0;
    const uint64_t budget = (uint64_t)std::max(dst->n_cu, 1) * 16; // blocks, as the plain copy launches
    uint64_t       gx = 1, gy;
    if (P.rpb)
        gy = std::min<uint64_t>((d.S + P.rpb - 1) / P.rpb, budget);
    else
    {
        gx = ((uint64_t)P.units + 255) / 256;
        gy = std::min<uint64_t>(d.S, std::max<uint64_t>(1, budget / gx));
    }
    gy = std::min<uint64_t>(gy, 65535);
    if (two)
        hipLaunchKernelGGL(gn_copy_ibf_spans_kernel<2>, dim3((uint32_t)gx, (uint32_t)gy), dim3(256), 0, nullptr, P);
    else
        hipLaunchKernelGGL(gn_copy_ibf_spans_kernel<1>, dim3((uint32_t)gx, (uint32_t)gy), dim3(256), 0, nullptr, P);
    GN_HIP(hipGetLastError());
    GN_HIP(hipDeviceSynchronize()); // (the table is freed behind it)
    return GN_OK;
}

// ---- gn_filter_fold_ibf: groups of bins of an IBF ORed into one bin each of another one ---------------------------------------------------
// The merged bin above a group of bins (`ganon-build --hibf --update --fold`): the members are turned into a table of segments per SOURCE
// word on the host (gn_fold_table.h, where the arithmetic and its traps are described) and uploaded once.  A block owns whole rows:
//   rows of at most 256 words   256 / stride rows lie one behind the other in the block's threads -- the flat array the popcount and the
//                               span-copy kernels read -- and a thread keeps its word of the row, and so its segments' place in the table,
//                               for every row it walks; GN_FOLD_K such row sets a step, their loads issued together
//   wider rows                  one row a step, in chunks of GN_FOLD_K * 256 words along the row, all chunks by the same block
// Every source word below W_src is read once, by neighbouring lanes; a word without a segment's bit set costs nothing more.  A segment
// that hits ORs its group's bit into the row's hits in LDS (an LDS OR without a return).  After ONE barrier a step the destination words
// the groups reach -- ceil(n_groups / 64) + 1 a row at most -- are composed from the hits and written by one thread each as load-OR-store,
// a word whose groups all missed not at all.  The hits are three buffers taken in turn, so that the step's second half also clears the
// buffer of the step after next: what it clears was last read before this step's barrier and is next written behind the next step's.
// No global atomic, no scratch.
struct GnFoldParams
{
    uint64_t*        dst;
    const uint64_t*  src;
    const uint32_t*  seg_off;
    const GnFoldSeg* segs;
    uint64_t         S;
    uint32_t         Ws_dst, Ws_src, W_src;
    uint32_t         rpb;       // whole source rows 256 threads cover; 0: rows of more than 256 words
    uint32_t         hw;        // hit words a row
    uint32_t         dw0, ndw;  // the destination words the groups reach: the first, and how many
    uint32_t         dst_first;
};

constexpr uint32_t GN_FOLD_K = 4;

__global__ __launch_bounds__(256) void gn_fold_ibf_kernel(const GnFoldParams P)
{
    extern __shared__ uint32_t gn_fold_hits[]; // 3 buffers of (rows a step) * hw words
    const uint32_t tid       = threadIdx.x;
    const uint32_t rows_step = P.rpb ? P.rpb * GN_FOLD_K : 1u;
    const uint32_t buf_words = rows_step * P.hw;
    for (uint32_t i = tid; i < 2u * buf_words; i += 256u)
        gn_fold_hits[i] = 0;
    __syncthreads();
    uint32_t rr = 0, u = tid, first = 0, n = 0; // rows of at most 256 words: the thread's row of the set, its word, its segments
    if (P.rpb)
    {
        rr = tid / P.Ws_src, u = tid % P.Ws_src;
        if (rr < P.rpb && u < P.W_src) // (the words from W_src to the stride are not trusted, and have no segment)
        {
            first = P.seg_off[u];
            n     = P.seg_off[u + 1] - first;
        }
    }
    uint32_t cur = 0;
    for (uint64_t r0 = (uint64_t)blockIdx.x * rows_step; r0 < P.S; r0 += (uint64_t)gridDim.x * rows_step) // (the same trips in every thread)
    {
        uint32_t* hits = gn_fold_hits + cur * buf_words;
        if (P.rpb)
        {
            if (n)
            {
                uint64_t x[GN_FOLD_K];
#pragma unroll
                for (uint32_t k = 0; k < GN_FOLD_K; ++k)
                {
                    const uint64_t row = r0 + k * P.rpb + rr; // (64-bit: row * stride passes 2^32 words in a large IBF)
                    x[k]               = row < P.S ? P.src[row * P.Ws_src + u] : 0ull;
                }
                for (uint32_t s = 0; s < n; ++s)
                {
                    const GnFoldSeg seg = P.segs[first + s];
#pragma unroll
                    for (uint32_t k = 0; k < GN_FOLD_K; ++k)
                        if (x[k] & seg.mask)
                            atomicOr(&hits[(k * P.rpb + rr) * P.hw + (seg.group >> 5)], 1u << (seg.group & 31u));
                }
            }
        }
        else
        {
            const uint64_t* row = P.src + r0 * P.Ws_src;
            for (uint32_t c = 0; c < P.W_src; c += GN_FOLD_K * 256u)
            {
                uint64_t x[GN_FOLD_K];
#pragma unroll
                for (uint32_t k = 0; k < GN_FOLD_K; ++k)
                {
                    const uint32_t w = c + k * 256u + tid;
                    x[k]             = w < P.W_src ? row[w] : 0ull;
                }
#pragma unroll
                for (uint32_t k = 0; k < GN_FOLD_K; ++k)
                {
                    if (!x[k])
                        continue;
                    const uint32_t w = c + k * 256u + tid;
                    for (uint32_t s = P.seg_off[w], end = P.seg_off[w + 1]; s < end; ++s)
                    {
                        const GnFoldSeg seg = P.segs[s];
                        if (x[k] & seg.mask)
                            atomicOr(&hits[seg.group >> 5], 1u << (seg.group & 31u));
                    }
                }
            }
        }
        __syncthreads();
        uint32_t* clear = gn_fold_hits + (cur + 2u) % 3u * buf_words;
        for (uint32_t i = tid; i < buf_words; i += 256u)
            clear[i] = 0;
        for (uint32_t i = tid; i < rows_step * P.ndw; i += 256u)
        {
            const uint32_t slot = i / P.ndw, k = i % P.ndw;
            const uint64_t row  = r0 + slot;
            if (row >= P.S)
                continue;
            const uint64_t v = gn_fold_word(hits + slot * P.hw, P.hw, P.dw0 + k, P.dst_first);
            if (v)
            {
                uint64_t* at = P.dst + row * P.Ws_dst + P.dw0 + k;
                *at |= v;
            }
        }
        cur = (cur + 1u) % 3u;
    }
}

extern "C" int gn_filter_fold_ibf(gn_filter* dst, uint32_t dst_ibf, uint32_t dst_first, uint32_t n_groups, const gn_filter* src, uint32_t src_ibf,
                                  const gn_fold_member* members, uint32_t n_members)
{
    if (!dst || !src || (n_members && !members))
        return gn_fail(GN_EINVAL, "gn_filter_fold_ibf: null argument");
    if (!dst->is_hibf || !src->is_hibf)
        return gn_fail(GN_EINVAL, "gn_filter_fold_ibf needs two HIBF filters");
    if (dst->device != src->device)
        return gn_fail(GN_EINVAL, "gn_filter_fold_ibf: the filters are on devices %d and %d", dst->device, src->device);
    if (dst_ibf >= dst->ibfs.size() || src_ibf >= src->ibfs.size())
        return gn_fail(GN_EINVAL, "gn_filter_fold_ibf: ibf %u of %zu into ibf %u of %zu", src_ibf, src->ibfs.size(), dst_ibf, dst->ibfs.size());
    GnIbfHost&       d = dst->ibfs[dst_ibf];
    const GnIbfHost& s = src->ibfs[src_ibf];
    if (!d.d_rows || !s.d_rows || d.d_rows.get() == s.d_rows.get())
        return gn_fail(GN_EINVAL, "gn_filter_fold_ibf: an IBF onto itself");
    if (d.S != s.S || d.h != s.h)
        return gn_fail(GN_EINVAL, "gn_filter_fold_ibf: %llu rows and %u hash functions into %llu rows and %u", (unsigned long long)s.S, s.h,
                       (unsigned long long)d.S, d.h);
    uint32_t    at  = 0;
    const char* why = gn_fold_check(members, n_members, n_groups, dst_first, s.B, d.B, &at);
    if (why && at < n_members)
        return gn_fail(GN_EINVAL, "gn_filter_fold_ibf: member %u {source %u, %u bins, group %u} of %u: %s (source %llu bins, %u groups)", at, members[at].src_first,
                       members[at].n_bins, members[at].group, n_members, why, (unsigned long long)s.B, n_groups);
    if (why)
        return gn_fail(GN_EINVAL, "gn_filter_fold_ibf: %u groups from bin %u on, %u members: %s (destination %llu bins)", n_groups, dst_first, n_members, why,
                       (unsigned long long)d.B);
    if (d.Ws * 64 < d.B || s.W * 64 < s.B || s.Ws < s.W || d.Ws > 0xFFFFFFFFull || s.Ws > 0xFFFFFFFFull)
        return gn_fail(GN_EINVAL, "gn_filter_fold_ibf: rows of %llu and %llu words for %llu and %llu bins", (unsigned long long)s.Ws, (unsigned long long)d.Ws,
                       (unsigned long long)s.B, (unsigned long long)d.B);
    if (n_groups == 0 || d.S == 0)
        return GN_OK;
    GnFoldParams P{};
    P.dst = d.d_rows.get(), P.src = s.d_rows.get();
    P.S = d.S, P.Ws_dst = (uint32_t)d.Ws, P.Ws_src = (uint32_t)s.Ws, P.W_src = (uint32_t)s.W;
    P.rpb = s.Ws <= 256 ? (uint32_t)(256 / s.Ws) : 0u;
    P.hw  = gn_fold_hit_words(n_groups);
    P.dw0 = dst_first >> 6, P.ndw = ((dst_first + n_groups - 1) >> 6) - P.dw0 + 1, P.dst_first = dst_first;
    const uint64_t rows_step = P.rpb ? (uint64_t)P.rpb * GN_FOLD_K : 1;
    const uint64_t lds       = 3 * rows_step * P.hw * sizeof(uint32_t);
    if (lds > 65536)
        return gn_fail(GN_ERANGE, "gn_filter_fold_ibf: %u groups in one call (%llu bytes of LDS, at most 65536)", n_groups, (unsigned long long)lds);
    std::vector<uint32_t>  seg_off;
    std::vector<GnFoldSeg> segs;
    gn_fold_table(members, n_members, s.W, seg_off, segs);
    GN_HIP(hipSetDevice(dst->device));
    GnDev<uint32_t>  d_off;
    GnDev<GnFoldSeg> d_segs;
    GN_HIP(d_off.upload(seg_off.data(), seg_off.size()));
    GN_HIP(d_segs.upload(segs.data(), segs.size()));
    P.seg_off = d_off.get(), P.segs = d_segs.get();
    const uint64_t blocks = std::min<uint64_t>((d.S + rows_step - 1) / rows_step, (uint64_t)std::max(dst->n_cu, 1) * 8);
    hipLaunchKernelGGL(gn_fold_ibf_kernel, dim3((uint32_t)blocks), dim3(256), (uint32_t)lds, nullptr, P);
    GN_HIP(hipGetLastError());
    GN_HIP(hipDeviceSynchronize()); // (the table is freed behind it)
    return GN_OK;
}
