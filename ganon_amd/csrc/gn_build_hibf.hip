// gn_build_hibf.hip -- the device work of `ganon-build --hibf` behind the C ABI:
//   gn_hashes_union          the ascending union of several ascending hash sets and its size -- the cardinality of a merged bin
//                            (raptor estimates it from HyperLogLog sketches; here it is exact: concatenate, radix sort, unique,
//                            as gn_stream_distinct_hashes does for a file)
//   gn_filter_emplace_path   one launch inserts a batch of user bins along their whole root-to-leaf paths: a hash is read once
//                            and ORed into h rows of EVERY IBF on its path (the user bin's own run of bins in its leaf IBF, one
//                            merged bin in each IBF above).  Inserting every member's set into a merged bin sets the bits the
//                            union of the sets would: the unions are never materialised.
// No counterpart in the reference's own sources: `ganon build --filter-type hibf` runs `raptor build`
// (/root/reference/src/ganon/build_update.py:411-518).  HBM-bound integer work: depth * h atomic ORs per hash, each to a row
// of its own.
#include "gn_build_row.h"
#include <hipcub/hipcub.hpp>
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

extern "C" int gn_filter_emplace_path(gn_filter* f, const uint64_t* hashes, const uint64_t* set_off, uint32_t n_sets, const gn_path_entry* paths,
                                      uint32_t depth)
{
    if (!f || !f->is_hibf)
        return gn_fail(GN_EINVAL, "gn_filter_emplace_path needs an HIBF filter");
    if (n_sets == 0)
        return GN_OK;
    if (!set_off || !paths || depth == 0)
        return gn_fail(GN_EINVAL, "gn_filter_emplace_path: null argument");
    const uint64_t total = set_off[n_sets];
    if (total && !hashes)
        return gn_fail(GN_EINVAL, "gn_filter_emplace_path: null argument");
    // every bin a hash can reach is checked here; the row is below S by construction (gn_build_row)
    std::vector<GnPathDev> dev((size_t)n_sets * depth);
    for (uint32_t s = 0; s < n_sets; ++s)
    {
        if (set_off[s + 1] < set_off[s])
            return gn_fail(GN_EINVAL, "gn_filter_emplace_path: set offsets descend at set %u", s);
        const uint64_t n    = set_off[s + 1] - set_off[s];
        bool           open = true;
        for (uint32_t d = 0; d < depth; ++d)
        {
            const gn_path_entry& e = paths[(size_t)s * depth + d];
            GnPathDev&           o = dev[(size_t)s * depth + d];
            o                      = GnPathDev{ nullptr, 1, 1, 1, 0, 0, 0 };
            if (e.n_bins == 0 || !open)
            {
                open = false;
                continue;
            }
            if (e.ibf >= f->ibfs.size())
                return gn_fail(GN_EINVAL, "gn_filter_emplace_path: set %u level %u: ibf %u of %zu", s, d, e.ibf, f->ibfs.size());
            const GnIbfHost& ib = f->ibfs[e.ibf];
            if ((uint64_t)e.first_bin + e.n_bins > ib.B)
                return gn_fail(GN_EINVAL, "gn_filter_emplace_path: set %u level %u: bins %u..%llu of an IBF with %llu", s, d, e.first_bin,
                               (unsigned long long)e.first_bin + e.n_bins - 1, (unsigned long long)ib.B);
            if (e.n_bins > 1 && (e.hashes_per_bin == 0 || (n && (n - 1) / e.hashes_per_bin >= e.n_bins)))
                return gn_fail(GN_EINVAL, "gn_filter_emplace_path: set %u level %u: %llu hashes at %llu a bin do not fit %u bins", s, d,
                               (unsigned long long)n, (unsigned long long)e.hashes_per_bin, e.n_bins);
            o = GnPathDev{ ib.d_rows, ib.S, e.n_bins > 1 ? e.hashes_per_bin : 1, (uint32_t)ib.Ws, ib.shift, e.first_bin, e.n_bins };
        }
    }
    if (total == 0)
        return GN_OK;
    GN_HIP(hipSetDevice(f->device));
    if (!f->load_st)
        GN_HIP(hipStreamCreateWithFlags(&f->load_st, hipStreamNonBlocking));
    // staged through the device buffer that stays with the filter, at most 32 M hashes at a time (as gn_filter_emplace_split)
    const uint64_t step = total < (32ull << 20) ? total : (32ull << 20);
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
        const uint32_t n_items = (uint32_t)items.size();
        hipLaunchKernelGGL(gn_emplace_path_kernel, dim3((n_items + 3) / 4), dim3(256), 0, f->load_st, f->d_emplace_stage, d_items, n_items,
                           d_paths, depth, f->ibfs[0].h);
        GN_HIP(hipGetLastError());
        GN_HIP(hipStreamSynchronize(f->load_st)); // (the staging buffer and `items` are reused, and `hashes` may be pageable)
    }
    return GN_OK;
}
