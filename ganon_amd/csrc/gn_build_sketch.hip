// gn_build_sketch.hip -- HyperLogLog sketches of the user bins of `ganon-build --hibf --layout sketch` behind the C ABI:
//   gn_sketches_create       one sketch of m = 4096 one-byte registers per ascending hash set, resident on the device
//   gn_sketches_union_table  for every start j and every length l <= width the estimated cardinality of the union of the sketches
//                            order[j .. j + l) -- the question a layout search asks n * width times
//   gn_sketches_pair_table   for every two sketches of a list the estimated cardinality of their union -- what `--layout similarity`
//                            orders the user bins of an interval by
// The definitions (mixer, register index, rank, estimate) are stated bit for bit in include/ganon_hip.h.
// No counterpart in the reference's own sources: `ganon build --filter-type hibf` runs `raptor layout`, which is chopper
// (/root/reference/src/ganon/build_update.py:411-518).  Integer work but for one division per table entry.
#include "gn_internal.h"

#include <math.h>
#include <string.h>

#include <algorithm>
#include <vector>

#define GN_SKETCH_CHUNK 8192u // hashes of one set a block folds into its LDS sketch

struct gn_sketches
{
    int             device = 0;
    uint32_t        n      = 0;
    GnDev<uint8_t>  d_regs;  // n * GN_SKETCH_M
    GnDev<double>   d_small; // small[z] = m * ln(m / z), z = 1 .. m; small[0] unused
    double          num = 0; // alpha * m^2 * 2^52
};

// A block's piece of work: `cnt` hashes of set `seg` from word `stage_at` of the staging buffer.  slot == ~0: the item is the whole
// set, the block writes its registers; else the set has more items (in this round or another) and the block maximises into the
// scratch words of `slot`, which gn_sketch_pack_kernel folds into the set's registers.
struct GnSketchItem
{
    uint32_t seg, cnt, slot, pad;
    uint64_t stage_at;
};

__device__ __forceinline__ uint64_t gn_sketch_mix(uint64_t h) // murmur3's 64-bit finaliser
{
    h ^= h >> 33;
    h *= 0xff51afd7ed558ccdULL;
    h ^= h >> 33;
    h *= 0xc4ceb9fe1a85ec53ULL;
    h ^= h >> 33;
    return h;
}

// One block per item: the item's hashes go into a sketch of 4096 words in LDS (LDS atomic max), which leaves the block either as
// the set's 4 KiB of registers (coalesced dword stores) or through global atomic max on the slot's scratch words.
__global__ __launch_bounds__(256) void gn_sketch_fill_kernel(const uint64_t* __restrict__ stage, const GnSketchItem* __restrict__ items,
                                                             uint32_t* __restrict__ scratch, uint8_t* __restrict__ regs)
{
    __shared__ __attribute__((aligned(16))) uint32_t sk[GN_SKETCH_M];
    const GnSketchItem  it = items[blockIdx.x];
    for (uint32_t r = threadIdx.x; r < GN_SKETCH_M; r += 256)
        sk[r] = 0;
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < it.cnt; i += 256)
    {
        const uint64_t x    = gn_sketch_mix(stage[it.stage_at + i]);
        const uint64_t rest = x & ((1ULL << 52) - 1);
        const uint32_t rank = rest ? (uint32_t)__clzll((long long)rest) - 11u : 52u; // leading zeros of the 52 bits, plus one
        atomicMax(&sk[(uint32_t)(x >> 52)], rank);
    }
    __syncthreads();
    if (it.slot == ~0u)
    {
        uint32_t* out = (uint32_t*)(regs + (uint64_t)it.seg * GN_SKETCH_M);
        for (uint32_t w = threadIdx.x; w < GN_SKETCH_M / 4; w += 256)
        {
            const uint4 v = ((const uint4*)sk)[w];
            out[w]        = v.x | (v.y << 8) | (v.z << 16) | (v.w << 24);
        }
    }
    else
    {
        uint32_t* out = scratch + (uint64_t)it.slot * GN_SKETCH_M;
        for (uint32_t r = threadIdx.x; r < GN_SKETCH_M; r += 256)
            if (sk[r])
                atomicMax(out + r, sk[r]);
    }
}

// bytes of a and b are at most 127: the byte-wise maximum
__device__ __forceinline__ uint32_t gn_bytemax(uint32_t a, uint32_t b)
{
    const uint32_t ge = (((a | 0x80808080u) - b) >> 7) & 0x01010101u; // 1 in every byte with a >= b (no borrow leaves a byte)
    const uint32_t m  = (ge << 8) - ge;                                // ... 0xFF
    return (a & m) | (b & ~m);
}

// a thread per four registers of a slot: registers = max(registers, scratch words).  One writer per dword.
__global__ __launch_bounds__(256) void gn_sketch_pack_kernel(const uint32_t* __restrict__ scratch, const uint32_t* __restrict__ slot_seg,
                                                             uint32_t n_slots, uint8_t* __restrict__ regs)
{
    const uint32_t t = blockIdx.x * 256 + threadIdx.x, slot = t / (GN_SKETCH_M / 4), w = t % (GN_SKETCH_M / 4);
    if (slot >= n_slots)
        return;
    const uint4 v   = ((const uint4*)(scratch + (uint64_t)slot * GN_SKETCH_M))[w];
    uint32_t*   out = (uint32_t*)(regs + (uint64_t)slot_seg[slot] * GN_SKETCH_M) + w;
    *out            = gn_bytemax(*out, v.x | (v.y << 8) | (v.z << 16) | (v.w << 24));
}

// E of include/ganon_hip.h from the sums over a union's registers
__device__ __forceinline__ unsigned long long gn_sketch_estimate(unsigned long long S, uint32_t Z, double num, const double* __restrict__ small)
{
    if (Z == GN_SKETCH_M) // (S is 2^64, the estimate 0)
        return 0;
    const double raw = __ddiv_rn(num, __ull2double_rn(S));
    return __double2ull_rn(raw <= 2.5 * GN_SKETCH_M && Z > 0 ? small[Z] : raw);
}

// One wave per start j.  The running union -- 4 KiB, 16 dwords a lane -- stays in registers; a step loads the next sketch with
// four coalesced 16-byte loads a lane (issued a step ahead), takes the byte-wise maximum, sums S = sum 2^(52 - reg) and Z = zero
// registers over the lane's 64 bytes as integers and reduces both across the wave; lane 0 turns (S, Z) into the estimate.
__global__ __launch_bounds__(256) void gn_sketch_union_kernel(const uint8_t* __restrict__ regs, const uint32_t* __restrict__ order, uint32_t n,
                                                              uint32_t j0, uint32_t j1, uint32_t width, double num,
                                                              const double* __restrict__ small, unsigned long long* __restrict__ out)
{
    const uint32_t j = j0 + (uint32_t)__builtin_amdgcn_readfirstlane((int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6));
    if (j >= j1)
        return;
    const uint32_t      lane  = threadIdx.x & 63u;
    const uint32_t      steps = width < n - j ? width : n - j;
    unsigned long long* row   = out + (uint64_t)(j - j0) * width;
    uint4               u[4], nx[4];
#pragma unroll
    for (uint32_t i = 0; i < 4; ++i)
    {
        u[i]  = make_uint4(0, 0, 0, 0);
        nx[i] = ((const uint4*)(regs + (uint64_t)order[j] * GN_SKETCH_M))[i * 64 + lane];
    }
    unsigned long long best = 0;
    for (uint32_t l = 1; l <= steps; ++l)
    {
        uint4 cur[4];
#pragma unroll
        for (uint32_t i = 0; i < 4; ++i)
            cur[i] = nx[i];
        if (l < steps)
        {
            const uint4* p = (const uint4*)(regs + (uint64_t)order[j + l] * GN_SKETCH_M);
#pragma unroll
            for (uint32_t i = 0; i < 4; ++i)
                nx[i] = p[i * 64 + lane];
        }
        unsigned long long S = 0;
        uint32_t           Z = 0;
#pragma unroll
        for (uint32_t i = 0; i < 4; ++i)
        {
            u[i].x = gn_bytemax(u[i].x, cur[i].x), u[i].y = gn_bytemax(u[i].y, cur[i].y);
            u[i].z = gn_bytemax(u[i].z, cur[i].z), u[i].w = gn_bytemax(u[i].w, cur[i].w);
            const uint32_t d[4] = { u[i].x, u[i].y, u[i].z, u[i].w };
#pragma unroll
            for (uint32_t k = 0; k < 4; ++k)
            {
                Z += 4u - (uint32_t)__popc((d[k] + 0x7F7F7F7Fu) & 0x80808080u); // a byte of at most 127 carries into its top bit unless it is 0
#pragma unroll
                for (uint32_t b = 0; b < 32; b += 8)
                    S += 1ULL << (52u - ((d[k] >> b) & 0xFFu));
            }
        }
#pragma unroll
        for (uint32_t off = 32; off; off >>= 1)
        {
            S += __shfl_xor(S, off);
            Z += __shfl_xor(Z, off);
        }
        if (lane == 0)
        {
            const unsigned long long est = gn_sketch_estimate(S, Z, num, small);
            best                         = est > best ? est : best;
            row[l - 1] = best;
        }
    }
    for (uint32_t l = steps + lane; l < width; l += 64) // past the last sketch
        row[l] = 0;
}

#define GN_PAIR_TILE 8u // sketches a side of a block's tile; two rows a wave

// One block per tile of GN_PAIR_TILE x GN_PAIR_TILE pairs (a, b) of positions of idx, a <= b: the grid is the tiles on and above
// the diagonal, block t = x * (x + 1) / 2 + y the tile of column tile x and row tile y <= x.  The tile's columns lie in LDS (32 KiB), read by all four waves; a wave holds one of its two rows in registers -- 4 KiB, 16
// dwords a lane, laid out as in the union kernel -- and walks the columns: four conflict-free 16-byte LDS reads a lane, then per
// register one byte maximum, one shift of 2^52 and one 64-bit add (the union kernel also keeps the running union and pays for that
// with a byte-wise maximum in dword arithmetic).  S and Z are reduced across the wave as integers, lane 0 makes the division and
// stores out[a * m + b] and out[b * m + a].  Positions at or beyond m (the last tile) are neither loaded nor paired.
__global__ __launch_bounds__(256) void gn_sketch_pair_kernel(const uint8_t* __restrict__ regs, const uint32_t* __restrict__ idx, uint32_t m, double num,
                                                             const double* __restrict__ small, unsigned long long* __restrict__ out)
{
    __shared__ __attribute__((aligned(16))) uint4 cols[GN_PAIR_TILE * (GN_SKETCH_M / 16)];
    const uint32_t t = blockIdx.x;
    uint32_t       x = (uint32_t)((sqrtf(8.0f * (float)t + 1.0f) - 1.0f) * 0.5f); // t < 2^18: off by one at the most, set right below
    while (x * (x + 1) / 2 > t)
        --x;
    while ((x + 1) * (x + 2) / 2 <= t)
        ++x;
    const uint32_t a0 = (t - x * (x + 1) / 2) * GN_PAIR_TILE, b0 = x * GN_PAIR_TILE; // (x < tiles, as t < tiles * (tiles + 1) / 2)
    const uint32_t n_cols = m - b0 < GN_PAIR_TILE ? m - b0 : GN_PAIR_TILE;
    for (uint32_t c = 0; c < n_cols; ++c)
        cols[c * 256 + threadIdx.x] = ((const uint4*)(regs + (uint64_t)idx[b0 + c] * GN_SKETCH_M))[threadIdx.x];
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u, wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    for (uint32_t r = 0; r < 2; ++r)
    {
        const uint32_t a = a0 + wave * 2 + r;
        if (a >= m)
            break;
        uint4 row[4];
#pragma unroll
        for (uint32_t i = 0; i < 4; ++i)
            row[i] = ((const uint4*)(regs + (uint64_t)idx[a] * GN_SKETCH_M))[i * 64 + lane];
        for (uint32_t c = a > b0 ? a - b0 : 0; c < n_cols; ++c) // (a > b0 on the diagonal tile only: pairs with a <= b)
        {
            unsigned long long S = 0;
            uint32_t           Z = 0;
#pragma unroll
            for (uint32_t i = 0; i < 4; ++i)
            {
                const uint4    v    = cols[c * 256 + i * 64 + lane];
                const uint32_t x[4] = { row[i].x, row[i].y, row[i].z, row[i].w }, y[4] = { v.x, v.y, v.z, v.w };
#pragma unroll
                for (uint32_t k = 0; k < 4; ++k)
                {
                    Z += 4u - (uint32_t)__popc(((x[k] | y[k]) + 0x7F7F7F7Fu) & 0x80808080u); // the maximum is 0 where both bytes are
#pragma unroll
                    for (uint32_t b = 0; b < 32; b += 8)
                    {
                        const uint32_t p = (x[k] >> b) & 0xFFu, q = (y[k] >> b) & 0xFFu;
                        S += (1ULL << 52) >> (p > q ? p : q);
                    }
                }
            }
#pragma unroll
            for (uint32_t off = 32; off; off >>= 1)
            {
                S += __shfl_xor(S, off);
                Z += __shfl_xor(Z, off);
            }
            if (lane == 0)
            {
                const unsigned long long est = gn_sketch_estimate(S, Z, num, small);
                const uint32_t           b   = b0 + c;
                out[(uint64_t)a * m + b]     = est;
                out[(uint64_t)b * m + a]     = est;
            }
        }
    }
}

extern "C" int gn_sketches_free(gn_sketches* s)
{
    if (!s)
        return GN_OK;
    (void)hipSetDevice(s->device);
    delete s;
    return GN_OK;
}

namespace
{
struct GnSketchesGuard // a handle that is not handed out yet
{
    gn_sketches* p;
    ~GnSketchesGuard() { delete p; }
};
} // namespace

// the handle of gn_sketches_create and gn_sketches_create_packed before a hash is read: n_sets sketches of zeros and the estimate's tables
static int gn_sketches_open(const char* who, int device, uint32_t n_sets, GnSketchesGuard& g)
{
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || device < 0 || device >= n_dev)
        return gn_fail(GN_ENODEV, "%s: no HIP device %d", who, device);
    GN_HIP(hipSetDevice(device));
    g.p            = new gn_sketches;
    gn_sketches* s = g.p;
    s->device      = device;
    s->n           = n_sets;
    GN_HIP(s->d_regs.alloc((size_t)n_sets * GN_SKETCH_M));
    GN_HIP(hipMemset(s->d_regs, 0, s->d_regs.cap())); // an empty set is all zeros
    const double        m     = (double)GN_SKETCH_M;
    const double        alpha = 0.7213 / (1.0 + 1.079 / m);
    std::vector<double> small(GN_SKETCH_M + 1, 0.0);
    for (uint32_t z = 1; z <= GN_SKETCH_M; ++z)
        small[z] = m * log(m / (double)z);
    s->num = alpha * 16777216.0 * 4503599627370496.0; // m^2 = 2^24, then 2^52: both products are exact
    GN_HIP(s->d_small.upload(small.data(), small.size()));
    return GN_OK;
}

// one round's items over the hashes in d_stage: the fill kernel, then the slots' scratch words folded into their sets' registers
static int gn_sketch_round(gn_sketches* s, const uint64_t* d_stage, const std::vector<GnSketchItem>& items, const std::vector<uint32_t>& slot_seg,
                           GnDev<GnSketchItem>& d_items, GnDev<uint32_t>& d_scratch, GnDev<uint32_t>& d_slot_seg, uint64_t max_slots)
{
    if (items.size() > d_items.cap() || slot_seg.size() > max_slots) // (cannot happen, see the bounds at the allocations)
        GN_HIP(hipErrorInvalidValue);
    GN_HIP(hipMemcpyAsync(d_items, items.data(), items.size() * sizeof(GnSketchItem), hipMemcpyHostToDevice, nullptr));
    if (!slot_seg.empty())
    {
        GN_HIP(hipMemsetAsync(d_scratch, 0, slot_seg.size() * GN_SKETCH_M * sizeof(uint32_t), nullptr));
        GN_HIP(hipMemcpyAsync(d_slot_seg, slot_seg.data(), slot_seg.size() * sizeof(uint32_t), hipMemcpyHostToDevice, nullptr));
    }
    hipLaunchKernelGGL(gn_sketch_fill_kernel, dim3((uint32_t)items.size()), dim3(256), 0, nullptr, d_stage, d_items, d_scratch, s->d_regs);
    GN_HIP(hipGetLastError());
    if (!slot_seg.empty())
    {
        const uint32_t n_slots = (uint32_t)slot_seg.size();
        hipLaunchKernelGGL(gn_sketch_pack_kernel, dim3(n_slots * (GN_SKETCH_M / 4 / 256)), dim3(256), 0, nullptr, d_scratch, d_slot_seg, n_slots, s->d_regs);
        GN_HIP(hipGetLastError());
    }
    GN_HIP(hipStreamSynchronize(nullptr)); // (the host's buffers, the staging buffer and the item lists are reused)
    return GN_OK;
}

extern "C" int gn_sketches_create(int device, const uint64_t* const* sets, const uint64_t* sizes, uint32_t n_sets, gn_sketches** out)
{
    if (!out || (n_sets && (!sets || !sizes)))
        return gn_fail(GN_EINVAL, "gn_sketches_create: null argument");
    *out = nullptr;
    for (uint32_t i = 0; i < n_sets; ++i)
        if (sizes[i] && !sets[i])
            return gn_fail(GN_EINVAL, "gn_sketches_create: set %u is null", i);
    GnSketchesGuard g{ nullptr };
    if (const int rc = gn_sketches_open("gn_sketches_create", device, n_sets, g))
        return rc;
    gn_sketches* s = g.p;

    // rounds of at most kStep hashes: sets below kDirect are gathered in pinned memory and go up in one copy, larger pieces go up
    // from where they lie
    constexpr uint64_t kStep = 8ull << 20, kDirect = 1ull << 20;
    uint64_t           total = 0;
    for (uint32_t i = 0; i < n_sets; ++i)
        total += sizes[i];
    if (total)
    {
        const uint64_t        step      = total < kStep ? total : kStep;
        const uint64_t        max_slots = step / GN_SKETCH_CHUNK + 2; // sets of more than one chunk that lie in a round, and one cut at each end
        const uint64_t        max_items = step / GN_SKETCH_CHUNK + (uint64_t)n_sets + 2;
        GnDev<uint64_t>       d_stage;
        GnDev<GnSketchItem>   d_items;
        GnDev<uint32_t>       d_scratch, d_slot_seg;
        GnPinned<uint64_t>    pool;
        std::vector<GnSketchItem> items;
        std::vector<uint32_t>     slot_seg;
        GN_HIP(d_stage.alloc(step));
        GN_HIP(d_items.alloc(max_items < step ? max_items : step)); // (an item holds at least one hash: at most `step` of them)
        GN_HIP(d_scratch.alloc(max_slots * GN_SKETCH_M));
        GN_HIP(d_slot_seg.alloc(max_slots));
        GN_HIP(pool.alloc(step));
        uint32_t seg = 0;
        uint64_t in  = 0; // hashes of set `seg` already sketched
        while (seg < n_sets)
        {
            items.clear(), slot_seg.clear();
            uint64_t at = 0, run = 0; // stage words filled; where the pooled words not yet uploaded begin
            auto     flush_pool = [&](uint64_t end) -> hipError_t {
                const hipError_t e = end > run ? hipMemcpyAsync(d_stage + run, pool + run, (end - run) * 8, hipMemcpyHostToDevice, nullptr) : hipSuccess;
                run                = end;
                return e;
            };
            while (seg < n_sets && at < step)
            {
                const uint64_t left = sizes[seg] - in, c = left < step - at ? left : step - at;
                if (c)
                {
                    if (c >= kDirect)
                    {
                        GN_HIP(flush_pool(at));
                        GN_HIP(hipMemcpyAsync(d_stage + at, sets[seg] + in, c * 8, hipMemcpyHostToDevice, nullptr));
                        run = at + c;
                    }
                    else
                        memcpy(pool + at, sets[seg] + in, c * 8);
                    uint32_t slot = ~0u;
                    if (sizes[seg] > GN_SKETCH_CHUNK || c != sizes[seg]) // more than one item, or a set the round's end cuts
                    {
                        slot = (uint32_t)slot_seg.size();
                        slot_seg.push_back(seg);
                    }
                    for (uint64_t a = 0; a < c; a += GN_SKETCH_CHUNK)
                        items.push_back(GnSketchItem{ seg, (uint32_t)(c - a < GN_SKETCH_CHUNK ? c - a : GN_SKETCH_CHUNK), slot, 0, at + a });
                    at += c, in += c;
                }
                if (in == sizes[seg])
                    ++seg, in = 0;
            }
            GN_HIP(flush_pool(at));
            if (items.empty())
                continue;
            if (const int rc = gn_sketch_round(s, d_stage, items, slot_seg, d_items, d_scratch, d_slot_seg, max_slots))
                return rc;
        }
    }
    GN_HIP(hipDeviceSynchronize());
    *out = s;
    g.p  = nullptr;
    return GN_OK;
}

// ---- gn_sketches_create_packed: the same sketches from packed runs --------------------------------------------------------------------
// A round stages the payload words and the tables of whole blocks -- at most kStep hashes and kBlocks blocks of them -- instead of
// hashes; gn_packed_decode_kernel (gn_build.hip) writes the round's hashes, run behind run, into the staging buffer gn_sketch_fill_kernel
// reads.  One more pass over HBM than the raw call makes, for a link that carries packed bytes; the sketch arithmetic stays in one place.
// A register is a maximum over the set's hashes: how a set is cut into rounds and items does not show in it.
extern "C" int gn_sketches_create_packed(int device, const gn_packed_block* const* blocks_abi, const uint64_t* n_blocks, const uint64_t* const* payload,
                                         uint32_t n_runs, gn_sketches** out)
{
    static const char* const    who    = "gn_sketches_create_packed";
    const GnPackedBlock* const* blocks = reinterpret_cast<const GnPackedBlock* const*>(blocks_abi);
    if (!out || (n_runs && (!blocks || !n_blocks || !payload)))
        return gn_fail(GN_EINVAL, "%s: null argument", who);
    *out           = nullptr;
    uint64_t total = 0;
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
        }
    }
    GnSketchesGuard g{ nullptr };
    if (const int rc = gn_sketches_open(who, device, n_runs, g))
        return rc;
    gn_sketches* s = g.p;
    if (total)
    {
        constexpr uint64_t kStep = 8ull << 20;
        const uint64_t     step  = std::max<uint64_t>(total < kStep ? total : kStep, GN_WIN_ITEM); // (a round holds any block)
        const uint64_t     kBlocks   = step / 64 + 16; // (a round of short blocks closes at this many of them)
        const uint64_t     max_slots = step / GN_SKETCH_CHUNK + 2; // runs of more than one chunk that lie in a round, and one cut at each end
        const uint64_t     max_items = step / GN_SKETCH_CHUNK + kBlocks + 2; // full chunks, and a short one per run (a run has a block)
        std::vector<GnSketchItem> items; // (before the buffers they are copied into: those are freed, which waits for the device, first)
        std::vector<uint32_t>     slot_seg;
        GnDev<uint64_t>           d_stage, d_words;
        GnDev<GnPackedItem>       d_blocks;
        GnDev<GnSketchItem>       d_items;
        GnDev<uint32_t>           d_scratch, d_slot_seg;
        GnPinned<uint64_t>        h_words;
        GnPinned<GnPackedItem>    h_blocks;
        GN_HIP(d_stage.alloc(step));
        GN_HIP(d_words.alloc(step)); // (a block has fewer words than hashes)
        GN_HIP(d_blocks.alloc(kBlocks));
        GN_HIP(d_items.alloc(max_items));
        GN_HIP(d_scratch.alloc(max_slots * GN_SKETCH_M));
        GN_HIP(d_slot_seg.alloc(max_slots));
        GN_HIP(h_words.alloc(step));
        GN_HIP(h_blocks.alloc(kBlocks));
        uint32_t run = 0;
        uint64_t blk = 0; // blocks of run `run` already sketched
        while (run < n_runs)
        {
            items.clear(), slot_seg.clear();
            uint64_t at = 0, words = 0, nb = 0; // hashes, payload words and blocks of the round
            while (run < n_runs && nb < kBlocks)
            {
                if (blk == n_blocks[run])
                {
                    ++run, blk = 0;
                    continue;
                }
                if (blocks[run][blk].cnt > step - at)
                    break;
                const uint64_t from = at, first_blk = blk; // the run's hashes of this round lie behind each other from `from` on
                for (; blk < n_blocks[run] && nb < kBlocks && blocks[run][blk].cnt <= step - at; ++blk, ++nb)
                {
                    const GnPackedBlock& b = blocks[run][blk];
                    const uint32_t       w = gn_packed_words(b.cnt, b.width);
                    if (w)
                        memcpy(h_words + words, payload[run] + b.word_at, (size_t)w * 8);
                    h_blocks[nb] = GnPackedItem{ run, b.cnt, b.width, 0, b.first, at, words, blk };
                    at += b.cnt, words += w;
                }
                const uint64_t c    = at - from;
                uint32_t       slot = ~0u;
                if (c > GN_SKETCH_CHUNK || first_blk != 0 || blk != n_blocks[run]) // more than one item, or a run the round's end cuts
                {
                    slot = (uint32_t)slot_seg.size();
                    slot_seg.push_back(run);
                }
                for (uint64_t a = 0; a < c; a += GN_SKETCH_CHUNK)
                    items.push_back(GnSketchItem{ run, (uint32_t)(c - a < GN_SKETCH_CHUNK ? c - a : GN_SKETCH_CHUNK), slot, 0, from + a });
                if (blk != n_blocks[run]) // (the round is full)
                    break;
            }
            if (items.empty())
                continue;
            if (words)
                GN_HIP(hipMemcpyAsync(d_words, h_words, words * 8, hipMemcpyHostToDevice, nullptr));
            GN_HIP(hipMemcpyAsync(d_blocks, h_blocks, nb * sizeof(GnPackedItem), hipMemcpyHostToDevice, nullptr));
            GN_HIP(gn_packed_decode_launch(nullptr, d_words, d_blocks, (uint32_t)nb, d_stage));
            if (const int rc = gn_sketch_round(s, d_stage, items, slot_seg, d_items, d_scratch, d_slot_seg, max_slots))
                return rc;
        }
    }
    GN_HIP(hipDeviceSynchronize());
    *out = s;
    g.p  = nullptr;
    return GN_OK;
}

extern "C" int gn_sketches_download(gn_sketches* s, uint32_t first, uint32_t n, uint8_t* out)
{
    if (!s || (n && !out))
        return gn_fail(GN_EINVAL, "gn_sketches_download: null argument");
    if ((uint64_t)first + n > s->n)
        return gn_fail(GN_EINVAL, "gn_sketches_download: sketches %u..%llu of %u", first, (unsigned long long)first + n, s->n);
    if (n == 0)
        return GN_OK;
    GN_HIP(hipSetDevice(s->device));
    GN_HIP(hipMemcpy(out, s->d_regs + (size_t)first * GN_SKETCH_M, (size_t)n * GN_SKETCH_M, hipMemcpyDeviceToHost));
    return GN_OK;
}

extern "C" int gn_sketches_union_table(gn_sketches* s, const uint32_t* order, uint32_t n, uint32_t j0, uint32_t j1, uint32_t width, uint64_t* out)
{
    if (!s || (n && !order))
        return gn_fail(GN_EINVAL, "gn_sketches_union_table: null argument");
    if (j0 > j1 || j1 > n)
        return gn_fail(GN_EINVAL, "gn_sketches_union_table: starts %u..%u of %u", j0, j1, n);
    const uint64_t entries = (uint64_t)(j1 - j0) * width;
    if (entries > GN_SKETCH_TABLE_MAX)
        return gn_fail(GN_ERANGE, "gn_sketches_union_table: %llu entries in one call, at most %llu: tile over the starts", (unsigned long long)entries,
                       (unsigned long long)GN_SKETCH_TABLE_MAX);
    if (entries == 0)
        return GN_OK;
    if (!out)
        return gn_fail(GN_EINVAL, "gn_sketches_union_table: null argument");
    for (uint32_t i = 0; i < n; ++i) // every sketch a wave can reach is checked here
        if (order[i] >= s->n)
            return gn_fail(GN_EINVAL, "gn_sketches_union_table: order[%u] = %u of %u sketches", i, order[i], s->n);
    GN_HIP(hipSetDevice(s->device));
    GnDev<uint32_t>           d_order;
    GnDev<unsigned long long> d_out;
    GN_HIP(d_order.upload(order, n));
    GN_HIP(d_out.alloc(entries));
    hipLaunchKernelGGL(gn_sketch_union_kernel, dim3((j1 - j0 + 3) / 4), dim3(256), 0, nullptr, s->d_regs, d_order, n, j0, j1, width, s->num, s->d_small,
                       d_out);
    GN_HIP(hipGetLastError());
    GN_HIP(hipMemcpy(out, d_out, entries * 8, hipMemcpyDeviceToHost));
    return GN_OK;
}

extern "C" int gn_sketches_pair_table(gn_sketches* s, const uint32_t* idx, uint32_t m, uint64_t* out)
{
    if (!s || (m && !idx))
        return gn_fail(GN_EINVAL, "gn_sketches_pair_table: null argument");
    const uint64_t entries = (uint64_t)m * m;
    if (entries > GN_SKETCH_TABLE_MAX)
        return gn_fail(GN_ERANGE, "gn_sketches_pair_table: %llu entries in one call, at most %llu", (unsigned long long)entries,
                       (unsigned long long)GN_SKETCH_TABLE_MAX);
    if (m == 0)
        return GN_OK;
    if (!out)
        return gn_fail(GN_EINVAL, "gn_sketches_pair_table: null argument");
    for (uint32_t i = 0; i < m; ++i) // every sketch a block can reach is checked here
        if (idx[i] >= s->n)
            return gn_fail(GN_EINVAL, "gn_sketches_pair_table: idx[%u] = %u of %u sketches", i, idx[i], s->n);
    GN_HIP(hipSetDevice(s->device));
    GnDev<uint32_t>           d_idx;
    GnDev<unsigned long long> d_out;
    GN_HIP(d_idx.upload(idx, m));
    GN_HIP(d_out.alloc(entries));
    const uint32_t tiles = (m + GN_PAIR_TILE - 1) / GN_PAIR_TILE;
    hipLaunchKernelGGL(gn_sketch_pair_kernel, dim3(tiles * (tiles + 1) / 2), dim3(256), 0, nullptr, s->d_regs, d_idx, m, s->num, s->d_small, d_out);
    GN_HIP(hipGetLastError());
    GN_HIP(hipMemcpy(out, d_out, entries * 8, hipMemcpyDeviceToHost));
    return GN_OK;
}
