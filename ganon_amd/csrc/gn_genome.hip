// gn_genome.hip -- wrapped, multi-record FASTA (a genome as it comes) tokenised on the device, for ganon-build.
//
// The builder's host path reads every genome with the sequential SeqReader (host/seq_io.cpp), which validates and copies every line, and
// Hasher::add (host/hasher.hpp) copies the letters a second time into overlapping pieces.  Here the host only reads the file into
// page-locked memory; the text travels as it is and the device does both steps:
//
//   1. every 4 KiB tile (256 threads x 16 bytes) yields a summary: the kind of its last line start (none / header / sequence), the
//      kept letters before and behind its first line start, its header line starts, its smallest illegal offsets;
//   2. ONE scan over the summaries (hipCUB, a non-commutative monoid: the line kind is a last-non-zero carry, and the letters before a
//      tile's first line start count only when the carry says "sequence") gives every tile the kind it starts in, the letters and the
//      headers before it;
//   3. a compaction pass writes the kept letters back to back and fills the record table (offset of the header, rank of the first letter);
//   4. one thread per record: its length, its state, the pieces Hasher::add would cut, their bytes; two scans; the records that fit;
//   5. one wave per piece copies at most stride + w - 1 letters into the stream's base buffer; off1 is closed form from the scanned
//      piece counts -- from here on the batch looks like one uploaded through gn_stream_upload_reads.
//
// The record rules are SeqReader::next's FASTA branch and RangeLines::line (host/seq_io.cpp): a line whose first byte is '>' or ';' begins
// a record and none of its bytes is a letter; in every other line isspace bytes and digits are ignored, the dna15 letters (either case)
// are kept, anything else is GN_GENOME_BAD_LETTER; before the first header only blank lines may stand (GN_GENOME_NO_HEADER otherwise).
// A record that is open at the end of a text (GN_GENOME_OPEN_END) leaves its last w - 1 letters and its length on the device; the next
// text (GN_GENOME_CONTINUES) puts them in front of its own letters, so every window across the cut is hashed exactly once.
#include "gn_internal.h"
#include "gn_scan.h"

#include <hip/hip_runtime.h>

#define GN_GX_TILE 4096u  // bytes per block: 256 threads x 16 bytes
#define GN_GX_PAD 65536u  // room in front of the compacted letters for the carried tail (w - 1 <= 65534 letters)
#define GN_GX_NONE 0xFFFFFFFFu

// d_ctl
enum
{
    GX_BAD = 0,     // smallest offset of an illegal byte in a sequence line
    GX_NOHDR,       // smallest offset of a byte of a non-blank line before the first header (without GN_GENOME_CONTINUES)
    GX_TAKEN,       // slots taken (slot 0 = what precedes the first header, slot j = the j-th header's record)
    GX_PIECES,      // ... their pieces
    GX_BASES,       // ... their bytes in d_bases
    GX_PARSED,      // offset of the first record not taken
    GX_OPEN,        // letters of the record left open (with what earlier texts carried)
    GX_STATUS,
    GX_RECORDS,     // records of the batch
    GX_SLOTS,       // slots of the text
    GX_BAD_AT,
    GX_NCTL = 16
};

// dna15 letters, either case (host/seq_io.cpp LegalTable): A B C D G H K M N R S T U V W Y
#define GN_GX_LEGAL                                                                                                                        \
    ((1u << 0) | (1u << 1) | (1u << 2) | (1u << 3) | (1u << 6) | (1u << 7) | (1u << 10) | (1u << 12) | (1u << 13) | (1u << 17) | (1u << 18) |   \
     (1u << 19) | (1u << 20) | (1u << 21) | (1u << 22) | (1u << 24))
// isspace (9-13, 32) and the digits (48-57): one 64-bit mask for the bytes below 64
#define GN_GX_IGNORED ((0x1Full << 9) | (1ull << 32) | (0x3FFull << 48))

// 0: a letter that is kept, 1: ignored, 2: illegal in a sequence line
__device__ __forceinline__ uint32_t gn_gx_class(uint32_t ch)
{
    const uint32_t u = (ch | 0x20u) - 'a';
    if (u < 26u && ((GN_GX_LEGAL >> u) & 1u) != 0u && (ch & 0x40u) != 0u)
        return 0u;
    return ch < 64u && ((GN_GX_IGNORED >> ch) & 1ull) != 0ull ? 1u : 2u;
}

__device__ __forceinline__ uint4 gn_gx_load16(const uint8_t* text, uint64_t n, uint64_t p)
{
    // (the buffer is padded beyond n; what the load brings from there is never looked at: every loop ends at `valid`)
    return p < n ? *reinterpret_cast<const uint4*>(text + p) : make_uint4(0, 0, 0, 0);
}

__device__ __forceinline__ uint32_t gn_gx_byte(const uint32_t (&w)[4], uint32_t j)
{
    return (w[j >> 2] >> ((j & 3u) * 8u)) & 0xFFu;
}

struct GnGxThread // what 16 bytes say without knowing the line they begin in
{
    uint32_t kind;     // of the last line start: 0 none, 1 header, 2 sequence
    uint32_t pre, post; // kept letters before the first line start (if that line is a sequence line) / behind it
    uint32_t nhdr;
    uint32_t bad_pre, bad_post; // smallest illegal offset of the two parts
};

__device__ __forceinline__ GnGxThread gn_gx_thread(const uint32_t (&w)[4], uint32_t valid, uint32_t prev, uint32_t p)
{
    GnGxThread t{ 0u, 0u, 0u, 0u, GN_GX_NONE, GN_GX_NONE };
#pragma unroll
    for (uint32_t j = 0; j < 16u; ++j)
    {
        const uint32_t ch = gn_gx_byte(w, j);
        if (j < valid)
        {
            if (prev == '\n')
            {
                t.kind = ch == '>' || ch == ';' ? 1u : 2u;
                t.nhdr += t.kind == 1u;
            }
            if (t.kind != 1u)
            {
                const uint32_t c = gn_gx_class(ch);
                if (t.kind == 0u)
                {
                    t.pre += c == 0u;
                    if (c == 2u && t.bad_pre == GN_GX_NONE)
                        t.bad_pre = p + j;
                }
                else
                {
                    t.post += c == 0u;
                    if (c == 2u && t.bad_post == GN_GX_NONE)
                        t.bad_post = p + j;
                }
            }
        }
        prev = ch;
    }
    return t;
}

// The kind of the last line start before this thread's bytes inside the tile (0: none), and the tile's own last kind.  The header and
// the sequence lanes are disjoint bit sets, so the one with the higher top bit is simply the larger number.
__device__ __forceinline__ uint32_t gn_gx_kind_in(uint32_t kind, uint32_t* wave_kind /* LDS [4] */, uint32_t& tile_kind)
{
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    const uint64_t h = __ballot(kind == 1u), s = __ballot(kind == 2u);
    const uint64_t below = (1ull << lane) - 1ull;
    const uint64_t hb = h & below, sb = s & below;
    uint32_t       kin = (hb | sb) ? (hb > sb ? 1u : 2u) : 0u;
    if (lane == 0)
        wave_kind[wv] = (h | s) ? (h > s ? 1u : 2u) : 0u;
    __syncthreads();
    tile_kind = 0;
    for (uint32_t x = 0; x < 4u; ++x)
    {
        const uint32_t k = wave_kind[x];
        if (k)
        {
            tile_kind = k;
            if (x < wv && (hb | sb) == 0ull)
                kin = k;
        }
    }
    return kin;
}

struct GnGxTile // a tile's summary; the scan's element
{
    uint32_t kind, pre, post, nhdr;
};

struct GnGxCombine // a then b
{
    __host__ __device__ __forceinline__ GnGxTile operator()(const GnGxTile& a, const GnGxTile& b) const
    {
        GnGxTile r;
        r.kind = b.kind ? b.kind : a.kind;
        r.nhdr = a.nhdr + b.nhdr;
        r.pre  = a.pre + (a.kind == 0u ? b.pre : 0u);
        r.post = a.post + b.post + (a.kind == 2u ? b.pre : 0u);
        return r;
    }
};

__global__ __launch_bounds__(256) void gn_gx_summary_kernel(const uint8_t* __restrict__ text, uint32_t n, GnGxTile* __restrict__ sum,
                                                            uint2* __restrict__ bad)
{
    __shared__ uint32_t wave_kind[4];
    __shared__ uint32_t red[4][5];
    const uint32_t p     = blockIdx.x * GN_GX_TILE + threadIdx.x * 16u;
    const uint4    v     = gn_gx_load16(text, n, p);
    const uint32_t w[4]  = { v.x, v.y, v.z, v.w };
    const uint32_t valid = p < n ? (n - p < 16u ? n - p : 16u) : 0u;
    const uint32_t prev  = p == 0u ? (uint32_t)'\n' : (p <= n ? (uint32_t)text[p - 1] : 0u);
    const GnGxThread t   = gn_gx_thread(w, valid, prev, p);
    uint32_t       tile_kind;
    const uint32_t kin = gn_gx_kind_in(t.kind, wave_kind, tile_kind);
    // what precedes the thread's first line start belongs to the line the tile's earlier bytes began -- or to the tile's own "pre"
    uint32_t pre = kin == 0u ? t.pre : 0u, post = t.post + (kin == 2u ? t.pre : 0u), nhdr = t.nhdr;
    uint32_t bpre = kin == 0u ? t.bad_pre : GN_GX_NONE, bpost = min(t.bad_post, kin == 2u ? t.bad_pre : GN_GX_NONE);
    for (int o = 32; o > 0; o >>= 1)
    {
        pre += (uint32_t)__shfl_xor((int)pre, o);
        post += (uint32_t)__shfl_xor((int)post, o);
        nhdr += (uint32_t)__shfl_xor((int)nhdr, o);
        bpre  = min(bpre, (uint32_t)__shfl_xor((int)bpre, o));
        bpost = min(bpost, (uint32_t)__shfl_xor((int)bpost, o));
    }
    if ((threadIdx.x & 63u) == 0)
    {
        uint32_t* r = red[threadIdx.x >> 6];
        r[0] = pre, r[1] = post, r[2] = nhdr, r[3] = bpre, r[4] = bpost;
    }
    __syncthreads();
    if (threadIdx.x == 0)
    {
        GnGxTile s{ tile_kind, 0u, 0u, 0u };
        uint2    b = make_uint2(GN_GX_NONE, GN_GX_NONE);
        for (uint32_t x = 0; x < 4u; ++x)
        {
            s.pre += red[x][0], s.post += red[x][1], s.nhdr += red[x][2];
            b.x = min(b.x, red[x][3]), b.y = min(b.y, red[x][4]);
        }
        sum[blockIdx.x] = s;
        bad[blockIdx.x] = b;
    }
}

// exclusive prefix of v over the block (LDS part[4]); the caller syncs before part is used again
__device__ __forceinline__ uint32_t gn_gx_block_excl(uint32_t v, uint32_t* part)
{
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    uint32_t       inc = v;
    for (int o = 1; o < 64; o <<= 1)
    {
        const uint32_t up = (uint32_t)__shfl_up((int)inc, o);
        if (lane >= (uint32_t)o)
            inc += up;
    }
    if (lane == 63u)
        part[wv] = inc;
    __syncthreads();
    uint32_t base = inc - v;
    for (uint32_t x = 0; x < wv; ++x)
        base += part[x];
    return base;
}

// pref[tile]: everything before the tile (the scan started in a sequence line: what precedes the first header is slot 0)
__global__ __launch_bounds__(256) void gn_gx_compact_kernel(const uint8_t* __restrict__ text, uint32_t n, const GnGxTile* __restrict__ pref,
                                                            const uint2* __restrict__ bad, uint32_t continues, uint32_t slot_cap,
                                                            uint8_t* __restrict__ letters /* behind the pad */, uint64_t* __restrict__ rec_at,
                                                            uint64_t* __restrict__ rec_l0, unsigned long long* __restrict__ ctl)
{
    __shared__ uint32_t wave_kind[4];
    __shared__ uint32_t part_l[4], part_h[4];
    const uint32_t p     = blockIdx.x * GN_GX_TILE + threadIdx.x * 16u;
    const uint4    v     = gn_gx_load16(text, n, p);
    const uint32_t w[4]  = { v.x, v.y, v.z, v.w };
    const uint32_t valid = p < n ? (n - p < 16u ? n - p : 16u) : 0u;
    const uint32_t prev0 = p == 0u ? (uint32_t)'\n' : (p <= n ? (uint32_t)text[p - 1] : 0u);
    const GnGxThread t   = gn_gx_thread(w, valid, prev0, p);
    const GnGxTile   in  = pref[blockIdx.x];
    uint32_t         tile_kind;
    uint32_t         kin = gn_gx_kind_in(t.kind, wave_kind, tile_kind);
    if (kin == 0u)
        kin = in.kind;
    const uint32_t mine  = t.post + (kin == 2u ? t.pre : 0u);
    uint32_t       rank  = in.pre + in.post + gn_gx_block_excl(mine, part_l);
    uint32_t       hdrs  = in.nhdr + gn_gx_block_excl(t.nhdr, part_h);
    if (threadIdx.x == 0)
    {
        const uint32_t b = min(in.kind == 2u ? bad[blockIdx.x].x : GN_GX_NONE, bad[blockIdx.x].y);
        if (b != GN_GX_NONE)
            atomicMin(&ctl[GX_BAD], (unsigned long long)b);
    }
    uint32_t prev = prev0, kind = kin;
#pragma unroll
    for (uint32_t j = 0; j < 16u; ++j)
    {
        const uint32_t ch = gn_gx_byte(w, j);
        if (j < valid)
        {
            if (prev == '\n')
            {
                kind = ch == '>' || ch == ';' ? 1u : 2u;
                if (kind == 1u)
                {
                    ++hdrs; // slot of this record
                    if (hdrs <= slot_cap)
                    {
                        rec_at[hdrs] = p + j;
                        rec_l0[hdrs] = rank;
                    }
                }
            }
            if (kind == 2u)
            {
                if (gn_gx_class(ch) == 0u)
                    letters[rank++] = (uint8_t)ch;
                // before the first header only blank lines may stand: "\n", or "\r\n" (the '\r' that RangeLines::line strips)
                if (hdrs == 0u && !continues && ch != '\n')
                {
                    bool blank = false;
                    if (ch == '\r')
                    {
                        const uint32_t q = p + j + 1u;
                        blank            = q >= n || text[q] == '\n';
                    }
                    if (!blank)
                        atomicMin(&ctl[GX_NOHDR], (unsigned long long)(p + j));
                }
            }
        }
        prev = ch;
    }
}

// the carried tail in front of the letters (GN_GENOME_CONTINUES); carry = { letters of the tail, letters of the open record }
__global__ void gn_gx_tail_in_kernel(const uint8_t* __restrict__ tail, const uint64_t* __restrict__ carry, uint8_t* __restrict__ letters)
{
    const uint32_t n = (uint32_t)carry[0];
    for (uint32_t i = threadIdx.x; i < n; i += blockDim.x)
        (letters - n)[i] = tail[i];
}

// One thread per slot: the record's letters, its state, the pieces Hasher::add cuts (host/hasher.hpp) and their bytes.  Slots at and
// beyond the text's own are written as empty, so that the two scans run over a fixed number of entries.
__global__ void gn_gx_records_kernel(const GnGxTile* __restrict__ total, const uint64_t* __restrict__ rec_l0, const uint64_t* __restrict__ carry,
                                     uint32_t continues, uint32_t open_end, uint32_t w, uint32_t stride, uint64_t min_length, uint32_t slot_cap,
                                     uint64_t* __restrict__ rec_len, uint8_t* __restrict__ rec_state, uint32_t* __restrict__ pieces,
                                     uint64_t* __restrict__ bytes, unsigned long long* __restrict__ ctl)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i > slot_cap)
        return;
    const uint32_t n_slots = total->nhdr + 1u;
    if (i == 0)
        ctl[GX_SLOTS] = n_slots;
    uint32_t np = 0;
    uint64_t nb = 0, len = 0;
    uint8_t  state = 1;
    if (i < n_slots && i < slot_cap && (i > 0 || continues))
    {
        const uint64_t letters = (uint64_t)total->pre + total->post;
        const uint64_t begin   = i ? rec_l0[i] : 0ull;
        const uint64_t fresh   = (i + 1u == n_slots ? letters : rec_l0[i + 1]) - begin;
        const uint64_t cut     = fresh + (i == 0 ? carry[0] : 0ull); // the letters pieces are cut from: the tail, then the text's
        len                    = fresh + (i == 0 ? carry[1] : 0ull);
        const bool open        = open_end && i + 1u == n_slots;
        state                  = open ? 3 : len < min_length ? 1 : len < w ? 2 : 0;
        if ((state == 0 || state == 3) && cut >= w)
        {
            np = (uint32_t)((cut - w) / stride) + 1u;
            const uint64_t last = cut - (uint64_t)(np - 1u) * stride;
            nb = (uint64_t)(np - 1u) * (stride + w - 1u) + (last < (uint64_t)stride + w - 1u ? last : (uint64_t)stride + w - 1u);
        }
    }
    rec_len[i]   = len;
    rec_state[i] = state;
    pieces[i]    = np;
    bytes[i]     = nb;
}

// whole records while their pieces and bytes fit: the last slot that does says how many are taken
__global__ void gn_gx_take_kernel(const uint64_t* __restrict__ piece_off, const uint64_t* __restrict__ byte_off, uint32_t slot_cap, uint32_t max_reads,
                                  uint64_t max_bases, unsigned long long* __restrict__ ctl)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t       n = (uint32_t)ctl[GX_SLOTS];
    if (n > slot_cap)
        n = slot_cap;
    if (i >= n)
        return;
    auto fits = [&](uint32_t x) { return piece_off[x + 1] <= max_reads && byte_off[x + 1] <= max_bases; };
    if (fits(i) && (i + 1u == n || !fits(i + 1u)))
        ctl[GX_TAKEN] = i + 1u;
}

__global__ void gn_gx_finish_kernel(const uint64_t* __restrict__ piece_off, const uint64_t* __restrict__ byte_off, const uint64_t* __restrict__ rec_at,
                                    const uint64_t* __restrict__ rec_len, const GnGxTile* __restrict__ total, uint32_t n_bytes, uint32_t continues,
                                    uint32_t open_end, uint32_t w, uint64_t* __restrict__ carry, uint64_t* __restrict__ off1,
                                    unsigned long long* __restrict__ ctl)
{
    const uint32_t n_slots = (uint32_t)ctl[GX_SLOTS], taken = (uint32_t)ctl[GX_TAKEN];
    const bool     all     = taken == n_slots;
    const uint64_t parsed  = all ? n_bytes : rec_at[taken];
    ctl[GX_PIECES]         = piece_off[taken];
    ctl[GX_BASES]          = byte_off[taken];
    ctl[GX_PARSED]         = parsed;
    ctl[GX_RECORDS]        = continues ? taken : (taken ? taken - 1u : 0u);
    off1[piece_off[taken]] = byte_off[taken];
    uint64_t status = 0, at = 0;
    if (ctl[GX_NOHDR] != ~0ull)
        status = GN_GENOME_NO_HEADER, at = ctl[GX_NOHDR];
    else if (ctl[GX_BAD] < parsed)
        status = GN_GENOME_BAD_LETTER, at = ctl[GX_BAD];
    ctl[GX_STATUS] = status;
    ctl[GX_BAD_AT] = at;
    // the record left open: its length so far, and how many of its last letters the next text needs in front of its own
    uint64_t open = 0, tail = 0;
    if (all && open_end && (n_slots > 1u || continues))
    {
        open = rec_len[n_slots - 1u];
        tail = open < w - 1u ? open : w - 1u;
    }
    ctl[GX_OPEN] = open;
    carry[2]     = tail; // (the old tail is still in use by this batch's pieces: gn_gx_tail_out_kernel moves the two over)
    carry[3]     = open;
    (void)total;
}

// one wave per piece: at most stride + w - 1 letters from the compacted letters into the stream's base buffer
__global__ __launch_bounds__(256) void gn_gx_pieces_kernel(const uint8_t* __restrict__ letters, const uint64_t* __restrict__ piece_off,
                                                           const uint64_t* __restrict__ byte_off, const uint64_t* __restrict__ rec_l0,
                                                           const uint64_t* __restrict__ carry, const GnGxTile* __restrict__ total, uint32_t continues,
                                                           uint32_t w, uint32_t stride, const unsigned long long* __restrict__ ctl,
                                                           uint8_t* __restrict__ bases, uint64_t* __restrict__ off1)
{
    const uint32_t lane    = threadIdx.x & 63u;
    const uint32_t wave    = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const uint32_t n_waves = (gridDim.x * blockDim.x) >> 6;
    const uint32_t taken = (uint32_t)ctl[GX_TAKEN], n_slots = (uint32_t)ctl[GX_SLOTS];
    const uint32_t n_pieces = (uint32_t)ctl[GX_PIECES];
    const uint64_t full     = (uint64_t)stride + w - 1u;
    for (uint32_t pc = wave; pc < n_pieces; pc += n_waves)
    {
        uint32_t lo = 0, hi = taken; // the slot with piece_off[slot] <= pc < piece_off[slot + 1]
        while (hi - lo > 1u)
        {
            const uint32_t mid = (lo + hi) >> 1;
            if (piece_off[mid] <= pc)
                lo = mid;
            else
                hi = mid;
        }
        const uint32_t slot  = lo;
        const uint64_t j     = pc - piece_off[slot];
        const uint64_t begin = slot ? rec_l0[slot] : 0ull;
        const uint64_t end   = slot + 1u == n_slots ? (uint64_t)total->pre + total->post : rec_l0[slot + 1];
        const uint64_t ahead = slot == 0 && continues ? carry[0] : 0ull;
        const uint64_t cut   = end - begin + ahead;
        const uint64_t at    = j * stride;
        const uint64_t n     = cut - at < full ? cut - at : full;
        const uint8_t* src   = letters + begin - ahead + at; // (begin is 0 where ahead is not)
        const uint64_t to    = byte_off[slot] + j * full;
        uint8_t*       dst   = bases + to;
        for (uint64_t x = lane; x < n; x += 64u)
            dst[x] = src[x];
        if (lane == 0)
            off1[pc] = to;
    }
}

// the open record's last letters, for the next text; they may reach back into the tail this text was given
__global__ void gn_gx_tail_out_kernel(const uint8_t* __restrict__ letters, const GnGxTile* __restrict__ total, uint64_t* __restrict__ carry,
                                      uint8_t* __restrict__ tail)
{
    const uint32_t n   = (uint32_t)carry[2];
    const uint8_t* src = letters + ((uint64_t)total->pre + total->post) - n;
    for (uint32_t i = threadIdx.x; i < n; i += blockDim.x)
        tail[i] = src[i];
    __syncthreads();
    if (threadIdx.x == 0)
        carry[0] = carry[2], carry[1] = carry[3];
}

static int gn_genome_prepare(gn_stream* s)
{
    if (s->gx.ready)
        return GN_OK;
    GnGenomeBufs b;
    b.tiles_cap = (uint32_t)((s->max_bases + GN_GX_TILE - 1) / GN_GX_TILE) + 1u;
    b.slot_cap  = s->max_reads + 1u; // records of one batch: every record with a piece needs a read of the stream, and slot 0
    GN_HIP(b.d_text.alloc(s->max_bases + 64));
    GN_HIP(b.d_letters.alloc((size_t)GN_GX_PAD + s->max_bases + 64));
    GN_HIP(b.d_tail.alloc(GN_GX_PAD));
    GN_HIP(b.d_sum.alloc(((size_t)b.tiles_cap + 1) * 2 * sizeof(GnGxTile)));
    GN_HIP(b.d_bad.alloc(((size_t)b.tiles_cap + 1) * 2));
    GN_HIP(b.d_rec_at.alloc((size_t)b.slot_cap + 2));
    GN_HIP(b.d_rec_l0.alloc((size_t)b.slot_cap + 2));
    GN_HIP(b.d_rec_len.alloc((size_t)b.slot_cap + 2));
    GN_HIP(b.d_rec_state.alloc((size_t)b.slot_cap + 2));
    GN_HIP(b.d_pieces.alloc((size_t)b.slot_cap + 2));
    GN_HIP(b.d_bytes.alloc((size_t)b.slot_cap + 2));
    GN_HIP(b.d_piece_off.alloc((size_t)b.slot_cap + 2));
    GN_HIP(b.d_byte_off.alloc((size_t)b.slot_cap + 2));
    GN_HIP(b.d_carry.alloc(4));
    GN_HIP(b.d_ctl.alloc(GX_NCTL));
    GN_HIP(b.h_ctl.alloc(GX_NCTL));
    GN_HIP(hipMemsetAsync(b.d_carry, 0, 4 * sizeof(uint64_t), s->st));
    size_t          t1 = 0, t2 = 0, t3 = 0;
    const GnGxTile* in  = reinterpret_cast<const GnGxTile*>(b.d_sum.get());
    GnGxTile*       out = reinterpret_cast<GnGxTile*>(b.d_sum.get());
    hipcub::DeviceScan::ExclusiveScan(nullptr, t1, in, out, GnGxCombine(), GnGxTile{ 2u, 0u, 0u, 0u }, (int)(b.tiles_cap + 1), s->st);
    gn_scan_counts(nullptr, t2, b.d_pieces, b.d_piece_off, (int)(b.slot_cap + 2), s->st);
    hipcub::DeviceScan::ExclusiveSum(nullptr, t3, b.d_bytes.get(), b.d_byte_off.get(), (int)(b.slot_cap + 2), s->st);
    b.scan_bytes = std::max(t1, std::max(t2, t3)) + 256;
    GN_HIP(b.d_scan.alloc(b.scan_bytes));
    b.ready = true;
    s->gx   = std::move(b);
    return GN_OK;
}

extern "C" int gn_stream_upload_genome_text(gn_stream* s, const uint8_t* text, uint64_t n_bytes, uint32_t w, uint32_t stride, uint64_t min_length,
                                            uint32_t flags)
{
    if (!s || (!text && n_bytes))
        return gn_fail(GN_EINVAL, "gn_stream_upload_genome_text: null argument");
    if (w == 0 || w > GN_GX_PAD - 1u || stride == 0 || (flags & ~(GN_GENOME_CONTINUES | GN_GENOME_OPEN_END)) != 0)
        return gn_fail(GN_EINVAL, "gn_stream_upload_genome_text: w %u, stride %u, flags %u", w, stride, flags);
    if (n_bytes > s->max_bases || n_bytes >= 0xFFFFFFF0ull)
        return gn_fail(GN_EINVAL, "text of %llu bytes exceeds the stream capacity (%llu bytes)", (unsigned long long)n_bytes,
                       (unsigned long long)s->max_bases);
    GN_HIP(hipSetDevice(s->f->device));
    int rc = gn_genome_prepare(s);
    if (rc)
        return rc;
    GnGenomeBufs& g = s->gx;
    GN_HIP(hipStreamSynchronize(s->st)); // previous batch must be done before its inputs are overwritten
    hipStream_t    st        = s->st;
    const uint32_t continues = (flags & GN_GENOME_CONTINUES) ? 1u : 0u, open_end = (flags & GN_GENOME_OPEN_END) ? 1u : 0u;
    const uint32_t n         = (uint32_t)n_bytes;
    const uint32_t tiles     = (n + GN_GX_TILE - 1) / GN_GX_TILE;
    GnGxTile*      sum       = reinterpret_cast<GnGxTile*>(g.d_sum.get());
    GnGxTile*      pref      = sum + g.tiles_cap + 1;
    uint2*         bad       = reinterpret_cast<uint2*>(g.d_bad.get());
    uint8_t*       letters   = g.d_letters.get() + GN_GX_PAD;
    if (n_bytes)
        GN_HIP(hipMemcpyAsync(g.d_text, text, n_bytes, hipMemcpyHostToDevice, st));
    if (!continues) // nothing is carried into this text
        GN_HIP(hipMemsetAsync(g.d_carry, 0, 4 * sizeof(uint64_t), st));
    GN_HIP(hipMemsetAsync(g.d_ctl, 0, GX_NCTL * sizeof(unsigned long long), st));
    GN_HIP(hipMemsetAsync(g.d_ctl, 0xFF, 2 * sizeof(unsigned long long), st)); // GX_BAD, GX_NOHDR
    GN_HIP(hipMemsetAsync(sum + tiles, 0, sizeof(GnGxTile), st));               // (the scan's last element: its prefix is the text's total)
    GN_HIP(hipMemsetAsync(g.d_rec_at, 0, sizeof(uint64_t), st));
    GN_HIP(hipMemsetAsync(g.d_rec_l0, 0, sizeof(uint64_t), st));
    if (continues)
        hipLaunchKernelGGL(gn_gx_tail_in_kernel, dim3(1), dim3(256), 0, st, g.d_tail.get(), g.d_carry.get(), letters);
    if (tiles)
        hipLaunchKernelGGL(gn_gx_summary_kernel, dim3(tiles), dim3(256), 0, st, g.d_text.get(), n, sum, bad);
    size_t tmp = g.scan_bytes;
    GN_HIP(hipcub::DeviceScan::ExclusiveScan(g.d_scan.get(), tmp, (const GnGxTile*)sum, pref, GnGxCombine(), GnGxTile{ 2u, 0u, 0u, 0u }, (int)(tiles + 1), st));
    const GnGxTile* total = pref + tiles;
    if (tiles)
        hipLaunchKernelGGL(gn_gx_compact_kernel, dim3(tiles), dim3(256), 0, st, g.d_text.get(), n, (const GnGxTile*)pref, (const uint2*)bad, continues,
                           g.slot_cap, letters, g.d_rec_at.get(), g.d_rec_l0.get(), g.d_ctl.get());
    const uint32_t n_entries = g.slot_cap + 1u;
    hipLaunchKernelGGL(gn_gx_records_kernel, dim3((n_entries + 255) / 256), dim3(256), 0, st, total, g.d_rec_l0.get(), g.d_carry.get(), continues, open_end, w,
                       stride, min_length, g.slot_cap, g.d_rec_len.get(), g.d_rec_state.get(), g.d_pieces.get(), g.d_bytes.get(), g.d_ctl.get());
    tmp = g.scan_bytes;
    GN_HIP(gn_scan_counts(g.d_scan.get(), tmp, g.d_pieces, g.d_piece_off, (int)n_entries, st));
    tmp = g.scan_bytes;
    GN_HIP(hipcub::DeviceScan::ExclusiveSum(g.d_scan.get(), tmp, g.d_bytes.get(), g.d_byte_off.get(), (int)n_entries, st));
    hipLaunchKernelGGL(gn_gx_take_kernel, dim3((g.slot_cap + 255) / 256), dim3(256), 0, st, g.d_piece_off.get(), g.d_byte_off.get(), g.slot_cap, s->max_reads,
                       s->max_bases, g.d_ctl.get());
    hipLaunchKernelGGL(gn_gx_finish_kernel, dim3(1), dim3(1), 0, st, g.d_piece_off.get(), g.d_byte_off.get(), g.d_rec_at.get(), g.d_rec_len.get(), total, n,
                       continues, open_end, w, g.d_carry.get(), s->d_off1.get(), g.d_ctl.get());
    const uint32_t blocks = std::max<uint32_t>(1u, std::min<uint32_t>((uint32_t)(n_bytes / (4u * stride)) + 1u, (uint32_t)s->f->n_cu * 8u));
    hipLaunchKernelGGL(gn_gx_pieces_kernel, dim3(blocks), dim3(256), 0, st, (const uint8_t*)letters, g.d_piece_off.get(), g.d_byte_off.get(),
                       g.d_rec_l0.get(), g.d_carry.get(), total, continues, w, stride, g.d_ctl.get(), s->d_bases.get(), s->d_off1.get());
    hipLaunchKernelGGL(gn_gx_tail_out_kernel, dim3(1), dim3(256), 0, st, (const uint8_t*)letters, total, g.d_carry.get(), g.d_tail.get());
    GN_HIP(hipMemcpyAsync(g.h_ctl, g.d_ctl, GX_NCTL * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    GN_HIP(hipGetLastError());
    g.pending     = true;
    g.continues   = continues != 0;
    s->have_reads = false;
    s->classified = false;
    s->ctr_copied = false;
    s->hashed     = false;
    return GN_OK;
}

extern "C" int gn_stream_genome_index(gn_stream* s, uint32_t* n_records, uint32_t* n_pieces, uint64_t* n_bases, uint64_t* parsed_bytes, int* status,
                                      uint64_t* bad_at, uint64_t* open_letters)
{
    if (!s)
        return gn_fail(GN_EINVAL, "null stream");
    if (!s->gx.ready || !s->gx.pending)
        return gn_fail(GN_EINVAL, "gn_stream_genome_index: no genome text was uploaded on this stream");
    GN_HIP(hipSetDevice(s->f->device));
    GN_HIP(hipStreamSynchronize(s->st));
    GnGenomeBufs&             g = s->gx;
    const unsigned long long* c = g.h_ctl;
    g.pending    = false;
    g.n_records  = (uint32_t)c[GX_RECORDS];
    s->v_hashes   = s->d_hashes; // (a batch of its own, as after gn_stream_upload_reads)
    s->v_slot_off = s->d_slot_off;
    s->v_nh       = s->d_nh;
    s->v_status   = s->d_status;
    s->src        = nullptr;
    s->n_reads    = (uint32_t)c[GX_PIECES];
    s->n_bases    = c[GX_BASES];
    s->paired     = false;
    s->have_reads = true;
    s->classified = false;
    s->hashed     = false;
    s->build_distinct = ~0ull;
    if (n_records)
        *n_records = g.n_records;
    if (n_pieces)
        *n_pieces = s->n_reads;
    if (n_bases)
        *n_bases = s->n_bases;
    if (parsed_bytes)
        *parsed_bytes = c[GX_PARSED];
    if (status)
        *status = (int)c[GX_STATUS];
    if (bad_at)
        *bad_at = c[GX_BAD_AT];
    if (open_letters)
        *open_letters = c[GX_OPEN];
    // not even the first record fits the stream (with a legal text: an illegal one is the caller's to read again anyway)
    if (c[GX_STATUS] == 0 && c[GX_TAKEN] < c[GX_SLOTS] && c[GX_RECORDS] == 0)
        return gn_fail(GN_ERANGE, "gn_stream_genome_index: the first record alone exceeds the stream capacity (%u pieces, %llu bytes)", s->max_reads,
                       (unsigned long long)s->max_bases);
    return GN_OK;
}

extern "C" int gn_stream_genome_records(gn_stream* s, uint64_t* rec_at, uint64_t* rec_letters, uint8_t* rec_state)
{
    if (!s || !s->gx.ready || s->gx.pending || !s->have_reads)
        return gn_fail(GN_EINVAL, "gn_stream_genome_records: not a tokenised genome text");
    GN_HIP(hipSetDevice(s->f->device));
    const GnGenomeBufs& g     = s->gx;
    const size_t        first = g.continues ? 0 : 1; // slot 0 is a record only where it continues one
    const size_t        n     = g.n_records;
    if (n)
    {
        if (rec_at)
            GN_HIP(hipMemcpyAsync(rec_at, g.d_rec_at.get() + first, n * sizeof(uint64_t), hipMemcpyDeviceToHost, s->st));
        if (rec_letters)
            GN_HIP(hipMemcpyAsync(rec_letters, g.d_rec_len.get() + first, n * sizeof(uint64_t), hipMemcpyDeviceToHost, s->st));
        if (rec_state)
            GN_HIP(hipMemcpyAsync(rec_state, g.d_rec_state.get() + first, n, hipMemcpyDeviceToHost, s->st));
    }
    GN_HIP(hipStreamSynchronize(s->st));
    return GN_OK;
}
