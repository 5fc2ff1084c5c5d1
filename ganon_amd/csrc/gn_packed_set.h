// gn_packed_set.h -- hash sets packed as deltas of fixed width (`ganon-build --hash-sets packed|spilled`): the format, its host encoder
// and decoder, the bit-extract the host and the insert kernel share, and the item builder of gn_filter_emplace_packed_window
// (gn_build.hip).  No device call in here: like gn_emplace_window.h it compiles for the host and for the device, so that a CPU program
// (tests/build_packed_driver.cpp) runs the very code the kernels run.
//
// A packed run is a sequence of blocks and one payload of 64-bit words.
//   block    `cnt` hashes v[0 .. cnt), 1 <= cnt <= 512 (GN_WIN_ITEM: one wave item of the windowed insert), strictly ascending;
//            `first` = v[0]; `width` = the bit length of the largest delta v[i] - v[i-1], i = 1 .. cnt-1 (0 when cnt == 1);
//            `word_at` = the word of the payload its deltas start at
//   payload  delta i-1 (the one that leads to v[i]) occupies bits [(i-1) * width, i * width) of the block's words, LSB first, running
//            across word boundaries; a block has ceil((cnt-1) * width / 64) words, starts on a word boundary, its padding bits are zero
//   cutting  a set (one file's distinct hashes, ascending) is cut every 512 hashes from its start; a block never crosses the end of a
//            set.  A target's run is its files' sets behind each other, so a short block may lie in the middle of a run.
// What can go wrong, and where it is handled:
//   width == 64          legal (at k = 32 a hash takes any 64-bit value): a delta that starts at bit 0 of a word is the word -- no mask
//                        is built by shifting by 64 and no second word is shifted by 64 (gn_packed_delta, gn_packed_put)
//   width == 0           a block of one hash has no payload word at all: nothing is read (gn_packed_delta returns before any load)
//   a read past a block  the second word of a delta is read only when the delta really runs into it, so it is a word of the block
//   8 deltas of a lane   are `width` BYTES: lane L of the insert kernel reads bytes [L * width, (L + 1) * width) of the block's payload
#pragma once

#include <stdint.h>

#include "gn_emplace_window.h" // GN_WIN_HD, GN_WIN_ITEM, GN_WIN_PER_LANE

#define GN_PACKED_MAX_WORDS (GN_WIN_ITEM - 1) // payload words of one block at most: 511 deltas of 64 bits
#define GN_PACKED_CHUNK (1ull << 20)          // payload words of a staging chunk when the caller names none (8 MiB, as GN_WIN_CHUNK)

// (the layout of gn_packed_block, include/ganon_hip.h)
struct GnPackedBlock
{
    uint64_t first, word_at;
    uint32_t cnt, width;
};

// A wave's piece of work in gn_emplace_packed_window_kernel: one block.  `begin` is the index of its first hash in the RUN (the bin of a
// hash is first_bin + (begin + q) / per_bin), `stage_at` the word of the staging chunk its payload starts at, `block` the block's number
// in the run (the host's gather finds the payload by it; the kernel does not read it).
struct GnPackedItem
{
    uint32_t run, cnt, width, reserved;
    uint64_t first, begin, stage_at, block;
};

// bit length of a delta: 0 for 0, 64 for a value with the top bit set
GN_WIN_HD uint32_t gn_packed_bits(uint64_t x)
{
    return x ? 64u - (uint32_t)__builtin_clzll(x) : 0u;
}

// payload words of a block of cnt hashes at `width` bits a delta
GN_WIN_HD uint32_t gn_packed_words(uint32_t cnt, uint32_t width)
{
    return (uint32_t)(((uint64_t)(cnt - 1) * width + 63) >> 6);
}

// Delta number e (0-based: the one that leads to hash e + 1) of a block whose payload starts at `words`.
GN_WIN_HD uint64_t gn_packed_delta(const uint64_t* words, uint32_t e, uint32_t width)
{
    if (width == 0)
        return 0;
    const uint32_t bit = e * width, w = bit >> 6, off = bit & 63u;
    uint64_t       x = words[w] >> off;
    if (off + width > 64) // (off >= 1 here: the shift below is 1 .. 63)
        x |= words[w + 1] << (64u - off);
    return width == 64 ? x : x & ((1ULL << width) - 1);
}

// Bounds on what n hashes of ONE set pack into: its blocks, and its payload words (every block's payload is shorter than its hashes).
GN_WIN_HD uint64_t gn_packed_max_blocks(uint64_t n)
{
    return (n + GN_WIN_ITEM - 1) / GN_WIN_ITEM;
}
GN_WIN_HD uint64_t gn_packed_max_words(uint64_t n)
{
    return n - gn_packed_max_blocks(n);
}

// what a packed set holds in bytes: its payload and its block list
GN_WIN_HD uint64_t gn_packed_bytes(uint64_t n_blocks, uint64_t n_words)
{
    return n_words * 8 + n_blocks * sizeof(GnPackedBlock);
}

#include <vector>

// writes delta e of a block into words that are zero where it lands
inline void gn_packed_put(uint64_t* words, uint32_t e, uint32_t width, uint64_t delta)
{
    const uint32_t bit = e * width, w = bit >> 6, off = bit & 63u;
    words[w] |= delta << off;
    if (off + width > 64)
        words[w + 1] |= delta >> (64u - off);
}

// The host encoder: the set v[0 .. n), strictly ascending, appended to `blocks` and `payload`; word_at counts from word_base +
// the words `payload` held before the call less `payload_base` (so a set can be appended to an arena whose earlier words are elsewhere:
// give word_base = the arena's length and payload_base = payload.size()).
inline void gn_packed_encode(const uint64_t* v, uint64_t n, std::vector<GnPackedBlock>& blocks, std::vector<uint64_t>& payload, uint64_t word_base = 0,
                             uint64_t payload_base = 0)
{
    for (uint64_t at = 0; at < n; at += GN_WIN_ITEM)
    {
        const uint32_t cnt = (uint32_t)(n - at < GN_WIN_ITEM ? n - at : GN_WIN_ITEM);
        uint64_t       widest = 0;
        for (uint32_t i = 1; i < cnt; ++i)
            widest |= v[at + i] - v[at + i - 1]; // (the OR has the bit length of the largest)
        const uint32_t width = gn_packed_bits(widest), words = gn_packed_words(cnt, width);
        const uint64_t here  = payload.size();
        blocks.push_back(GnPackedBlock{ v[at], word_base + (here - payload_base), cnt, width });
        payload.resize(here + words, 0);
        for (uint32_t i = 1; i < cnt; ++i)
            if (width)
                gn_packed_put(payload.data() + here, i - 1, width, v[at + i] - v[at + i - 1]);
    }
}

// The host decoder: the hashes of blocks[0 .. n_blocks), whose word_at count from payload[0], appended to `out`.
inline void gn_packed_decode(const GnPackedBlock* blocks, uint64_t n_blocks, const uint64_t* payload, std::vector<uint64_t>& out)
{
    for (uint64_t b = 0; b < n_blocks; ++b)
    {
        uint64_t v = blocks[b].first;
        out.push_back(v);
        for (uint32_t i = 1; i < blocks[b].cnt; ++i)
            out.push_back(v += gn_packed_delta(payload + blocks[b].word_at, i - 1, blocks[b].width));
    }
}

// where the next chunk starts: block `block` of run `run`, whose first hash is hash `at` of the run
struct GnPackedCursor
{
    uint32_t run   = 0;
    uint64_t block = 0, at = 0;
};

// The items of the next staging chunk: blocks from the cursor on, runs in order, at most cap_words payload words and at most cap_items
// items (cap_words >= GN_PACKED_MAX_WORDS, so that every block fits an empty chunk; cap_items >= 1).  An item is a whole block: none is
// split.  Returns the items taken -- 0 when the cursor is behind the last run -- with their payload words in *words, and leaves the
// cursor behind them.
inline uint64_t gn_packed_next_chunk(const GnPackedBlock* const* blocks, const uint64_t* n_blocks, uint32_t n_runs, GnPackedCursor& cur, uint64_t cap_words,
                                     uint64_t cap_items, std::vector<GnPackedItem>& items, uint64_t* words)
{
    items.clear();
    uint64_t taken = 0;
    while (cur.run < n_runs && items.size() < cap_items)
    {
        if (cur.block == n_blocks[cur.run])
        {
            ++cur.run, cur.block = 0, cur.at = 0;
            continue;
        }
        const GnPackedBlock& b = blocks[cur.run][cur.block];
        const uint32_t       w = gn_packed_words(b.cnt, b.width);
        if (w > cap_words - taken)
            break;
        items.push_back(GnPackedItem{ cur.run, b.cnt, b.width, 0, b.first, cur.at, taken, cur.block });
        taken += w;
        cur.at += b.cnt;
        ++cur.block;
    }
    *words = taken;
    return items.size();
}
