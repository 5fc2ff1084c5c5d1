// gn_fold_table.h -- the bit arithmetic of gn_filter_fold_ibf: groups of bins of a source row ORed into one bit each of a destination row
// (`ganon-build --hibf --update --fold`: the merged bin a build would have put above a group of bins is the row-wise OR of their columns).
// No device call in here: the checks and the table builder are host code, the hits of a source word and the composition of a
// destination word compile for the host and for the device, so that a CPU program (tests/hibf_fold_driver.cpp) runs the very code the
// kernel runs.
//
// The members become a table over the SOURCE's words: word w has the SEGMENTS seg[seg_off[w] .. seg_off[w + 1]), each a group and the
// 64-bit mask of that group's bins in the word.  Group g HITS in a row when (word & mask) != 0 for one of its segments.  The hits of a
// row are kept as a bit array of 32-bit words, bit g of it for group g (32 bits: what an LDS OR without a return takes); bit
// dst_first + g of the destination row is ORed with bit g of the hits.
// What can go wrong, and where it is handled:
//   a shift by 64     a member that covers a whole word has the mask ~0, not (1 << 64) - 1 (gn_fold_mask); a destination word takes
//                     its 64 hits from three neighbouring hit words shifted by r and by 64 - r with r in 1 .. 31, r == 0 apart
//   hits before 0     the first destination word starts dst_first % 64 bits BEFORE group 0: hit words below 0 and at or beyond the
//                     array's length read as zero (gn_fold_word), so the bits of the word below dst_first and behind the last group stay
//   padding bins      a member lies inside the source's bins (gn_fold_check), so no mask names a padding bin of the last word, and no
//                     word at or beyond the source's words has a segment: such words are never read
//   two members of a group in one word   are one segment (their masks ORed): a word has at most one segment per run of one group
#pragma once

#include "../../include/ganon_hip.h"

#include <stdint.h>

#if defined(__HIPCC__)
#define GN_FOLD_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define GN_FOLD_HD inline
#endif

struct GnFoldSeg // 16 bytes: one load
{
    uint64_t mask;  // the group's bins in this source word
    uint32_t group; // < n_groups
    uint32_t reserved;
};

GN_FOLD_HD uint64_t gn_fold_mask(uint32_t first, uint32_t len) // bits [first, first + len) of a word: len 1 .. 64, first + len <= 64
{
    return (len >= 64u ? ~0ull : (1ull << len) - 1ull) << first;
}

// 32-bit words of a row's hits
GN_FOLD_HD uint32_t gn_fold_hit_words(uint32_t n_groups)
{
    return (n_groups + 31u) >> 5;
}

// hit word i of a row, zero outside the array
GN_FOLD_HD uint32_t gn_fold_hits_at(const uint32_t* hits, uint32_t hit_words, int64_t i)
{
    return i >= 0 && i < (int64_t)hit_words ? hits[i] : 0u;
}

// Destination word `word` of a row, as far as the groups reach into it: bit p of it is the hit of group word * 64 + p - dst_first.
// hits[0 .. hit_words) hold no bit at or beyond n_groups, so every bit of the result outside [dst_first, dst_first + n_groups) is zero.
GN_FOLD_HD uint64_t gn_fold_word(const uint32_t* hits, uint32_t hit_words, uint32_t word, uint32_t dst_first)
{
    const int64_t  s = (int64_t)word * 64 - (int64_t)dst_first; // the hit that bit 0 of the word takes; below 0 in the first word
    const int64_t  q = s >> 5;                                   // (floor: >> of a negative number is arithmetic on every compiler used here)
    const uint32_t r = (uint32_t)(s & 31);
    const uint64_t lo = (uint64_t)gn_fold_hits_at(hits, hit_words, q) | (uint64_t)gn_fold_hits_at(hits, hit_words, q + 1) << 32;
    return r ? (lo >> r | (uint64_t)gn_fold_hits_at(hits, hit_words, q + 2) << (64u - r)) : lo;
}

#include <vector>

// nullptr when the members are what gn_filter_fold_ibf takes for a source of bins_src bins and a destination of bins_dst, else why not
// (*at: the member the answer speaks of, n_members where it speaks of none)
inline const char* gn_fold_check(const gn_fold_member* members, uint32_t n_members, uint32_t n_groups, uint32_t dst_first, uint64_t bins_src, uint64_t bins_dst,
                                 uint32_t* at)
{
    if (at)
        *at = n_members;
    if ((uint64_t)dst_first + n_groups > bins_dst)
        return "the groups' bins are beyond the destination's bins";
    std::vector<bool> has(n_groups, false);
    uint64_t          src_end = 0; // of the members so far
    for (uint32_t i = 0; i < n_members; ++i)
    {
        const gn_fold_member& m = members[i];
        if (at)
            *at = i;
        if (m.n_bins == 0)
            return "a member of 0 bins";
        if ((uint64_t)m.src_first + m.n_bins > bins_src)
            return "a member beyond the source's bins";
        if (m.src_first < src_end)
            return "members that overlap or do not ascend";
        if (m.group >= n_groups)
            return "a group at or beyond the number of groups";
        src_end      = (uint64_t)m.src_first + m.n_bins;
        has[m.group] = true;
    }
    if (at)
        *at = n_members;
    for (uint32_t g = 0; g < n_groups; ++g)
        if (!has[g])
            return "a group without a member";
    return nullptr;
}

// The table over words [0, words_src) of the source: seg_off gets words_src + 1 entries.  The members have passed gn_fold_check, and
// words_src * 64 is at least the source's bins.
inline void gn_fold_table(const gn_fold_member* members, uint32_t n_members, uint64_t words_src, std::vector<uint32_t>& seg_off, std::vector<GnFoldSeg>& segs)
{
    seg_off.assign(words_src + 1, 0);
    segs.clear();
    uint64_t last = ~0ull; // the word of the last segment
    for (uint32_t i = 0; i < n_members; ++i)
        for (uint64_t b = members[i].src_first, end = b + members[i].n_bins; b < end;)
        {
            const uint64_t w = b >> 6, stop = end < (w + 1) * 64 ? end : (w + 1) * 64;
            const uint64_t mask = gn_fold_mask((uint32_t)(b & 63), (uint32_t)(stop - b));
            if (last == w && segs.back().group == members[i].group)
                segs.back().mask |= mask;
            else
            {
                segs.push_back(GnFoldSeg{ mask, members[i].group, 0 });
                ++seg_off[w + 1];
            }
            last = w;
            b    = stop;
        }
    for (uint64_t w = 0; w < words_src; ++w) // (ascending members: the segments are in word order already)
        seg_off[w + 1] += seg_off[w];
}

// One row on the host, as the kernel composes it: the hits of the row's words, then every destination word the groups reach.
// `hits` is scratch of gn_fold_hit_words(n_groups) words.
inline void gn_fold_row(uint64_t* dst_row, const uint64_t* src_row, uint64_t words_src, const uint32_t* seg_off, const GnFoldSeg* segs, uint32_t n_groups,
                        uint32_t dst_first, uint32_t* hits)
{
    if (n_groups == 0)
        return;
    const uint32_t hw = gn_fold_hit_words(n_groups);
    for (uint32_t k = 0; k < hw; ++k)
        hits[k] = 0;
    for (uint64_t w = 0; w < words_src; ++w)
        for (uint32_t k = seg_off[w]; k < seg_off[w + 1]; ++k)
            if (src_row[w] & segs[k].mask)
                hits[segs[k].group >> 5] |= 1u << (segs[k].group & 31u);
    for (uint32_t w = dst_first >> 6; w <= (dst_first + n_groups - 1) >> 6; ++w)
        dst_row[w] |= gn_fold_word(hits, hw, w, dst_first);
}
