// gn_bin_spans.h -- the bit arithmetic of gn_filter_copy_ibf_spans: a row of an IBF rewritten with some runs of bins left out (or moved).
// No device call in here: the checks and the table builder are host code, the composition of a destination word compiles for the host
// and for the device, so that a CPU program (tests/hibf_remove_driver.cpp) runs the very code the kernel runs.
//
// The spans become a table over the destination's words: word w is the OR of its SEGMENTS seg[seg_off[w] .. seg_off[w + 1]), each
// `len` bits of the source row from bit 64 * src_word + sh on, put at bit dst_off of the word.  A word no span reaches has no segment
// and is zero; so is every bit of a word that no segment covers (the padding bins of the last word among them).  A destination word is
// composed from ALL of its segments by whoever owns it and stored once: two spans that end in one word are two segments of that one
// word, never two writers.
// What can go wrong, and where it is handled:
//   a shift by 64     a whole word is len == 64, whose mask is not (1 << 64) - 1 (gn_span_mask); the upper part of a window is shifted
//                     by 1 and by 63 - sh, never by 64 - sh (gn_span_bits)
//   the second word   of a window is word src_word + 1 only when the window reaches into it (sh + len > 64); otherwise the first word is
//                     loaded twice, so that the two loads need no branch between them.  The builder has checked that the span lies
//                     inside the source's bins, so a word the window reaches into is below W_src: nothing at or beyond W_src is ever
//                     read -- such words are not trusted, and behind the last row of an unpadded source they are not there
//   the row offset    is the caller's: row * stride in 64 bits
//   a narrower destination   the table is over the DESTINATION's words; source words no span names are not read at all
#pragma once

#include "../../include/ganon_hip.h"

#include <stdint.h>

#if defined(__HIPCC__)
#define GN_SPAN_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define GN_SPAN_HD inline
#endif

struct GnSpanSeg // 8 bytes: one load
{
    uint32_t src_word; // first source word of the window
    uint8_t  sh;       // the window starts at this bit of it (0 .. 63)
    uint8_t  dst_off;  // and goes to this bit of the destination word (0 .. 63)
    uint8_t  len;      // 1 .. 64 bits, dst_off + len <= 64
    uint8_t  reserved;
};

GN_SPAN_HD uint64_t gn_span_mask(uint32_t len) // len 0 .. 64
{
    return len >= 64u ? ~0ull : (1ull << len) - 1ull;
}

// 1 when the segment's window reaches into the word behind src_word, which is then below W_src; 0 when src_word holds all of it
GN_SPAN_HD uint32_t gn_span_second(const GnSpanSeg s)
{
    return (uint32_t)s.sh + s.len > 64u ? 1u : 0u;
}

// the segment's bits at bit 0, from lo = word src_word and hi = word src_word + gn_span_second(s) of the source row.  Without a second
// word hi is lo again and is dropped; (hi << 1) << (63 - sh) is hi << (64 - sh) without a shift by 64 at sh == 0.
GN_SPAN_HD uint64_t gn_span_bits(uint64_t lo, uint64_t hi, const GnSpanSeg s)
{
    const uint64_t upper = gn_span_second(s) ? (hi << 1) << (63u - s.sh) : 0ull;
    return (lo >> s.sh | upper) & gn_span_mask(s.len);
}

// the same from the row: the two loads are independent of each other, and neither is at or beyond W_src
GN_SPAN_HD uint64_t gn_span_window(const uint64_t* row, const GnSpanSeg s)
{
    return gn_span_bits(row[s.src_word], row[s.src_word + gn_span_second(s)], s);
}

GN_SPAN_HD uint64_t gn_span_compose(const uint64_t* row, const GnSpanSeg* segs, uint32_t n)
{
    uint64_t v = 0;
    for (uint32_t k = 0; k < n; ++k)
        v |= gn_span_window(row, segs[k]) << segs[k].dst_off;
    return v;
}

// a destination word that is one whole aligned source word: a plain move
GN_SPAN_HD bool gn_span_is_move(const GnSpanSeg s)
{
    return s.sh == 0 && s.dst_off == 0 && s.len == 64;
}

#include <vector>

// nullptr when the spans are what gn_filter_copy_ibf_spans takes for a source of bins_src and a destination of bins_dst bins, else why not
inline const char* gn_spans_check(const gn_bin_span* spans, uint32_t n_spans, uint64_t bins_src, uint64_t bins_dst, uint32_t* at)
{
    uint64_t dst_end = 0; // of the spans so far
    for (uint32_t i = 0; i < n_spans; ++i)
    {
        const gn_bin_span& s = spans[i];
        if (at)
            *at = i;
        if (s.n_bins == 0)
            return "a span of 0 bins";
        if ((uint64_t)s.src_first + s.n_bins > bins_src)
            return "a span beyond the source's bins";
        if ((uint64_t)s.dst_first + s.n_bins > bins_dst)
            return "a span beyond the destination's bins";
        if (s.dst_first < dst_end)
            return "destination spans that overlap or do not ascend";
        dst_end = (uint64_t)s.dst_first + s.n_bins;
    }
    return nullptr;
}

// The table over words [0, words_dst) of the destination: seg_off gets words_dst + 1 entries.  The spans have passed gn_spans_check, and
// words_dst * 64 is at least the destination's bins.
inline void gn_spans_table(const gn_bin_span* spans, uint32_t n_spans, uint64_t words_dst, std::vector<uint32_t>& seg_off, std::vector<GnSpanSeg>& segs)
{
    seg_off.assign(words_dst + 1, 0);
    segs.clear();
    for (uint32_t i = 0; i < n_spans; ++i)
        for (uint64_t d = spans[i].dst_first, end = d + spans[i].n_bins; d < end;)
        {
            const uint64_t w = d >> 6, stop = end < (w + 1) * 64 ? end : (w + 1) * 64, s = spans[i].src_first + (d - spans[i].dst_first);
            segs.push_back(GnSpanSeg{ (uint32_t)(s >> 6), (uint8_t)(s & 63), (uint8_t)(d & 63), (uint8_t)(stop - d), 0 });
            ++seg_off[w + 1];
            d = stop;
        }
    for (uint64_t w = 0; w < words_dst; ++w) // (ascending destinations: the segments are in word order already)
        seg_off[w + 1] += seg_off[w];
}
