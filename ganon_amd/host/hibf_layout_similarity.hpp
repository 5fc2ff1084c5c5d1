// hibf_layout_similarity.hpp -- the tree of `ganon-build --hibf --layout similarity`: the search of hibf_layout_sketch.hpp over an
// order in which related user bins are neighbours.  Host only: no device, no I/O.  A merged bin is a contiguous slice of the order,
// and a merged bin over relatives holds little more than one of them, so what the order puts side by side decides how large the
// lower levels come out.  chopper rearranges user bins by sketch similarity before it lays them out; this is that step, with the
// caller's estimates of the union of two user bins (the builder: gn_sketches_pair_table; a test: exact unions).
//
// The order.  The size order (sketch_order: count descending, index ascending) is cut into intervals: one starts at position a and
// goes on while 2 * count >= the count at a (chopper's rearrangement ratio of one half) and it has fewer than kSimilarityWindow
// positions.  User bins never leave their interval, so the order stays sorted by size up to a factor of two, which is what the
// search's runs and merged bins rely on to waste little.  Inside an interval a nearest-neighbour chain:
//   1. the first member, the largest, stays first;
//   2. with `last` the member placed most recently, an unplaced member c shares  shared = count(last) + count(c) - U(last, c);
//   3. c is a candidate when shared > 0 and 8 * shared >= min(count(last), count(c)) -- an eighth of the smaller set is about four
//      standard errors (1.04 / sqrt(4096) each) of a 4096-register sketch of two strangers' union, which is about twice that set;
//   4. the candidate with the largest (count(last) + count(c)) / U(last, c) comes next (compared by cross-multiplication in 128-bit
//      integers; ties: the earlier position of the size order);
//   5. with no candidate, the unplaced member that is first in the size order comes next: strangers keep their size order, but
//      for the few pairs of them whose estimate is four standard errors low (about one pair in 16 000).
// The counts are exact, only U is an estimate.  No floating point, no hash container: the same input gives the same order.
//
// The layout.  lay_out_sketch in the size order, as `--layout sketch` gives it (the rule's tree costed in that order and kept when
// smaller); when the similarity order differs, the search over it (lay_out_order) with union estimates of that order; the second is
// kept only when its estimated bits, plus one part in kSimilarityMargin of them, are below the first's.  The margin is one standard
// error of a sketch (1.04 / sqrt(4096), about 1 / 64): among the half a million pairs of an interval of 1024 strangers a few dozen pass
// the threshold of step 3 by chance, the two searches then run over different estimates, and which of them comes out a fraction of a
// per cent lower says nothing about the bytes written.  A gain the estimates cannot tell from their own error is not taken; relatives
// gain tens of per cent.  So by the estimates `similarity` is never larger than `sketch`; where nothing moves (always with exact
// unions of strangers) it is `sketch`; where only chance moved strangers it is `sketch` unless chance also gains more than the
// margin, which a sum over many bins does not; and everything hibf_layout_sketch.hpp promises a reader of the file holds.
#pragma once

#include "hibf_layout_sketch.hpp"

namespace gnhibf
{

constexpr uint64_t kSimilarityWindow = 1024; // positions of one interval: a pair table of at most 2^20 entries
constexpr uint64_t kSimilarityMargin = 64;   // the similarity tree is kept when it is estimated lower by more than 1 / 64: one standard error

// U(p, q): estimated cardinality of the union of the user bins at positions p and q of ONE interval (both below its length)
using PairEstimate = std::function<uint64_t(uint64_t p, uint64_t q)>;
// pairs(a, b): the estimates of the interval [a, b) of the size order.  Asked once per interval of three members and more, in
// ascending order of a; what it returns is let go before the next interval is asked for.
using IntervalPairs = std::function<PairEstimate(uint64_t a, uint64_t b)>;
// unions(order): the UnionEstimate (hibf_layout_sketch.hpp) over the positions of `order`; let go before the next is asked for
using OrderUnions = std::function<UnionEstimate(const std::vector<uint32_t>& order)>;

// where the intervals of the size order start, and n at the end
inline std::vector<uint64_t> similarity_intervals(const std::vector<uint64_t>& counts, const std::vector<uint32_t>& size_order)
{
    std::vector<uint64_t> starts;
    const uint64_t        n = size_order.size();
    for (uint64_t a = 0; a < n;)
    {
        starts.push_back(a);
        uint64_t b = a + 1;
        while (b < n && b - a < kSimilarityWindow && 2 * counts[size_order[b]] >= counts[size_order[a]])
            ++b;
        a = b;
    }
    starts.push_back(n);
    return starts;
}

// a permutation of size_order: see the head of this file
inline std::vector<uint32_t> similarity_order(const std::vector<uint64_t>& counts, const std::vector<uint32_t>& size_order, const IntervalPairs& pairs)
{
    typedef unsigned __int128   u128;
    std::vector<uint32_t>       out;
    const std::vector<uint64_t> starts = similarity_intervals(counts, size_order);
    out.reserve(size_order.size());
    for (size_t i = 0; i + 1 < starts.size(); ++i)
    {
        const uint64_t a = starts[i], len = starts[i + 1] - a;
        if (len < 3) // (the first stays, a second has nowhere else to go)
        {
            out.insert(out.end(), size_order.begin() + a, size_order.begin() + a + len);
            continue;
        }
        const PairEstimate U = pairs(a, a + len);
        std::vector<char>  placed(len, 0);
        uint64_t           last = 0;
        placed[0]               = 1;
        out.push_back(size_order[a]);
        for (uint64_t step = 1; step < len; ++step)
        {
            const uint64_t c_last = counts[size_order[a + last]];
            uint64_t       best = len, first = len, best_sum = 0, best_u = 0;
            for (uint64_t p = 0; p < len; ++p)
            {
                if (placed[p])
                    continue;
                if (first == len)
                    first = p;
                const uint64_t c = counts[size_order[a + p]], sum = c_last + c, u = U(last, p);
                if (u >= sum || (u128)8 * (sum - u) < std::min(c_last, c))
                    continue;
                if (best == len || (u128)sum * best_u > (u128)best_sum * u) // sum / u > best_sum / best_u
                    best = p, best_sum = sum, best_u = u;
            }
            last         = best != len ? best : first;
            placed[last] = 1;
            out.push_back(size_order[a + last]);
        }
    }
    return out;
}

struct SimilarityLayout
{
    Layout      layout;
    uint64_t    intervals = 0, moved = 0; // intervals of the size order; user bins whose position is not the size order's
    uint64_t    bits      = 0;            // of `layout`, by the estimates of the order it was searched in
    const char* kept      = "sketch";     // "sketch" | "similarity" | "rule": the tree `layout` is
};

// counts, tmax, max_fp, hash_functions as lay_out_sketch takes them.  One IBF (sketch_width 1): nothing is asked for.
inline SimilarityLayout lay_out_similarity(const std::vector<uint64_t>& counts, uint32_t tmax, double max_fp, uint8_t hash_functions,
                                           const OrderUnions& unions, const IntervalPairs& pairs)
{
    SimilarityLayout out;
    if (counts.empty() || tmax < 2)
        return out;
    const std::vector<uint32_t> size_order = sketch_order(counts);
    out.intervals                          = similarity_intervals(counts, size_order).size() - 1;
    if (sketch_width(counts.size(), tmax) < 2)
    {
        out.layout = lay_out_sketch(counts, tmax, max_fp, hash_functions, [](uint64_t, uint64_t) -> uint64_t { return 0; });
        return out;
    }
    {
        bool                kept_rule = false;
        const UnionEstimate by_size   = unions(size_order);
        out.layout                    = lay_out_sketch_costed(counts, tmax, max_fp, hash_functions, by_size, &out.bits, &kept_rule);
        out.kept                      = kept_rule ? "rule" : "sketch";
    }
    const std::vector<uint32_t> order = similarity_order(counts, size_order, pairs);
    for (uint64_t j = 0; j < order.size(); ++j)
        out.moved += order[j] != size_order[j];
    if (out.moved == 0)
        return out;
    uint64_t            bits     = 0;
    const UnionEstimate by_order = unions(order);
    Layout              similar  = lay_out_order(counts, order, tmax, max_fp, hash_functions, by_order, &bits);
    if (bits + bits / kSimilarityMargin < out.bits)
    {
        out.layout = std::move(similar);
        out.bits   = bits;
        out.kept   = "similarity";
    }
    return out;
}

} // namespace gnhibf
