// hibf_layout_sketch.hpp -- the tree of `ganon-build --hibf --layout sketch`: the same gnhibf::Layout as hibf_layout.hpp gives, chosen
// by size.  Host only: no device, no I/O.  The caller says how large the union of neighbouring user bins is -- the builder from
// HyperLogLog sketches (gn_sketches_union_table), a test with exact sums -- and the search balances split and merged bins on it, as
// chopper does for `raptor layout` (/root/reference/src/ganon/build_update.py:411-518).  Not taken over from chopper: the weight of
// the query cost, its layout files.  (Its rearrangement of user bins by similarity is `--layout similarity`, hibf_layout_similarity.hpp:
// the same search over another order.)
//
// User bins are sorted once by (count descending, index ascending); every IBF's members are a contiguous slice [a, b) of that order.
// An IBF has a level budget Lb: the root's is levels_for(n, tmax), a child's its parent's minus one; cap = tmax^(Lb - 1) is the most
// user bins one of its merged bins may hold (Lb == 1: nothing is merged).  For a number of rows x, plan(x) walks j from a:
//   1. l = the largest length <= min(cap, b - j) whose union, as the caller estimates it, fits x rows as one bin
//      (hibf_run_bits(estimate, 1) <= x);
//   2. l >= 2: one merged bin over [j, j + l);
//   3. otherwise user bin j gets a run of s bins, s the least number with hibf_run_bits(count_j, s) <= x (its count is exact).
// A plan is feasible when it needs at most tmax bins.  The IBF works at the least feasible x (bisection between 1 and an x at which
// every step reaches min(cap, b - j), which needs ceil((b - a) / cap) <= tmax bins).  At that x it keeps every user bin it can pay
// for in a run of its own and merges, as plan(x) does, only where the bins would run out otherwise (settle() below): a merged bin
// costs a child IBF, a run in this IBF nothing more at the same x.  The merged bins are laid out the same way.
// Each IBF is settled on its own, top down, so on deep trees (a small tmax) the sum over the levels can come out above the rule's;
// the rule's tree (hibf_layout.hpp: its IBFs hold contiguous slices of the same order too) is therefore costed with the same
// estimates and kept when it is strictly smaller.  Everything hibf_layout.hpp promises a reader of the file holds here too: every user bin is one run of consecutive bins
// in one IBF; a bin is merged exactly when it has a child; the children form a tree rooted at IBF 0 that reaches every IBF; no IBF
// has more than tmax bins; the depth is at most levels_for(n, tmax); the same input gives the same tree.
// The estimates choose the tree and nothing else: the builder sizes every IBF from exact unions afterwards, so an estimate that is
// off costs size, never a false negative or the --max-fp bound.
#pragma once

#include "build_params.hpp"
#include "hibf_layout.hpp"

#include <functional>

namespace gnhibf
{

// estimate(j, l): cardinality of the union of the user bins at positions j .. j + l - 1 of the sorted order; asked for
// 2 <= l <= min(sketch_width(n, tmax), n - j) only, and expected not to fall as l grows
using UnionEstimate = std::function<uint64_t(uint64_t j, uint64_t l)>;

// the longest union the search asks for: the root's cap, at most n (1: no estimate is asked for, the tree is one IBF)
inline uint64_t sketch_width(uint64_t n, uint64_t tmax)
{
    uint64_t cap = 1;
    levels_for(n, tmax, &cap);
    return std::min(cap, n);
}

namespace detail
{

struct SketchSearch
{
    const std::vector<uint64_t>& counts;
    const std::vector<uint32_t>& order;
    uint32_t                     tmax;
    double                       max_fp;
    uint8_t                      h;
    const UnionEstimate&         estimate;

    struct Piece // l >= 2: a merged bin over positions [j, j + l); l == 1: user bin order[j] in s bins
    {
        uint64_t j, l, s;
    };

    uint64_t rows_merged(uint64_t j, uint64_t l) const { return gnbuild::hibf_run_bits(estimate(j, l), 1, max_fp, h); }
    uint64_t rows_split(uint64_t j, uint64_t s) const { return gnbuild::hibf_run_bits(counts[order[j]], s, max_fp, h); }

    bool plan(uint64_t a, uint64_t b, uint64_t cap, uint64_t x, std::vector<Piece>* pieces) const
    {
        uint64_t bins = 0;
        for (uint64_t j = a; j < b;)
        {
            const uint64_t most = std::min(cap, b - j);
            uint64_t       l    = 1;
            if (most >= 2 && rows_merged(j, 2) <= x)
            {
                uint64_t lo = 2, hi = most;
                while (lo < hi)
                {
                    const uint64_t mid = (lo + hi + 1) / 2;
                    if (rows_merged(j, mid) <= x)
                        lo = mid;
                    else
                        hi = mid - 1;
                }
                l = lo;
            }
            uint64_t s = 1;
            if (l == 1)
            {
                while (bins + s <= tmax && rows_split(j, s) > x)
                    ++s;
            }
            bins += s;
            if (bins > tmax)
                return false;
            if (pieces)
                pieces->push_back(Piece{ j, l, s });
            j += l;
        }
        return true;
    }

    // The plan the IBF takes at its least feasible x.  plan(x) merges wherever it can, which is what needs the fewest bins; a merged
    // bin costs a child IBF, though, and a user bin that stays in this IBF costs nothing more at the same x.  So with need[j] = the
    // bins plan(x) takes from position j on, user bin j keeps a run of its own whenever the bins left pay for it and for need[j + 1];
    // only then is it merged with its neighbours as plan(x) does.  The merged bins end up where the small user bins are.
    std::vector<Piece> settle(uint64_t a, uint64_t b, uint64_t cap, uint64_t x) const
    {
        const uint64_t        n = b - a, never = (uint64_t)tmax + 1;
        std::vector<uint64_t> reach(n, 1), split(n, never), need(n + 1, 0);
        for (uint64_t i = n; i-- > 0;)
        {
            const uint64_t j = a + i, most = std::min(cap, b - j);
            if (most >= 2 && rows_merged(j, 2) <= x)
            {
                uint64_t lo = 2, hi = most;
                while (lo < hi)
                {
                    const uint64_t mid = (lo + hi + 1) / 2;
                    if (rows_merged(j, mid) <= x)
                        lo = mid;
                    else
                        hi = mid - 1;
                }
                reach[i] = lo;
            }
            for (uint64_t s = 1; s <= tmax; ++s)
                if (rows_split(j, s) <= x)
                {
                    split[i] = s;
                    break;
                }
            need[i] = std::min(never, reach[i] >= 2 ? 1 + need[i + reach[i]] : split[i] + need[i + 1]);
        }
        std::vector<Piece> pieces;
        uint64_t           left = tmax;
        for (uint64_t i = 0; i < n;)
        {
            if (split[i] + need[i + 1] <= left)
            {
                pieces.push_back(Piece{ a + i, 1, split[i] });
                left -= split[i];
                i += 1;
            }
            else // (need[i] <= left all along: reach[i] >= 2 here, and the rest fits behind the merged bin)
            {
                pieces.push_back(Piece{ a + i, reach[i], 1 });
                left -= 1;
                i += reach[i];
            }
        }
        return pieces;
    }

    // what the builder would allocate for a tree whose IBFs hold contiguous slices of the order, by the same estimates:
    // rows of every IBF (the largest need of its runs) times its bins rounded up to whole 64-bit words
    uint64_t bits(const Layout& l) const
    {
        std::vector<uint64_t> at(order.size());
        for (uint64_t j = 0; j < order.size(); ++j)
            at[order[j]] = j;
        uint64_t total = 0;
        for (const Ibf& f : l.ibfs)
        {
            uint64_t rows = 0;
            for (const Run& r : f.runs)
            {
                const std::vector<uint32_t>* below = r.user < 0 ? &l.ibfs[r.child].members : nullptr;
                rows = std::max(rows, below ? rows_merged(at[below->front()], below->size()) : rows_split(at[r.user], r.n_bins));
            }
            total += rows * ((f.bins + 63) / 64 * 64);
        }
        return total;
    }

    uint32_t lay(Layout& out, uint64_t a, uint64_t b, uint32_t budget, int64_t parent, uint32_t parent_bin, uint32_t depth) const
    {
        const uint32_t idx = (uint32_t)out.ibfs.size();
        out.ibfs.emplace_back();
        out.levels = std::max(out.levels, depth + 1);
        uint64_t cap = 1;
        for (uint32_t i = 1; i < budget; ++i)
            cap = cap > (~0ull) / tmax ? ~0ull : cap * tmax;
        uint64_t hi = 1; // every step of plan(hi) reaches as far as cap lets it
        for (uint64_t j = a; j < b; ++j)
        {
            const uint64_t most = std::min(cap, b - j);
            hi                  = std::max(hi, most >= 2 ? rows_merged(j, most) : rows_split(j, 1));
        }
        uint64_t lo = 1;
        while (lo < hi)
        {
            const uint64_t mid = lo + (hi - lo) / 2;
            if (plan(a, b, cap, mid, nullptr))
                hi = mid;
            else
                lo = mid + 1;
        }
        const std::vector<Piece> pieces = settle(a, b, cap, hi);
        std::vector<Run> runs;
        uint32_t         first = 0;
        for (const Piece& p : pieces)
        {
            runs.push_back(p.l >= 2 ? Run{ first, 1, -1, -1 } : Run{ first, (uint32_t)p.s, (int64_t)order[p.j], -1 });
            first += (uint32_t)p.s;
        }
        for (size_t i = 0; i < pieces.size(); ++i)
            if (pieces[i].l >= 2)
                runs[i].child = lay(out, pieces[i].j, pieces[i].j + pieces[i].l, budget - 1, idx, runs[i].first, depth + 1);
        Ibf& me       = out.ibfs[idx];
        me.parent     = parent;
        me.parent_bin = parent_bin;
        me.depth      = depth;
        me.bins       = first;
        me.runs       = std::move(runs);
        me.members.assign(order.begin() + a, order.begin() + b);
        return idx;
    }
};

} // namespace detail

// the order the estimates refer to: user bins by (count descending, index ascending)
inline std::vector<uint32_t> sketch_order(const std::vector<uint64_t>& counts)
{
    std::vector<uint32_t> order(counts.size());
    for (uint32_t i = 0; i < order.size(); ++i)
        order[i] = i;
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return counts[a] > counts[b]; });
    return order;
}

// The search over a given order -- any permutation of the user bins, `estimate` speaking of its positions -- with no comparison
// against the rule: the tree and, in *bits, what the estimates say it takes.  counts, tmax, max_fp, hash_functions as below.
inline Layout lay_out_order(const std::vector<uint64_t>& counts, const std::vector<uint32_t>& order, uint32_t tmax, double max_fp, uint8_t hash_functions,
                            const UnionEstimate& estimate, uint64_t* bits)
{
    Layout out;
    *bits = 0;
    if (counts.empty() || tmax < 2)
        return out;
    const detail::SketchSearch search{ counts, order, tmax, max_fp, hash_functions, estimate };
    search.lay(out, 0, counts.size(), levels_for(counts.size(), tmax), -1, 0, 0);
    *bits = search.bits(out);
    return out;
}

// lay_out_sketch below, which also says what it kept: *bits = the estimated bits of the tree returned, *kept_rule = it is the rule's
inline Layout lay_out_sketch_costed(const std::vector<uint64_t>& counts, uint32_t tmax, double max_fp, uint8_t hash_functions, const UnionEstimate& estimate,
                                    uint64_t* bits, bool* kept_rule)
{
    Layout out;
    *bits      = 0;
    *kept_rule = false;
    if (counts.empty() || tmax < 2)
        return out;
    const std::vector<uint32_t> order = sketch_order(counts);
    const detail::SketchSearch  search{ counts, order, tmax, max_fp, hash_functions, estimate };
    search.lay(out, 0, counts.size(), levels_for(counts.size(), tmax), -1, 0, 0);
    *bits = search.bits(out);
    Layout                     rule      = lay_out(counts, tmax);
    const uint64_t             rule_bits = search.bits(rule);
    if (rule_bits < *bits)
    {
        *bits      = rule_bits;
        *kept_rule = true;
        return rule;
    }
    return out;
}

// counts[u] = distinct hashes of user bin u (all > 0), tmax >= 2, max_fp and hash_functions as the IBFs will be sized with.
// No user bin: an empty layout.
inline Layout lay_out_sketch(const std::vector<uint64_t>& counts, uint32_t tmax, double max_fp, uint8_t hash_functions, const UnionEstimate& estimate)
{
    uint64_t bits      = 0;
    bool     kept_rule = false;
    return lay_out_sketch_costed(counts, tmax, max_fp, hash_functions, estimate, &bits, &kept_rule);
}

} // namespace gnhibf
