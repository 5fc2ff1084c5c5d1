// hibf_layout.hpp -- which technical bin of which IBF a user bin of `ganon-build --hibf` goes to.  Host only: no device, no I/O.
//
// raptor gets this tree from chopper's dynamic programme over HyperLogLog sketches (/root/reference/src/ganon/build_update.py:
// 411-518 calls `raptor layout`); that stays out of scope.  The rule here is deterministic and needs the user bins' distinct-hash
// counts only:
//   * user bins sorted by (count descending, index ascending);
//   * at most tmax of them: a LEAF IBF.  Bins = their number rounded up to a multiple of 64, capped at tmax; the spare bins go
//     one at a time to the user bin whose share ceil(n / s) is largest (ties: lower user bin index) while that share is above 1
//     -- a split user bin of s consecutive bins, hash i of its ascending set in bin first + i / ceil(n / s)
//     (gn_filter_emplace_split's rule).  Spare bins nobody can use are dropped: every bin of the tree belongs to a run;
//   * more than tmax: tmax bins.  With L the smallest integer with tmax^L >= n and cap = tmax^(L-1), m is the smallest number of
//     merged bins with (tmax - m) + m * cap >= n.  The tmax - m largest user bins keep a bin of their own, the others are cut, in
//     sorted order, into m contiguous groups of balanced count sums with at most cap members each.  A group of one is a single
//     bin, every other group a merged bin whose child IBF is the layout of its members (at most cap of them: depth <= L).
// What a reader of the file may rely on: every user bin is one run of consecutive bins in one IBF; a bin is merged exactly when it
// has a child; the children form a tree rooted at IBF 0 that reaches every IBF; no IBF has more than tmax bins; the depth is at
// most L; the same input gives the same tree.
#pragma once

#include <algorithm>
#include <cstdint>
#include <vector>

namespace gnhibf
{

struct Run // the shape the device's run table uses: {first bin, n bins, user bin | -1, child}
{
    uint32_t first = 0, n_bins = 0;
    int64_t  user = -1, child = -1; // a merged bin: user == -1, n_bins == 1, child = index of the IBF below it
};

struct Ibf
{
    std::vector<Run>      runs; // ascending bins, no gaps
    uint32_t              bins = 0;
    int64_t               parent = -1; // IBF above (-1: the root) and the merged bin there that leads here
    uint32_t              parent_bin = 0, depth = 0; // depth 0 = the root
    std::vector<uint32_t> members;     // user bins below, in sorted order
};

struct Layout
{
    std::vector<Ibf> ibfs;
    uint32_t         levels = 0; // deepest IBF's depth + 1
};

// the smallest L >= 1 with tmax^L >= n, and tmax^(L-1) (integer powers; saturates far above any n)
inline uint32_t levels_for(uint64_t n, uint64_t tmax, uint64_t* cap_below = nullptr)
{
    uint32_t L = 1;
    uint64_t p = tmax, below = 1;
    while (p < n)
    {
        below = p;
        p     = p > (~0ull) / tmax ? ~0ull : p * tmax;
        ++L;
    }
    if (cap_below)
        *cap_below = below;
    return L;
}

namespace detail
{

inline uint64_t ceil_div(uint64_t a, uint64_t b)
{
    return (a + b - 1) / b;
}

inline uint32_t lay(Layout& out, const std::vector<uint64_t>& counts, std::vector<uint32_t> members, uint32_t tmax, int64_t parent,
                    uint32_t parent_bin, uint32_t depth)
{
    const uint32_t idx = (uint32_t)out.ibfs.size();
    out.ibfs.emplace_back();
    out.levels = std::max(out.levels, depth + 1);
    const uint64_t n = members.size();
    {
        Ibf& me       = out.ibfs[idx];
        me.parent     = parent;
        me.parent_bin = parent_bin;
        me.depth      = depth;
    }
    std::vector<Run>                                      runs;
    std::vector<std::pair<size_t, std::vector<uint32_t>>> below; // (run, members) of the merged bins
    if (n <= tmax)
    {
        const uint64_t        bins = std::min<uint64_t>((n + 63) / 64 * 64, tmax);
        std::vector<uint64_t> s(n, 1);
        for (uint64_t spare = bins - n; spare; --spare)
        {
            size_t   best  = n;
            uint64_t share = 1;
            for (size_t i = 0; i < n; ++i)
            {
                const uint64_t sh = ceil_div(counts[members[i]], s[i]);
                if (sh > share || (sh == share && best != n && members[i] < members[best]))
                    best = i, share = sh;
            }
            if (best == n) // every share is 1 (or 0): another bin helps nobody
                break;
            ++s[best];
        }
        uint32_t first = 0;
        for (size_t i = 0; i < n; ++i)
        {
            runs.push_back(Run{ first, (uint32_t)s[i], (int64_t)members[i], -1 });
            first += (uint32_t)s[i];
        }
    }
    else
    {
        uint64_t cap = 1;
        levels_for(n, tmax, &cap);
        uint64_t m = 1;
        while ((tmax - m) + m * cap < n)
            ++m;
        const uint64_t singles = tmax - m;
        for (uint64_t i = 0; i < singles; ++i)
            runs.push_back(Run{ (uint32_t)i, 1, (int64_t)members[i], -1 });
        uint64_t rest_sum = 0;
        for (uint64_t i = singles; i < n; ++i)
            rest_sum += counts[members[i]];
        uint64_t at = singles;
        for (uint64_t g = 0; g < m; ++g)
        {
            const uint64_t left = n - at, groups = m - g;
            const uint64_t lo     = std::max<uint64_t>(1, left > (groups - 1) * cap ? left - (groups - 1) * cap : 0);
            const uint64_t hi     = std::min<uint64_t>(cap, left - (groups - 1));
            const uint64_t target = ceil_div(rest_sum, groups);
            uint64_t       take = 0, sum = 0;
            while (take < hi && (take < lo || sum < target))
                sum += counts[members[at + take]], ++take;
            rest_sum -= sum;
            const uint32_t bin = (uint32_t)(singles + g);
            if (take == 1)
                runs.push_back(Run{ bin, 1, (int64_t)members[at], -1 });
            else
            {
                runs.push_back(Run{ bin, 1, -1, -1 });
                below.emplace_back(runs.size() - 1, std::vector<uint32_t>(members.begin() + at, members.begin() + at + take));
            }
            at += take;
        }
    }
    for (auto& b : below)
        runs[b.first].child = lay(out, counts, std::move(b.second), tmax, idx, runs[b.first].first, depth + 1);
    Ibf& me    = out.ibfs[idx];
    me.bins    = runs.empty() ? 0 : runs.back().first + runs.back().n_bins;
    me.runs    = std::move(runs);
    me.members = std::move(members);
    return idx;
}

} // namespace detail

// counts[u] = distinct hashes of user bin u (all > 0), tmax >= 2.  No user bin: an empty layout.
inline Layout lay_out(const std::vector<uint64_t>& counts, uint32_t tmax)
{
    Layout out;
    if (counts.empty() || tmax < 2)
        return out;
    std::vector<uint32_t> order(counts.size());
    for (uint32_t i = 0; i < order.size(); ++i)
        order[i] = i;
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return counts[a] > counts[b]; });
    detail::lay(out, counts, std::move(order), tmax, -1, 0, 0);
    return out;
}

// next_ibf_id / bin_to_user of IBF i as the raptor index stores them (hierarchical_interleaved_bloom_filter.hpp:124-136,188)
inline void tables_of(const Layout& l, uint32_t i, std::vector<int64_t>& next_ibf_id, std::vector<int64_t>& bin_to_user)
{
    const Ibf& f = l.ibfs[i];
    next_ibf_id.assign(f.bins, (int64_t)i);
    bin_to_user.assign(f.bins, -1);
    for (const Run& r : f.runs)
        for (uint32_t b = r.first; b < r.first + r.n_bins; ++b)
        {
            next_ibf_id[b] = r.user < 0 ? r.child : (int64_t)i;
            bin_to_user[b] = r.user;
        }
}

} // namespace gnhibf
