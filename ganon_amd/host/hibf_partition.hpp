// hibf_partition.hpp -- the plan that spreads an HIBF too large for one device over several, by subtree (host only, no device calls).
//
// The reference loads an HIBF of any size into host memory (GanonClassify.cpp:875-938) and its counting agent walks the one tree
// (hierarchical_interleaved_bloom_filter.hpp:432-460).  A read's threshold depends on its own minimiser count alone; a technical bin of
// the ROOT is reported (user bin) or descended into (merged bin) on its own count alone, and everything below a merged bin is reached
// through that bin only.  So the root's bins, each with its whole subtree, can be dealt to different devices; every device then holds an
// ordinary, smaller HIBF (gn_filter_upload_hibf with ABSENT bins), classifies every read against it, and the parts' results are merged
// per read by user-bin id (gn_gather_create_merged).
//
//   unit       a maximal piece of the root's bin sequence that cannot be separated: the consecutive bins of one (split) user bin, or
//              one merged bin with every IBF reachable from it
//   part       a contiguous range of units = a contiguous range [bin_lo, bin_hi) of root bins, cut between units; cuts need not fall
//              on a word boundary.  Its root is words [word_lo, word_hi) of the root's rows -- same bin_size, hash_funs and hash_shift,
//              so every hash lands in the same row -- and in a boundary word shared with a neighbour the neighbour's bins are absent
//              (next_ibf_id == -1 and bin_to_user == -1).  A root of one word is held whole by every part.
//   bytes      device bytes: bin_size * stride(bin_words) * 8 of every IBF of the part's subtrees, plus the part's root,
//              root.bin_size * stride(word_hi - word_lo) * 8 (stride = gn_hibf_row_stride_words: rows are padded to whole lines)
//   partition  parts are given to the placement devices IN DEVICE ORDER, each at most what its device has left, the largest part as
//              small as possible (linear partition: bisection over the bound, the longest range that fits from the left -- the cost of a
//              range only grows when the range does).  A device that cannot take even the next unit gets nothing and is skipped; when
//              the units run out the trailing devices stay empty and unused.  Cutting below the root is not done.
//   numbering  inside a part the root is IBF 0, the owned IBFs follow in ascending global id, and the owned user bins are renumbered
//              densely in ascending GLOBAL user-bin id: local -> global is strictly increasing, so a read's result sorted by local id
//              is sorted by global id.
#pragma once

#include "filter_io.hpp"

#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

namespace gnhost
{

struct HibfPart
{
    size_t   slot = 0;                   // index into the budgets given (= placement device)
    uint64_t unit_lo = 0, unit_hi = 0;   // units [unit_lo, unit_hi)
    uint64_t bin_lo = 0, bin_hi = 0;     // root bins owned
    uint64_t word_lo = 0, word_hi = 0;   // root words held
    uint64_t bytes = 0;                  // on the device
    std::vector<uint32_t> ibf_global;    // local IBF -> global (ibf_global[0] == 0, ascending)
    std::vector<uint32_t> user_global;   // local user bin -> global (strictly increasing)
    // the part's own tree, as gn_filter_upload_hibf takes it (local ids; absent bins: -1 / -1)
    std::vector<IbfShape>             shapes;
    std::vector<std::vector<int64_t>> next_ibf_id, bin_to_user;
};

struct HibfPlan
{
    std::vector<HibfPart> parts;
    std::string           refusal; // not empty: nothing can be placed, and why (names the piece)
    uint64_t              n_units = 0;
};

typedef uint64_t (*HibfStrideFn)(uint64_t bin_words);

inline HibfPlan plan_hibf_partition(const FilterMeta& f, const std::vector<uint64_t>& budgets, HibfStrideFn stride)
{
    HibfPlan plan;
    auto     mib = [](uint64_t b) { return std::to_string((b + (1u << 20) - 1) >> 20) + " MiB"; };
    const size_t n_ibf = f.shapes.size();
    if (n_ibf == 0 || f.next_ibf_id.size() != n_ibf || f.bin_to_user.size() != n_ibf)
    {
        plan.refusal = "the HIBF has no IBFs: it does not fit and cannot be partitioned";
        return plan;
    }
    for (size_t i = 0; i < n_ibf; ++i)
        for (uint64_t t = 0; t < f.shapes[i].bins; ++t)
        {
            const int64_t u = f.bin_to_user[i][t], c = f.next_ibf_id[i][t];
            if (u >= (int64_t)f.n_user_bins || (u < 0 && (c <= 0 || (size_t)c >= n_ibf || (size_t)c == i)))
            {
                plan.refusal = "ibf " + std::to_string(i) + " bin " + std::to_string(t) + " of the HIBF leads nowhere: the tree does not fit one "
                               "device and cannot be partitioned by subtree";
                return plan;
            }
        }
    auto ibf_bytes = [&](size_t i) { return f.shapes[i].bin_size * stride(f.shapes[i].bin_words) * 8; };
    uint64_t total = 0;
    for (size_t i = 0; i < n_ibf; ++i)
        total += ibf_bytes(i);
    const IbfShape& root = f.shapes[0];
    const uint64_t  B    = root.bins;

    // ---- units, and the IBFs under every merged bin of the root ----
    struct Unit
    {
        uint64_t bin_lo, bin_hi, sub_bytes;
    };
    std::vector<Unit>    units;
    std::vector<int64_t> owner(n_ibf, -1); // IBF -> unit it hangs under (root: none)
    for (uint64_t b = 0; b < B;)
    {
        const int64_t u = f.bin_to_user[0][b];
        if (u >= 0)
        {
            uint64_t e = b + 1;
            while (e < B && f.bin_to_user[0][e] == u)
                ++e;
            units.push_back(Unit{ b, e, 0 });
            b = e;
            continue;
        }
        Unit                  un{ b, b + 1, 0 };
        std::vector<uint32_t> stack;
        const int64_t         c = f.next_ibf_id[0][b];
        if (c > 0 && (size_t)c < n_ibf)
            stack.push_back((uint32_t)c);
        while (!stack.empty())
        {
            const uint32_t i = stack.back();
            stack.pop_back();
            if (owner[i] != -1)
            {
                plan.refusal = "IBF " + std::to_string(i) + " of the HIBF is reached through two merged bins: it does not fit one device and "
                               "cannot be partitioned by subtree";
                return plan;
            }
            owner[i] = (int64_t)units.size();
            un.sub_bytes += ibf_bytes(i);
            for (uint64_t t = 0; t < f.shapes[i].bins; ++t)
            {
                const int64_t cc = f.next_ibf_id[i][t];
                if (f.bin_to_user[i][t] < 0 && cc > 0 && (size_t)cc < n_ibf && (size_t)cc != i)
                    stack.push_back((uint32_t)cc);
            }
        }
        units.push_back(un);
        ++b;
    }
    const size_t U = units.size();
    plan.n_units   = U;
    std::vector<uint64_t> pre(U + 1, 0);
    for (size_t i = 0; i < U; ++i)
        pre[i + 1] = pre[i] + units[i].sub_bytes;
    // device bytes of a part of units [a, b), b > a: monotone in the range
    auto cost = [&](size_t a, size_t b) {
        const uint64_t wl = units[a].bin_lo >> 6, wh = (units[b - 1].bin_hi + 63) >> 6;
        return pre[b] - pre[a] + root.bin_size * stride(wh - wl) * 8;
    };
    // the longest range from unit a that costs at most `bound` (a = nothing fits)
    auto reach = [&](size_t a, uint64_t bound) {
        size_t lo = a, hi = U; // cost(a, lo) <= bound (or lo == a), cost(a, hi + 1) > bound
        while (lo < hi)
        {
            const size_t mid = (lo + hi + 1) >> 1;
            if (cost(a, mid) <= bound)
                lo = mid;
            else
                hi = mid - 1;
        }
        return lo;
    };
    // ranges per budget slot under a bound on the largest part; true when every unit is placed
    auto deal = [&](uint64_t bound, std::vector<size_t>* cuts) {
        size_t at = 0;
        if (cuts)
            cuts->assign(budgets.size() + 1, 0);
        for (size_t d = 0; d < budgets.size(); ++d)
        {
            if (at < U)
                at = reach(at, std::min(bound, budgets[d]));
            if (cuts)
                (*cuts)[d + 1] = at;
        }
        return at == U;
    };
    uint64_t hi = U ? cost(0, U) : 0;
    if (U == 0 || !deal(hi, nullptr))
    {
        // name the piece: a unit no budget takes, or the lack of an assignment
        const uint64_t most = budgets.empty() ? 0 : *std::max_element(budgets.begin(), budgets.end());
        size_t         worst = 0;
        for (size_t i = 0; i < U; ++i)
            if (cost(i, i + 1) > cost(worst, worst + 1))
                worst = i;
        plan.refusal = "the HIBF (" + mib(total) + ") does not fit into the memory of one device beside the filters loaded before it and ";
        if (U && cost(worst, worst + 1) > most)
            plan.refusal += "cannot be partitioned by subtree within the devices' memory: the subtree under root bin " + std::to_string(units[worst].bin_lo)
                            + " takes " + mib(cost(worst, worst + 1)) + " with its share of the root (" + std::to_string(cost(worst, worst + 1))
                            + " bytes; the largest device budget left is " + std::to_string(most) + " bytes); cuts below the root are not made";
        else
            plan.refusal += "cannot be partitioned by subtree within the devices' memory: no assignment of the root's " + std::to_string(U)
                            + " units to the " + std::to_string(budgets.size()) + " device(s) in order fits their budgets";
        return plan;
    }
    uint64_t lo = 0;
    while (lo < hi) // smallest bound that still places everything
    {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (deal(mid, nullptr))
            hi = mid;
        else
            lo = mid + 1;
    }
    std::vector<size_t> cuts;
    deal(hi, &cuts);

    // ---- the parts' own trees ----
    for (size_t d = 0; d < budgets.size(); ++d)
    {
        const size_t a = cuts[d], b = cuts[d + 1];
        if (a == b)
            continue;
        HibfPart p;
        p.slot    = d;
        p.unit_lo = a;
        p.unit_hi = b;
        p.bin_lo  = units[a].bin_lo;
        p.bin_hi  = units[b - 1].bin_hi;
        p.word_lo = p.bin_lo >> 6;
        p.word_hi = (p.bin_hi + 63) >> 6;
        p.bytes   = cost(a, b);
        std::vector<int64_t> ibf_local(n_ibf, -1), user_local(f.n_user_bins, -1);
        p.ibf_global.push_back(0);
        ibf_local[0] = 0;
        for (size_t i = 1; i < n_ibf; ++i)
            if (owner[i] >= (int64_t)a && owner[i] < (int64_t)b)
            {
                ibf_local[i] = (int64_t)p.ibf_global.size();
                p.ibf_global.push_back((uint32_t)i);
            }
        std::vector<uint8_t> owned(f.n_user_bins, 0);
        for (uint32_t g : p.ibf_global)
        {
            const uint64_t t0 = g == 0 ? p.bin_lo : 0, t1 = g == 0 ? p.bin_hi : f.shapes[g].bins;
            for (uint64_t t = t0; t < t1; ++t)
            {
                const int64_t u = f.bin_to_user[g][t];
                if (u >= 0 && (uint64_t)u < f.n_user_bins)
                    owned[u] = 1;
            }
        }
        for (uint64_t u = 0; u < f.n_user_bins; ++u)
            if (owned[u])
            {
                user_local[u] = (int64_t)p.user_global.size();
                p.user_global.push_back((uint32_t)u);
            }
        for (uint32_t g : p.ibf_global)
        {
            IbfShape             m = f.shapes[g];
            std::vector<int64_t> nx, bu;
            if (g == 0)
            {
                // words [word_lo, word_hi) of the root; bins outside [bin_lo, bin_hi) are absent
                const uint64_t first = p.word_lo * 64, last = std::min<uint64_t>(B, p.word_hi * 64);
                m.bin_words      = p.word_hi - p.word_lo;
                m.bins           = last - first;
                m.technical_bins = m.bin_words * 64;
                nx.assign(m.bins, -1);
                bu.assign(m.bins, -1);
                for (uint64_t t = p.bin_lo; t < p.bin_hi; ++t)
                {
                    const int64_t u = f.bin_to_user[0][t], c = f.next_ibf_id[0][t];
                    bu[t - first] = u >= 0 ? user_local[u] : -1;
                    nx[t - first] = u >= 0 ? 0 : ibf_local[c];
                }
            }
            else
            {
                nx.assign(m.bins, -1);
                bu.assign(m.bins, -1);
                for (uint64_t t = 0; t < m.bins; ++t)
                {
                    const int64_t u = f.bin_to_user[g][t], c = f.next_ibf_id[g][t];
                    bu[t] = u >= 0 ? user_local[u] : -1;
                    nx[t] = u >= 0 ? (int64_t)ibf_local[g] : ibf_local[c];
                }
            }
            p.shapes.push_back(m);
            p.next_ibf_id.push_back(std::move(nx));
            p.bin_to_user.push_back(std::move(bu));
        }
        plan.parts.push_back(std::move(p));
    }
    return plan;
}

} // namespace gnhost
