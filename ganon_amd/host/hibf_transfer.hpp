// hibf_transfer.hpp -- which device calls move the columns of the index loaded (A) into the updated one (B) of
// `ganon-build --hibf --update`, after plan_remove, plan_update and plan_fold have said what B's tables are.  Host only: no device, no
// I/O, and the same input gives the same lists.
//
// MOVES, one per IBF of B in IBF order; each takes the columns of one IBF of A:
//   neither --remove nor --fold   IBF i whole from IBF i (gn_filter_copy_ibf: bin b stays bin b, the bins B gains stay empty)
//   --remove only                 IBF i from IBF old_ibf[i], by the removal's own spans, unchanged (gn_filter_copy_ibf_spans)
//   --fold                        IBF f from the IBF of A behind src_ibf[f], by the fold's spans composed with the removal's through
//                                 the A-BIN MAP: per bin of the tables the fold worked on, the bin of A that holds its column -- bin b
//                                 itself below A's bins, the removal's span otherwise -- or none for a bin this command adds, which
//                                 is dropped (the inserts fill it).  Bins are taken in destination order and joined into one span as
//                                 long as source and destination are both contiguous; an IBF of new bins alone has a move of no span,
//                                 which zeroes it.
// FOLD CALLS (gn_filter_fold_ibf), in (parent, group) order: the new merged bins of a parent are the OR of their groups' columns of A,
// one call for every maximal sequence of the parent's groups that each have a column in A, with the groups numbered from the first of
// the call.  A group of new user bins alone has no column there: the call ends before it, the next starts behind it, and its merged bin
// is left to the inserts.  The members of a call are sorted by their first bin of A, and neighbours of one group are one member.
// Refused (std::runtime_error): plans that do not belong together (the IBF counts differ, or an IBF has fewer bins than it moves).
#pragma once

#include "hibf_fold.hpp"
#include "hibf_remove.hpp"
#include "hibf_update.hpp"

#include <algorithm>
#include <numeric>

namespace gnhibf
{

struct TransferMove
{
    uint32_t                 dst_ibf = 0, src_ibf = 0; // of B, of A
    bool                     whole = false;            // gn_filter_copy_ibf; else gn_filter_copy_ibf_spans with `spans` (which may be empty)
    std::vector<gn_bin_span> spans;
};

struct TransferFold
{
    uint32_t                    parent = 0, merged_bin = 0, n_groups = 0; // of B: groups g < n_groups go to bin merged_bin + g
    uint32_t                    src_ibf = 0;                              // of A
    std::vector<gn_fold_member> members;
};

struct Transfer
{
    std::vector<TransferMove> moves;
    std::vector<TransferFold> folds;
};

// bins_a: the bins per IBF of A; gone / fold: nullptr without --remove / --fold
inline Transfer plan_transfer(const std::vector<uint64_t>& bins_a, const RemovePlan* gone, const UpdatePlan& plan, const FoldPlan* fold)
{
    auto refuse = [](const std::string& m) -> void { throw std::runtime_error("HIBF transfer: " + m); };
    const uint64_t n_b = plan.bins.size(); // the IBFs of the tables B starts from, which plan_update leaves as many
    if ((gone ? gone->old_ibf.size() : bins_a.size()) != n_b || (gone && gone->spans.size() != n_b) || (fold && fold->where.size() != n_b))
        refuse("the plans do not have the same IBFs");
    auto     a_ibf = [&](uint32_t i) { return gone ? gone->old_ibf[i] : i; };
    Transfer out;
    if (!fold)
    {
        for (uint32_t i = 0; i < n_b; ++i)
            out.moves.push_back(gone ? TransferMove{ i, a_ibf(i), false, gone->spans[i] } : TransferMove{ i, i, true, {} });
        return out;
    }
    // the A-bin map
    std::vector<std::vector<int64_t>> a_bin(n_b);
    for (uint32_t i = 0; i < n_b; ++i)
    {
        a_bin[i].assign(plan.bins[i], -1);
        if (a_ibf(i) >= bins_a.size() || (!gone && bins_a[i] > plan.bins[i]))
            refuse("IBF " + std::to_string(i) + " has no IBF of the index behind it, or fewer bins than it");
        if (!gone)
            std::iota(a_bin[i].begin(), a_bin[i].begin() + bins_a[i], int64_t(0));
        else
            for (const gn_bin_span& s : gone->spans[i])
            {
                if ((uint64_t)s.dst_first + s.n_bins > plan.bins[i])
                    refuse("IBF " + std::to_string(i) + " has fewer bins than the removal leaves it");
                std::iota(a_bin[i].begin() + s.dst_first, a_bin[i].begin() + s.dst_first + s.n_bins, (int64_t)s.src_first);
            }
    }
    for (uint32_t f = 0; f < fold->bins.size(); ++f)
    {
        const uint32_t si = fold->src_ibf[f];
        TransferMove   m{ f, a_ibf(si), false, {} };
        for (const gn_bin_span& s : fold->spans[f])
            for (uint32_t j = 0; j < s.n_bins; ++j)
            {
                const int64_t from = a_bin[si][s.src_first + j];
                if (from < 0)
                    continue;
                if (!m.spans.empty() && m.spans.back().src_first + m.spans.back().n_bins == (uint64_t)from &&
                    m.spans.back().dst_first + m.spans.back().n_bins == s.dst_first + j)
                    ++m.spans.back().n_bins;
                else
                    m.spans.push_back(gn_bin_span{ (uint32_t)from, s.dst_first + j, 1, 0 });
            }
        out.moves.push_back(std::move(m));
    }
    for (size_t g0 = 0; g0 < fold->groups.size();)
    {
        const uint32_t              parent = fold->groups[g0].parent;
        std::vector<gn_fold_member> members;
        size_t                      g = g0;
        for (; g < fold->groups.size() && fold->groups[g].parent == parent; ++g)
        {
            const FoldGroup& G   = fold->groups[g];
            const size_t     had = members.size();
            for (size_t k = 0; k < G.run_first.size(); ++k)
                for (uint32_t b = G.run_first[k]; b < G.run_first[k] + G.run_bins[k]; ++b)
                    if (a_bin[parent][b] >= 0)
                        members.push_back(gn_fold_member{ (uint32_t)a_bin[parent][b], 1, (uint32_t)(g - g0), 0 });
            if (members.size() == had)
                break;
        }
        if (g == g0) // the group at g0 has no column in A
        {
            ++g0;
            continue;
        }
        std::sort(members.begin(), members.end(), [](const gn_fold_member& x, const gn_fold_member& y) { return x.src_first < y.src_first; });
        TransferFold call{ parent, fold->groups[g0].merged_bin, (uint32_t)(g - g0), a_ibf(parent), {} };
        for (const gn_fold_member& m : members)
            if (!call.members.empty() && call.members.back().group == m.group && call.members.back().src_first + call.members.back().n_bins == m.src_first)
                ++call.members.back().n_bins;
            else
                call.members.push_back(m);
        out.folds.push_back(std::move(call));
        g0 = g;
    }
    return out;
}

} // namespace gnhibf
