// hibf_fold.hpp -- the tables of an index after `ganon-build --hibf --update --fold N` has held its IBFs to N bins.  Host only: no device,
// no I/O, and the same input gives the same plan.
//
// A hash's row depends on the hash, the seed and the IBF's row count only, so the column of a bin can be moved unchanged into a new IBF of
// the same rows, and the merged bin a build would have put above a group of such bins is the row-wise OR of their columns
// (gn_filter_fold_ibf).  So an IBF that an update has widened can be narrowed without the genomes: groups of its user bins move one level
// down, each group into a new IBF, and leave one merged bin behind.
//
// The rule runs last, on the tables plan_remove, plan_extend and plan_update leave, and on a fill t per bin: the carried bit count of an
// old bin, update_predict(0, hashes_per_bin, m, h) for a bin of a new run, the plan's prediction for a merged bin it touched.  For every
// IBF i of those tables with more than N bins (m rows, in IBF order):
//   candidates   the runs of user bins, a run never split; key = the sum of the run's fills, ascending, ties by the run's first bin.
//                Merged bins are no candidates and stay where they are.
//   grouping     candidates are taken in that order into an open group.  A run joins while the group stays at <= N bins and the predicted
//                fill of the OR, m * (1 - prod_j (1 - t_j / m)) over all member bins (the product taken bin by bin in the order the bins
//                joined), stays <= pow(fpr, 1.0 / h) * m: the merged-bin bound of plan_update.  Otherwise the group is closed and the run
//                opens the next.
//   stopping     a run that is over the bound alone, or wider than N alone, ends the candidates (the keys only grow from there).  A closed
//                group saves its bins - 1; the rule stops as soon as closing the open group brings IBF i to <= N.  A group of one bin
//                is dropped: its run stays.
//   result       each group becomes a new IBF, numbered behind the existing ones in (parent, group) order, with the parent's rows and the
//                group's bins in their old left-to-right order, and one merged bin of the parent.  The parent's surviving bins close up
//                to the left in order; the new merged bins follow at its end, in group order.
// An IBF that cannot reach N this way refuses the plan (FoldUnreachable: the IBF, its bins, the bins reachable and N).  One level of
// folding per call: the children have at most N bins by construction and are not looked at; merged bins are never folded.
// Also refused (std::runtime_error): malformed tables (derive_paths is called first), inconsistent sizes, N < 2.
#pragma once

#include "hibf_paths.hpp"

#include <algorithm>
#include <cmath>

namespace gnhibf
{

struct FoldGroup
{
    uint32_t              parent = 0, merged_bin = 0, new_ibf = 0; // new numbers
    uint32_t              runs = 0, bins = 0;
    double                bits_predicted = 0;
    std::vector<uint32_t> run_first, run_bins; // the group's runs in the parent as it was, ascending
};

struct FoldWhere // where a bin of the tables given went
{
    uint32_t ibf = 0, bin = 0;
    int64_t  merged_bin = -1; // the merged bin of the bin's old IBF that is above it now, or -1: it stayed in its IBF
};

struct FoldPlan
{
    std::vector<uint64_t>                 bins, rows;  // per IBF of the new tables
    std::vector<std::vector<int64_t>>     next_ibf_id; // the new tables
    std::vector<std::vector<int64_t>>     bin_to_user;
    std::vector<uint32_t>                 src_ibf;     // per new IBF: the IBF of the tables given that its columns come from
    std::vector<std::vector<gn_bin_span>> spans;       // per new IBF: bins of src_ibf -> its bins (the new merged bins have no source)
    std::vector<std::vector<double>>      fills;       // per new IBF and bin: carried, or the group's prediction for a new merged bin
    std::vector<std::vector<FoldWhere>>   where;       // per IBF and bin of the tables given
    std::vector<FoldGroup>                groups;      // in (parent, group) order: group k is IBF (IBFs given) + k
    std::vector<uint32_t>                 folded;      // the parents, ascending
    uint32_t                              depth = 0;   // of the new tables
};

struct FoldUnreachable : std::runtime_error
{
    using std::runtime_error::runtime_error;
};

inline FoldPlan plan_fold(const std::vector<uint64_t>& bins, const std::vector<uint64_t>& rows, const std::vector<std::vector<int64_t>>& next_ibf_id,
                          const std::vector<std::vector<int64_t>>& bin_to_user, uint64_t n_user_bins, uint8_t h, double fpr,
                          const std::vector<std::vector<double>>& fills, uint64_t N)
{
    auto refuse = [](const std::string& m) -> void { throw std::runtime_error("HIBF fold: " + m); };
    derive_paths(bins, next_ibf_id, bin_to_user, n_user_bins); // (refuses malformed tables)
    const uint64_t n_ibf = bins.size();
    if (rows.size() != n_ibf || fills.size() != n_ibf)
        refuse("rows / fills do not have one entry per IBF");
    if (h < 1 || h > 5 || !(fpr > 0.0 && fpr < 1.0))
        refuse("hash functions " + std::to_string(h) + " / false-positive rate " + std::to_string(fpr) + " out of range");
    if (N < 2)
        refuse("a bound of " + std::to_string(N) + " bins: at least 2");
    for (uint64_t i = 0; i < n_ibf; ++i)
    {
        if (rows[i] == 0)
            refuse("IBF " + std::to_string(i) + " has no rows");
        if (fills[i].size() < bins[i])
            refuse("IBF " + std::to_string(i) + ": " + std::to_string(bins[i]) + " bins, but " + std::to_string(fills[i].size()) + " fills");
        for (uint64_t b = 0; b < bins[i]; ++b)
            if (!(fills[i][b] >= 0.0 && fills[i][b] <= (double)rows[i]))
                refuse("IBF " + std::to_string(i) + " bin " + std::to_string(b) + ": a fill of " + std::to_string(fills[i][b]) + " bits in " + std::to_string(rows[i]) + " rows");
    }
    FoldPlan plan;
    plan.bins.assign(n_ibf, 0), plan.rows = rows;
    plan.next_ibf_id.resize(n_ibf), plan.bin_to_user.resize(n_ibf), plan.spans.resize(n_ibf), plan.fills.resize(n_ibf), plan.where.resize(n_ibf);
    for (uint64_t i = 0; i < n_ibf; ++i)
        plan.src_ibf.push_back((uint32_t)i);
    struct Cand
    {
        uint32_t first, n;
        double   key;
    };
    for (uint64_t i = 0; i < n_ibf; ++i)
    {
        const uint64_t              B = bins[i], m = rows[i];
        const std::vector<int64_t>& nx = next_ibf_id[i], &bu = bin_to_user[i];
        const std::vector<double>&  t  = fills[i];
        std::vector<int64_t>        group_of(B, -1); // per bin: its group in this IBF
        std::vector<std::vector<Cand>> groups;
        std::vector<double>            predicted;
        if (B > N)
        {
            std::vector<Cand> cand;
            for (uint64_t b = 0; b < B;)
            {
                uint64_t e = b + 1;
                if (bu[b] < 0)
                {
                    b = e;
                    continue;
                }
                double key = t[b];
                for (; e < B && bu[e] == bu[b]; ++e)
                    key += t[e];
                cand.push_back(Cand{ (uint32_t)b, (uint32_t)(e - b), key });
                b = e;
            }
            std::stable_sort(cand.begin(), cand.end(), [](const Cand& x, const Cand& y) { return x.key < y.key; }); // (key, first bin)
            const double      bound = std::pow(fpr, 1.0 / h) * m;
            std::vector<Cand> open;
            uint64_t          open_bins = 0, left = B; // left: the bins of IBF i with every closed group one bin
            double            open_prod = 1.0;
            auto              close     = [&]() {
                if (open_bins > 1)
                {
                    left -= open_bins - 1;
                    groups.push_back(open);
                    predicted.push_back(m * (1.0 - open_prod));
                }
                open.clear(), open_bins = 0, open_prod = 1.0;
            };
            for (const Cand& c : cand)
            {
                double alone = 1.0;
                for (uint32_t b = c.first; b < c.first + c.n; ++b)
                    alone *= 1.0 - t[b] / m;
                if (c.n > N || !(m * (1.0 - alone) <= bound))
                    break;
                double with = open_prod;
                for (uint32_t b = c.first; b < c.first + c.n; ++b)
                    with *= 1.0 - t[b] / m;
                if (!open.empty() && (open_bins + c.n > N || !(m * (1.0 - with) <= bound)))
                {
                    close();
                    with = alone;
                }
                open.push_back(c), open_bins += c.n, open_prod = with;
                if (left - (open_bins - 1) <= N)
                    break;
            }
            close();
            if (left > N)
                throw FoldUnreachable("HIBF fold: IBF " + std::to_string(i) + " has " + std::to_string(B) + " bins; folding its runs of user bins reaches " + std::to_string(left) +
                                      " bins, not " + std::to_string(N) + ": rebuild or give a larger --fold");
            plan.folded.push_back((uint32_t)i);
        }
        for (size_t g = 0; g < groups.size(); ++g)
        {
            std::sort(groups[g].begin(), groups[g].end(), [](const Cand& x, const Cand& y) { return x.first < y.first; });
            for (const Cand& c : groups[g])
                for (uint32_t b = c.first; b < c.first + c.n; ++b)
                    group_of[b] = (int64_t)g;
        }
        // the parent: the surviving bins closed up to the left, then one merged bin per group
        // (built apart: the children are appended to the plan's tables meanwhile)
        std::vector<int64_t>     pnx, pbu;
        std::vector<double>      pfill;
        std::vector<gn_bin_span> pspans;
        plan.where[i].resize(B);
        for (uint64_t b = 0; b < B; ++b)
        {
            if (group_of[b] >= 0)
                continue;
            const uint32_t to = (uint32_t)pnx.size();
            plan.where[i][b]  = FoldWhere{ (uint32_t)i, to, -1 };
            if (!pspans.empty() && pspans.back().src_first + pspans.back().n_bins == b)
                ++pspans.back().n_bins;
            else
                pspans.push_back(gn_bin_span{ (uint32_t)b, to, 1, 0 });
            pnx.push_back(nx[b]), pbu.push_back(bu[b]), pfill.push_back(t[b]);
        }
        for (size_t g = 0; g < groups.size(); ++g)
        {
            FoldGroup G;
            G.parent = (uint32_t)i, G.merged_bin = (uint32_t)pnx.size(), G.new_ibf = (uint32_t)plan.bins.size();
            G.bits_predicted = predicted[g];
            std::vector<int64_t>     cnx, cbu;
            std::vector<double>      cfill;
            std::vector<gn_bin_span> cspans;
            for (const Cand& c : groups[g])
            {
                G.run_first.push_back(c.first), G.run_bins.push_back(c.n);
                ++G.runs, G.bins += c.n;
                if (!cspans.empty() && cspans.back().src_first + cspans.back().n_bins == c.first)
                    cspans.back().n_bins += c.n;
                else
                    cspans.push_back(gn_bin_span{ c.first, (uint32_t)cnx.size(), c.n, 0 });
                for (uint32_t b = c.first; b < c.first + c.n; ++b)
                {
                    plan.where[i][b] = FoldWhere{ G.new_ibf, (uint32_t)cnx.size(), (int64_t)G.merged_bin };
                    cnx.push_back((int64_t)G.new_ibf), cbu.push_back(bu[b]), cfill.push_back(t[b]);
                }
            }
            pnx.push_back((int64_t)G.new_ibf), pbu.push_back(-1), pfill.push_back(G.bits_predicted);
            plan.bins.push_back(cnx.size()), plan.rows.push_back(m), plan.src_ibf.push_back((uint32_t)i);
            plan.next_ibf_id.push_back(std::move(cnx)), plan.bin_to_user.push_back(std::move(cbu));
            plan.fills.push_back(std::move(cfill)), plan.spans.push_back(std::move(cspans));
            plan.groups.push_back(std::move(G));
        }
        plan.bins[i] = pnx.size();
        plan.next_ibf_id[i] = std::move(pnx), plan.bin_to_user[i] = std::move(pbu), plan.fills[i] = std::move(pfill), plan.spans[i] = std::move(pspans);
    }
    plan.depth = derive_paths(plan.bins, plan.next_ibf_id, plan.bin_to_user, n_user_bins).depth; // (the result is a tree a reader accepts)
    return plan;
}

// Paths along the tables given, rewritten for the new ones: every entry through the bin map, and the merged entry {parent, merged bin, 1}
// above a leaf entry whose run was folded.  hashes_per_bin of the entries stay.
inline Paths fold_paths(const Paths& in, const FoldPlan& plan)
{
    Paths out;
    out.depth = plan.depth;
    const size_t n = in.depth ? in.entries.size() / in.depth : 0;
    out.entries.assign(n * (size_t)out.depth, gn_path_entry{ 0, 0, 0, 0, 0 });
    for (size_t u = 0; u < n; ++u)
    {
        const gn_path_entry* p = &in.entries[u * in.depth];
        gn_path_entry*       q = &out.entries[u * out.depth];
        uint32_t             used = 0;
        for (uint32_t d = 0; d < in.depth && p[d].n_bins; ++d)
        {
            if (p[d].ibf >= plan.where.size() || (uint64_t)p[d].first_bin + p[d].n_bins > plan.where[p[d].ibf].size())
                throw std::runtime_error("HIBF fold: path " + std::to_string(u) + " entry " + std::to_string(d) + " is outside the tables");
            const FoldWhere& w = plan.where[p[d].ibf][p[d].first_bin];
            if (used + (w.merged_bin >= 0 ? 2u : 1u) > out.depth || (w.merged_bin >= 0 && d != 0))
                throw std::runtime_error("HIBF fold: path " + std::to_string(u) + " does not fit the folded tree");
            q[used]           = p[d];
            q[used].ibf       = w.ibf;
            q[used].first_bin = w.bin;
            ++used;
            if (w.merged_bin >= 0)
                q[used++] = gn_path_entry{ p[d].ibf, (uint32_t)w.merged_bin, 1, 0, 1 };
        }
    }
    return out;
}

} // namespace gnhibf
