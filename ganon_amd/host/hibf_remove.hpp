// hibf_remove.hpp -- the tables of an index after `ganon-build --hibf --update --remove` has taken user bins out.  Host only: no device, no I/O.
//
// The format has no "deleted bin": a user bin has exactly one run, every technical bin is a user bin's or a merged bin, and a reader
// sizes its result by the user bins the file names.  So a removed user bin vanishes:
//   the bins of its run are dropped;
//   an IBF left without a bin is dropped with the merged bin that leads to it, and so on upwards until nothing changes (an IBF of 0 bins
//   is refused by every reader);
//   IBF 0 left without a bin refuses the plan: the removal would leave no target;
//   the surviving IBFs keep their order and are renumbered densely (IBF 0 stays IBF 0), and so are the surviving user bins;
//   the surviving bins keep their order inside their IBF and close up to the left; next_ibf_id is rewritten with the new IBF numbers
//   (a user bin's bins name their own IBF).
// The plan also says how the columns move -- per surviving IBF its old index and the spans gn_filter_copy_ibf_spans takes, one per
// maximal run of surviving bins -- and carries the bit counts of the old bins to their new places, so that nothing is counted twice.
// Stated limits: a merged bin above a removed run keeps that run's hashes (it cannot be recomputed from its child, whose rows differ),
// rows never shrink, and a merged bin whose child is left with one user bin is not collapsed.  What the plan can say about the first is an
// estimate: per surviving merged bin on a removed path, the sum over the removed runs below it of deal_run's estimate of the hashes a
// bin holds, e = ceil(-(m / h) * log1p(-t / m)) for t of m rows set; a bin with t == m is full and says nothing.
// Refused (std::runtime_error): malformed tables (derive_paths is called first), a user bin out of range or named twice, inconsistent
// sizes, and a removal that empties IBF 0.
#pragma once

#include "hibf_paths.hpp"

#include <algorithm>
#include <cmath>

namespace gnhibf
{

struct RemovedRun
{
    uint64_t user_bin = 0;                       // old number
    uint32_t ibf = 0, first_bin = 0, n_bins = 0; // old numbers
    uint64_t bits = 0, hashes = 0;               // set bits of the run's bins, and the estimate of what they hold (0 without bit counts)
    bool     full = false;                       // a bin of the run has every row set: no estimate
};

struct RemoveDropped // an IBF left without a bin, and the merged bin that led to it (old numbers)
{
    uint32_t ibf = 0, parent_ibf = 0, parent_bin = 0;
};

struct RemoveStale // a surviving merged bin above at least one removed run
{
    uint32_t old_ibf = 0, old_bin = 0, ibf = 0, bin = 0;
    uint64_t bits = 0, hashes = 0; // its set bits; the estimated hashes of the removed runs below it
    bool     full = false;         // one of those runs has a full bin
};

struct RemovePlan
{
    std::vector<uint64_t>                 bins;        // per surviving IBF
    std::vector<std::vector<int64_t>>     next_ibf_id; // the new tables
    std::vector<std::vector<int64_t>>     bin_to_user;
    uint64_t                              n_user_bins = 0;
    std::vector<uint32_t>                 old_ibf;     // per surviving IBF
    std::vector<std::vector<gn_bin_span>> spans;       // per surviving IBF: old bins -> new bins
    std::vector<int64_t>                  ibf_map;     // old -> new, -1: dropped
    std::vector<int64_t>                  user_map;    // old -> new, -1: removed
    std::vector<RemoveDropped>            dropped;     // ascending by IBF
    std::vector<std::vector<uint64_t>>    popcounts;   // per surviving IBF and new bin (empty without bit counts)
    std::vector<RemovedRun>               removed;     // ascending by user bin
    std::vector<RemoveStale>              stale;       // ascending by (new IBF, new bin)
};

// rows / h / popcounts: the rows and hash functions of the IBFs and t[i][b] of gn_filter_bin_popcounts, for the estimates; popcounts may be
// nullptr (rows and h are then not looked at)
inline RemovePlan plan_remove(const std::vector<uint64_t>& bins, const std::vector<std::vector<int64_t>>& next_ibf_id,
                              const std::vector<std::vector<int64_t>>& bin_to_user, uint64_t n_user_bins, const std::vector<uint64_t>& remove,
                              const std::vector<uint64_t>& rows = {}, uint8_t h = 0, const std::vector<std::vector<uint64_t>>* popcounts = nullptr)
{
    auto refuse = [](const std::string& m) -> void { throw std::runtime_error("HIBF remove: " + m); };
    const Paths    old   = derive_paths(bins, next_ibf_id, bin_to_user, n_user_bins); // (refuses malformed tables)
    const uint64_t n_ibf = bins.size();
    if (popcounts)
    {
        if (rows.size() != n_ibf || popcounts->size() != n_ibf || h < 1 || h > 5)
            refuse("rows / bit counts do not have one entry per IBF, or " + std::to_string(h) + " hash functions");
        for (uint64_t i = 0; i < n_ibf; ++i)
        {
            if (rows[i] == 0 || (*popcounts)[i].size() < bins[i])
                refuse("IBF " + std::to_string(i) + ": " + std::to_string(rows[i]) + " rows, " + std::to_string(bins[i]) + " bins, " + std::to_string((*popcounts)[i].size()) + " bit counts");
            for (uint64_t b = 0; b < bins[i]; ++b)
                if ((*popcounts)[i][b] > rows[i])
                    refuse("IBF " + std::to_string(i) + " bin " + std::to_string(b) + ": " + std::to_string((*popcounts)[i][b]) + " bits set in " + std::to_string(rows[i]) + " rows");
        }
    }
    RemovePlan plan;
    plan.user_map.assign(n_user_bins, 0);
    for (const uint64_t u : remove)
    {
        if (u >= n_user_bins || plan.user_map[u] < 0)
            refuse("user bin " + std::to_string(u) + " of " + std::to_string(n_user_bins) + ", or named twice");
        plan.user_map[u] = -1;
    }
    // the parents (derive_paths has checked that every IBF but 0 has exactly one)
    std::vector<RemoveDropped> parent(n_ibf);
    for (uint64_t i = 0; i < n_ibf; ++i)
        for (uint64_t b = 0; b < bins[i]; ++b)
            if (bin_to_user[i][b] < 0)
                parent[next_ibf_id[i][b]] = RemoveDropped{ (uint32_t)next_ibf_id[i][b], (uint32_t)i, (uint32_t)b };
    // what goes: the removed runs, then the IBFs they empty and the merged bins above those
    std::vector<std::vector<bool>> keep(n_ibf);
    std::vector<uint64_t>          left(bins);
    for (uint64_t i = 0; i < n_ibf; ++i)
        keep[i].assign(bins[i], true);
    std::vector<uint64_t> emptied;
    for (uint64_t u = 0; u < n_user_bins; ++u)
        if (plan.user_map[u] < 0)
        {
            const gn_path_entry& run = old.entries[u * old.depth];
            for (uint32_t b = run.first_bin; b < run.first_bin + run.n_bins; ++b)
                keep[run.ibf][b] = false;
            left[run.ibf] -= run.n_bins;
            if (left[run.ibf] == 0)
                emptied.push_back(run.ibf);
        }
    plan.ibf_map.assign(n_ibf, 0);
    while (!emptied.empty())
    {
        const uint64_t i = emptied.back();
        emptied.pop_back();
        if (i == 0)
            refuse("every user bin of the index would be removed: nothing would be left");
        plan.ibf_map[i] = -1;
        plan.dropped.push_back(parent[i]);
        keep[parent[i].parent_ibf][parent[i].parent_bin] = false;
        if (--left[parent[i].parent_ibf] == 0)
            emptied.push_back(parent[i].parent_ibf);
    }
    std::sort(plan.dropped.begin(), plan.dropped.end(), [](const RemoveDropped& a, const RemoveDropped& b) { return a.ibf < b.ibf; });
    // the new numbers
    int64_t next = 0;
    for (uint64_t u = 0; u < n_user_bins; ++u)
        if (plan.user_map[u] >= 0)
            plan.user_map[u] = next++;
    plan.n_user_bins = (uint64_t)next;
    next             = 0;
    for (uint64_t i = 0; i < n_ibf; ++i)
        if (plan.ibf_map[i] >= 0)
            plan.ibf_map[i] = next++;
    // the new tables, the spans and the carried counts
    std::vector<std::vector<int64_t>> new_bin(n_ibf); // old bin -> new bin, -1: gone
    for (uint64_t i = 0; i < n_ibf; ++i)
    {
        new_bin[i].assign(bins[i], -1);
        if (plan.ibf_map[i] < 0)
            continue;
        std::vector<int64_t>     nx, bu;
        std::vector<gn_bin_span> spans;
        std::vector<uint64_t>    pop;
        for (uint64_t b = 0; b < bins[i]; ++b)
        {
            if (!keep[i][b])
                continue;
            const uint32_t to = (uint32_t)nx.size();
            new_bin[i][b]     = to;
            if (!spans.empty() && spans.back().src_first + spans.back().n_bins == b) // (then it ends at `to` in the destination too)
                ++spans.back().n_bins;
            else
                spans.push_back(gn_bin_span{ (uint32_t)b, to, 1, 0 });
            const bool merged = bin_to_user[i][b] < 0;
            nx.push_back(merged ? plan.ibf_map[next_ibf_id[i][b]] : plan.ibf_map[i]);
            bu.push_back(merged ? bin_to_user[i][b] : plan.user_map[bin_to_user[i][b]]);
            if (popcounts)
                pop.push_back((*popcounts)[i][b]);
        }
        plan.bins.push_back(nx.size());
        plan.next_ibf_id.push_back(std::move(nx)), plan.bin_to_user.push_back(std::move(bu));
        plan.old_ibf.push_back((uint32_t)i), plan.spans.push_back(std::move(spans));
        if (popcounts)
            plan.popcounts.push_back(std::move(pop));
    }
    // the report: what the removed runs held, and which surviving merged bins still hold it
    auto estimate = [&](uint64_t i, uint64_t b, bool& full) -> uint64_t {
        const uint64_t t = (*popcounts)[i][b], m = rows[i];
        if (t >= m)
        {
            full = true;
            return 0;
        }
        return (uint64_t)std::ceil(-((double)m / h) * std::log1p(-(double)t / m));
    };
    std::vector<std::vector<int64_t>> stale_at(n_ibf); // index into plan.stale, or -1
    for (uint64_t i = 0; i < n_ibf; ++i)
        stale_at[i].assign(bins[i], -1);
    for (uint64_t u = 0; u < n_user_bins; ++u)
    {
        if (plan.user_map[u] >= 0)
            continue;
        const gn_path_entry* p = &old.entries[u * old.depth];
        RemovedRun           r;
        r.user_bin = u, r.ibf = p[0].ibf, r.first_bin = p[0].first_bin, r.n_bins = p[0].n_bins;
        if (popcounts)
            for (uint32_t b = r.first_bin; b < r.first_bin + r.n_bins; ++b)
                r.bits += (*popcounts)[r.ibf][b], r.hashes += estimate(r.ibf, b, r.full);
        plan.removed.push_back(r);
        for (uint32_t d = 1; d < old.depth && p[d].n_bins; ++d)
        {
            const uint32_t i = p[d].ibf, b = p[d].first_bin;
            if (new_bin[i][b] < 0)
                continue; // (dropped with its child)
            if (stale_at[i][b] < 0)
            {
                stale_at[i][b] = (int64_t)plan.stale.size();
                plan.stale.push_back(RemoveStale{ i, b, (uint32_t)plan.ibf_map[i], (uint32_t)new_bin[i][b], popcounts ? (*popcounts)[i][b] : 0, 0, false });
            }
            RemoveStale& s = plan.stale[stale_at[i][b]];
            s.hashes += r.hashes, s.full = s.full || r.full;
        }
    }
    std::sort(plan.stale.begin(), plan.stale.end(), [](const RemoveStale& a, const RemoveStale& b) { return a.ibf != b.ibf ? a.ibf < b.ibf : a.bin < b.bin; });
    return plan;
}

// Which user bins a list of target names takes out.  targets / target_bins are what a reader makes of the file's bin_path
// (FilterMeta): the distinct names, and per name the user bins whose file lists hold it -- several when several user bins carry the
// name (all of them go), and a user bin is listed under several names when a foreign writer gave it several files.
struct RemoveNames
{
    std::vector<uint64_t>                         user_bins; // ascending, each once
    std::vector<std::string>                      unknown;   // names the index does not hold, in the order given
    std::vector<std::pair<uint64_t, std::string>> shared;    // a user bin to remove, and a target it also names that is to stay
};

inline RemoveNames resolve_remove(const std::vector<std::string>& targets, const std::vector<std::vector<uint64_t>>& target_bins, uint64_t n_user_bins,
                                  const std::vector<std::string>& names)
{
    RemoveNames       out;
    std::vector<bool> goes(n_user_bins, false), named(targets.size(), false);
    for (const std::string& name : names)
    {
        const auto at = std::find(targets.begin(), targets.end(), name);
        if (at == targets.end())
        {
            if (std::find(out.unknown.begin(), out.unknown.end(), name) == out.unknown.end())
                out.unknown.push_back(name);
            continue;
        }
        const size_t t = (size_t)(at - targets.begin());
        named[t]       = true;
        for (const uint64_t u : t < target_bins.size() ? target_bins[t] : std::vector<uint64_t>{})
            if (u < n_user_bins)
                goes[u] = true;
    }
    for (size_t t = 0; t < targets.size() && t < target_bins.size(); ++t)
        if (!named[t])
            for (const uint64_t u : target_bins[t])
                if (u < n_user_bins && goes[u])
                    out.shared.emplace_back(u, targets[t]);
    for (uint64_t u = 0; u < n_user_bins; ++u)
        if (goes[u])
            out.user_bins.push_back(u);
    return out;
}

} // namespace gnhibf
