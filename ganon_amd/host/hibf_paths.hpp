// hibf_paths.hpp -- the root-to-leaf path of every user bin of an HIBF, as gn_filter_emplace_path and gn_filter_probe_path take it.
// Host only: no device, no I/O.
//
// A path is `depth` gn_path_entry: entry 0 is the user bin's run {leaf ibf, first bin, n bins}, then the merged bin that leads there
// in each IBF above, up to IBF 0; n_bins == 0 ends a path shorter than `depth`, the longest path of the tree.
//   paths_of       from the builder's own layout (what `ganon-build --hibf` inserts along)
//   derive_paths   from the tables of an index FILE (next_ibf_id, bin_to_user: hierarchical_interleaved_bloom_filter.hpp:124-136,188),
//                  whoever wrote it -- what `ganon-build --verify-index` looks up along.  Everything a reader of the tree relies on
//                  is checked and refused with the IBF and the bin named: a user bin has exactly one run of consecutive bins in one
//                  IBF, each of those bins with its own IBF as next_ibf_id; a bin without a user bin is merged and leads to another
//                  IBF of the file; every IBF but IBF 0 is led to by exactly one merged bin, IBF 0 by none; following the parents
//                  from any IBF ends at IBF 0.  No bound on the bins of an IBF or on the depth: those are a layout's business.
#pragma once

#include "hibf_layout.hpp"

#include "ganon_hip.h"

#include <stdexcept>
#include <string>

namespace gnhibf
{

struct Paths
{
    std::vector<gn_path_entry> entries; // user bin u: entries[u * depth .. (u + 1) * depth)
    uint32_t                   depth = 0;
};

// counts[u] = distinct hashes of user bin u: hash i of its ascending set goes to bin first + i / ceil(count / n_bins) of its run
inline Paths paths_of(const Layout& lay, const std::vector<uint64_t>& counts)
{
    Paths out;
    out.depth = lay.levels;
    out.entries.assign(counts.size() * (size_t)out.depth, gn_path_entry{ 0, 0, 0, 0, 0 });
    for (uint32_t i = 0; i < lay.ibfs.size(); ++i)
        for (const Run& r : lay.ibfs[i].runs)
        {
            if (r.user < 0)
                continue;
            gn_path_entry* p = &out.entries[(size_t)r.user * out.depth];
            *p++             = gn_path_entry{ i, r.first, r.n_bins, 0, (counts[r.user] + r.n_bins - 1) / r.n_bins };
            for (uint32_t at = i; lay.ibfs[at].parent >= 0; at = (uint32_t)lay.ibfs[at].parent)
                *p++ = gn_path_entry{ (uint32_t)lay.ibfs[at].parent, lay.ibfs[at].parent_bin, 1, 0, 1 };
        }
    return out;
}

// bins[i] = technical bins of IBF i; next_ibf_id[i] / bin_to_user[i] hold at least that many entries.  hashes_per_bin of the entries
// is 0: a file does not say how its writer dealt a user bin's hashes to the bins of its run.  Throws std::runtime_error.
inline Paths derive_paths(const std::vector<uint64_t>& bins, const std::vector<std::vector<int64_t>>& next_ibf_id,
                          const std::vector<std::vector<int64_t>>& bin_to_user, uint64_t n_user_bins)
{
    auto at = [](uint64_t i, uint64_t b) { return "IBF " + std::to_string(i) + " bin " + std::to_string(b); };
    auto refuse = [](const std::string& m) -> void { throw std::runtime_error("HIBF tables: " + m); };
    const uint64_t n_ibf = bins.size();
    if (n_ibf == 0 || n_ibf > 0xFFFFFFFFull || next_ibf_id.size() != n_ibf || bin_to_user.size() != n_ibf)
        refuse("next_ibf_id / bin_to_user do not have one entry per IBF");
    struct Where
    {
        uint32_t ibf = 0, first = 0, n = 0; // n == 0: no run seen
    };
    struct Parent
    {
        int64_t  ibf = -1;
        uint32_t bin = 0;
    };
    std::vector<Where>  where(n_user_bins);
    std::vector<Parent> parent(n_ibf);
    for (uint64_t i = 0; i < n_ibf; ++i)
    {
        const uint64_t B = bins[i];
        if (B > 0xFFFFFFFFull || next_ibf_id[i].size() < B || bin_to_user[i].size() < B)
            refuse("IBF " + std::to_string(i) + ": " + std::to_string(B) + " bins, but " + std::to_string(next_ibf_id[i].size()) + " / " +
                   std::to_string(bin_to_user[i].size()) + " table entries");
        const std::vector<int64_t>&nx = next_ibf_id[i], &bu = bin_to_user[i];
        for (uint64_t b = 0; b < B;)
        {
            const int64_t u = bu[b];
            if (u < 0) // a merged bin
            {
                const int64_t c = nx[b];
                if (c <= 0 || (uint64_t)c >= n_ibf)
                    refuse(at(i, b) + ": a merged bin whose child, IBF " + std::to_string(c) + ", is out of range (1.." + std::to_string(n_ibf - 1) + ")");
                if ((uint64_t)c == i)
                    refuse(at(i, b) + ": a merged bin whose child is its own IBF");
                if (parent[c].ibf >= 0)
                    refuse(at(i, b) + ": IBF " + std::to_string(c) + " has two parents, " + at(parent[c].ibf, parent[c].bin) + " is the other");
                parent[c] = Parent{ (int64_t)i, (uint32_t)b };
                ++b;
                continue;
            }
            if ((uint64_t)u >= n_user_bins)
                refuse(at(i, b) + ": user bin " + std::to_string(u) + " of " + std::to_string(n_user_bins));
            uint64_t e = b;
            for (; e < B && bu[e] == u; ++e)
                if (nx[e] != (int64_t)i)
                    refuse(at(i, e) + ": a bin of user bin " + std::to_string(u) + " whose next_ibf_id is " + std::to_string(nx[e]) + ", not its own IBF");
            if (where[u].n != 0)
                refuse(at(i, b) + ": user bin " + std::to_string(u) + " has two runs, or one that is not contiguous: the other starts at " +
                       at(where[u].ibf, where[u].first));
            where[u] = Where{ (uint32_t)i, (uint32_t)b, (uint32_t)(e - b) };
            b        = e;
        }
    }
    for (uint64_t u = 0; u < n_user_bins; ++u)
        if (where[u].n == 0)
            refuse("user bin " + std::to_string(u) + " has no run: no bin of IBF 0.." + std::to_string(n_ibf - 1) + " names it");
    for (uint64_t i = 1; i < n_ibf; ++i)
        if (parent[i].ibf < 0)
            refuse("IBF " + std::to_string(i) + " has no parent: no merged bin leads to it (bin 0.." + std::to_string(bins[i] ? bins[i] - 1 : 0) + " are never reached)");
    // every chain of parents ends at IBF 0; the longest of them is the tree's depth
    Paths                 out;
    for (uint64_t i = 1; i < n_ibf; ++i)
    {
        uint64_t steps = 0;
        for (uint64_t a = i; a != 0; a = (uint64_t)parent[a].ibf)
            if (++steps >= n_ibf)
                refuse("cycle: following the parents of IBF " + std::to_string(i) + " (led to by " + at(parent[i].ibf, parent[i].bin) + ") never reaches IBF 0");
        out.depth = std::max(out.depth, (uint32_t)steps);
    }
    out.depth += 1;
    out.entries.assign(n_user_bins * (size_t)out.depth, gn_path_entry{ 0, 0, 0, 0, 0 });
    for (uint64_t u = 0; u < n_user_bins; ++u)
    {
        gn_path_entry* p = &out.entries[u * out.depth];
        *p++             = gn_path_entry{ where[u].ibf, where[u].first, where[u].n, 0, 0 };
        for (uint64_t a = where[u].ibf; a != 0; a = (uint64_t)parent[a].ibf)
            *p++ = gn_path_entry{ (uint32_t)parent[a].ibf, parent[a].bin, 1, 0, 0 };
    }
    return out;
}

} // namespace gnhibf
