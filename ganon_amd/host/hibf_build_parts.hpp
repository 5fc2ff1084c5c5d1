// hibf_build_parts.hpp -- the plan of a `ganon-build --hibf` in parts: which IBFs of the tree, or which rows of one, are filled together
// on which entry of --hibf-devices, when the tree does not fit what an entry may hold at one time (--hibf-memory, or what the device has
// free).  Every IBF is a matrix of its own, a hash's rows in it depend on the hash and on that IBF's row count alone, and its payload has
// a fixed place in the file: any set of IBFs, and any contiguous row range of one, is filled on its own from the same hash sets
// (gn_filter_emplace_path_window) and written to its own byte range.  Also here: a user bin's path cut down to the IBFs of a part.
// Pure host code, no device call: the test driver (tests/build_hibf_parts_driver.cpp) compiles it on its own.
#pragma once

#include "build_slabs.hpp"

#include "ganon_hip.h"

#include <algorithm>

namespace gnbuild
{

struct HibfPiece // rows [row_begin, row_begin + n_rows) of IBF `ibf` of the tree
{
    uint32_t ibf = 0;
    uint64_t row_begin = 0, n_rows = 0;
};

// The plan is a list of groups, each a run of consecutive parts: one part of whole IBFs (`whole` in file order), or the slabs of one IBF
// that does not fit the budget, one piece a part (`slabs`, the rule of plan_slabs: a list would not do for an IBF of 2^32 - 1 rows under
// a budget of one row).
struct HibfPartGroup
{
    uint64_t              first_part = 0;
    std::vector<uint32_t> whole;   // empty: a cut IBF
    uint32_t              cut_ibf = 0;
    SlabPlan              slabs;
    uint64_t              n_parts() const { return whole.empty() ? slabs.n_slabs : 1; }
};

struct HibfPartPlan
{
    std::vector<HibfPartGroup> groups;
    std::vector<uint64_t>      rows, row_bytes; // per IBF, as given
    uint64_t                   n_parts = 0;
    uint32_t                   n_devices = 1;

    uint32_t entry_of(uint64_t p) const { return (uint32_t)(p % n_devices); } // index into the list, not a device number
    std::vector<HibfPiece> part(uint64_t p) const // p < n_parts; pieces in file order
    {
        auto g = std::upper_bound(groups.begin(), groups.end(), p, [](uint64_t v, const HibfPartGroup& x) { return v < x.first_part; });
        --g;
        std::vector<HibfPiece> out;
        if (g->whole.empty())
        {
            const Slab s = g->slabs.at(p - g->first_part);
            out.push_back(HibfPiece{ g->cut_ibf, s.row_begin, s.n_rows });
        }
        else
            for (uint32_t i : g->whole)
                out.push_back(HibfPiece{ i, 0, rows[i] });
        return out;
    }
    uint64_t bytes_of(uint64_t p) const // device bytes of the part's rows
    {
        uint64_t b = 0;
        for (const HibfPiece& x : part(p))
            b += x.n_rows * row_bytes[x.ibf];
        return b;
    }
};

// rows[i] rows of row_bytes[i] DEVICE bytes (the padded stride, gn_hibf_row_stride_words) for IBF i in file order; at most budget_bytes
// of rows on a list entry at one time; n_devices list entries.  IBFs are taken in file order: one that fits what the open part has left
// joins it, one that fits the budget opens a new part, one that does not is cut into as few equal slabs as the budget allows, a part
// each.  Part p goes to entry p mod n_devices.  No part is empty, every row of every IBF lies in exactly one piece, no part holds more
// than the budget.  One part is the one-pass build.  Throws when not one row of an IBF fits, naming the IBF.
inline HibfPartPlan plan_hibf_parts(const std::vector<uint64_t>& rows, const std::vector<uint64_t>& row_bytes, uint64_t budget_bytes, uint32_t n_devices)
{
    if (rows.empty() || rows.size() != row_bytes.size() || rows.size() > 0xFFFFFFFFull || n_devices == 0)
        throw std::invalid_argument("plan_hibf_parts: an empty tree or an empty device list");
    HibfPartPlan plan;
    plan.rows = rows, plan.row_bytes = row_bytes, plan.n_devices = n_devices;
    HibfPartGroup cur;
    uint64_t      left = budget_bytes;
    auto          close = [&]() {
        if (cur.whole.empty())
            return;
        cur.first_part = plan.n_parts;
        plan.n_parts += 1;
        plan.groups.push_back(std::move(cur));
        cur = HibfPartGroup{};
    };
    for (uint32_t i = 0; i < rows.size(); ++i)
    {
        if (rows[i] == 0 || row_bytes[i] == 0)
            throw std::invalid_argument("plan_hibf_parts: IBF " + std::to_string(i) + " is empty");
        const bool     fits = rows[i] <= budget_bytes / row_bytes[i]; // (rows * row_bytes <= budget, without the product)
        const uint64_t need = fits ? rows[i] * row_bytes[i] : 0;
        if (fits && need <= left)
        {
            cur.whole.push_back(i);
            left -= need;
        }
        else if (fits)
        {
            close();
            cur.whole.push_back(i);
            left = budget_bytes - need;
        }
        else
        {
            close();
            HibfPartGroup cut;
            cut.cut_ibf = i;
            try
            {
                cut.slabs = plan_slabs(rows[i], row_bytes[i], budget_bytes, n_devices);
            }
            catch (const std::runtime_error& e)
            {
                throw std::runtime_error("IBF " + std::to_string(i) + ": " + e.what());
            }
            cut.first_part = plan.n_parts;
            plan.n_parts += cut.slabs.n_slabs;
            plan.groups.push_back(std::move(cut));
            left = budget_bytes;
        }
    }
    close();
    return plan;
}

// A user bin's path (depth entries, n_bins == 0 ends it) cut down to the IBFs of a part: local[i] = IBF i's index in the part's filter,
// -1 when the part does not hold it.  The entries kept go to `out` in their order, renumbered, the rest of `out`'s depth entries end the
// path.  Returns how many were kept: a user bin with none is not the part's business.
inline uint32_t compact_path(const gn_path_entry* path, uint32_t depth, const std::vector<int64_t>& local, gn_path_entry* out)
{
    uint32_t kept = 0;
    for (uint32_t d = 0; d < depth && path[d].n_bins != 0; ++d)
    {
        if (path[d].ibf >= local.size() || local[path[d].ibf] < 0)
            continue;
        out[kept]     = path[d];
        out[kept].ibf = (uint32_t)local[path[d].ibf];
        ++kept;
    }
    for (uint32_t d = kept; d < depth; ++d)
        out[d] = gn_path_entry{ 0, 0, 0, 0, 0 };
    return kept;
}

} // namespace gnbuild
