// build_verify.hpp -- what the two ways of `ganon-build --hibf --verify-index` share: the index on one device in one piece
// (build_verify.cpp) and in parts over a device list (build_verify_parts.cpp).  Both count the same things and print them through one
// function, so the report is the same to the byte.
#pragma once

#include "build_common.hpp"
#include "hibf_paths.hpp"

#include <algorithm>
#include <functional>

namespace gnbuild
{

constexpr uint64_t kVerifyProbes = 65536; // P of the false-positive pass

// the P probes of the false-positive pass (include/ganon_hip.h states the generator)
std::vector<uint64_t> verify_probes();

// the user bins in the order the false-positive pass asks them: by (leaf ibf, first bin), so that neighbours share what they read
inline std::vector<uint64_t> verify_fp_order(const gnhibf::Paths& paths, uint64_t n_user)
{
    std::vector<uint64_t> order(n_user);
    for (uint64_t u = 0; u < n_user; ++u)
        order[u] = u;
    std::sort(order.begin(), order.end(), [&](uint64_t a, uint64_t b) {
        const gn_path_entry &x = paths.entries[a * paths.depth], &y = paths.entries[b * paths.depth];
        return std::make_pair(x.ibf, x.first_bin) < std::make_pair(y.ibf, y.first_bin);
    });
    return order;
}

// what was counted: per target its user bin (~0: the index has none of that name), the hashes found along the whole path and the index of
// the first one that was not (~0: none); per user bin the probes it answers to
struct VerifyCounts
{
    const std::vector<uint64_t>&user, &found, &first_lost, &false_hits;
    uint64_t                    looked_up;
    bool                        fp_pass;
};

// For the note of a first false negative: hash v along path p (`used` entries) -> the first entry that lacks it (the last one when none
// does), the hash's h rows in that entry's IBF and their words, bin_words each behind each other.
using VerifyLookup = std::function<uint32_t(const gn_path_entry* p, uint32_t used, uint64_t v, std::vector<uint64_t>& rows, std::vector<uint64_t>& words)>;

// the report on stdout; true when every named target was found whole and at least one was checked
bool print_verify_report(const Config& c, const std::vector<Target>& targets, const gnhost::FilterMeta& meta, const gnhibf::Paths& paths, const VerifyCounts& r,
                         const VerifyLookup& lookup);

} // namespace gnbuild
