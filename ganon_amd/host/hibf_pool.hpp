// hibf_pool.hpp -- how hash sets that go along paths of a hierarchical filter are handed to the device, for the insert of
// `ganon-build --hibf` and `--update` (gn_filter_emplace_path) and the membership pass of `--verify-index` (gn_filter_probe_path):
// large sets go as they lie; small ones are gathered so that a launch has enough of them.  No device, no HIP: gn_path_entry is
// plain C (include/ganon_hip.h).
#pragma once

#include "ganon_hip.h"

#include <cstddef>
#include <cstdint>
#include <vector>

namespace gnhibf
{

constexpr uint64_t kPoolBatch = 16ull << 20; // the pool is handed over once it holds this many hashes
constexpr uint64_t kPoolAlone = 4ull << 20;  // a set of this many hashes goes by itself

// Sets 0 .. n_sets-1 in order; set_of(i) -> its hashes as a (pointer, size) pair (std::pair<const uint64_t*, uint64_t>),
// path_of(i) -> its `depth` path entries.
//   call(hashes, offsets, n, paths, ids): n sets, set j = hashes[offsets[j] .. offsets[j+1]), its path at paths[j * depth], and the
//   caller's index of it ids[j] (a std::vector<size_t> of n).
// A set of `alone` hashes or more is handed over by itself out of its own storage the moment it is met -- sets gathered before it
// stay in the pool and go later; any other set is appended to the pool, which is handed over when it holds `batch` hashes or more
// and once more after the last set when something is left in it.  Empty sets are pooled like any other: a caller that does not
// want them leaves them out.  Whatever `call` throws passes through.
template <typename SetOf, typename PathOf, typename Call>
void for_each_pooled(size_t n_sets, SetOf&& set_of, PathOf&& path_of, uint32_t depth, Call&& call, uint64_t batch = kPoolBatch,
                     uint64_t alone = kPoolAlone)
{
    std::vector<uint64_t>      pool, off{ 0 };
    std::vector<gn_path_entry> paths;
    std::vector<size_t>        ids;
    auto                       flush = [&] {
        if (!ids.empty())
            call(pool.data(), off.data(), ids.size(), paths.data(), ids);
        pool.clear(), paths.clear(), ids.clear(), off.assign(1, 0);
    };
    for (size_t i = 0; i < n_sets; ++i)
    {
        const auto [hashes, n] = set_of(i);
        const gn_path_entry* p = path_of(i);
        if (n >= alone)
        {
            const uint64_t one[2] = { 0, n };
            call(hashes, one, size_t(1), p, std::vector<size_t>{ i });
            continue;
        }
        pool.insert(pool.end(), hashes, hashes + n);
        off.push_back(pool.size());
        paths.insert(paths.end(), p, p + depth);
        ids.push_back(i);
        if (pool.size() >= batch)
            flush();
    }
    flush();
}

} // namespace gnhibf
