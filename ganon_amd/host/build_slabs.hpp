// build_slabs.hpp -- the slab plan of a flat `ganon-build`: which rows of the bit matrix are filled on which entry of the --device list,
// when the matrix does not fit what a device may hold at one time (--device-memory, or what the device has free).  The filter is
// row-major and a hash's rows depend on the hash alone, so a contiguous range of rows -- a slab -- is filled on its own from the same
// hash sets (gn_filter_emplace_runs_window) and is a contiguous byte range of the file.  Pure host code, no device call: the test
// driver (tests/build_slabs_driver.cpp) compiles it on its own.
#pragma once

#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

namespace gnbuild
{

struct Slab
{
    uint64_t row_begin = 0, n_rows = 0;
    uint32_t device_entry = 0; // index into the --device list, not a device number
};

// Slabs of a matrix of total_rows rows of row_bytes bytes (bin_words * 8: a flat filter's rows are not padded on the device, device bytes
// are file bytes), at most budget_bytes of rows on a device entry at one time, dealt to n_devices list entries:
//   per = budget_bytes / row_bytes rows fit; none: the plan refuses
//   P = ceil(total_rows / per) slabs, of ceil(total_rows / P) rows each: equal but for a shorter last one, never more slabs than needed
//   and none empty; slab i goes to entry i mod n_devices.  P == 1 is the one-pass build: one slab on the first entry.
// The plan is the rule, not a list: a matrix of 2^32 - 1 rows under a budget of one row has as many slabs.
struct SlabPlan
{
    uint64_t total_rows = 0, rows_per_slab = 0, n_slabs = 0;
    uint32_t n_devices = 1;
    Slab     at(uint64_t i) const // i < n_slabs
    {
        const uint64_t row = i * rows_per_slab;
        return Slab{ row, rows_per_slab < total_rows - row ? rows_per_slab : total_rows - row, (uint32_t)(i % n_devices) };
    }
    // the slabs of one list entry, ascending: entry, entry + n_devices, ...
    std::vector<Slab> of_entry(uint32_t entry) const
    {
        std::vector<Slab> v;
        for (uint64_t i = entry; i < n_slabs; i += n_devices)
            v.push_back(at(i));
        return v;
    }
};

inline SlabPlan plan_slabs(uint64_t total_rows, uint64_t row_bytes, uint64_t budget_bytes, uint32_t n_devices)
{
    if (total_rows == 0 || row_bytes == 0 || n_devices == 0)
        throw std::invalid_argument("plan_slabs: an empty matrix or an empty device list");
    uint64_t per = budget_bytes / row_bytes;
    if (per == 0)
        throw std::runtime_error("one row of the filter takes " + std::to_string(row_bytes) + " bytes, " + std::to_string(budget_bytes) +
                                 " may be held on a device at one time: not one row fits");
    if (per > total_rows)
        per = total_rows;
    const uint64_t P = (total_rows + per - 1) / per;
    return SlabPlan{ total_rows, (total_rows + P - 1) / P, P, n_devices };
}

} // namespace gnbuild
