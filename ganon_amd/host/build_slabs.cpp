// build_slabs.cpp -- the bit matrix of the flat .ibf: created, filled and written.  When it fits what a device may hold (the budget:
// --device-memory, or what is free) it is one filter on the first entry of --device, filled in one pass and written behind the header,
// the one-pass build.  Otherwise it is cut into slabs of rows (build_slabs.hpp): the file is laid out first, then one worker thread per
// list entry takes its slabs in ascending order -- an empty storage-only filter of the slab's rows, every target's hashes through the
// windowed insert (gn_filter_emplace_runs_window: the rows are those of the whole filter, a slab takes the bits of the rows it holds),
// the rows streamed to their place in the file, the filter freed.  The hash sets stay in host memory and are read by all workers; every
// slab is one more pass over them.  The file is byte for byte the one-pass build's.  With --hash-sets packed|spilled the sets are packed
// (csrc/gn_packed_set.h) in the hashing threads' arenas, in memory or in mapped files, and go through gn_filter_emplace_packed_window: a
// pass uploads the payload words and the tables of the blocks instead of 8 bytes a hash; the same bits, the same file.
#include "build_common.hpp"
#include "build_slabs.hpp"

#include <algorithm>
#include <atomic>
#include <map>
#include <mutex>
#include <thread>
#include <unistd.h>

namespace gnbuild
{

namespace
{

// Device memory a fill takes besides the filter's rows: the two staging chunks of gn_filter_emplace_runs_window (1 Mi hashes each; 1 Mi
// payload words each for gn_filter_emplace_packed_window) and their item tables, rounded up.
constexpr uint64_t kFillStagingBytes = 24ull << 20;
// What a budget taken from the free memory leaves alone on every device: the runtime's own allocations on first use of a stream or a
// kernel, and room for whatever else runs on a shared card to grow a little while the build runs.
constexpr uint64_t kDeviceReserveBytes = 512ull << 20;

// the runs of a build as the insert takes them: one per target with hashes, in the order of `targets`
struct Runs
{
    std::vector<const uint64_t*> ptr;
    std::vector<uint64_t>        size, per_bin;
    std::vector<uint32_t>        first_bin;
    uint64_t                     hashes = 0;
    // packed sets: per run its blocks and the words of its arena instead of `ptr`; what one pass uploads
    bool                                packed = false;
    std::vector<const gn_packed_block*> blocks;
    std::vector<uint64_t>               n_blocks;
    uint64_t                            pass_bytes = 0;
    explicit Runs(const FlatFill& w) : packed(w.arenas != nullptr)
    {
        uint32_t bin = 0;
        for (size_t t = 0; t < w.targets.size(); ++t)
        {
            const Target&  tg = w.targets[t];
            const uint64_t n  = n_hashes(tg);
            if (n == 0)
                continue;
            if (packed)
            {
                ptr.push_back((*w.arenas)[tg.arena]), blocks.push_back(reinterpret_cast<const gn_packed_block*>(tg.blocks.data())), n_blocks.push_back(tg.blocks.size());
                for (const GnPackedBlock& b : tg.blocks)
                    pass_bytes += 8ull * gn_packed_words(b.cnt, b.width) + sizeof(GnPackedItem);
            }
            else
                ptr.push_back(tg.hashes.data()), pass_bytes += n * 8;
            size.push_back(n), per_bin.push_back(w.shares[t]), first_bin.push_back(bin);
            bin += (uint32_t)((n + w.shares[t] - 1) / w.shares[t]);
            hashes += n;
        }
    }
    bool insert(gn_filter* f, uint64_t total_rows, uint64_t row_begin) const
    {
        if (packed)
            return gn_filter_emplace_packed_window(f, blocks.data(), n_blocks.data(), ptr.data(), first_bin.data(), per_bin.data(), (uint32_t)ptr.size(), total_rows,
                                                   row_begin, 0) == GN_OK;
        return gn_filter_emplace_runs_window(f, ptr.data(), size.data(), first_bin.data(), per_bin.data(), (uint32_t)ptr.size(), total_rows, row_begin, 0) == GN_OK;
    }
};

// most bytes of rows on a list entry at one time: --device-memory, else what the free memory allows
bool budget_of(const Config& c, uint64_t& budget, std::string& err)
{
    if (c.device_memory_given)
    {
        budget = c.device_memory;
        return true;
    }
    return budget_from_free_memory(c.devices, budget, err);
}

} // namespace

bool budget_from_free_memory(const std::vector<int>& devices, uint64_t& budget, std::string& err)
{
    std::map<int, uint64_t> named;
    for (int d : devices)
        ++named[d];
    budget = ~0ull;
    for (const auto& [d, k] : named)
    {
        uint64_t free_b = 0, total_b = 0;
        if (gn_device_memory(d, &free_b, &total_b) != GN_OK)
        {
            err = gn_last_error();
            return false;
        }
        const uint64_t taken = k * kFillStagingBytes + kDeviceReserveBytes;
        budget               = std::min(budget, free_b > taken ? (free_b - taken) / k : 0);
    }
    return true;
}

bool fill_and_save_flat(const FlatFill& w, Lap& filling, Lap& writing)
{
    const Config&  c         = w.c;
    const uint64_t rows      = w.p.bin_size_bits, row_bytes = ((w.p.n_bins + 63) >> 6) * 8;
    const Runs     runs(w);
    filling.start();
    uint64_t    budget = 0;
    std::string err;
    if (!budget_of(c, budget, err))
        return fail(err);
    SlabPlan plan;
    try
    {
        plan = plan_slabs(rows, row_bytes, budget, (uint32_t)c.devices.size());
    }
    catch (const std::exception& e)
    {
        return fail(std::string(c.device_memory_given ? "--device-memory: " : "--device: ") + e.what());
    }
    if (c.verbose)
        for (uint64_t i = 0; i < plan.n_slabs; ++i)
        {
            const Slab s = plan.at(i);
            std::cerr << "slab " << i << ": rows [" << s.row_begin << ", " << s.row_begin + s.n_rows << ") device " << c.devices[s.device_entry] << '\n';
        }

    if (plan.n_slabs == 1) // the one-pass build
    {
        gnhost::OwnedFilter flt = gnhost::upload_ibf(c.devices[0], w.p.n_bins, rows, w.p.hash_functions, nullptr, 0); // storage only: no bin map
        if (!flt || !runs.insert(flt.get(), rows, 0))
            return fail(gn_last_error());
        filling.stop();
        writing.start();
        if (!save_filter(c, flt.get(), w.p, w.targets, w.bins, err))
            return fail(err);
        writing.stop();
    }
    else
    {
        uint64_t  payload_at = 0;
        const int fd         = open_filter(c, w.p, w.targets, w.bins, payload_at, err);
        if (fd < 0)
            return fail(err);
        std::mutex               mu;
        std::atomic<bool>        failed{ false };
        std::vector<double>      fill_s(plan.n_slabs, 0), write_s(plan.n_slabs, 0);
        std::vector<std::thread> workers;
        for (uint32_t e = 0; e < c.devices.size(); ++e)
            workers.emplace_back([&, e] {
                auto give_up = [&](const std::string& m) {
                    std::lock_guard<std::mutex> lk(mu);
                    if (!failed.exchange(true))
                        err = m;
                };
                gnhost::PinnedBlock stage;
                for (uint64_t i = e; i < plan.n_slabs && !failed; i += c.devices.size())
                {
                    const Slab s  = plan.at(i);
                    auto       t0 = std::chrono::steady_clock::now();
                    gnhost::OwnedFilter flt = gnhost::upload_ibf(c.devices[e], w.p.n_bins, s.n_rows, w.p.hash_functions, nullptr, 0);
                    if (!flt || !runs.insert(flt.get(), rows, s.row_begin))
                        return give_up(gn_last_error());
                    fill_s[i] = since(t0);
                    t0        = std::chrono::steady_clock::now();
                    std::string why;
                    if (!save_slab(fd, flt.get(), s.n_rows, row_bytes, payload_at + s.row_begin * row_bytes, stage, why))
                        return give_up(why == "write error on the output file" ? "write error on " + c.output_file : why);
                    write_s[i] = since(t0);
                }
            });
        for (auto& t : workers)
            t.join();
        ::close(fd);
        if (failed)
            return fail(err);
        filling.stop();
        writing.start(), writing.stop(); // (the rows went out slab by slab, inside the fill)
        if (c.verbose)
            for (uint64_t i = 0; i < plan.n_slabs; ++i)
                std::cerr << "slab " << i << ": filled in " << fill_s[i] << " s, written in " << write_s[i] << " s\n";
    }
    if (c.verbose)
        std::cerr << "filled in " << plan.n_slabs << (plan.n_slabs == 1 ? " pass" : " passes") << " over the hash sets, " << runs.pass_bytes * plan.n_slabs
                  << " hash bytes uploaded" << std::endl;
    return true;
}

} // namespace gnbuild
