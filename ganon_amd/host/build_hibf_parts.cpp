// build_hibf_parts.cpp -- the tree of `ganon-build --hibf` filled in parts (hibf_build_parts.hpp), when it does not fit what a device may
// hold at one time: the file is laid out first (open_hibf), then one worker thread per entry of --hibf-devices takes its parts in ascending
// order -- an empty storage-only filter of the part's pieces, the user bins with a path entry in one of the part's IBFs through the
// windowed insert (gn_filter_emplace_path_window: the rows are those of the whole IBF, a piece takes the bits of the rows it holds), every
// piece streamed to its place in the file, the filter freed.  The hash sets stay in host memory and are read by all workers -- raw, or
// packed (--hibf-hash-sets packed|spilled: blocks and arena words through gn_filter_emplace_path_packed_window).  The file is
// byte for byte the one-pass build's.  Modelled on build_slabs.cpp, the flat build in row slabs.
#include "build_common.hpp"

#include <atomic>
#include <mutex>
#include <thread>
#include <unistd.h>

namespace gnbuild
{

namespace
{

uint64_t file_row_bytes(uint64_t bins)
{
    return ((bins + 63) >> 6) * 8;
}

// what a part takes: the storage filter's shapes, the windows, the user bins with an entry in one of its IBFs and their compacted paths
struct PartInput
{
    std::vector<HibfPiece>       pieces;
    std::vector<gn_ibf_desc>     descs;
    std::vector<uint64_t>        total_rows, row_begin, set_sizes;
    std::vector<const uint64_t*> sets;
    std::vector<gn_path_entry>   paths;
    // packed sets: per user bin taken its blocks and the words of its arena instead of pointer and size
    std::vector<const gn_packed_block*> blocks;
    std::vector<uint64_t>               n_blocks;
    uint64_t                     bytes = 0; // what the part's pass uploads
    PartInput(const HibfPartsFill& w, uint64_t p) : pieces(w.plan.part(p))
    {
        std::vector<int64_t> local(w.ibfs.size(), -1);
        for (size_t k = 0; k < pieces.size(); ++k)
        {
            const HibfPiece& x = pieces[k];
            local[x.ibf]       = (int64_t)k;
            descs.push_back(gnhost::ibf_desc(w.ibfs[x.ibf].bins, x.n_rows, w.hash_functions));
            total_rows.push_back(w.ibfs[x.ibf].rows), row_begin.push_back(x.row_begin);
        }
        const uint32_t             depth = w.paths.depth;
        std::vector<gn_path_entry> cut(depth);
        for (size_t u = 0; u < w.sets.size(); ++u)
        {
            if (compact_path(&w.paths.entries[u * depth], depth, local, cut.data()) == 0)
                continue;
            if (w.packed)
                sets.push_back(w.packed->payload[u]), blocks.push_back(w.packed->blocks[u]), n_blocks.push_back(w.packed->n_blocks[u]);
            else
                sets.push_back(w.sets[u].first);
            set_sizes.push_back(w.sets[u].second);
            paths.insert(paths.end(), cut.begin(), cut.end());
            bytes += w.packed ? w.packed->bytes[u] : w.sets[u].second * 8;
        }
    }
};

} // namespace

bool fill_and_save_hibf_parts(const HibfPartsFill& w, uint64_t& hash_bytes_uploaded)
{
    const Config&         c = w.c;
    const HibfPartPlan&   plan = w.plan;
    std::string           err;
    std::vector<uint64_t> payload_at;
    const int             fd = open_hibf(c, w.ibfs, w.hash_functions, w.bin_path, w.user_files, payload_at, err);
    if (fd < 0)
        return fail(err);
    std::mutex               mu;
    std::atomic<bool>        failed{ false };
    std::atomic<uint64_t>    uploaded{ 0 };
    std::vector<std::thread> workers;
    const uint32_t           n_entries = (uint32_t)w.devices.size();
    for (uint32_t e = 0; e < n_entries; ++e)
        workers.emplace_back([&, e] {
            auto give_up = [&](const std::string& m) {
                std::lock_guard<std::mutex> lk(mu);
                if (!failed.exchange(true))
                    err = m;
            };
            gnhost::PinnedBlock stage;
            for (uint64_t p = e; p < plan.n_parts && !failed; p += n_entries)
            {
                const PartInput in(w, p);
                auto            t0 = std::chrono::steady_clock::now();
                gn_filter*      raw = nullptr;
                if (gn_filter_create_hibf_storage(w.devices[e], (uint32_t)in.descs.size(), in.descs.data(), &raw) != GN_OK)
                    return give_up(gn_last_error());
                gnhost::OwnedFilter flt(raw);
                const int rc = w.packed ? gn_filter_emplace_path_packed_window(flt.get(), in.blocks.data(), in.n_blocks.data(), in.sets.data(), (uint32_t)in.sets.size(),
                                                                               in.paths.data(), w.paths.depth, in.total_rows.data(), in.row_begin.data(), 0)
                                        : gn_filter_emplace_path_window(flt.get(), in.sets.data(), in.set_sizes.data(), (uint32_t)in.sets.size(), in.paths.data(),
                                                                        w.paths.depth, in.total_rows.data(), in.row_begin.data(), 0);
                if (rc != GN_OK)
                    return give_up(gn_last_error());
                const double fill_s = since(t0);
                t0                  = std::chrono::steady_clock::now();
                for (size_t k = 0; k < in.pieces.size(); ++k)
                {
                    const HibfPiece& x  = in.pieces[k];
                    const uint64_t   rb = file_row_bytes(w.ibfs[x.ibf].bins);
                    std::string      why;
                    if (!save_piece(fd, flt.get(), (uint32_t)k, x.n_rows, rb, payload_at[x.ibf] + x.row_begin * rb, stage, why))
                        return give_up(why == "write error on the output file" ? "write error on " + c.output_file : why);
                }
                const double write_s = since(t0);
                uploaded += in.bytes;
                if (c.verbose)
                {
                    std::lock_guard<std::mutex> lk(mu);
                    std::cerr << "part " << p << " entry " << e << ": " << plan.bytes_of(p) << " device bytes, " << in.sets.size() << " sets taken, filled in " << fill_s
                              << " s, written in " << write_s << " s\n";
                }
            }
        });
    for (auto& t : workers)
        t.join();
    ::close(fd);
    if (failed)
    {
        ::unlink(c.output_file.c_str());
        return fail(err);
    }
    hash_bytes_uploaded = uploaded;
    return true;
}

} // namespace gnbuild
