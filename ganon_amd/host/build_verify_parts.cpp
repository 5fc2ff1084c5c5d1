// build_verify_parts.cpp -- `ganon-build --hibf --verify-index` on an index that does not fit what a device may hold at one time
// (--verify-memory, or what is free), checked in the parts of hibf_build_parts.hpp over the entries of --verify-devices: one worker
// thread per entry takes its parts in ascending order -- a storage-only filter of the part's pieces, only those rows read from the file
// at their offsets, the targets with a path entry in the part through gn_filter_probe_path_window, the user bins with one through
// gn_filter_probe_paths_shared_window, the filter freed.  What a part says about a hash is not final when the hash's other rows, or the
// other levels of its path, lie in other parts: hibf_verify_parts.hpp carries it.  A worker answers a part into bitmaps of its own and
// ANDs them into the carried state under one lock, so no two calls ever write the same words; the last slab of a cut IBF to come in
// closes its entries.  The hash sets stay in host memory and are read by all workers.  The report is the one-device report to the byte
// (build_verify.hpp).  Modelled on build_hibf_parts.cpp.
#include "build_verify.hpp"
#include "hibf_verify_parts.hpp"

#include <atomic>
#include <cstring>
#include <fcntl.h>
#include <iomanip>
#include <map>
#include <mutex>
#include <thread>
#include <unistd.h>

namespace gnbuild
{

namespace
{

constexpr size_t kLoadChunkBytes = 64ull << 20; // of a piece's rows, read and sent to the device at one time (two such buffers a worker)

struct Closer // close() on every exit
{
    int fd;
    ~Closer()
    {
        if (fd >= 0)
            ::close(fd);
    }
};

void pread_all(int fd, void* dst, size_t bytes, uint64_t at, const std::string& path)
{
    for (size_t done = 0; done < bytes;)
    {
        const ssize_t got = ::pread(fd, (char*)dst + done, bytes - done, (off_t)(at + done));
        if (got <= 0)
            throw std::runtime_error(path + ": read error / unexpected end of file in the filter payload");
        done += (size_t)got;
    }
}

// the units (targets, or user bins) of a part: which of the caller's, their paths cut down to the part's IBFs, and for every kept entry
// the entry of the whole path it was and whether its piece is a slab
struct PartUnits
{
    std::vector<size_t>        ids;
    std::vector<gn_path_entry> paths; // ids.size() * depth
    std::vector<uint32_t>      orig;  // ids.size() * depth: the entry of the unit's whole path (kept entries only)
    std::vector<uint8_t>       slab;  // likewise
    void take(size_t id, const gn_path_entry* path, uint32_t depth, const std::vector<int64_t>& local, const std::vector<uint8_t>& piece_is_slab)
    {
        std::vector<gn_path_entry> cut(depth);
        if (compact_path(path, depth, local, cut.data()) == 0)
            return;
        ids.push_back(id);
        paths.insert(paths.end(), cut.begin(), cut.end());
        uint32_t kept = 0;
        orig.resize(orig.size() + depth, 0), slab.resize(slab.size() + depth, 0);
        for (uint32_t d = 0; d < depth && path[d].n_bins != 0; ++d) // (the rule of compact_path, for the entry numbers it does not return)
            if (path[d].ibf < local.size() && local[path[d].ibf] >= 0)
            {
                orig[orig.size() - depth + kept] = d;
                slab[slab.size() - depth + kept] = piece_is_slab[(size_t)local[path[d].ibf]];
                ++kept;
            }
    }
};

} // namespace

bool run_verify_parts(const Config& c, std::vector<Target>& targets, const gnhost::FilterMeta& meta, const std::vector<uint64_t>& payload_at,
                      const HibfPartPlan& plan, const std::vector<int>& devices, double hash_s)
{
    try
    {
        std::vector<uint64_t> bins;
        for (const gnhost::IbfShape& m : meta.shapes)
            bins.push_back(m.bins);
        const gnhibf::Paths paths  = gnhibf::derive_paths(bins, meta.next_ibf_id, meta.bin_to_user, meta.n_user_bins);
        const uint32_t      depth  = paths.depth;
        const uint64_t      n_user = meta.n_user_bins;
        const unsigned      k = meta.ibf_config.kmer_size;
        const bool          fp_pass = k <= 31 && n_user; // (k = 32: a hash can take any 64-bit value, no probe is a certain negative)
        std::map<std::string, uint64_t> user_of;         // names as the loader recovers them -> user bin
        for (size_t t = 0; t < meta.targets.size(); ++t)
            user_of[meta.targets[t]] = meta.target_bins[t].at(0);
        constexpr uint64_t    none = ~0ull;
        std::vector<uint64_t> user(targets.size(), none), sizes(targets.size(), 0);
        std::vector<size_t>   asked; // the targets with a user bin and a hash
        uint64_t              looked_up = 0, one_pass_bytes = 0;
        for (size_t t = 0; t < targets.size(); ++t)
        {
            auto it = user_of.find(name_as_read(targets[t].name));
            if (it == user_of.end())
                continue;
            user[t] = it->second;
            if (targets[t].hashes.empty())
                continue;
            looked_up += targets[t].hashes.size();
            sizes[t] = targets[t].hashes.size();
            asked.push_back(t);
        }
        one_pass_bytes = looked_up * 8 + (fp_pass ? kVerifyProbes * 8 : 0);
        const std::vector<uint64_t> probes = verify_probes(), order = verify_fp_order(paths, n_user);

        // the carried state: one unit per target for the membership pass, one per user bin for the false-positive pass
        VerifyCarry           member(sizes, depth), fp(std::vector<uint64_t>(fp_pass ? n_user : 0, kVerifyProbes), depth);
        std::vector<uint64_t> slabs_left(plan.groups.size(), 0); // of a cut IBF's group
        for (size_t g = 0; g < plan.groups.size(); ++g)
            slabs_left[g] = plan.groups[g].whole.empty() ? plan.groups[g].n_parts() : 0;

        if (c.verbose && plan.n_parts <= 100000)
            for (uint64_t p = 0; p < plan.n_parts; ++p)
                for (const HibfPiece& x : plan.part(p))
                    std::cerr << "part " << p << " device " << devices[plan.entry_of(p)] << ": ibf " << x.ibf << " rows [" << x.row_begin << ", "
                              << x.row_begin + x.n_rows << ")\n";

        const int fd = ::open(c.verify_index.c_str(), O_RDONLY);
        if (fd < 0)
            return fail("ERROR: cannot open filter file " + c.verify_index);
        const Closer closer{ fd };

        std::mutex               mu; // the carried state, the laps and stderr
        std::string              err;
        std::atomic<bool>        failed{ false };
        double                   load_s = 0, member_s = 0, fp_s = 0;
        uint64_t                 uploaded = 0;
        std::vector<std::thread> workers;
        const uint32_t           n_entries = (uint32_t)devices.size();
        for (uint32_t e = 0; e < n_entries; ++e)
            workers.emplace_back([&, e] {
                auto give_up = [&](const std::string& m) {
                    std::lock_guard<std::mutex> lk(mu);
                    if (!failed.exchange(true))
                        err = m;
                };
                try
                {
                    gnhost::PinnedBlock stage[2];
                    for (uint64_t p = e; p < plan.n_parts && !failed; p += n_entries)
                    {
                        // ---- the part's filter: its pieces, zero-filled, then their rows from the file
                        auto                           t0 = std::chrono::steady_clock::now();
                        const std::vector<HibfPiece>   pieces = plan.part(p);
                        std::vector<int64_t>           local(meta.shapes.size(), -1);
                        std::vector<gn_ibf_desc>       descs;
                        std::vector<uint64_t>          total_rows, row_begin;
                        std::vector<uint8_t>           is_slab;
                        for (size_t j = 0; j < pieces.size(); ++j)
                        {
                            const HibfPiece&        x = pieces[j];
                            const gnhost::IbfShape& m = meta.shapes[x.ibf];
                            local[x.ibf] = (int64_t)j;
                            descs.push_back(gnhost::ibf_desc(m.bins, x.n_rows, m.hash_funs));
                            total_rows.push_back(m.bin_size), row_begin.push_back(x.row_begin);
                            is_slab.push_back(x.n_rows != m.bin_size);
                        }
                        gn_filter* raw = nullptr;
                        if (gn_filter_create_hibf_storage(devices[e], (uint32_t)descs.size(), descs.data(), &raw) != GN_OK)
                            return give_up(gn_last_error());
                        gnhost::OwnedFilter flt(raw);
                        uint32_t            turn = 0;
                        for (size_t j = 0; j < pieces.size(); ++j)
                        {
                            const HibfPiece& x  = pieces[j];
                            const uint64_t   W  = meta.shapes[x.ibf].bin_words, rb = W * 8;
                            const uint64_t   step = std::max<uint64_t>(1, kLoadChunkBytes / rb);
                            for (uint64_t r = 0; r < x.n_rows; r += step, ++turn)
                            {
                                const uint64_t n = std::min(step, x.n_rows - r);
                                // (a buffer is read into while the one before it is on its way; then that copy is waited for, so that
                                // the next turn may fill its buffer)
                                gnhost::PinnedBlock& buf = stage[turn & 1];
                                if (!buf.reserve((size_t)(std::min(step, x.n_rows) * rb)))
                                    return give_up(gn_last_error());
                                pread_all(fd, buf.get(), (size_t)(n * rb), payload_at[x.ibf] + (x.row_begin + r) * rb, c.verify_index);
                                if (gn_filter_write_sync(flt.get()) != GN_OK ||
                                    gn_filter_write_rows(flt.get(), (uint32_t)j, r, n, static_cast<const uint64_t*>(buf.get()), W, 0) != GN_OK)
                                    return give_up(gn_last_error());
                            }
                        }
                        if (gn_filter_write_sync(flt.get()) != GN_OK)
                            return give_up(gn_last_error());
                        const double part_load_s = since(t0);

                        // ---- membership: the targets with an entry in the part, answered into bitmaps of this worker's own
                        t0 = std::chrono::steady_clock::now();
                        PartUnits mine;
                        for (size_t t : asked)
                            mine.take(t, &paths.entries[user[t] * depth], depth, local, is_slab);
                        const size_t                       n_sets = mine.ids.size();
                        std::vector<const uint64_t*>       sets(n_sets);
                        std::vector<uint64_t>              set_sizes(n_sets), lost(n_sets * (size_t)depth, 0);
                        std::vector<std::vector<uint64_t>> alive(n_sets), planes(n_sets * (size_t)depth);
                        std::vector<uint64_t*>             alive_at(n_sets), planes_at(n_sets * (size_t)depth, nullptr);
                        uint64_t                           part_hashes = 0;
                        for (size_t j = 0; j < n_sets; ++j)
                        {
                            const auto hs = hash_set(targets[mine.ids[j]]);
                            sets[j] = hs.first, set_sizes[j] = hs.second, part_hashes += hs.second;
                            alive[j]    = bitmap_ones(hs.second);
                            alive_at[j] = alive[j].data();
                            for (uint32_t d = 0; d < depth && mine.paths[j * depth + d].n_bins != 0; ++d)
                                if (mine.slab[j * depth + d])
                                {
                                    planes[j * depth + d].assign((size_t)mine.paths[j * depth + d].n_bins * bitmap_words(hs.second), ~0ull);
                                    planes_at[j * depth + d] = planes[j * depth + d].data();
                                }
                        }
                        if (n_sets &&
                            gn_filter_probe_path_window(flt.get(), sets.data(), set_sizes.data(), (uint32_t)n_sets, mine.paths.data(), depth, total_rows.data(),
                                                        row_begin.data(), alive_at.data(), planes_at.data(), lost.data(), 0) != GN_OK)
                            return give_up(gn_last_error());
                        const double part_member_s = since(t0);

                        // ---- false positives: the user bins with an entry in the part, in the order of the one-device pass
                        t0 = std::chrono::steady_clock::now();
                        PartUnits theirs;
                        if (fp_pass)
                            for (uint64_t u : order)
                                theirs.take((size_t)u, &paths.entries[u * depth], depth, local, is_slab);
                        const size_t                       n_paths = theirs.ids.size(), fp_words = bitmap_words(kVerifyProbes);
                        std::vector<uint64_t>              fp_alive(n_paths * fp_words, ~0ull); // (65 536 probes: no padding bits)
                        std::vector<std::vector<uint64_t>> fp_planes(n_paths * (size_t)depth);
                        std::vector<uint64_t*>             fp_planes_at(n_paths * (size_t)depth, nullptr);
                        for (size_t j = 0; j < n_paths; ++j)
                            for (uint32_t d = 0; d < depth && theirs.paths[j * depth + d].n_bins != 0; ++d)
                                if (theirs.slab[j * depth + d])
                                {
                                    fp_planes[j * depth + d].assign((size_t)theirs.paths[j * depth + d].n_bins * fp_words, ~0ull);
                                    fp_planes_at[j * depth + d] = fp_planes[j * depth + d].data();
                                }
                        if (n_paths && gn_filter_probe_paths_shared_window(flt.get(), probes.data(), probes.size(), theirs.paths.data(), (uint32_t)n_paths, depth,
                                                                           total_rows.data(), row_begin.data(), fp_alive.data(), fp_planes_at.data()) != GN_OK)
                            return give_up(gn_last_error());
                        const double part_fp_s = since(t0);
                        flt.reset();

                        // ---- into the carried state, one worker at a time
                        std::lock_guard<std::mutex> lk(mu);
                        for (size_t j = 0; j < n_sets; ++j)
                        {
                            member.and_alive(mine.ids[j], alive[j].data());
                            for (uint32_t d = 0; d < depth && mine.paths[j * depth + d].n_bins != 0; ++d)
                                if (mine.slab[j * depth + d])
                                    member.and_planes(mine.ids[j], mine.orig[j * depth + d], mine.paths[j * depth + d].n_bins, planes[j * depth + d].data());
                                else
                                    member.add_lost(mine.ids[j], mine.orig[j * depth + d], lost[j * depth + d]);
                        }
                        for (size_t j = 0; j < n_paths; ++j)
                        {
                            fp.and_alive(theirs.ids[j], fp_alive.data() + j * fp_words);
                            for (uint32_t d = 0; d < depth && theirs.paths[j * depth + d].n_bins != 0; ++d)
                                if (theirs.slab[j * depth + d])
                                    fp.and_planes(theirs.ids[j], theirs.orig[j * depth + d], theirs.paths[j * depth + d].n_bins, fp_planes[j * depth + d].data());
                        }
                        // the last slab of a cut IBF to come in closes every entry in that IBF
                        auto g = std::upper_bound(plan.groups.begin(), plan.groups.end(), p, [](uint64_t v, const HibfPartGroup& x) { return v < x.first_part; });
                        --g;
                        if (g->whole.empty() && --slabs_left[(size_t)(g - plan.groups.begin())] == 0)
                        {
                            for (size_t t : asked)
                                for (uint32_t d = 0; d < depth && paths.entries[user[t] * depth + d].n_bins != 0; ++d)
                                    if (paths.entries[user[t] * depth + d].ibf == g->cut_ibf)
                                        member.close(t, d);
                            for (uint64_t u = 0; fp_pass && u < n_user; ++u)
                                for (uint32_t d = 0; d < depth && paths.entries[u * depth + d].n_bins != 0; ++d)
                                    if (paths.entries[u * depth + d].ibf == g->cut_ibf)
                                        fp.close((size_t)u, d);
                        }
                        load_s += part_load_s, member_s += part_member_s, fp_s += part_fp_s;
                        uploaded += part_hashes * 8 + (n_paths ? kVerifyProbes * 8 : 0);
                        if (c.verbose)
                            std::cerr << "part " << p << " entry " << e << ": " << plan.bytes_of(p) << " device bytes, " << n_sets << " sets and " << n_paths
                                      << " user bins probed, loaded in " << part_load_s << " s, membership in " << part_member_s << " s, fp in " << part_fp_s
                                      << " s\n";
                    }
                }
                catch (const std::exception& ex)
                {
                    give_up(std::string("ERROR: ") + ex.what());
                }
            });
        for (auto& t : workers)
            t.join();
        if (failed)
            return fail(err);
        if (member.open_entries() || fp.open_entries())
            return fail("internal error: an entry of a cut IBF was left open");

        std::vector<uint64_t> found(targets.size(), 0), first_lost(targets.size(), none), false_hits(n_user, 0);
        for (size_t t : asked)
            found[t] = member.found(t), first_lost[t] = member.first_lost(t);
        for (uint64_t u = 0; fp_pass && u < n_user; ++u)
            false_hits[u] = fp.found((size_t)u);

        // the first false negative of a target, from the file: per entry of the path the hash's h rows, ANDed and masked to the run
        auto lookup = [&](const gn_path_entry* p, uint32_t used, uint64_t v, std::vector<uint64_t>& rows, std::vector<uint64_t>& words) {
            for (uint32_t d = 0; d < used; ++d)
            {
                const gnhost::IbfShape& m = meta.shapes.at(p[d].ibf);
                rows.assign(m.hash_funs, 0), words.assign(m.hash_funs * m.bin_words, 0);
                for (unsigned i = 0; i < m.hash_funs; ++i)
                {
                    rows[i] = gnhost::ibf_row(v, i, m);
                    pread_all(fd, words.data() + i * m.bin_words, m.bin_words * 8, payload_at[p[d].ibf] + rows[i] * m.bin_words * 8, c.verify_index);
                }
                bool hit = false;
                for (uint32_t b = p[d].first_bin; b < p[d].first_bin + p[d].n_bins && !hit; ++b)
                {
                    hit = true;
                    for (unsigned i = 0; i < m.hash_funs; ++i)
                        hit = hit && ((words[i * m.bin_words + (b >> 6)] >> (b & 63)) & 1);
                }
                if (!hit || d + 1 == used)
                    return d;
            }
            return 0u;
        };
        const VerifyCounts counts{ user, found, first_lost, false_hits, looked_up, k <= 31 };
        const bool         ok = print_verify_report(c, targets, meta, paths, counts, lookup);
        if (c.verbose)
            std::cerr << "checked in " << plan.n_parts << " parts, " << uploaded << " hash bytes uploaded (one pass: " << one_pass_bytes << ")" << std::endl;
        if (c.verbose && !c.quiet) // (load, membership and fp: summed over the parts, whichever worker took them)
            std::cerr << std::setprecision(6) << " - seconds: hash " << hash_s << " load " << load_s << " membership " << member_s << " fp " << fp_s << std::endl;
        return ok;
    }
    catch (const std::exception& e)
    {
        return fail(std::string("ERROR: ") + e.what());
    }
}

} // namespace gnbuild
