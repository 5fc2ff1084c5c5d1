// build_update.cpp -- `ganon-build --hibf --update F` (this project's extension).
// Adds the inputs' targets to an index without its genomes: the file into filter A, how full every bin is off A's bits
// (gn_filter_bin_popcounts), the placement (hibf_update.hpp), filter B with the new bins, every IBF moved over (gn_filter_copy_ibf),
// the new sets along their paths, B written with the file's own header fields and strings and the new names behind them.
#include "build_common.hpp"
#include "hibf_pool.hpp"
#include "hibf_update.hpp"

#include <algorithm>
#include <cmath>
#include <iomanip>
#include <memory>
#include <numeric>
#include <set>
#include <sstream>

namespace gnbuild
{

bool run_update(const Config& c, std::vector<Target>& targets, const Lap& counting)
{
    auto t0 = std::chrono::steady_clock::now();
    std::vector<uint32_t> fresh_target; // the new targets with a hash, in input order: new user bin n_user_old + position
    std::vector<uint64_t> fresh_counts;
    std::vector<uint32_t> ext_target;   // --extend: the targets the index holds, in input order, and their user bins
    std::vector<uint64_t> ext_user;
    for (uint32_t t = 0; t < targets.size(); ++t)
    {
        if (targets[t].hashes.empty())
            continue;
        if (!unite_files(c, targets[t]))
            return fail(gn_last_error());
        fresh_target.push_back(t);
    }
    if (fresh_target.empty())
        return fail("No valid sequences to build");
    const double hash_s = counting.seconds() + since(t0);
    try
    {
        {
            gnhost::FilterMeta names;
            gnhost::read_hibf_meta(c.update, names);
            const std::set<std::string> have(names.targets.begin(), names.targets.end());
            std::vector<uint32_t>       added;
            for (uint32_t t : fresh_target)
            {
                const std::string name = name_as_read(targets[t].name);
                if (!have.count(name))
                {
                    added.push_back(t);
                    continue;
                }
                if (!c.extend)
                    return fail("--update: target " + targets[t].name + " is already in the index (adding sequences to an existing user bin is not supported); nothing written");
                uint64_t held = 0, user = 0;
                for (size_t i = 0; i < names.targets.size(); ++i)
                    if (names.targets[i] == name)
                    {
                        held += i < names.target_bins.size() ? names.target_bins[i].size() : 1;
                        user = i < names.target_bins.size() && !names.target_bins[i].empty() ? names.target_bins[i][0] : i;
                    }
                if (held != 1)
                    return fail("--update --extend: " + std::to_string(held) + " user bins of the index are named " + targets[t].name + "; nothing written");
                ext_target.push_back(t), ext_user.push_back(user);
            }
            fresh_target.swap(added);
            for (uint32_t t : fresh_target)
                fresh_counts.push_back(targets[t].hashes.size());
        }
        t0 = std::chrono::steady_clock::now();
        gnhost::FilterMeta meta;
        auto               sink = std::make_unique<gnhost::DeviceSink>(c.device);
        gnhost::load_filter_file(c.update, true, meta, *sink);
        const double load_s = since(t0);
        const uint64_t n_ibf = meta.shapes.size(), n_old = meta.n_user_bins;
        const uint8_t  h   = (uint8_t)meta.shapes.at(0).hash_funs;
        const double   fpr = meta.ibf_config.max_fp;
        if (meta.raw_bin_path.size() != n_old || meta.raw_user_bin_filenames.size() != n_old)
            return fail("--update: the index names " + std::to_string(meta.raw_bin_path.size()) + " file lists for " + std::to_string(n_old) + " user bins");
        std::vector<uint64_t> bins, rows;
        for (const gnhost::IbfShape& m : meta.shapes)
        {
            bins.push_back(m.bins), rows.push_back(m.bin_size);
            if (m.hash_funs != h)
                return fail("--update: the IBFs of the index differ in their hash functions");
        }

        t0 = std::chrono::steady_clock::now();
        std::vector<std::vector<uint64_t>> pop(n_ibf);
        for (uint64_t i = 0; i < n_ibf; ++i)
        {
            pop[i].assign(bins[i], 0);
            if (gn_filter_bin_popcounts(sink->filter(), (uint32_t)i, pop[i].data()) != GN_OK)
                throw std::runtime_error(gn_last_error());
        }
        const double count_s = since(t0);

        t0 = std::chrono::steady_clock::now();
        // --extend: what every extension set's path lacks (A's bits), the quotas of its run and the fills the new user bins start from
        gnhibf::Paths      old_paths;
        gnhibf::ExtendPlan ex;
        double             probe_s = 0;
        if (!ext_target.empty())
        {
            old_paths = gnhibf::derive_paths(bins, meta.next_ibf_id, meta.bin_to_user, n_old);
            const uint32_t                   d0 = old_paths.depth;
            std::vector<gnhibf::ExtendInput> in(ext_target.size());
            for (size_t j = 0; j < in.size(); ++j)
            {
                if (ext_user[j] >= n_old)
                    return fail("--update --extend: the index names user bin " + std::to_string(ext_user[j]) + " of " + std::to_string(n_old));
                in[j].user_bin = ext_user[j], in[j].hashes = targets[ext_target[j]].hashes.size();
                in[j].lost_at.assign(d0, 0);
            }
            gnhibf::for_each_pooled(
                in.size(), [&](size_t j) { return hash_set(targets[ext_target[j]]); }, [&](size_t j) { return &old_paths.entries[(size_t)ext_user[j] * d0]; }, d0,
                [&](const uint64_t* hashes, const uint64_t* off, size_t n, const gn_path_entry* p, const std::vector<size_t>& ids) {
                    std::vector<uint64_t> found(n), first(n), lost(n * d0);
                    if (gn_filter_probe_path(sink->filter(), hashes, off, (uint32_t)n, p, d0, found.data(), lost.data(), first.data()) != GN_OK)
                        throw std::runtime_error(gn_last_error());
                    for (size_t k = 0; k < n; ++k)
                        in[ids[k]].lost_at.assign(lost.begin() + k * d0, lost.begin() + (k + 1) * d0);
                });
            probe_s = since(t0);
            ex      = gnhibf::plan_extend(old_paths, bins, rows, h, fpr, pop, in);
            if (!ex.over.empty())
            {
                std::ostringstream m;
                m << "--update --extend: " << ex.over.size() << " bin(s) would be over their bound; nothing written:";
                for (const gnhibf::ExtendOver& o : ex.over)
                    m << "\n  target " << targets[ext_target[o.extension]].name << ": IBF " << o.ibf << " bin " << o.bin << " predicted " << std::fixed << std::setprecision(1)
                      << o.bits_predicted << " bits, bound " << o.bound;
                m << "\na run is never moved or widened: leave it out or rebuild";
                return fail(m.str());
            }
        }
        const gnhibf::UpdatePlan plan =
            gnhibf::plan_update(bins, rows, meta.next_ibf_id, meta.bin_to_user, n_old, h, fpr, pop, fresh_counts, ext_target.empty() ? nullptr : &ex.fills);
        const uint32_t depth  = plan.paths.depth;
        const double   plan_s = since(t0) - probe_s;

        // filter B: the same rows, the new bins.  A and B are on the device together until every IBF is moved
        t0 = std::chrono::steady_clock::now();
        std::vector<HibfShape> ibfs(n_ibf);
        uint64_t               a_bytes = 0, b_bytes = 0;
        for (uint64_t i = 0; i < n_ibf; ++i)
        {
            ibfs[i].bins = plan.bins[i], ibfs[i].rows = rows[i];
            ibfs[i].next_ibf_id = plan.next_ibf_id[i], ibfs[i].bin_to_user = plan.bin_to_user[i];
            a_bytes += rows[i] * gn_hibf_row_stride_words((bins[i] + 63) >> 6) * 8;
            b_bytes += rows[i] * gn_hibf_row_stride_words((plan.bins[i] + 63) >> 6) * 8;
        }
        {
            uint64_t free_b = 0, total_b = 0;
            if (gn_device_memory(c.device, &free_b, &total_b) != GN_OK)
                throw std::runtime_error(gn_last_error());
            // (free_b is what is left beside A.  The 256 MiB on top of B are for what is still to come on this device: the staging buffer
            // of the inserts (32 M hashes, 256 MiB at most, usually far less), their item and path tables, the bit counts, and whatever
            // the hasher streams of the counting phase have not yet given back)
            if (b_bytes + (256ull << 20) > free_b)
                return fail("--update: the index (" + std::to_string(a_bytes) + " bytes on the device) and the updated one (" + std::to_string(b_bytes) +
                            " bytes) do not fit device " + std::to_string(c.device) + " together (" + std::to_string(free_b) + " bytes free beside the index)");
        }
        gnhost::HibfDescs descs;
        for (const HibfShape& s : ibfs)
            descs.add(s.bins, s.rows, h, s.next_ibf_id, s.bin_to_user);
        gnhost::OwnedFilter b_flt = descs.upload(c.device, plan.n_user_bins);
        if (!b_flt)
            throw std::runtime_error(gn_last_error());
        for (uint64_t i = 0; i < n_ibf; ++i)
            if (gn_filter_copy_ibf(b_flt.get(), (uint32_t)i, sink->filter(), (uint32_t)i) != GN_OK)
                throw std::runtime_error(gn_last_error());
        sink.reset(); // (frees A)
        const double copy_s = since(t0);

        // the new sets along their paths, pooled as run_hibf pools them; before them the extensions, by their quotas
        // (the pooler may cut the extensions into several calls.  A later call takes presence against B after the earlier ORs, not against A,
        // where lost_at was counted; the counts still agree, because presence is a matter of the run's own columns and only the run's own set
        // writes them -- one extension per user bin, and the new targets are inserted afterwards)
        t0 = std::chrono::steady_clock::now();
        gnhibf::for_each_pooled(
            ext_target.size(), [&](size_t j) { return hash_set(targets[ext_target[j]]); }, [&](size_t j) { return &old_paths.entries[(size_t)ext_user[j] * depth]; }, depth,
            [&](const uint64_t* hashes, const uint64_t* off, size_t n, const gn_path_entry* p, const std::vector<size_t>& ids) {
                std::vector<uint64_t> deal_off{ 0 }, deal;
                for (size_t k = 0; k < n; ++k)
                {
                    deal.insert(deal.end(), ex.quotas[ids[k]].begin(), ex.quotas[ids[k]].end());
                    deal_off.push_back(deal.size());
                }
                if (gn_filter_extend_path(b_flt.get(), hashes, off, (uint32_t)n, p, depth, deal_off.data(), deal.data()) != GN_OK)
                    throw std::runtime_error(gn_last_error());
            });
        gnhibf::for_each_pooled(
            fresh_target.size(),
            [&](size_t j) { return hash_set(targets[fresh_target[j]]); },
            [&](size_t j) { return &plan.paths.entries[j * depth]; }, depth,
            [&](const uint64_t* hashes, const uint64_t* off, size_t n, const gn_path_entry* p, const std::vector<size_t>&) {
                if (gn_filter_emplace_path(b_flt.get(), hashes, off, (uint32_t)n, p, depth) != GN_OK)
                    throw std::runtime_error(gn_last_error());
            });
        const double emplace_s = since(t0);

        // B's bit counts, for the IBFs the report speaks of: those that gained bins or lie on a new path
        t0 = std::chrono::steady_clock::now();
        std::vector<bool> shown(n_ibf, false);
        for (uint64_t i = 0; i < n_ibf; ++i)
            shown[i] = plan.bins[i] != bins[i];
        for (const gn_path_entry& e : plan.paths.entries)
            if (e.n_bins)
                shown[e.ibf] = true;
        for (const uint64_t u : ext_user)
            for (uint32_t d = 0; d < depth && old_paths.entries[(size_t)u * depth + d].n_bins; ++d)
                shown[old_paths.entries[(size_t)u * depth + d].ibf] = true;
        std::vector<std::vector<uint64_t>> pop_b(n_ibf);
        for (uint64_t i = 0; i < n_ibf; ++i)
            if (shown[i])
            {
                pop_b[i].assign(plan.bins[i], 0);
                if (gn_filter_bin_popcounts(b_flt.get(), (uint32_t)i, pop_b[i].data()) != GN_OK)
                    throw std::runtime_error(gn_last_error());
            }
        const double count_b_s = since(t0);

        // the file: its header fields and strings as they are, the new names behind them in the form run_hibf writes
        t0 = std::chrono::steady_clock::now();
        std::vector<std::vector<std::string>> bin_path   = meta.raw_bin_path;
        std::vector<std::string>              user_files = meta.raw_user_bin_filenames;
        const std::string dir = output_folder(c);
        for (uint32_t t : fresh_target)
        {
            const std::string f = dir + "/" + user_bin_file_name(targets[t].name) + ".minimiser";
            bin_path.push_back({ f });
            user_files.push_back(f);
        }
        std::string err;
        const bool  saved = save_hibf(c, b_flt.get(), ibfs, h, bin_path, user_files, err); // (c holds the file's k, w and fpr: validate())
        b_flt.reset();
        if (!saved)
            return fail(err);
        const double write_s = since(t0);

        // the report
        const double bound_fill = std::pow(fpr, 1.0 / h);
        std::cout << "index\t" << c.update << "\t->\t" << c.output_file << "\tk=" << unsigned(c.kmer_size) << " w=" << c.window_size << " h=" << unsigned(h)
                  << " ibfs=" << n_ibf << " levels=" << depth << " user_bins=" << n_old << "->" << plan.n_user_bins << " fpr=" << fpr << "\n";
        std::cout << "#target\tuser_bin\tdistinct_hashes\tleaf_ibf\tfirst_bin\tbins\tdepth\tpath\n";
        uint64_t bins_added = 0;
        for (size_t j = 0; j < fresh_target.size(); ++j)
        {
            const gn_path_entry* p    = &plan.paths.entries[j * depth];
            uint32_t             used = 0;
            while (used < depth && p[used].n_bins)
                ++used;
            std::cout << "target\t" << targets[fresh_target[j]].name << "\t" << n_old + j << "\t" << fresh_counts[j] << "\t" << p[0].ibf << "\t" << p[0].first_bin << "\t"
                      << p[0].n_bins << "\t" << used << "\t";
            for (uint32_t d = used; d-- > 0;)
                std::cout << p[d].ibf << ":" << p[d].first_bin << (d ? " " : "");
            std::cout << "\n";
            bins_added += p[0].n_bins;
        }
        if (c.extend)
        {
            std::cout << "#extended\ttarget\tuser_bin\thashes\talready_present\tinserted\tleaf_ibf\tfirst_bin\tbins\tpath\n";
            for (size_t j = 0; j < ext_target.size(); ++j)
            {
                const gn_path_entry* p        = &old_paths.entries[(size_t)ext_user[j] * depth];
                const uint64_t       n        = targets[ext_target[j]].hashes.size();
                const uint64_t       inserted = std::accumulate(ex.quotas[j].begin(), ex.quotas[j].end(), uint64_t(0));
                uint32_t             used     = 0;
                while (used < depth && p[used].n_bins)
                    ++used;
                std::cout << "extended\t" << targets[ext_target[j]].name << "\t" << ext_user[j] << "\t" << n << "\t" << n - inserted << "\t" << inserted << "\t" << p[0].ibf
                          << "\t" << p[0].first_bin << "\t" << p[0].n_bins << "\t";
                for (uint32_t d = used; d-- > 0;)
                    std::cout << p[d].ibf << ":" << p[d].first_bin << (d ? " " : "");
                std::cout << "\n";
            }
            std::cout << "#run\tibf\tbin\tdealt\tbits_before\tbits_predicted\tbits_after\n";
            for (const gnhibf::ExtendRunBin& r : ex.run)
                std::cout << "run\t" << r.ibf << "\t" << r.bin << "\t" << r.dealt << "\t" << r.bits_before << "\t" << std::fixed << std::setprecision(1) << r.bits_predicted << "\t"
                          << pop_b[r.ibf][r.bin] << "\n";
        }
        std::cout << "#ibf\trows\tbins_before\tbins_after\tmax_fill_before\tmax_fill_after\n" << std::fixed << std::setprecision(6);
        for (uint64_t i = 0; i < n_ibf; ++i)
            if (shown[i])
                std::cout << "ibf\t" << i << "\t" << rows[i] << "\t" << bins[i] << "\t" << plan.bins[i] << "\t"
                          << *std::max_element(pop[i].begin(), pop[i].end()) / (double)rows[i] << "\t"
                          << *std::max_element(pop_b[i].begin(), pop_b[i].end()) / (double)rows[i] << "\n";
        std::cout << "#merged\tibf\tbin\tbits_before\tbits_predicted\tbits_after\n";
        uint64_t fullest = 0, fullest_rows = 1;
        bool     any_touched = false;
        std::vector<gnhibf::UpdateTouched> touched = ex.touched; // the extensions' merged bins, then the new user bins'; a bin of both once,
        for (const gnhibf::UpdateTouched& t : plan.touched)      // with the later prediction (which starts from the earlier)
        {
            auto at = std::find_if(touched.begin(), touched.end(), [&](const gnhibf::UpdateTouched& x) { return x.ibf == t.ibf && x.bin == t.bin; });
            if (at == touched.end())
                touched.push_back(t);
            else
                at->bits_predicted = t.bits_predicted;
        }
        for (const gnhibf::UpdateTouched& t : touched)
        {
            const uint64_t after = pop_b[t.ibf][t.bin];
            std::cout << "merged\t" << t.ibf << "\t" << t.bin << "\t" << t.bits_before << "\t" << std::setprecision(1) << t.bits_predicted << std::setprecision(6) << "\t"
                      << after << (after > bound_fill * rows[t.ibf] ? "\tWARN fill" : "") << "\n";
            if (!any_touched || after * (double)fullest_rows > fullest * (double)rows[t.ibf])
                fullest = after, fullest_rows = rows[t.ibf];
            any_touched = true;
        }
        std::error_code ec;
        std::cout << "result\tok\t";
        if (c.extend)
            std::cout << ext_target.size() << " user bin(s) extended, ";
        std::cout << fresh_target.size() << " user bin(s) added, " << bins_added << " bin(s) added, " << fs::file_size(c.update, ec) << " -> "
                  << fs::file_size(c.output_file, ec) << " bytes, fullest touched merged bin ";
        if (!any_touched)
            std::cout << "n/a";
        else if (fullest >= fullest_rows)
            std::cout << "full";
        else
            std::cout << std::setprecision(0) << -((double)fullest_rows / h) * std::log(1.0 - (double)fullest / fullest_rows) << " estimated hashes at fill " << std::setprecision(6)
                      << (double)fullest / fullest_rows;
        std::cout << std::endl;
        if (c.verbose && !c.quiet)
            std::cerr << std::setprecision(6) << " - seconds: hash " << hash_s << " load " << load_s << " count " << count_s + count_b_s + probe_s << " plan " << plan_s << " copy " << copy_s
                      << " emplace " << emplace_s << " write " << write_s << std::endl;
        return true;
    }
    catch (const std::exception& e)
    {
        return fail(std::string("ERROR: ") + e.what());
    }
}

} // namespace gnbuild
