// build_verify.cpp -- `ganon-build --hibf --verify-index F` (this project's extension): nothing is built.  The inputs are hashed as for a
// build, the file's bits are streamed into HBM, and per user bin the device answers two questions: is every distinct minimiser of the
// target found in every IBF on the user bin's root-to-leaf path (gn_filter_probe_path along hibf_paths.hpp:derive_paths -- the paths
// come from the FILE's tables, whoever wrote it), and how often does the user bin answer to values that are no target's minimiser
// (gn_filter_probe_paths_shared).
// An index that does not fit what the device may hold at one time (--verify-memory, or what is free) is checked in parts over
// --verify-devices instead (build_verify_parts.cpp) and gives the same report, which is why the report is a function of its own here.
#include "build_verify.hpp"
#include "hibf_pool.hpp"

#include <algorithm>
#include <cmath>
#include <iomanip>
#include <map>

namespace gnbuild
{

namespace
{

// probe i of the false-positive pass (include/ganon_hip.h states the generator): splitmix64 of i + 1 with bit 63 set -- a
// (k,w)-minimiser hash is below 4^k, so for k <= 31 no target holds such a value
uint64_t verify_probe(uint64_t i)
{
    uint64_t z = (i + 1) * 0x9E3779B97F4A7C15ull;
    z          = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z          = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    return z | (1ull << 63);
}

} // namespace

std::vector<uint64_t> verify_probes()
{
    std::vector<uint64_t> probes(kVerifyProbes);
    for (uint64_t i = 0; i < kVerifyProbes; ++i)
        probes[i] = verify_probe(i);
    return probes;
}

bool print_verify_report(const Config& c, const std::vector<Target>& targets, const gnhost::FilterMeta& meta, const gnhibf::Paths& paths, const VerifyCounts& r,
                         const VerifyLookup& lookup)
{
    constexpr uint64_t           none = ~0ull;
    const std::vector<uint64_t>& user = r.user, &found = r.found, &first_lost = r.first_lost, &false_hits = r.false_hits;
    const uint64_t               looked_up = r.looked_up, n_user = meta.n_user_bins;
    const bool                   fp_pass = r.fp_pass;
    const uint32_t               depth = paths.depth;
    const unsigned               k = meta.ibf_config.kmer_size, h = (unsigned)meta.shapes.at(0).hash_funs;
    const double                 fpr = meta.ibf_config.max_fp;
    const double                 P = (double)kVerifyProbes;
    const uint64_t               warn_above = (uint64_t)std::ceil(P * fpr + 4.0 * std::sqrt(P * fpr * (1.0 - fpr)));

    std::cout << "index\t" << c.verify_index << "\tk=" << k << " w=" << meta.ibf_config.window_size << " h=" << h << " ibfs=" << meta.shapes.size()
              << " levels=" << depth << " user_bins=" << n_user << " fpr=" << fpr << "\n";
    std::cout << "#target\tuser_bin\tleaf_ibf\tbins\tdepth\tdistinct_hashes\tmissing\tfalse_hits\tobserved_fp\tverdict\n";
    uint64_t          n_checked = 0, n_bad = 0, fp_sum = 0, fp_max = 0;
    std::vector<bool> named(n_user, false);
    std::cout << std::fixed << std::setprecision(6);
    for (size_t t = 0; t < targets.size(); ++t)
    {
        const std::vector<uint64_t>& hs = targets[t].hashes;
        if (user[t] == none)
        {
            // a target without a hash has no user bin in an index built from these inputs: nothing to look for
            std::cout << targets[t].name << "\t-\t-\t0\t0\t" << hs.size() << "\t0\t" << (fp_pass ? "0" : "n/a") << "\t" << (fp_pass ? "0.000000" : "n/a") << "\t"
                      << (hs.empty() ? "ok" : "FAIL: no such user bin") << "\n";
            n_bad += !hs.empty();
            continue;
        }
        const gn_path_entry* p = &paths.entries[user[t] * depth];
        uint32_t             used = 0;
        while (used < depth && p[used].n_bins)
            ++used;
        const uint64_t missing = hs.size() - found[t], hits = false_hits[user[t]];
        const bool     warn    = fp_pass && hits > warn_above;
        ++n_checked;
        named[user[t]] = true;
        n_bad += missing != 0;
        fp_sum += hits, fp_max = std::max(fp_max, hits);
        std::cout << targets[t].name << "\t" << user[t] << "\t" << p[0].ibf << "\t" << p[0].n_bins << "\t" << used << "\t" << hs.size() << "\t" << missing << "\t";
        if (fp_pass)
            std::cout << hits << "\t" << hits / P;
        else
            std::cout << "n/a\tn/a";
        std::cout << "\t" << (missing ? "FAIL" : warn ? "WARN fp" : "ok") << "\n";
        if (missing)
        {
            // the first false negative: its hash, the first entry of the path that lacks it, its h rows there and the bits found
            const uint64_t          v = hs[first_lost[t]];
            std::vector<uint64_t>   rows, words;
            const uint32_t          d = lookup(p, used, v, rows, words);
            const gnhost::IbfShape& m = meta.shapes.at(p[d].ibf);
            std::cout << "  first false negative: hash " << v << " (index " << first_lost[t] << " of the sorted distinct hashes); lost at level " << d << ", ibf "
                      << p[d].ibf << ", bins " << p[d].first_bin << ".." << p[d].first_bin + p[d].n_bins - 1 << "; rows";
            for (auto r : rows)
                std::cout << " " << r;
            std::cout << "; bits [bin: one per hash function]";
            for (uint32_t b = p[d].first_bin; b < p[d].first_bin + p[d].n_bins && b < p[d].first_bin + 8; ++b)
            {
                std::cout << " [" << b << ":";
                for (unsigned i = 0; i < m.hash_funs; ++i)
                    std::cout << " " << ((words[i * m.bin_words + (b >> 6)] >> (b & 63)) & 1);
                std::cout << "]";
            }
            std::cout << "\n";
        }
    }
    uint64_t unnamed = 0;
    for (uint64_t u = 0; u < n_user; ++u)
        unnamed += !named[u];
    std::cout << "result\t" << (n_bad ? "FAIL" : "ok") << "\t" << n_checked << " target(s) checked, " << n_bad << " failing, " << unnamed
              << " user bin(s) of the index not named by the input, " << looked_up << " distinct minimisers looked up, max_observed_fp ";
    if (fp_pass)
        std::cout << fp_max / P << ", mean_observed_fp " << (n_checked ? fp_sum / P / (double)n_checked : 0.0);
    else
        std::cout << "n/a, mean_observed_fp n/a";
    std::cout << std::endl;
    return n_bad == 0 && n_checked > 0;
}

bool run_verify(const Config& c, std::vector<Target>& targets, const Lap& counting)
{
    auto t0 = std::chrono::steady_clock::now();
    for (Target& tg : targets)
        if (!unite_files(c, tg))
            return fail(gn_last_error());
    const double hash_s = counting.seconds() + since(t0);
    // the parts the index is checked in: one when it fits what an entry of the list may hold at one time
    const std::vector<int> entries = c.verify_devices.empty() ? std::vector<int>{ c.device } : c.verify_devices;
    {
        gnhost::FilterMeta    meta;
        std::vector<uint64_t> payload_at;
        try
        {
            gnhost::read_hibf_meta(c.verify_index, meta, payload_at);
        }
        catch (const std::exception& e)
        {
            return fail(std::string("ERROR: ") + e.what());
        }
        uint64_t budget = c.verify_memory;
        if (!c.verify_memory_given)
        {
            std::string why;
            if (!budget_from_free_memory(entries, budget, why))
                return fail(why);
        }
        HibfPartPlan plan;
        try
        {
            std::vector<uint64_t> rows, row_bytes;
            for (const gnhost::IbfShape& m : meta.shapes)
                rows.push_back(m.bin_size), row_bytes.push_back(gn_hibf_row_stride_words(m.bin_words) * 8);
            plan = plan_hibf_parts(rows, row_bytes, budget, (uint32_t)entries.size());
        }
        catch (const std::exception& e)
        {
            return fail(std::string(c.verify_memory_given ? "--verify-memory: " : "--verify-devices: ") + e.what());
        }
        if (plan.n_parts > 1)
            return run_verify_parts(c, targets, meta, payload_at, plan, entries, hash_s);
    }
    try
    {
        t0 = std::chrono::steady_clock::now();
        gnhost::FilterMeta meta;
        gnhost::DeviceSink sink(entries[0]);
        gnhost::load_filter_file(c.verify_index, true, meta, sink);
        gn_filter* const flt    = sink.filter();
        const double     load_s = since(t0);
        std::vector<uint64_t> bins;
        for (const gnhost::IbfShape& m : meta.shapes)
            bins.push_back(m.bins);
        const gnhibf::Paths paths  = gnhibf::derive_paths(bins, meta.next_ibf_id, meta.bin_to_user, meta.n_user_bins);
        const uint32_t      depth  = paths.depth;
        const uint64_t      n_user = meta.n_user_bins;
        const unsigned      k = meta.ibf_config.kmer_size, h = (unsigned)meta.shapes.at(0).hash_funs;
        const double        fpr = meta.ibf_config.max_fp;
        std::map<std::string, uint64_t> user_of; // names as the loader recovers them -> user bin
        for (size_t t = 0; t < meta.targets.size(); ++t)
            user_of[meta.targets[t]] = meta.target_bins[t].at(0);

        // membership: every target's set along its user bin's path, pooled as run_hibf pools its inserts
        t0 = std::chrono::steady_clock::now();
        constexpr uint64_t    none = ~0ull;
        std::vector<uint64_t> user(targets.size(), none), found(targets.size(), 0), first_lost(targets.size(), none);
        std::vector<uint64_t> lost_at(targets.size() * (size_t)depth, 0);
        uint64_t              looked_up = 0;
        {
            std::vector<size_t> asked; // the targets with a user bin and a hash
            for (size_t t = 0; t < targets.size(); ++t)
            {
                auto it = user_of.find(name_as_read(targets[t].name));
                if (it == user_of.end())
                    continue;
                user[t] = it->second;
                if (targets[t].hashes.empty())
                    continue;
                looked_up += targets[t].hashes.size();
                asked.push_back(t);
            }
            std::vector<uint64_t> r_found, r_lost, r_first;
            gnhibf::for_each_pooled(
                asked.size(),
                [&](size_t j) { return hash_set(targets[asked[j]]); },
                [&](size_t j) { return &paths.entries[user[asked[j]] * depth]; }, depth,
                [&](const uint64_t* hashes, const uint64_t* set_off, size_t n, const gn_path_entry* p, const std::vector<size_t>& ids) {
                    r_found.assign(n, 0), r_first.assign(n, none), r_lost.assign(n * (size_t)depth, 0);
                    if (gn_filter_probe_path(flt, hashes, set_off, (uint32_t)n, p, depth, r_found.data(), r_lost.data(), r_first.data()) != GN_OK)
                        throw std::runtime_error(gn_last_error());
                    for (size_t j = 0; j < n; ++j)
                    {
                        const size_t t = asked[ids[j]];
                        found[t] = r_found[j], first_lost[t] = r_first[j];
                        std::copy(r_lost.begin() + j * depth, r_lost.begin() + (j + 1) * depth, lost_at.begin() + t * depth);
                    }
                });
        }
        const double member_s = since(t0);

        // false positives: the same P probes against every user bin of the file, paths sorted by (leaf ibf, first bin)
        t0 = std::chrono::steady_clock::now();
        const bool            fp_pass = k <= 31; // (k = 32: a hash can take any 64-bit value, no probe is a certain negative)
        std::vector<uint64_t> false_hits(n_user, 0);
        if (fp_pass && n_user)
        {
            const std::vector<uint64_t> probes = verify_probes(), order = verify_fp_order(paths, n_user);
            std::vector<uint64_t>       got(n_user, 0);
            std::vector<gn_path_entry> sorted;
            for (uint64_t u : order)
                sorted.insert(sorted.end(), paths.entries.begin() + u * depth, paths.entries.begin() + (u + 1) * depth);
            if (gn_filter_probe_paths_shared(flt, probes.data(), probes.size(), sorted.data(), (uint32_t)n_user, depth, got.data()) != GN_OK)
                throw std::runtime_error(gn_last_error());
            for (uint64_t j = 0; j < n_user; ++j)
                false_hits[order[j]] = got[j];
        }
        const double fp_s = since(t0);
        // the first false negative of a target: the first entry of the path that lacks the hash, its h rows there and their words
        auto lookup = [&](const gn_path_entry* p, uint32_t used, uint64_t v, std::vector<uint64_t>& rows, std::vector<uint64_t>& words) {
            const uint64_t        one[2] = { 0, 1 };
            uint64_t              f1 = 0, fl = 0;
            std::vector<uint64_t> l1(depth, 0);
            if (gn_filter_probe_path(flt, &v, one, 1, p, depth, &f1, l1.data(), &fl) != GN_OK)
                throw std::runtime_error(gn_last_error());
            uint32_t d = 0;
            while (d + 1 < used && l1[d] == 0)
                ++d;
            const gnhost::IbfShape& m = meta.shapes.at(p[d].ibf);
            rows.resize(m.hash_funs), words.resize(m.hash_funs * m.bin_words);
            for (unsigned i = 0; i < m.hash_funs; ++i)
                rows[i] = gnhost::ibf_row(v, i, m);
            if (gn_filter_download_row_list(flt, p[d].ibf, rows.data(), rows.size(), words.data()) != GN_OK)
                throw std::runtime_error(gn_last_error());
            return d;
        };
        const VerifyCounts counts{ user, found, first_lost, false_hits, looked_up, fp_pass };
        const bool         ok = print_verify_report(c, targets, meta, paths, counts, lookup);
        if (c.verbose && !c.quiet)
            std::cerr << std::setprecision(6) << " - seconds: hash " << hash_s << " load " << load_s << " membership " << member_s << " fp " << fp_s << std::endl;
        return ok;
    }
    catch (const std::exception& e)
    {
        return fail(std::string("ERROR: ") + e.what());
    }
}

} // namespace gnbuild
