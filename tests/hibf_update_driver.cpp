// hibf_update_driver.cpp -- test harness: runs the PRODUCT's update placement (ganon_amd/host/hibf_update.hpp) so that
// tests/test_build_update_cpu.py can check it.  One case per line of stdin:
//   update <fpr> <h> <n_user> <n_ibf> { <bins> <rows> next_ibf_id[0..bins) bin_to_user[0..bins) popcounts[0..bins) } per IBF  <n_new> c_0 ... c_{n_new-1}
//   layout <fpr> <h> <tmax> <fill_percent> <n> c_0 ... c_{n-1} <n_new> d_0 ... d_{n_new-1}
//          gnhibf::lay_out of the n counts, rows sized as the builder sizes them with a merged bin holding the sum of its members, and
//          popcounts synthesised from the textbook fill rows * (1 - exp(-h * share / rows)) scaled by fill_percent / 100
// stdout: case <n_ibf> <depth> <n_user_bins>
//         table <ibf> <bins> <rows> next_ibf_id[0..bins) bin_to_user[0..bins)       the NEW tables
//         pop <ibf> popcounts[0..old bins)                                           (layout only: what the plan was made from)
//         old <ibf> <old bins> next_ibf_id[0..old bins) bin_to_user[0..old bins)     (layout only)
//         path <new index> <entry> <ibf> <first_bin> <n_bins> <hashes_per_bin>       every entry, unused ones (n_bins 0) too
//         touched <ibf> <bin> <bits_before> <bits_predicted as %.17g>
//     or  refused <message>
// A line that cannot be read in full is refused as such.
#include "../ganon_amd/host/hibf_update.hpp"

#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

int main()
{
    std::string line;
    while (std::getline(std::cin, line))
    {
        std::istringstream in(line);
        std::string        what;
        in >> what;
        if (what != "update" && what != "layout")
            continue;
        double                            fpr = 0;
        unsigned                          h = 0;
        uint64_t                          n_user = 0, n_ibf = 0;
        std::vector<uint64_t>             bins, rows, fresh;
        std::vector<std::vector<int64_t>> nx, bu;
        std::vector<std::vector<uint64_t>> pop;
        try
        {
            in >> fpr >> h;
            if (what == "update")
            {
                in >> n_user >> n_ibf;
                if (!in || n_ibf > 100000)
                    throw std::runtime_error("driver: unreadable case");
                bins.resize(n_ibf), rows.resize(n_ibf), nx.resize(n_ibf), bu.resize(n_ibf), pop.resize(n_ibf);
                for (uint64_t i = 0; i < n_ibf; ++i)
                {
                    in >> bins[i] >> rows[i];
                    if (!in || bins[i] > 1000000)
                        throw std::runtime_error("driver: unreadable case");
                    nx[i].resize(bins[i]), bu[i].resize(bins[i]), pop[i].resize(bins[i]);
                    for (auto& v : nx[i])
                        in >> v;
                    for (auto& v : bu[i])
                        in >> v;
                    for (auto& v : pop[i])
                        in >> v;
                }
            }
            else
            {
                uint64_t tmax = 0, percent = 0, n = 0;
                in >> tmax >> percent >> n;
                if (!in || n > 1000000 || h < 1 || h > 5 || !(fpr > 0.0 && fpr < 1.0))
                    throw std::runtime_error("driver: unreadable case");
                std::vector<uint64_t> counts(n);
                for (auto& c : counts)
                    in >> c;
                const gnhibf::Layout lay = gnhibf::lay_out(counts, (uint32_t)tmax);
                n_user                   = n;
                n_ibf                    = lay.ibfs.size();
                bins.resize(n_ibf), rows.assign(n_ibf, 1), nx.resize(n_ibf), bu.resize(n_ibf), pop.resize(n_ibf);
                std::vector<std::vector<uint64_t>> hashes(n_ibf);
                for (uint64_t i = 0; i < n_ibf; ++i)
                {
                    const gnhibf::Ibf& f = lay.ibfs[i];
                    bins[i]              = f.bins;
                    gnhibf::tables_of(lay, (uint32_t)i, nx[i], bu[i]);
                    for (const gnhibf::Run& r : f.runs)
                    {
                        uint64_t c = 0;
                        if (r.user >= 0)
                            c = counts[r.user];
                        else
                            for (uint32_t u : lay.ibfs[r.child].members)
                                c += counts[u];
                        hashes[i].push_back(c);
                        rows[i] = std::max(rows[i], gnbuild::hibf_run_bits(c, r.n_bins, fpr, (uint8_t)h));
                    }
                }
                for (uint64_t i = 0; i < n_ibf; ++i)
                {
                    const gnhibf::Ibf& f = lay.ibfs[i];
                    pop[i].assign(f.bins, 0);
                    for (size_t j = 0; j < f.runs.size(); ++j)
                    {
                        const uint64_t share = (hashes[i][j] + f.runs[j].n_bins - 1) / f.runs[j].n_bins;
                        const double   fill  = rows[i] * (1.0 - std::exp(-(double)h * share / rows[i])) * percent / 100.0;
                        for (uint32_t b = f.runs[j].first; b < f.runs[j].first + f.runs[j].n_bins; ++b)
                            pop[i][b] = std::min<uint64_t>(rows[i], (uint64_t)fill);
                    }
                }
            }
            uint64_t n_new = 0;
            in >> n_new;
            if (!in || n_new > 1000000)
                throw std::runtime_error("driver: unreadable case");
            fresh.resize(n_new);
            for (auto& c : fresh)
                in >> c;
            if (!in)
                throw std::runtime_error("driver: unreadable case");
            const gnhibf::UpdatePlan plan = gnhibf::plan_update(bins, rows, nx, bu, n_user, (uint8_t)h, fpr, pop, fresh);
            std::printf("case %zu %u %llu\n", plan.bins.size(), plan.paths.depth, (unsigned long long)plan.n_user_bins);
            for (size_t i = 0; i < plan.bins.size(); ++i)
            {
                std::printf("table %zu %llu %llu", i, (unsigned long long)plan.bins[i], (unsigned long long)rows[i]);
                for (int64_t v : plan.next_ibf_id[i])
                    std::printf(" %lld", (long long)v);
                for (int64_t v : plan.bin_to_user[i])
                    std::printf(" %lld", (long long)v);
                std::printf("\n");
                if (what == "layout")
                {
                    std::printf("pop %zu", i);
                    for (uint64_t v : pop[i])
                        std::printf(" %llu", (unsigned long long)v);
                    std::printf("\nold %zu %llu", i, (unsigned long long)bins[i]);
                    for (int64_t v : nx[i])
                        std::printf(" %lld", (long long)v);
                    for (int64_t v : bu[i])
                        std::printf(" %lld", (long long)v);
                    std::printf("\n");
                }
            }
            for (size_t j = 0; j < plan.paths.entries.size(); ++j)
            {
                const gn_path_entry& e = plan.paths.entries[j];
                std::printf("path %zu %zu %u %u %u %llu\n", j / plan.paths.depth, j % plan.paths.depth, e.ibf, e.first_bin, e.n_bins, (unsigned long long)e.hashes_per_bin);
            }
            for (const gnhibf::UpdateTouched& t : plan.touched)
                std::printf("touched %u %u %llu %.17g\n", t.ibf, t.bin, (unsigned long long)t.bits_before, t.bits_predicted);
        }
        catch (const std::exception& e)
        {
            std::printf("refused %s\n", e.what());
        }
    }
    return 0;
}
