// hibf_extend_driver.cpp -- test harness: runs the PRODUCT's plan of `ganon-build --hibf --update --extend` (deal_run, plan_extend and
// plan_update started from the extensions' fills, ganon_amd/host/hibf_update.hpp) so that tests/test_build_extend_cpu.py can check it.
// One case per line of stdin:
//   deal <m> <h> <a> <s> t[0..s)
//   extend <fpr> <h> <n_user> <n_ibf> { <bins> <rows> next_ibf_id[0..bins) bin_to_user[0..bins) popcounts[0..bins) } per IBF
//          <n_ext> <depth> { <user_bin> <hashes> lost_at[0..depth) } per extension  <n_new> c_0 ... c_{n_new-1}
// stdout: quotas q[0..s)                                                              (deal)
//         case <depth> <n_user_bins after>                                            (extend; then, in this order)
//         quota <extension> q[0..bins of its run)
//         run <ibf> <bin> <dealt> <bits_before> <bits_predicted as %.17g>
//         merged <ibf> <bin> <bits_before> <bits_predicted>                           the merged bins on extended paths
//         over <extension> <ibf> <bin> <bits_predicted> <bound>
//         path <new index> <entry> <ibf> <first_bin> <n_bins> <hashes_per_bin>        of the new user bins, placed with the carried fills
//         touched <ibf> <bin> <bits_before> <bits_predicted>                          the merged bins the new user bins pass through
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
        if (what != "deal" && what != "extend")
            continue;
        auto unreadable = []() { throw std::runtime_error("driver: unreadable case"); };
        try
        {
            if (what == "deal")
            {
                uint64_t m = 0, a = 0, s = 0;
                unsigned h = 0;
                in >> m >> h >> a >> s;
                if (!in || s > 1000000 || h > 255)
                    unreadable();
                std::vector<uint64_t> t(s);
                for (auto& v : t)
                    in >> v;
                if (!in)
                    unreadable();
                const std::vector<uint64_t> q = gnhibf::deal_run(t, m, (uint8_t)h, a);
                std::printf("quotas");
                for (uint64_t v : q)
                    std::printf(" %llu", (unsigned long long)v);
                std::printf("\n");
                continue;
            }
            double   fpr = 0;
            unsigned h   = 0;
            uint64_t n_user = 0, n_ibf = 0;
            in >> fpr >> h >> n_user >> n_ibf;
            if (!in || n_ibf > 100000 || h > 255)
                unreadable();
            std::vector<uint64_t>              bins(n_ibf), rows(n_ibf);
            std::vector<std::vector<int64_t>>  nx(n_ibf), bu(n_ibf);
            std::vector<std::vector<uint64_t>> pop(n_ibf);
            for (uint64_t i = 0; i < n_ibf; ++i)
            {
                in >> bins[i] >> rows[i];
                if (!in || bins[i] > 1000000)
                    unreadable();
                nx[i].resize(bins[i]), bu[i].resize(bins[i]), pop[i].resize(bins[i]);
                for (auto& v : nx[i])
                    in >> v;
                for (auto& v : bu[i])
                    in >> v;
                for (auto& v : pop[i])
                    in >> v;
            }
            uint64_t n_ext = 0, depth = 0, n_new = 0;
            in >> n_ext >> depth;
            if (!in || n_ext > 1000000 || depth > 64)
                unreadable();
            std::vector<gnhibf::ExtendInput> ext(n_ext);
            for (auto& e : ext)
            {
                in >> e.user_bin >> e.hashes;
                e.lost_at.resize(depth);
                for (auto& v : e.lost_at)
                    in >> v;
            }
            in >> n_new;
            if (!in || n_new > 1000000)
                unreadable();
            std::vector<uint64_t> fresh(n_new);
            for (auto& c : fresh)
                in >> c;
            if (!in)
                unreadable();
            const gnhibf::Paths      old = gnhibf::derive_paths(bins, nx, bu, n_user);
            const gnhibf::ExtendPlan ex  = gnhibf::plan_extend(old, bins, rows, (uint8_t)h, fpr, pop, ext);
            const gnhibf::UpdatePlan up  = gnhibf::plan_update(bins, rows, nx, bu, n_user, (uint8_t)h, fpr, pop, fresh, &ex.fills);
            std::printf("case %u %llu\n", old.depth, (unsigned long long)up.n_user_bins);
            for (size_t x = 0; x < ex.quotas.size(); ++x)
            {
                std::printf("quota %zu", x);
                for (uint64_t v : ex.quotas[x])
                    std::printf(" %llu", (unsigned long long)v);
                std::printf("\n");
            }
            for (const gnhibf::ExtendRunBin& r : ex.run)
                std::printf("run %u %u %llu %llu %.17g\n", r.ibf, r.bin, (unsigned long long)r.dealt, (unsigned long long)r.bits_before, r.bits_predicted);
            for (const gnhibf::UpdateTouched& t : ex.touched)
                std::printf("merged %u %u %llu %.17g\n", t.ibf, t.bin, (unsigned long long)t.bits_before, t.bits_predicted);
            for (const gnhibf::ExtendOver& o : ex.over)
                std::printf("over %u %u %u %.17g %.17g\n", o.extension, o.ibf, o.bin, o.bits_predicted, o.bound);
            for (size_t j = 0; j < up.paths.entries.size(); ++j)
            {
                const gn_path_entry& e = up.paths.entries[j];
                std::printf("path %zu %zu %u %u %u %llu\n", j / up.paths.depth, j % up.paths.depth, e.ibf, e.first_bin, e.n_bins, (unsigned long long)e.hashes_per_bin);
            }
            for (const gnhibf::UpdateTouched& t : up.touched)
                std::printf("touched %u %u %llu %.17g\n", t.ibf, t.bin, (unsigned long long)t.bits_before, t.bits_predicted);
        }
        catch (const std::exception& e)
        {
            std::printf("refused %s\n", e.what());
        }
    }
    return 0;
}
