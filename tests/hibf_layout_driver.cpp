// hibf_layout_driver.cpp -- test harness: runs the PRODUCT's HIBF layout (ganon_amd/host/hibf_layout.hpp) and sizing
// (gnbuild::hibf_run_bits) on counts given on stdin and prints the tree, so that tests/test_build_hibf_cpu.py can check it.
// stdin:  tmax max_fp hash_functions shared_percent n  c_0 ... c_{n-1}      (one case per line)
//         a merged bin is given the made-up cardinality max(largest member, sum of members * (100 - shared_percent) / 100)
// stdout: case <ibfs> <levels> <L>
//         ibf <index> <bins> <rows> <parent> <parent_bin> <depth> <runs>
//         run <first> <n_bins> <user> <child> <hashes>
#include "../ganon_amd/host/build_params.hpp"
#include "../ganon_amd/host/hibf_layout.hpp"

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
        uint64_t           tmax, shared, n;
        double             max_fp;
        unsigned           h;
        in >> tmax >> max_fp >> h >> shared >> n;
        std::vector<uint64_t> counts(n);
        for (auto& c : counts)
            in >> c;
        const gnhibf::Layout lay = gnhibf::lay_out(counts, (uint32_t)tmax);
        std::printf("case %zu %u %u\n", lay.ibfs.size(), lay.levels, gnhibf::levels_for(n, tmax));
        for (size_t i = 0; i < lay.ibfs.size(); ++i)
        {
            const gnhibf::Ibf&    f = lay.ibfs[i];
            std::vector<uint64_t> hashes;
            uint64_t              rows = 0;
            for (const gnhibf::Run& r : f.runs)
            {
                uint64_t c = 0;
                if (r.user >= 0)
                    c = counts[r.user];
                else
                {
                    uint64_t sum = 0, top = 0;
                    for (uint32_t u : lay.ibfs[r.child].members)
                        sum += counts[u], top = std::max(top, counts[u]);
                    c = std::max(top, sum * (100 - shared) / 100);
                }
                hashes.push_back(c);
                rows = std::max(rows, gnbuild::hibf_run_bits(c, r.n_bins, max_fp, (uint8_t)h));
            }
            std::printf("ibf %zu %u %llu %lld %u %u %zu\n", i, f.bins, (unsigned long long)rows, (long long)f.parent, f.parent_bin, f.depth, f.runs.size());
            for (size_t j = 0; j < f.runs.size(); ++j)
                std::printf("run %u %u %lld %lld %llu\n", f.runs[j].first, f.runs[j].n_bins, (long long)f.runs[j].user, (long long)f.runs[j].child,
                            (unsigned long long)hashes[j]);
        }
    }
    return 0;
}
