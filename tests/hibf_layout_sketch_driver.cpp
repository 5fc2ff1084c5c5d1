// hibf_layout_sketch_driver.cpp -- test harness: runs the PRODUCT's size-aware HIBF layout (ganon_amd/host/hibf_layout_sketch.hpp)
// with EXACT sums as its union estimates -- the user bins are taken to be disjoint sets -- and prints the tree in the format of
// hibf_layout_driver.cpp, so that tests/test_build_sketch_cpu.py can check it and compare it with the rule's tree.
// stdin:  layout tmax max_fp hash_functions n  c_0 ... c_{n-1}      (one case per line; layout = sketch | rule)
// stdout: case <ibfs> <levels> <L>
//         ibf <index> <bins> <rows> <parent> <parent_bin> <depth> <runs>
//         run <first> <n_bins> <user> <child> <hashes>          (a merged bin holds the sum of the counts below it)
//         asked <estimates asked for> <longest> <width>         (sketch only)
#include "../ganon_amd/host/build_params.hpp"
#include "../ganon_amd/host/hibf_layout.hpp"
#include "../ganon_amd/host/hibf_layout_sketch.hpp"

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
        std::string        which;
        uint64_t           tmax, n;
        double             max_fp;
        unsigned           h;
        in >> which >> tmax >> max_fp >> h >> n;
        std::vector<uint64_t> counts(n);
        for (auto& c : counts)
            in >> c;
        const std::vector<uint32_t> order = gnhibf::sketch_order(counts);
        std::vector<uint64_t>       prefix(n + 1, 0);
        for (uint64_t i = 0; i < n; ++i)
            prefix[i + 1] = prefix[i] + counts[order[i]];
        uint64_t                    asked = 0, longest = 0;
        const gnhibf::UnionEstimate exact = [&](uint64_t j, uint64_t l) {
            ++asked;
            longest = std::max(longest, l);
            if (l < 2 || j + l > n)
                std::abort(); // outside what the header says is asked for
            return prefix[j + l] - prefix[j];
        };
        const gnhibf::Layout lay = which == "sketch" ? gnhibf::lay_out_sketch(counts, (uint32_t)tmax, max_fp, (uint8_t)h, exact)
                                                     : gnhibf::lay_out(counts, (uint32_t)tmax);
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
                    for (uint32_t u : lay.ibfs[r.child].members)
                        c += counts[u];
                hashes.push_back(c);
                rows = std::max(rows, gnbuild::hibf_run_bits(c, r.n_bins, max_fp, (uint8_t)h));
            }
            std::printf("ibf %zu %u %llu %lld %u %u %zu\n", i, f.bins, (unsigned long long)rows, (long long)f.parent, f.parent_bin, f.depth, f.runs.size());
            for (size_t j = 0; j < f.runs.size(); ++j)
                std::printf("run %u %u %lld %lld %llu\n", f.runs[j].first, f.runs[j].n_bins, (long long)f.runs[j].user, (long long)f.runs[j].child,
                            (unsigned long long)hashes[j]);
        }
        if (which == "sketch")
            std::printf("asked %llu %llu %llu\n", (unsigned long long)asked, (unsigned long long)longest, (unsigned long long)gnhibf::sketch_width(n, tmax));
    }
    return 0;
}
