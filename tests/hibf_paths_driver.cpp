// hibf_paths_driver.cpp -- test harness: runs the PRODUCT's path derivation (ganon_amd/host/hibf_paths.hpp) so that
// tests/test_build_verify_cpu.py can check it.  One case per line of stdin:
//   layout <tmax> <n> c_0 ... c_{n-1}      gnhibf::lay_out -> tables_of -> derive_paths, and paths_of of the same layout (what the builder
//                                          inserts along)
//   tables <n_user> <n_ibf> { <bins> next_ibf_id[0..bins) bin_to_user[0..bins) } per IBF      derive_paths of hand-made tables
// stdout: case <depth> <levels | -1>
//         derived <user> <entry> <ibf> <first_bin> <n_bins>      every entry of every user bin, unused ones (n_bins 0) too
//         built   <user> <entry> <ibf> <first_bin> <n_bins>      (layout only)
//     or  refused <message>
#include "../ganon_amd/host/hibf_paths.hpp"

#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

static void print(const char* tag, const gnhibf::Paths& p)
{
    for (size_t j = 0; j < p.entries.size(); ++j)
        std::printf("%s %zu %zu %u %u %u\n", tag, j / p.depth, j % p.depth, p.entries[j].ibf, p.entries[j].first_bin, p.entries[j].n_bins);
}

int main()
{
    std::string line;
    while (std::getline(std::cin, line))
    {
        std::istringstream in(line);
        std::string        what;
        in >> what;
        std::vector<uint64_t>             bins;
        std::vector<std::vector<int64_t>> nx, bu;
        uint64_t                          n_user = 0;
        gnhibf::Layout                    lay;
        std::vector<uint64_t>             counts;
        if (what == "layout")
        {
            uint64_t tmax, n;
            in >> tmax >> n;
            counts.resize(n);
            for (auto& c : counts)
                in >> c;
            lay    = gnhibf::lay_out(counts, (uint32_t)tmax);
            n_user = n;
            nx.resize(lay.ibfs.size()), bu.resize(lay.ibfs.size());
            for (uint32_t i = 0; i < lay.ibfs.size(); ++i)
            {
                bins.push_back(lay.ibfs[i].bins);
                gnhibf::tables_of(lay, i, nx[i], bu[i]);
            }
        }
        else if (what == "tables")
        {
            uint64_t n_ibf;
            in >> n_user >> n_ibf;
            bins.resize(n_ibf), nx.resize(n_ibf), bu.resize(n_ibf);
            for (uint64_t i = 0; i < n_ibf; ++i)
            {
                in >> bins[i];
                nx[i].resize(bins[i]), bu[i].resize(bins[i]);
                for (auto& v : nx[i])
                    in >> v;
                for (auto& v : bu[i])
                    in >> v;
            }
        }
        else
            continue;
        try
        {
            const gnhibf::Paths derived = gnhibf::derive_paths(bins, nx, bu, n_user);
            std::printf("case %u %d\n", derived.depth, what == "layout" ? (int)lay.levels : -1);
            print("derived", derived);
            if (what == "layout")
                print("built", gnhibf::paths_of(lay, counts));
        }
        catch (const std::exception& e)
        {
            std::printf("refused %s\n", e.what());
        }
    }
    return 0;
}
