// hibf_pool_driver.cpp -- test harness: runs the PRODUCT's set pooler (ganon_amd/host/hibf_pool.hpp) with a recording `call` so that
// tests/test_build_pool_cpu.py can check which sets go to the device together.  One case per line of stdin:
//   <alone> <batch> <n> size_0 ... size_{n-1}      (alone = batch = 0: the header's defaults)
// Set i holds the values (i << 32) + 0 .. size_i - 1 and has the two-entry path (ibf i, first_bin 2i), (ibf i, first_bin 2i + 1).
// stdout: defaults <batch> <alone>                  once, first
//         case <n>
//         call own|pool ids=<i,..> offsets=<o,..> paths=<ibf:first_bin,..> data=ok|bad      one per call, in order; own = the hash
//                                                   pointer was set ids[0]'s own storage; data = the hashes of every set lie where
//                                                   the offsets say
//         end
#include "../ganon_amd/host/hibf_pool.hpp"

#include <algorithm>
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

int main()
{
    std::printf("defaults %llu %llu\n", (unsigned long long)gnhibf::kPoolBatch, (unsigned long long)gnhibf::kPoolAlone);
    constexpr uint32_t depth = 2;
    std::string        line;
    while (std::getline(std::cin, line))
    {
        std::istringstream in(line);
        uint64_t           alone = 0, batch = 0, n = 0;
        if (!(in >> alone >> batch >> n))
            continue;
        std::vector<std::vector<uint64_t>> sets(n);
        std::vector<gn_path_entry>         paths(n * depth);
        for (uint64_t i = 0; i < n; ++i)
        {
            uint64_t size = 0;
            in >> size;
            for (uint64_t k = 0; k < size; ++k)
                sets[i].push_back((i << 32) + k);
            for (uint32_t d = 0; d < depth; ++d)
                paths[i * depth + d] = gn_path_entry{ (uint32_t)i, (uint32_t)(2 * i + d), 1, 0, 0 };
        }
        std::printf("case %llu\n", (unsigned long long)n);
        auto set_of  = [&](size_t i) { return std::pair<const uint64_t*, uint64_t>(sets[i].data(), sets[i].size()); };
        auto path_of = [&](size_t i) { return &paths[i * depth]; };
        auto call    = [&](const uint64_t* hashes, const uint64_t* off, size_t m, const gn_path_entry* p, const std::vector<size_t>& ids) {
            bool good = ids.size() == m && off[0] == 0;
            std::printf("call %s ids=", m == 1 && !sets[ids[0]].empty() && hashes == sets[ids[0]].data() ? "own" : "pool");
            for (size_t j = 0; j < m; ++j)
            {
                std::printf("%s%zu", j ? "," : "", ids[j]);
                const std::vector<uint64_t>& s = sets[ids[j]];
                good = good && off[j + 1] - off[j] == s.size() && std::equal(s.begin(), s.end(), hashes + off[j]);
            }
            std::printf(" offsets=");
            for (size_t j = 0; j <= m; ++j)
                std::printf("%s%llu", j ? "," : "", (unsigned long long)off[j]);
            std::printf(" paths=");
            for (size_t j = 0; j < m * depth; ++j)
                std::printf("%s%u:%u", j ? "," : "", p[j].ibf, p[j].first_bin);
            std::printf(" data=%s\n", good ? "ok" : "bad");
        };
        if (alone == 0 && batch == 0)
            gnhibf::for_each_pooled(n, set_of, path_of, depth, call);
        else
            gnhibf::for_each_pooled(n, set_of, path_of, depth, call, batch, alone);
        std::printf("end\n");
    }
    return 0;
}
