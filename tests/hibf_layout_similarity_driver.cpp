// hibf_layout_similarity_driver.cpp -- test harness: runs the PRODUCT's similarity order and layout
// (ganon_amd/host/hibf_layout_similarity.hpp) with EXACT unions as its estimates -- of explicit sets, or sums when the user bins are
// taken to be disjoint -- or, for the order alone, with a table of pair estimates the test brings (the device's).  The tree is
// printed in the format of hibf_layout_sketch_driver.cpp, so that tests/test_build_similarity_cpu.py can compare the two line for
// line.
// stdin, one case, tokens separated by white space:
//     mode tmax max_fp hash_functions n source   c_0 ... c_{n-1}   <what the source needs>
//     mode   = order | similarity | sketch | rule
//     source = disjoint                 nothing more: every union is the sum of the counts
//            | sets                     the c_u values of user bin u, for u = 0 .. n - 1
//            | noisy                    nothing more: strangers as a sketch sees them -- the sum of the counts, off by a relative error
//                                       of standard deviation 1 / 64 that depends on which user bins are united and on nothing else
//            | matrix                   (order only) n * n values, U[u * n + v] = the union of user bins u and v
// stdout, order:  intervals <k> <start_0> ... <start_{k-1}>
//                 order <u_0> ... <u_{n-1}>
//                 tables <pair tables asked for> <largest, in positions>
//         others: case / ibf / run lines and the last line `asked <estimates asked for> <longest> <width>` as hibf_layout_sketch_driver
//                 prints them (a merged bin holds the exact union of the sets below it)
// stderr, similarity: similarity <intervals> <moved> <kept> <bits>;  sketch: sketch <bits> <kept>
#include "../ganon_amd/host/build_params.hpp"
#include "../ganon_amd/host/hibf_layout.hpp"
#include "../ganon_amd/host/hibf_layout_similarity.hpp"
#include "../ganon_amd/host/hibf_layout_sketch.hpp"

#include <cstdio>
#include <iostream>
#include <memory>
#include <string>

int main()
{
    std::string mode, source;
    uint64_t    tmax, n;
    double      max_fp;
    unsigned    h;
    std::ios::sync_with_stdio(false);
    std::cin >> mode >> tmax >> max_fp >> h >> n >> source;
    std::vector<uint64_t> counts(n);
    for (auto& c : counts)
        std::cin >> c;
    std::vector<std::vector<uint64_t>> sets;
    std::vector<uint64_t>              matrix;
    if (source == "sets")
    {
        sets.resize(n);
        for (uint64_t u = 0; u < n; ++u)
        {
            sets[u].resize(counts[u]);
            for (auto& v : sets[u])
                std::cin >> v;
        }
    }
    else if (source == "matrix")
    {
        matrix.resize(n * n);
        for (auto& v : matrix)
            std::cin >> v;
    }
    if (!std::cin || (source == "matrix" && mode != "order"))
    {
        std::fprintf(stderr, "bad input\n");
        return 2;
    }
    // every value becomes its rank among all values, so that a union is counted with one mark per rank
    std::vector<uint32_t> mark;
    uint32_t              round = 0;
    {
        std::vector<uint64_t> all;
        for (const auto& set : sets)
            all.insert(all.end(), set.begin(), set.end());
        std::sort(all.begin(), all.end());
        all.erase(std::unique(all.begin(), all.end()), all.end());
        for (auto& set : sets)
            for (auto& v : set)
                v = (uint64_t)(std::lower_bound(all.begin(), all.end(), v) - all.begin());
        mark.assign(all.size(), 0);
    }
    auto add = [&](uint32_t u) { // how many values of user bin u the current round has not seen yet
        uint64_t fresh = 0;
        for (uint64_t v : sets[u])
            if (mark[v] != round)
                mark[v] = round, ++fresh;
        return fresh;
    };
    // noisy: the sum of the counts of two or more user bins, `key` the sum of mix(u + 1) over them.  Twelve uniform 16-bit values,
    // centred, have standard deviation 65536 and are as good as normal out to six of them.
    auto mix = [](uint64_t x) {
        x += 0x9E3779B97F4A7C15ull;
        x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
        x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
        return x ^ (x >> 31);
    };
    auto noise = [&](uint64_t sum, uint64_t key) {
        int64_t z = -12 * 32768 + 6;
        for (int r = 0; r < 3; ++r)
        {
            key = mix(key + r);
            for (int f = 0; f < 64; f += 16)
                z += (int64_t)((key >> f) & 0xFFFF);
        }
        return (uint64_t)((int64_t)sum + (int64_t)((__int128)sum * z / (65536 * 64)));
    };
    // the exact union of some user bins (noisy: what a sketch would make of it)
    auto united = [&](const uint32_t* first, uint64_t l) {
        uint64_t sum = 0, key = 0;
        ++round;
        if (source == "noisy")
        {
            for (uint64_t i = 0; i < l; ++i)
                sum += counts[first[i]], key += mix(first[i] + 1);
            return l < 2 ? sum : noise(sum, key);
        }
        for (uint64_t i = 0; i < l; ++i)
            sum += source == "sets" ? add(first[i]) : counts[first[i]];
        return sum;
    };
    const std::vector<uint32_t> size_order = gnhibf::sketch_order(counts);
    const uint64_t              width      = gnhibf::sketch_width(n, tmax);
    uint64_t                    asked = 0, longest = 0, n_tables = 0, largest = 0;

    const gnhibf::IntervalPairs pairs = [&](uint64_t a, uint64_t b) -> gnhibf::PairEstimate {
        ++n_tables;
        largest = std::max(largest, b - a);
        if (b - a < 3 || b > n || b - a > gnhibf::kSimilarityWindow)
            std::abort(); // outside what the header says is asked for
        return [&, a, b](uint64_t p, uint64_t q) -> uint64_t {
            if (p >= b - a || q >= b - a)
                std::abort();
            const uint32_t two[2] = { size_order[a + p], size_order[a + q] };
            if (source == "matrix")
                return matrix[(uint64_t)two[0] * n + two[1]];
            return two[0] == two[1] ? counts[two[0]] : united(two, 2);
        };
    };
    // every union of up to `width` neighbours of an order, as the builder's table holds them
    const gnhibf::OrderUnions unions = [&](const std::vector<uint32_t>& order) -> gnhibf::UnionEstimate {
        auto table = std::make_shared<std::vector<uint64_t>>(n * width, 0);
        for (uint64_t j = 0; j < n; ++j)
        {
            uint64_t sum = 0, key = 0, best = 0;
            ++round;
            for (uint64_t l = 1; l <= width && j + l <= n; ++l)
            {
                sum += source == "sets" ? add(order[j + l - 1]) : counts[order[j + l - 1]];
                key += mix(order[j + l - 1] + 1);
                best = std::max(best, source == "noisy" && l >= 2 ? noise(sum, key) : sum); // (the builder's table keeps the running maximum)
                (*table)[j * width + l - 1] = best;
            }
        }
        return [&, table](uint64_t j, uint64_t l) {
            ++asked;
            longest = std::max(longest, l);
            if (l < 2 || j + l > n || l > width)
                std::abort();
            return (*table)[j * width + l - 1];
        };
    };

    if (mode == "order")
    {
        const std::vector<uint64_t> starts = gnhibf::similarity_intervals(counts, size_order);
        std::printf("intervals %zu", starts.size() - 1);
        for (size_t i = 0; i + 1 < starts.size(); ++i)
            std::printf(" %llu", (unsigned long long)starts[i]);
        std::printf("\norder");
        for (uint32_t u : gnhibf::similarity_order(counts, size_order, pairs))
            std::printf(" %u", u);
        std::printf("\ntables %llu %llu\n", (unsigned long long)n_tables, (unsigned long long)largest);
        return 0;
    }

    gnhibf::Layout lay;
    if (mode == "similarity")
    {
        gnhibf::SimilarityLayout got = gnhibf::lay_out_similarity(counts, (uint32_t)tmax, max_fp, (uint8_t)h, unions, pairs);
        std::fprintf(stderr, "similarity %llu %llu %s %llu\n", (unsigned long long)got.intervals, (unsigned long long)got.moved, got.kept,
                     (unsigned long long)got.bits);
        lay = std::move(got.layout);
    }
    else if (mode == "sketch")
    {
        uint64_t bits = 0;
        bool     rule = false;
        if (width >= 2)
            lay = gnhibf::lay_out_sketch_costed(counts, (uint32_t)tmax, max_fp, (uint8_t)h, unions(size_order), &bits, &rule);
        else
            lay = gnhibf::lay_out_sketch(counts, (uint32_t)tmax, max_fp, (uint8_t)h, [](uint64_t, uint64_t) -> uint64_t { std::abort(); });
        std::fprintf(stderr, "sketch %llu %s\n", (unsigned long long)bits, rule ? "rule" : "sketch");
    }
    else
        lay = gnhibf::lay_out(counts, (uint32_t)tmax);
    std::printf("case %zu %u %u\n", lay.ibfs.size(), lay.levels, gnhibf::levels_for(n, tmax));
    for (size_t i = 0; i < lay.ibfs.size(); ++i)
    {
        const gnhibf::Ibf&    f = lay.ibfs[i];
        std::vector<uint64_t> hashes;
        uint64_t              rows = 0;
        for (const gnhibf::Run& r : f.runs)
        {
            const std::vector<uint32_t>* below = r.user >= 0 ? nullptr : &lay.ibfs[r.child].members;
            const uint64_t               c     = below ? united(below->data(), below->size()) : counts[r.user];
            hashes.push_back(c);
            rows = std::max(rows, gnbuild::hibf_run_bits(c, r.n_bins, max_fp, (uint8_t)h));
        }
        std::printf("ibf %zu %u %llu %lld %u %u %zu\n", i, f.bins, (unsigned long long)rows, (long long)f.parent, f.parent_bin, f.depth, f.runs.size());
        for (size_t j = 0; j < f.runs.size(); ++j)
            std::printf("run %u %u %lld %lld %llu\n", f.runs[j].first, f.runs[j].n_bins, (long long)f.runs[j].user, (long long)f.runs[j].child,
                        (unsigned long long)hashes[j]);
    }
    if (mode != "rule")
        std::printf("asked %llu %llu %llu\n", (unsigned long long)asked, (unsigned long long)longest, (unsigned long long)width);
    return 0;
}
