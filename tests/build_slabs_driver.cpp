// build_slabs_driver.cpp -- test harness: runs the PRODUCT's slab plan (ganon_amd/host/build_slabs.hpp) and the arithmetic the windowed insert
// is made of (ganon_amd/csrc/gn_emplace_window.h: the item builder, the bin of a hash of an item, the window test -- the very functions the
// kernel and its host call) so that tests/test_build_slabs_cpu.py can check them.  One case per line of stdin:
//   plan <total_rows> <row_bytes> <budget_bytes> <n_devices> [<slab index> ...]        (no index: every slab)
//   items <cap_hashes> <cap_items> <n_runs> <size> per run
//   window <total_rows> <bins> <h> <row_begin> <n_rows> <cap_hashes> <n_runs> { <first_bin> <per_bin> <size> <hash in hex> per hash } per run
// stdout:
//   plan:   plan <n_slabs> <rows_per_slab>, then `slab <i> <row_begin> <n_rows> <device_entry>` per slab asked for     or  refused <message>
//   items:  per chunk `chunk <hashes taken>`, then `item <run> <cnt> <begin> <stage_at>` per item
//   window: n_rows lines of ceil(bins / 64) words in hex: the slab after a host model of gn_emplace_window_kernel -- per chunk and item,
//           per hash of the item, per hash function: the row of the WHOLE filter (hash_and_fit restated with unsigned __int128 for
//           __umul64hi), the window test, the bit -- into a buffer of EXACTLY n_rows * ceil(bins / 64) words (a write outside the slab
//           is a heap overflow the sanitizer sees)
#include "../ganon_amd/csrc/gn_emplace_window.h"
#include "../ganon_amd/host/build_slabs.hpp"
#include "../include/ganon_ibf_hash.h"

#include <cstdio>
#include <iostream>
#include <memory>
#include <sstream>
#include <string>

static const uint64_t kSeeds[GN_IBF_MAX_HASH_FUNS] = GN_IBF_SEED_LIST;

// gn_build_row (ganon_amd/csrc/gn_build_row.h) on the host
static uint32_t build_row(uint64_t v, uint32_t i, uint32_t shift, uint64_t S)
{
    uint64_t x = v * kSeeds[i];
    x ^= x >> shift;
    x *= GN_IBF_MULTIPLIER;
    return (uint32_t)(((unsigned __int128)x * S) >> 64);
}

static void plan_case(std::istringstream& in)
{
    uint64_t total = 0, row_bytes = 0, budget = 0, n_dev = 0;
    in >> total >> row_bytes >> budget >> n_dev;
    if (!in)
        throw std::runtime_error("driver: unreadable case");
    const gnbuild::SlabPlan plan = gnbuild::plan_slabs(total, row_bytes, budget, (uint32_t)n_dev);
    std::printf("plan %llu %llu\n", (unsigned long long)plan.n_slabs, (unsigned long long)plan.rows_per_slab);
    auto show = [&](uint64_t i) {
        const gnbuild::Slab s = plan.at(i);
        std::printf("slab %llu %llu %llu %u\n", (unsigned long long)i, (unsigned long long)s.row_begin, (unsigned long long)s.n_rows, s.device_entry);
    };
    uint64_t i     = 0;
    bool     asked = false;
    while (in >> i)
    {
        asked = true;
        if (i >= plan.n_slabs)
            throw std::runtime_error("driver: no such slab");
        show(i);
    }
    if (!asked)
    {
        if (plan.n_slabs > 1000000)
            throw std::runtime_error("driver: too many slabs to list");
        for (i = 0; i < plan.n_slabs; ++i)
            show(i);
    }
}

static void items_case(std::istringstream& in)
{
    uint64_t cap_hashes = 0, cap_items = 0, n_runs = 0;
    in >> cap_hashes >> cap_items >> n_runs;
    if (!in || cap_hashes == 0 || cap_items == 0 || n_runs > 1000000)
        throw std::runtime_error("driver: unreadable case");
    std::unique_ptr<uint64_t[]> sizes(new uint64_t[n_runs]);
    for (uint64_t r = 0; r < n_runs; ++r)
        in >> sizes[r];
    if (!in)
        throw std::runtime_error("driver: unreadable case");
    std::vector<GnRunItem> items;
    GnRunCursor            cur;
    for (;;)
    {
        const uint64_t taken = gn_window_next_chunk(sizes.get(), (uint32_t)n_runs, cur, cap_hashes, cap_items, items);
        if (taken == 0)
            break;
        std::printf("chunk %llu\n", (unsigned long long)taken);
        for (const GnRunItem& it : items)
            std::printf("item %u %u %llu %llu\n", it.run, it.cnt, (unsigned long long)it.begin, (unsigned long long)it.stage_at);
    }
}

static void window_case(std::istringstream& in)
{
    uint64_t total_rows = 0, bins = 0, h = 0, row_begin = 0, n_rows = 0, cap_hashes = 0, n_runs = 0;
    in >> total_rows >> bins >> h >> row_begin >> n_rows >> cap_hashes >> n_runs;
    if (!in || total_rows == 0 || total_rows > 0xFFFFFFFFull || bins == 0 || bins > 1000000 || h < 1 || h > GN_IBF_MAX_HASH_FUNS || n_rows == 0 ||
        row_begin + n_rows > total_rows || cap_hashes == 0 || n_runs > 100000)
        throw std::runtime_error("driver: unreadable case");
    std::vector<std::unique_ptr<uint64_t[]>> runs(n_runs);
    std::unique_ptr<uint64_t[]>              sizes(new uint64_t[n_runs]), per_bin(new uint64_t[n_runs]);
    std::unique_ptr<uint32_t[]>              first_bin(new uint32_t[n_runs]);
    for (uint64_t r = 0; r < n_runs; ++r)
    {
        in >> std::dec >> first_bin[r] >> per_bin[r] >> sizes[r];
        if (!in || sizes[r] > 10000000 || per_bin[r] == 0 || (sizes[r] && first_bin[r] + (sizes[r] - 1) / per_bin[r] >= bins))
            throw std::runtime_error("driver: unreadable run");
        runs[r].reset(new uint64_t[sizes[r]]);
        in >> std::hex;
        for (uint64_t i = 0; i < sizes[r]; ++i)
            in >> runs[r][i];
    }
    if (!in)
        throw std::runtime_error("driver: unreadable case");
    const uint64_t W     = (bins + 63) / 64;
    const uint32_t shift = (uint32_t)__builtin_clzll(total_rows);
    // (new[], not a vector: exactly as many words as the slab has, with the sanitizer's red zone right behind and before them)
    std::unique_ptr<uint64_t[]> slab(new uint64_t[n_rows * W]()), stage(new uint64_t[cap_hashes]);
    std::vector<GnRunItem>      items;
    GnRunCursor                 cur;
    for (;;)
    {
        const uint64_t taken = gn_window_next_chunk(sizes.get(), (uint32_t)n_runs, cur, cap_hashes, cap_hashes / 64 + 16, items);
        if (taken == 0)
            break;
        for (const GnRunItem& it : items) // the host's gather into the staging chunk
            for (uint32_t q = 0; q < it.cnt; ++q)
                stage[it.stage_at + q] = runs[it.run][it.begin + q];
        for (const GnRunItem& it : items) // the kernel: one wave per item, lane `q % 64` slot `q / 64`
        {
            const uint64_t b0 = it.begin / per_bin[it.run], r0 = it.begin - b0 * per_bin[it.run];
            const uint32_t bin0 = first_bin[it.run] + (uint32_t)b0;
            for (uint32_t q = 0; q < it.cnt; ++q)
            {
                const uint64_t v   = stage[it.stage_at + q];
                const uint32_t bin = gn_window_item_bin(bin0, r0, q, per_bin[it.run]);
                if (bin != gn_window_bin(first_bin[it.run], it.begin + q, per_bin[it.run]))
                    throw std::runtime_error("driver: the item's bin differs from the rule's");
                for (uint32_t i = 0; i < h; ++i)
                {
                    uint32_t local;
                    if (gn_window_local(build_row(v, i, shift, total_rows), (uint32_t)row_begin, (uint32_t)n_rows, &local))
                        slab[(uint64_t)local * W + (bin >> 6)] |= 1ULL << (bin & 63);
                }
            }
        }
    }
    for (uint64_t r = 0; r < n_rows; ++r)
    {
        for (uint64_t w = 0; w < W; ++w)
            std::printf("%s%llx", w ? " " : "", (unsigned long long)slab[r * W + w]);
        std::printf("\n");
    }
}

int main()
{
    std::string line;
    while (std::getline(std::cin, line))
    {
        std::istringstream in(line);
        std::string        what;
        in >> what;
        try
        {
            if (what == "plan")
                plan_case(in);
            else if (what == "items")
                items_case(in);
            else if (what == "window")
                window_case(in);
        }
        catch (const std::exception& e)
        {
            std::printf("refused %s\n", e.what());
        }
    }
    return 0;
}
