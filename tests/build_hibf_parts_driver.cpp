// build_hibf_parts_driver.cpp -- test harness: runs the PRODUCT's plan of a hierarchical build in parts and its path compaction
// (ganon_amd/host/hibf_build_parts.hpp) and the arithmetic the windowed path insert is made of (ganon_amd/csrc/gn_path_window.h with
// gn_emplace_window.h: the item builder, the bin of a hash of an item in a path entry, the window test -- the very functions the kernel and
// its host call) so that tests/test_build_hibf_parts_cpu.py can check them.  One case per line of stdin:
//   plan <budget_bytes> <n_devices> <n_ibf> { <rows> <row_bytes> } per IBF [<part index> ...]              (no index: every part)
//   compact <depth> <n_ibf> { <local> } per IBF { <ibf> <first_bin> <n_bins> <hashes_per_bin> } per entry
//   items <cap_hashes> <cap_items> <n_sets> <size> per set
//   window <h> <cap_hashes> <n_ibf> { <bins> <total_rows> <row_begin> <n_rows> } per IBF <depth> <n_sets>
//          { { <ibf> <first_bin> <n_bins> <per_bin> } per entry <size> <hash in hex> per hash } per set
// stdout:
//   plan:    plan <n_parts>, then `piece <part> <entry> <ibf> <row_begin> <n_rows>` per piece of every part asked for   or  refused <message>
//   compact: kept <n>, then `entry <ibf> <first_bin> <n_bins> <hashes_per_bin>` for each of the depth entries
//   items:   per chunk `chunk <hashes taken>`, then `item <set> <cnt> <begin> <stage_at>` per item
//   window:  per IBF `ibf <j>` and n_rows lines of ceil(bins / 64) words in hex: the pieces after a host model of
//            gn_emplace_path_window_kernel -- per chunk and item, per entry of the item's path, per hash, per hash function: the row of
//            the WHOLE IBF (hash_and_fit restated with unsigned __int128 for __umul64hi), the window test, the bit -- into buffers of
//            EXACTLY n_rows * ceil(bins / 64) words (a write outside a piece is a heap overflow the sanitizer sees)
#include "../ganon_amd/csrc/gn_path_window.h"
#include "../ganon_amd/host/hibf_build_parts.hpp"
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

static void unreadable(bool bad)
{
    if (bad)
        throw std::runtime_error("driver: unreadable case");
}

static void plan_case(std::istringstream& in)
{
    uint64_t budget = 0, n_dev = 0, n_ibf = 0;
    in >> budget >> n_dev >> n_ibf;
    unreadable(!in || n_ibf > 1000000);
    std::vector<uint64_t> rows(n_ibf), rb(n_ibf);
    for (uint64_t i = 0; i < n_ibf; ++i)
        in >> rows[i] >> rb[i];
    unreadable(!in);
    const gnbuild::HibfPartPlan plan = gnbuild::plan_hibf_parts(rows, rb, budget, (uint32_t)n_dev);
    std::printf("plan %llu\n", (unsigned long long)plan.n_parts);
    auto show = [&](uint64_t p) {
        for (const gnbuild::HibfPiece& x : plan.part(p))
            std::printf("piece %llu %u %u %llu %llu\n", (unsigned long long)p, plan.entry_of(p), x.ibf, (unsigned long long)x.row_begin, (unsigned long long)x.n_rows);
    };
    uint64_t p     = 0;
    bool     asked = false;
    while (in >> p)
    {
        asked = true;
        if (p >= plan.n_parts)
            throw std::runtime_error("driver: no such part");
        show(p);
    }
    if (!asked)
    {
        if (plan.n_parts > 1000000)
            throw std::runtime_error("driver: too many parts to list");
        for (p = 0; p < plan.n_parts; ++p)
            show(p);
    }
}

static void compact_case(std::istringstream& in)
{
    uint64_t depth = 0, n_ibf = 0;
    in >> depth >> n_ibf;
    unreadable(!in || depth == 0 || depth > 64 || n_ibf > 100000);
    std::vector<int64_t> local(n_ibf);
    for (int64_t& x : local)
        in >> x;
    // (new[], not a vector: exactly `depth` entries, with the sanitizer's red zone right behind them)
    std::unique_ptr<gn_path_entry[]> path(new gn_path_entry[depth]), out(new gn_path_entry[depth]);
    for (uint64_t d = 0; d < depth; ++d)
    {
        path[d].reserved = 0;
        in >> path[d].ibf >> path[d].first_bin >> path[d].n_bins >> path[d].hashes_per_bin;
    }
    unreadable(!in);
    const uint32_t kept = gnbuild::compact_path(path.get(), (uint32_t)depth, local, out.get());
    std::printf("kept %u\n", kept);
    for (uint64_t d = 0; d < depth; ++d)
        std::printf("entry %u %u %u %llu\n", out[d].ibf, out[d].first_bin, out[d].n_bins, (unsigned long long)out[d].hashes_per_bin);
}

static void items_case(std::istringstream& in)
{
    uint64_t cap_hashes = 0, cap_items = 0, n_sets = 0;
    in >> cap_hashes >> cap_items >> n_sets;
    unreadable(!in || cap_hashes == 0 || cap_items == 0 || n_sets > 1000000);
    std::unique_ptr<uint64_t[]> sizes(new uint64_t[n_sets]);
    for (uint64_t r = 0; r < n_sets; ++r)
        in >> sizes[r];
    unreadable(!in);
    std::vector<GnRunItem> items;
    GnRunCursor            cur;
    for (;;)
    {
        const uint64_t taken = gn_window_next_chunk(sizes.get(), (uint32_t)n_sets, cur, cap_hashes, cap_items, items);
        if (taken == 0)
            break;
        std::printf("chunk %llu\n", (unsigned long long)taken);
        for (const GnRunItem& it : items)
            std::printf("item %u %u %llu %llu\n", it.run, it.cnt, (unsigned long long)it.begin, (unsigned long long)it.stage_at);
    }
}

static void window_case(std::istringstream& in)
{
    uint64_t h = 0, cap_hashes = 0, n_ibf = 0, depth = 0, n_sets = 0;
    in >> h >> cap_hashes >> n_ibf;
    unreadable(!in || h < 1 || h > GN_IBF_MAX_HASH_FUNS || cap_hashes == 0 || n_ibf == 0 || n_ibf > 1000);
    std::vector<uint64_t>                    bins(n_ibf), total(n_ibf), begin(n_ibf), n_rows(n_ibf), W(n_ibf);
    std::vector<std::unique_ptr<uint64_t[]>> piece(n_ibf);
    for (uint64_t j = 0; j < n_ibf; ++j)
    {
        in >> bins[j] >> total[j] >> begin[j] >> n_rows[j];
        unreadable(!in || bins[j] == 0 || bins[j] > 1000000 || total[j] == 0 || total[j] > 0xFFFFFFFFull || n_rows[j] == 0 || begin[j] + n_rows[j] > total[j] ||
                   n_rows[j] > 10000000);
        W[j] = (bins[j] + 63) / 64;
        piece[j].reset(new uint64_t[n_rows[j] * W[j]]()); // (exactly as many words as the piece has)
    }
    in >> depth >> n_sets;
    unreadable(!in || depth == 0 || depth > 64 || n_sets > 100000);
    std::vector<GnPathWinDev>                paths(n_sets * depth, GnPathWinDev{ nullptr, 1, 1, 1, 0, 0, 0, 0, 0 });
    std::vector<std::unique_ptr<uint64_t[]>> sets(n_sets);
    std::unique_ptr<uint64_t[]>              sizes(new uint64_t[n_sets]);
    for (uint64_t s = 0; s < n_sets; ++s)
    {
        std::vector<uint64_t> per(depth);
        for (uint64_t d = 0; d < depth; ++d)
        {
            uint64_t      ibf = 0;
            GnPathWinDev& e   = paths[s * depth + d];
            in >> std::dec >> ibf >> e.first_bin >> e.n_bins >> e.per_bin;
            unreadable(!in || ibf >= n_ibf || (uint64_t)e.first_bin + e.n_bins > bins[ibf] || (e.n_bins > 1 && e.per_bin == 0));
            // what the library's host resolves: the piece and the WHOLE IBF's geometry
            e.rows    = piece[ibf].get();
            e.S_total = total[ibf], e.shift = (uint32_t)__builtin_clzll(total[ibf]);
            e.Ws      = (uint32_t)W[ibf]; // (no padding on the host: the model's rows are the file's)
            e.row_begin = (uint32_t)begin[ibf], e.n_rows = (uint32_t)n_rows[ibf];
        }
        in >> std::dec >> sizes[s];
        unreadable(!in || sizes[s] > 10000000);
        for (uint64_t d = 0; d < depth && paths[s * depth + d].n_bins; ++d)
            if (paths[s * depth + d].n_bins > 1 && sizes[s] && (sizes[s] - 1) / paths[s * depth + d].per_bin >= paths[s * depth + d].n_bins)
                throw std::runtime_error("driver: the hashes do not fit the run");
        sets[s].reset(new uint64_t[sizes[s]]);
        in >> std::hex;
        for (uint64_t i = 0; i < sizes[s]; ++i)
            in >> sets[s][i];
    }
    unreadable(!in);
    std::unique_ptr<uint64_t[]> stage(new uint64_t[cap_hashes]);
    std::vector<GnRunItem>      items;
    GnRunCursor                 cur;
    for (;;)
    {
        const uint64_t taken = gn_window_next_chunk(sizes.get(), (uint32_t)n_sets, cur, cap_hashes, cap_hashes / 64 + 16, items);
        if (taken == 0)
            break;
        for (const GnRunItem& it : items) // the host's gather into the staging chunk
            for (uint32_t q = 0; q < it.cnt; ++q)
                stage[it.stage_at + q] = sets[it.run][it.begin + q];
        for (const GnRunItem& it : items) // the kernel: one wave per item, lane `q % 64` slot `q / 64`
            for (uint64_t d = 0; d < depth; ++d)
            {
                const GnPathWinDev& e = paths[it.run * depth + d];
                if (e.n_bins == 0)
                    break;
                uint32_t bin0;
                uint64_t r0;
                gn_path_window_start(e.first_bin, e.n_bins, e.per_bin, it.begin, &bin0, &r0);
                for (uint32_t q = 0; q < it.cnt; ++q)
                {
                    const uint64_t v   = stage[it.stage_at + q];
                    const uint32_t bin = gn_path_window_bin(bin0, r0, q, e.n_bins, e.per_bin);
                    if (bin != (e.n_bins == 1 ? e.first_bin : gn_window_bin(e.first_bin, it.begin + q, e.per_bin)))
                        throw std::runtime_error("driver: the item's bin differs from the rule's");
                    for (uint32_t i = 0; i < h; ++i)
                    {
                        uint32_t local;
                        if (gn_window_local(build_row(v, i, e.shift, e.S_total), e.row_begin, e.n_rows, &local))
                            e.rows[(uint64_t)local * e.Ws + (bin >> 6)] |= 1ULL << (bin & 63);
                    }
                }
            }
    }
    for (uint64_t j = 0; j < n_ibf; ++j)
    {
        std::printf("ibf %llu\n", (unsigned long long)j);
        for (uint64_t r = 0; r < n_rows[j]; ++r)
        {
            for (uint64_t w = 0; w < W[j]; ++w)
                std::printf("%s%llx", w ? " " : "", (unsigned long long)piece[j][r * W[j] + w]);
            std::printf("\n");
        }
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
            else if (what == "compact")
                compact_case(in);
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
