// hibf_fold_driver.cpp -- test harness: runs the PRODUCT's fold plan (ganon_amd/host/hibf_fold.hpp) and the arithmetic the device kernel
// is made of (ganon_amd/csrc/gn_fold_table.h) so that tests/test_build_fold_cpu.py can check them.  One case per line of stdin:
//   fold <h> <fpr> <N> <n_user> <n_ibf> { <bins> <rows> next_ibf_id[0..bins) bin_to_user[0..bins) fills[0..bins) } per IBF
//   rows <rows> <bins_src> <bins_dst> <words_dst> <dst_first> <n_groups> <n_members> { <src_first> <n_bins> <group> } per member
//        then rows * ceil(bins_src / 64) source words and rows * words_dst destination words in hex
// stdout for fold:
//         case <n_ibf> <depth>
//         table <new ibf> <source ibf> <bins> <rows> next_ibf_id[0..bins) bin_to_user[0..bins)
//         fills <new ibf> fills[0..bins)                                                     (%.17g)
//         span <new ibf> <src_first> <dst_first> <n_bins>
//         group <parent> <merged bin> <new ibf> <runs> <bins> <bits predicted> { <first> <n> } per run
//         folded <parent> ...
//         path <user bin> { <ibf> <first_bin> <n_bins> } per entry: derive_paths of the tables given, through fold_paths
//     or  unreachable <message>   /   refused <message>
// stdout for rows: `rows` lines of words_dst words in hex, each the destination row after gn_fold_row, from a source buffer of EXACTLY
//         rows * ceil(bins_src / 64) words and a destination of exactly rows * words_dst (a read or write beyond either is a heap
//         overflow the sanitizer sees); then `segments <n>`
#include "../ganon_amd/csrc/gn_fold_table.h"
#include "../ganon_amd/host/hibf_fold.hpp"

#include <cstdio>
#include <iostream>
#include <memory>
#include <sstream>
#include <string>

static void fold_case(std::istringstream& in)
{
    unsigned h = 0;
    double   fpr = 0;
    uint64_t N = 0, n_user = 0, n_ibf = 0;
    in >> h >> fpr >> N >> n_user >> n_ibf;
    if (!in || n_ibf > 100000)
        throw std::runtime_error("driver: unreadable case");
    std::vector<uint64_t>             bins(n_ibf), rows(n_ibf);
    std::vector<std::vector<int64_t>> nx(n_ibf), bu(n_ibf);
    std::vector<std::vector<double>>  fills(n_ibf);
    for (uint64_t i = 0; i < n_ibf; ++i)
    {
        in >> bins[i] >> rows[i];
        if (!in || bins[i] > 1000000)
            throw std::runtime_error("driver: unreadable case");
        nx[i].resize(bins[i]), bu[i].resize(bins[i]), fills[i].resize(bins[i]);
        for (auto& v : nx[i])
            in >> v;
        for (auto& v : bu[i])
            in >> v;
        for (auto& v : fills[i])
            in >> v;
    }
    if (!in)
        throw std::runtime_error("driver: unreadable case");
    const gnhibf::FoldPlan plan = gnhibf::plan_fold(bins, rows, nx, bu, n_user, (uint8_t)h, fpr, fills, N);
    std::printf("case %zu %u\n", plan.bins.size(), plan.depth);
    for (size_t i = 0; i < plan.bins.size(); ++i)
    {
        std::printf("table %zu %u %llu %llu", i, plan.src_ibf[i], (unsigned long long)plan.bins[i], (unsigned long long)plan.rows[i]);
        for (int64_t v : plan.next_ibf_id[i])
            std::printf(" %lld", (long long)v);
        for (int64_t v : plan.bin_to_user[i])
            std::printf(" %lld", (long long)v);
        std::printf("\nfills %zu", i);
        for (double v : plan.fills[i])
            std::printf(" %.17g", v);
        std::printf("\n");
        for (const gn_bin_span& s : plan.spans[i])
            std::printf("span %zu %u %u %u\n", i, s.src_first, s.dst_first, s.n_bins);
    }
    for (const gnhibf::FoldGroup& g : plan.groups)
    {
        std::printf("group %u %u %u %u %u %.17g", g.parent, g.merged_bin, g.new_ibf, g.runs, g.bins, g.bits_predicted);
        for (size_t k = 0; k < g.run_first.size(); ++k)
            std::printf(" %u %u", g.run_first[k], g.run_bins[k]);
        std::printf("\n");
    }
    std::printf("folded");
    for (uint32_t i : plan.folded)
        std::printf(" %u", i);
    std::printf("\n");
    const gnhibf::Paths old = gnhibf::derive_paths(bins, nx, bu, n_user), now = gnhibf::fold_paths(old, plan);
    for (uint64_t u = 0; u < n_user; ++u)
    {
        std::printf("path %llu", (unsigned long long)u);
        for (uint32_t d = 0; d < now.depth && now.entries[u * now.depth + d].n_bins; ++d)
            std::printf(" %u %u %u", now.entries[u * now.depth + d].ibf, now.entries[u * now.depth + d].first_bin, now.entries[u * now.depth + d].n_bins);
        std::printf("\n");
    }
}

static void rows_case(std::istringstream& in)
{
    uint64_t rows = 0, bins_src = 0, bins_dst = 0, words_dst = 0, dst_first = 0, n_groups = 0, n_members = 0;
    in >> rows >> bins_src >> bins_dst >> words_dst >> dst_first >> n_groups >> n_members;
    if (!in || rows > 100000 || bins_src == 0 || bins_src > 1000000 || words_dst > 100000 || words_dst * 64 < bins_dst || n_members > 1000000 || n_groups > 1000000 ||
        dst_first > 0xFFFFFFFFull)
        throw std::runtime_error("driver: unreadable case");
    std::vector<gn_fold_member> members(n_members);
    for (auto& m : members)
        in >> m.src_first >> m.n_bins >> m.group, m.reserved = 0;
    const uint64_t W_src = (bins_src + 63) / 64;
    // (new[], not a vector: exactly as many words as there are, with the sanitizer's red zone right behind them)
    std::unique_ptr<uint64_t[]> src(new uint64_t[rows * W_src]), dst(new uint64_t[rows * words_dst]);
    in >> std::hex;
    for (uint64_t i = 0; i < rows * W_src; ++i)
        in >> src[i];
    for (uint64_t i = 0; i < rows * words_dst; ++i)
        in >> dst[i];
    if (!in)
        throw std::runtime_error("driver: unreadable case");
    uint32_t    at  = 0;
    const char* why = gn_fold_check(members.data(), (uint32_t)n_members, (uint32_t)n_groups, (uint32_t)dst_first, bins_src, bins_dst, &at);
    if (why)
        throw std::runtime_error("member " + std::to_string(at) + ": " + why);
    std::vector<uint32_t>  seg_off;
    std::vector<GnFoldSeg> segs;
    gn_fold_table(members.data(), (uint32_t)n_members, W_src, seg_off, segs);
    if (seg_off.size() != W_src + 1 || seg_off.back() != segs.size())
        throw std::runtime_error("driver: a table of the wrong size");
    for (const GnFoldSeg& s : segs)
        if (s.group >= n_groups || s.mask == 0)
            throw std::runtime_error("driver: a segment without a group or without a bin");
    std::unique_ptr<uint32_t[]> hits(new uint32_t[gn_fold_hit_words((uint32_t)n_groups)]);
    for (uint64_t r = 0; r < rows; ++r)
    {
        gn_fold_row(dst.get() + r * words_dst, src.get() + r * W_src, W_src, seg_off.data(), segs.data(), (uint32_t)n_groups, (uint32_t)dst_first, hits.get());
        for (uint64_t w = 0; w < words_dst; ++w)
            std::printf("%s%llx", w ? " " : "", (unsigned long long)dst[r * words_dst + w]);
        std::printf("\n");
    }
    std::printf("segments %zu\n", segs.size());
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
            if (what == "fold")
                fold_case(in);
            else if (what == "rows")
                rows_case(in);
        }
        catch (const gnhibf::FoldUnreachable& e)
        {
            std::printf("unreachable %s\n", e.what());
        }
        catch (const std::exception& e)
        {
            std::printf("refused %s\n", e.what());
        }
    }
    return 0;
}
