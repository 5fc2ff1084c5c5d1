// hibf_remove_driver.cpp -- test harness: runs the PRODUCT's removal plan (ganon_amd/host/hibf_remove.hpp) and the span arithmetic the
// device kernel is made of (ganon_amd/csrc/gn_bin_spans.h) so that tests/test_build_remove_cpu.py can check them.  One case per line of stdin:
//   remove <h> <n_user> <n_ibf> { <bins> <rows> next_ibf_id[0..bins) bin_to_user[0..bins) popcounts[0..bins) } per IBF  <n_remove> u_0 ...
//   resolve <n_user> <n_targets> { <name> <k> user_bin_0 ... user_bin_{k-1} } per target  <n_names> name_0 ...        (names without blanks)
//   spans <rows> <bins_src> <bins_dst> <words_dst> <n_spans> { <src_first> <dst_first> <n_bins> } per span  then rows * ceil(bins_src / 64) words in hex
// stdout for remove:
//         case <n_ibf> <n_user_bins>
//         table <new ibf> <old ibf> <bins> next_ibf_id[0..bins) bin_to_user[0..bins)
//         pop <new ibf> popcounts[0..bins)
//         span <new ibf> <src_first> <dst_first> <n_bins>
//         ibfmap m[0..old n_ibf)          usermap m[0..old n_user)
//         dropped <ibf> <parent ibf> <parent bin>
//         removed <user bin> <ibf> <first_bin> <n_bins> <bits> <hashes> <full>
//         stale <old ibf> <old bin> <new ibf> <new bin> <bits> <hashes> <full>
// stdout for resolve: resolved u_0 ... ; unknown <name> per name the index does not hold ; shared <user bin> <kept target> per clash
// stdout for spans: `rows` lines of words_dst words in hex, each composed by gn_span_compose from a source buffer of EXACTLY
//         rows * ceil(bins_src / 64) words (a read at or beyond a row's last word of the last row is a heap overflow the sanitizer sees)
//     or  refused <message>
#include "../ganon_amd/csrc/gn_bin_spans.h"
#include "../ganon_amd/host/hibf_remove.hpp"

#include <cstdio>
#include <iostream>
#include <memory>
#include <sstream>
#include <string>

static void remove_case(std::istringstream& in)
{
    unsigned h = 0;
    uint64_t n_user = 0, n_ibf = 0, n_remove = 0;
    in >> h >> n_user >> n_ibf;
    if (!in || n_ibf > 100000)
        throw std::runtime_error("driver: unreadable case");
    std::vector<uint64_t>              bins(n_ibf), rows(n_ibf);
    std::vector<std::vector<int64_t>>  nx(n_ibf), bu(n_ibf);
    std::vector<std::vector<uint64_t>> pop(n_ibf);
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
    in >> n_remove;
    if (!in || n_remove > 1000000)
        throw std::runtime_error("driver: unreadable case");
    std::vector<uint64_t> remove(n_remove);
    for (auto& u : remove)
        in >> u;
    if (!in)
        throw std::runtime_error("driver: unreadable case");
    const gnhibf::RemovePlan plan = gnhibf::plan_remove(bins, nx, bu, n_user, remove, rows, (uint8_t)h, &pop);
    std::printf("case %zu %llu\n", plan.bins.size(), (unsigned long long)plan.n_user_bins);
    for (size_t i = 0; i < plan.bins.size(); ++i)
    {
        std::printf("table %zu %u %llu", i, plan.old_ibf[i], (unsigned long long)plan.bins[i]);
        for (int64_t v : plan.next_ibf_id[i])
            std::printf(" %lld", (long long)v);
        for (int64_t v : plan.bin_to_user[i])
            std::printf(" %lld", (long long)v);
        std::printf("\npop %zu", i);
        for (uint64_t v : plan.popcounts[i])
            std::printf(" %llu", (unsigned long long)v);
        std::printf("\n");
        for (const gn_bin_span& s : plan.spans[i])
            std::printf("span %zu %u %u %u\n", i, s.src_first, s.dst_first, s.n_bins);
    }
    std::printf("ibfmap");
    for (int64_t v : plan.ibf_map)
        std::printf(" %lld", (long long)v);
    std::printf("\nusermap");
    for (int64_t v : plan.user_map)
        std::printf(" %lld", (long long)v);
    std::printf("\n");
    for (const gnhibf::RemoveDropped& d : plan.dropped)
        std::printf("dropped %u %u %u\n", d.ibf, d.parent_ibf, d.parent_bin);
    for (const gnhibf::RemovedRun& r : plan.removed)
        std::printf("removed %llu %u %u %u %llu %llu %d\n", (unsigned long long)r.user_bin, r.ibf, r.first_bin, r.n_bins, (unsigned long long)r.bits, (unsigned long long)r.hashes, (int)r.full);
    for (const gnhibf::RemoveStale& s : plan.stale)
        std::printf("stale %u %u %u %u %llu %llu %d\n", s.old_ibf, s.old_bin, s.ibf, s.bin, (unsigned long long)s.bits, (unsigned long long)s.hashes, (int)s.full);
}

static void resolve_case(std::istringstream& in)
{
    uint64_t n_user = 0, n_targets = 0, n_names = 0;
    in >> n_user >> n_targets;
    if (!in || n_targets > 100000)
        throw std::runtime_error("driver: unreadable case");
    std::vector<std::string>           targets(n_targets);
    std::vector<std::vector<uint64_t>> target_bins(n_targets);
    for (uint64_t t = 0; t < n_targets; ++t)
    {
        uint64_t k = 0;
        in >> targets[t] >> k;
        if (!in || k > 100000)
            throw std::runtime_error("driver: unreadable case");
        target_bins[t].resize(k);
        for (auto& u : target_bins[t])
            in >> u;
    }
    in >> n_names;
    if (!in || n_names > 100000)
        throw std::runtime_error("driver: unreadable case");
    std::vector<std::string> names(n_names);
    for (auto& n : names)
        in >> n;
    if (!in)
        throw std::runtime_error("driver: unreadable case");
    const gnhibf::RemoveNames got = gnhibf::resolve_remove(targets, target_bins, n_user, names);
    std::printf("resolved");
    for (uint64_t u : got.user_bins)
        std::printf(" %llu", (unsigned long long)u);
    std::printf("\n");
    for (const std::string& n : got.unknown)
        std::printf("unknown %s\n", n.c_str());
    for (const auto& [u, t] : got.shared)
        std::printf("shared %llu %s\n", (unsigned long long)u, t.c_str());
}

static void spans_case(std::istringstream& in)
{
    uint64_t rows = 0, bins_src = 0, bins_dst = 0, words_dst = 0, n_spans = 0;
    in >> rows >> bins_src >> bins_dst >> words_dst >> n_spans;
    if (!in || rows > 100000 || bins_src == 0 || bins_src > 1000000 || words_dst > 100000 || words_dst * 64 < bins_dst || n_spans > 1000000)
        throw std::runtime_error("driver: unreadable case");
    std::vector<gn_bin_span> spans(n_spans);
    for (auto& s : spans)
        in >> s.src_first >> s.dst_first >> s.n_bins, s.reserved = 0;
    const uint64_t W_src = (bins_src + 63) / 64;
    // (new[], not a vector: exactly rows * W_src words, with the sanitizer's red zone right behind them)
    std::unique_ptr<uint64_t[]> src(new uint64_t[rows * W_src]);
    in >> std::hex;
    for (uint64_t i = 0; i < rows * W_src; ++i)
        in >> src[i];
    if (!in)
        throw std::runtime_error("driver: unreadable case");
    uint32_t    at  = 0;
    const char* why = gn_spans_check(spans.data(), (uint32_t)n_spans, bins_src, bins_dst, &at);
    if (why)
        throw std::runtime_error("span " + std::to_string(at) + ": " + why);
    std::vector<uint32_t>  seg_off;
    std::vector<GnSpanSeg> segs;
    gn_spans_table(spans.data(), (uint32_t)n_spans, words_dst, seg_off, segs);
    for (const GnSpanSeg& s : segs)
        if (s.src_word >= W_src || ((uint32_t)s.sh + s.len > 64 && s.src_word + 1 >= W_src) || s.len == 0 || (uint32_t)s.dst_off + s.len > 64)
            throw std::runtime_error("driver: a segment outside the source's words");
    for (uint64_t r = 0; r < rows; ++r)
    {
        const uint64_t* row = src.get() + r * W_src;
        for (uint64_t w = 0; w < words_dst; ++w)
            std::printf("%s%llx", w ? " " : "", (unsigned long long)gn_span_compose(row, segs.data() + seg_off[w], seg_off[w + 1] - seg_off[w]));
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
            if (what == "remove")
                remove_case(in);
            else if (what == "resolve")
                resolve_case(in);
            else if (what == "spans")
                spans_case(in);
        }
        catch (const std::exception& e)
        {
            std::printf("refused %s\n", e.what());
        }
    }
    return 0;
}
