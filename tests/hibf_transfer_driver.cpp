// hibf_transfer_driver.cpp -- test harness: runs the PRODUCT's plans of `ganon-build --hibf --update` in the order the command runs them
// (plan_remove, plan_update, plan_fold, then plan_transfer of ganon_amd/host/hibf_transfer.hpp) and applies the transfer on the host to a
// bit matrix of A, with the functions the two kernels are made of (ganon_amd/csrc/gn_bin_spans.h, gn_fold_table.h), so that
// tests/test_build_transfer_cpu.py can check B against the tables alone.  One case per line of stdin:
//   transfer <h> <fpr> <n_user> <n_ibf> { <bins> <rows> next_ibf_id[0..bins) bin_to_user[0..bins) popcounts[0..bins) } per IBF
//            <n_remove> u_0 ...  <n_fresh> count_0 ...  <N, 0: no fold>   then per IBF rows * ceil(bins / 64) words of A in hex
// stdout:  case <n_ibf of B> <n_user of B>
//          table <ibf> <bins> <rows> next_ibf_id[0..bins) bin_to_user[0..bins)        (the final tables)
//          row <ibf> <row> words in hex                                               (B after the moves and the fold calls)
//          move <dst ibf> <src ibf> whole | move <dst ibf> <src ibf> spans <n> { <src_first> <dst_first> <n_bins> }
//          fold <parent> <merged bin> <n_groups> <src ibf> <n> { <src_first> <n_bins> <group> }
//      or  unreachable <message>   /   refused <message>
// Every buffer holds EXACTLY the words there are (new[]): a read or write beyond one is a heap overflow the sanitizer sees.
#include "../ganon_amd/csrc/gn_bin_spans.h"
#include "../ganon_amd/csrc/gn_fold_table.h"
#include "../ganon_amd/host/hibf_transfer.hpp"

#include <cstdio>
#include <iostream>
#include <memory>
#include <sstream>
#include <string>

using Matrix = std::unique_ptr<uint64_t[]>;

static uint64_t words(uint64_t bins)
{
    return (bins + 63) / 64;
}

// one move: every word of every row of the destination composed from the source's row
static void apply_move(uint64_t* dst, uint64_t bins_dst, const uint64_t* src, uint64_t bins_src, uint64_t rows, const std::vector<gn_bin_span>& spans)
{
    uint32_t    at  = 0;
    const char* why = gn_spans_check(spans.data(), (uint32_t)spans.size(), bins_src, bins_dst, &at);
    if (why)
        throw std::runtime_error("driver: span " + std::to_string(at) + ": " + why);
    std::vector<uint32_t>  seg_off;
    std::vector<GnSpanSeg> segs;
    gn_spans_table(spans.data(), (uint32_t)spans.size(), words(bins_dst), seg_off, segs);
    for (uint64_t r = 0; r < rows; ++r)
        for (uint64_t w = 0; w < words(bins_dst); ++w)
            dst[r * words(bins_dst) + w] = gn_span_compose(src + r * words(bins_src), segs.data() + seg_off[w], seg_off[w + 1] - seg_off[w]);
}

static void apply_fold(uint64_t* dst, uint64_t bins_dst, const uint64_t* src, uint64_t bins_src, uint64_t rows, const gnhibf::TransferFold& f)
{
    uint32_t    at  = 0;
    const char* why = gn_fold_check(f.members.data(), (uint32_t)f.members.size(), f.n_groups, f.merged_bin, bins_src, bins_dst, &at);
    if (why)
        throw std::runtime_error("driver: member " + std::to_string(at) + ": " + why);
    std::vector<uint32_t>  seg_off;
    std::vector<GnFoldSeg> segs;
    gn_fold_table(f.members.data(), (uint32_t)f.members.size(), words(bins_src), seg_off, segs);
    std::unique_ptr<uint32_t[]> hits(new uint32_t[gn_fold_hit_words(f.n_groups)]);
    for (uint64_t r = 0; r < rows; ++r)
        gn_fold_row(dst + r * words(bins_dst), src + r * words(bins_src), words(bins_src), seg_off.data(), segs.data(), f.n_groups, f.merged_bin, hits.get());
}

static void transfer_case(std::istringstream& in)
{
    unsigned h = 0;
    double   fpr = 0;
    uint64_t n_user = 0, n_ibf = 0, n_remove = 0, n_fresh = 0, N = 0;
    in >> h >> fpr >> n_user >> n_ibf;
    if (!in || n_ibf > 100000)
        throw std::runtime_error("driver: unreadable case");
    std::vector<uint64_t>              bins_a(n_ibf), rows(n_ibf);
    std::vector<std::vector<int64_t>>  nx(n_ibf), bu(n_ibf);
    std::vector<std::vector<uint64_t>> pop(n_ibf);
    for (uint64_t i = 0; i < n_ibf; ++i)
    {
        in >> bins_a[i] >> rows[i];
        if (!in || bins_a[i] == 0 || bins_a[i] > 100000 || rows[i] > 100000)
            throw std::runtime_error("driver: unreadable case");
        nx[i].resize(bins_a[i]), bu[i].resize(bins_a[i]), pop[i].resize(bins_a[i]);
        for (auto& v : nx[i])
            in >> v;
        for (auto& v : bu[i])
            in >> v;
        for (auto& v : pop[i])
            in >> v;
    }
    in >> n_remove;
    std::vector<uint64_t> remove(in && n_remove <= 100000 ? n_remove : 0);
    for (auto& u : remove)
        in >> u;
    in >> n_fresh;
    std::vector<uint64_t> fresh(in && n_fresh <= 100000 ? n_fresh : 0);
    for (auto& c : fresh)
        in >> c;
    in >> N;
    if (!in)
        throw std::runtime_error("driver: unreadable case");
    std::vector<Matrix> A;
    in >> std::hex;
    for (uint64_t i = 0; i < n_ibf; ++i)
    {
        A.emplace_back(new uint64_t[rows[i] * words(bins_a[i])]);
        for (uint64_t k = 0; k < rows[i] * words(bins_a[i]); ++k)
            in >> A[i][k];
    }
    if (!in)
        throw std::runtime_error("driver: unreadable case");

    // the plans, as the command makes them: the tables after the removal are what the placement works on, the fold runs last
    const bool         removing = !remove.empty(), folding = N != 0;
    gnhibf::RemovePlan gone;
    std::vector<uint64_t> bins = bins_a, rows_b = rows;
    if (removing)
    {
        gone = gnhibf::plan_remove(bins_a, nx, bu, n_user, remove, rows, (uint8_t)h, &pop);
        rows_b.clear();
        for (const uint32_t i : gone.old_ibf)
            rows_b.push_back(rows[i]);
        bins = gone.bins, pop = gone.popcounts, nx = gone.next_ibf_id, bu = gone.bin_to_user, n_user = gone.n_user_bins;
    }
    const gnhibf::UpdatePlan plan = gnhibf::plan_update(bins, rows_b, nx, bu, n_user, (uint8_t)h, fpr, pop, fresh);
    gnhibf::FoldPlan         fold;
    if (folding)
    {
        std::vector<std::vector<double>> fills(bins.size());
        for (size_t i = 0; i < bins.size(); ++i)
        {
            fills[i].assign(pop[i].begin(), pop[i].begin() + bins[i]);
            fills[i].resize(plan.bins[i], 0.0);
        }
        for (const gnhibf::UpdateTouched& t : plan.touched)
            fills[t.ibf][t.bin] = t.bits_predicted;
        for (size_t j = 0; j < fresh.size(); ++j)
        {
            const gn_path_entry& run = plan.paths.entries[j * plan.paths.depth];
            for (uint32_t b = run.first_bin; b < run.first_bin + run.n_bins; ++b)
                fills[run.ibf][b] = gnhibf::update_predict(0.0, run.hashes_per_bin, rows_b[run.ibf], (uint8_t)h);
        }
        fold = gnhibf::plan_fold(plan.bins, rows_b, plan.next_ibf_id, plan.bin_to_user, plan.n_user_bins, (uint8_t)h, fpr, fills, N);
    }
    const gnhibf::Transfer t = gnhibf::plan_transfer(bins_a, removing ? &gone : nullptr, plan, folding ? &fold : nullptr);
    const std::vector<uint64_t>&             f_bins = folding ? fold.bins : plan.bins;
    const std::vector<uint64_t>&             f_rows = folding ? fold.rows : rows_b;
    const std::vector<std::vector<int64_t>>& f_nx   = folding ? fold.next_ibf_id : plan.next_ibf_id;
    const std::vector<std::vector<int64_t>>& f_bu   = folding ? fold.bin_to_user : plan.bin_to_user;

    // B: created empty, every IBF moved over, then the fold calls
    std::vector<Matrix> B;
    for (size_t i = 0; i < f_bins.size(); ++i)
        B.emplace_back(new uint64_t[f_rows[i] * words(f_bins[i])]());
    auto check = [&](uint32_t dst, uint32_t src) {
        if (dst >= f_bins.size() || src >= n_ibf || f_rows[dst] != rows[src])
            throw std::runtime_error("driver: a call from IBF " + std::to_string(src) + " to IBF " + std::to_string(dst) + ": out of range, or rows that differ");
    };
    for (const gnhibf::TransferMove& m : t.moves)
    {
        check(m.dst_ibf, m.src_ibf);
        if (m.whole && bins_a[m.src_ibf] > f_bins[m.dst_ibf])
            throw std::runtime_error("driver: a whole move into fewer bins");
        apply_move(B[m.dst_ibf].get(), f_bins[m.dst_ibf], A[m.src_ibf].get(), bins_a[m.src_ibf], rows[m.src_ibf],
                   m.whole ? std::vector<gn_bin_span>{ gn_bin_span{ 0, 0, (uint32_t)bins_a[m.src_ibf], 0 } } : m.spans); // (the one span that gives what gn_filter_copy_ibf gives)
    }
    for (const gnhibf::TransferFold& f : t.folds)
    {
        check(f.parent, f.src_ibf);
        apply_fold(B[f.parent].get(), f_bins[f.parent], A[f.src_ibf].get(), bins_a[f.src_ibf], rows[f.src_ibf], f);
    }

    std::printf("case %zu %llu\n", f_bins.size(), (unsigned long long)plan.n_user_bins);
    for (size_t i = 0; i < f_bins.size(); ++i)
    {
        std::printf("table %zu %llu %llu", i, (unsigned long long)f_bins[i], (unsigned long long)f_rows[i]);
        for (uint64_t b = 0; b < f_bins[i]; ++b)
            std::printf(" %lld", (long long)f_nx[i][b]);
        for (uint64_t b = 0; b < f_bins[i]; ++b)
            std::printf(" %lld", (long long)f_bu[i][b]);
        std::printf("\n");
        for (uint64_t r = 0; r < f_rows[i]; ++r)
        {
            std::printf("row %zu %llu", i, (unsigned long long)r);
            for (uint64_t w = 0; w < words(f_bins[i]); ++w)
                std::printf(" %llx", (unsigned long long)B[i][r * words(f_bins[i]) + w]);
            std::printf("\n");
        }
    }
    for (const gnhibf::TransferMove& m : t.moves)
    {
        std::printf("move %u %u %s", m.dst_ibf, m.src_ibf, m.whole ? "whole" : "spans");
        if (!m.whole)
            std::printf(" %zu", m.spans.size());
        for (const gn_bin_span& s : m.spans)
            std::printf(" %u %u %u", s.src_first, s.dst_first, s.n_bins);
        std::printf("\n");
    }
    for (const gnhibf::TransferFold& f : t.folds)
    {
        std::printf("fold %u %u %u %u %zu", f.parent, f.merged_bin, f.n_groups, f.src_ibf, f.members.size());
        for (const gn_fold_member& m : f.members)
            std::printf(" %u %u %u", m.src_first, m.n_bins, m.group);
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
            if (what == "transfer")
                transfer_case(in);
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
