// hibf_update.hpp -- where the user bins that `ganon-build --hibf --update` adds to an existing index go.  Host only: no device, no I/O.
//
// The tree of the file stays: no IBF is created, removed or resized in its rows; IBFs only gain bins at their end.  A file does not say
// how many hashes a bin holds, so the rule works on what the bits show: t[i][b] = rows of IBF i whose bit b is set
// (gn_filter_bin_popcounts).  With rows[i] = m rows and h hash functions:
//   fits(n, s, i)       gnbuild::hibf_run_bits(n, s, fpr, h) <= rows[i]: n hashes dealt to a run of s bins of IBF i stay at fpr
//   predict(t, n, m)    m * (1 - (1 - t / m) * exp(-(double)h * n / m)): the expected set bits of a bin with t set bits after n more
//                       hashes, none of which it holds already (which maximises it)
//   a merged bin b of IBF i with child c is ELIGIBLE for a set of n hashes when
//                       predict(t_now[i][b], n, rows[i]) <= pow(fpr, 1.0 / h) * rows[i]   (the fill at which one bin answers falsely at
//                                                                                           fpr: the bound hibf_run_bits sizes to)
//                       and fits(n, 1, c)                                                  (the set goes unsplit into the child)
// New user bins are taken in the order (count descending, input order); user bin ids are n_user_old + position in the input.  Each
// descends from IBF 0: where the current IBF has an eligible merged bin, the one with the lowest predicted fill is taken (ties: the
// lower bin), its t_now becomes the prediction, and the descent goes on in its child.  Otherwise the user bin becomes a new run at the
// end of the current IBF: the least s >= 1 with fits(n, s, i), bins [bins_i, bins_i + s).  t_now carries over from one new user bin
// to the next, so that two of them do not claim the same room.
// Doubles occur in predict, in the eligibility bound, and inside hibf_run_bits; everything else is integers, and the same input gives
// the same plan.
// Stated limits: this plan creates no IBF and grafts no subtree -- a user bin that fits no merged bin of the root widens the root; what
// holds an updated IBF to a number of bins is plan_fold (hibf_fold.hpp, `--fold`), which runs on the tables this plan leaves.  Refused (std::runtime_error): malformed tables (derive_paths is called first), inconsistent sizes, a count of 0 or
// above 2^48, and a run that would need more than 65536 bins.
//
// `--update --extend` adds hashes to user bins the index holds already (plan_extend; it comes first, since an extension has no choice of
// place, and plan_update then starts from the fills it predicts).  A user bin's run stays where and as wide as it is.  The hashes the run
// does not hold yet (gn_filter_probe_path's lost_at of the leaf entry) are dealt to its bins by what the bits show (deal_run):
//   e_j = ceil(-(m / h) * log1p(-t_j / m))   the estimated number of hashes bin j holds (doubles; everything after it is integers)
//   level L = the largest with sum_j max(0, L - e_j) <= a;  q_j = max(0, L - e_j);  what is left of a goes one each to the bins with
//   e_j <= L in the order (e_j, j): the emptiest bins are filled up to a common level.
// A run bin is predicted at predict(t_j, q_j, m), a merged bin on the path at predict(t, lost_at of its entry, m).  A bin is OVER ITS BOUND
// when the prediction exceeds, for a bin of a run of s bins, pow(1 - exp(log(1 - fpr) / s), 1 / h) * m (the fill at which the bin answers
// falsely at the per-bin rate hibf_run_bits sizes to) and, for a merged bin, pow(fpr, 1 / h) * m as above.  The plan lists such bins;
// a run is never moved or widened, so the caller refuses the update.
#pragma once

#include "build_params.hpp"
#include "hibf_paths.hpp"

#include <cmath>
#include <numeric>

namespace gnhibf
{

struct UpdateTouched // a merged bin on the path of at least one new user bin
{
    uint32_t ibf = 0, bin = 0;
    uint64_t bits_before = 0;
    double   bits_predicted = 0; // after every new user bin that passes through it
};

struct UpdatePlan
{
    Paths                             paths;       // of the new user bins, in input order; depth = the tree's
    std::vector<uint64_t>             bins;        // per IBF, after the update
    std::vector<std::vector<int64_t>> next_ibf_id; // the new tables
    std::vector<std::vector<int64_t>> bin_to_user;
    std::vector<UpdateTouched>        touched;     // in the order they were first taken
    uint64_t                          n_user_bins = 0;
};

constexpr uint64_t kUpdateMaxCount = 1ull << 48; // hibf_run_bits stays far inside 64 bits
constexpr uint64_t kUpdateMaxSplit = 1ull << 16;

inline double update_predict(double t, uint64_t n, uint64_t m, uint8_t h)
{
    return m * (1.0 - (1.0 - t / m) * std::exp(-(double)h * n / m));
}

// a hashes that a run does not hold yet, dealt to its bins: t[j] of m rows are set in bin j.  -> the quotas, which sum to a
inline std::vector<uint64_t> deal_run(const std::vector<uint64_t>& t, uint64_t m, uint8_t h, uint64_t a)
{
    auto refuse = [](const std::string& msg) -> void { throw std::runtime_error("HIBF update: " + msg); };
    const size_t s = t.size();
    if (s == 0 || m == 0 || h < 1 || h > 5 || a > kUpdateMaxCount)
        refuse("a run of " + std::to_string(s) + " bins of " + std::to_string(m) + " rows, " + std::to_string(a) + " hashes to deal");
    std::vector<uint64_t> e(s);
    for (size_t j = 0; j < s; ++j)
    {
        if (t[j] >= m)
            refuse("bin " + std::to_string(j) + " of the run is full (" + std::to_string(t[j]) + " bits set in " + std::to_string(m) + " rows)");
        e[j] = (uint64_t)std::ceil(-((double)m / h) * std::log1p(-(double)t[j] / m));
    }
    std::vector<uint32_t> order(s);
    std::iota(order.begin(), order.end(), 0u);
    std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return e[x] < e[y]; }); // (e_j, j)
    // with the k emptiest bins taking part the level costs k * L - (e of those k, summed); it rises while the next bin is reached
    uint64_t level = e[order[0]], sum = 0;
    size_t   k     = 0;
    while (k < s)
    {
        sum += e[order[k]];
        ++k;
        if (k < s && k * e[order[k]] - sum <= a)
            continue;
        level = (a + sum) / k;
        break;
    }
    std::vector<uint64_t> q(s, 0);
    uint64_t              dealt = 0;
    for (size_t j = 0; j < s; ++j)
        if (e[j] < level)
            q[j] = level - e[j], dealt += q[j];
    for (size_t i = 0; i < s && dealt < a; ++i) // (fewer are left than bins at or below the level: the level would be higher otherwise)
        if (e[order[i]] <= level)
            ++q[order[i]], ++dealt;
    return q;
}

struct ExtendInput // an old user bin that gains hashes
{
    uint64_t              user_bin = 0, hashes = 0;
    std::vector<uint64_t> lost_at; // gn_filter_probe_path's, one per entry of the user bin's path (depth of them)
};

struct ExtendRunBin
{
    uint32_t ibf = 0, bin = 0;
    uint64_t dealt = 0, bits_before = 0;
    double   bits_predicted = 0;
};

struct ExtendOver // a bin predicted over its bound
{
    uint32_t extension = 0, ibf = 0, bin = 0; // index into the inputs
    double   bits_predicted = 0, bound = 0;
};

struct ExtendPlan
{
    std::vector<std::vector<uint64_t>> quotas;  // per extension: one per bin of its run
    std::vector<ExtendRunBin>          run;     // every bin of every extended run, in input order
    std::vector<UpdateTouched>         touched; // the merged bins on the extended paths, in the order they were first met
    std::vector<ExtendOver>            over;
    std::vector<std::vector<double>>   fills;   // per IBF and bin: the prediction where the plan touches a bin, the bit count elsewhere
};

inline ExtendPlan plan_extend(const Paths& old, const std::vector<uint64_t>& bins, const std::vector<uint64_t>& rows, uint8_t h, double fpr,
                              const std::vector<std::vector<uint64_t>>& popcounts, const std::vector<ExtendInput>& ext)
{
    auto refuse = [](const std::string& m) -> void { throw std::runtime_error("HIBF update: " + m); };
    const uint64_t n_ibf = bins.size(), n_user = old.depth ? old.entries.size() / old.depth : 0;
    if (rows.size() != n_ibf || popcounts.size() != n_ibf || old.depth == 0)
        refuse("rows / bit counts do not have one entry per IBF");
    if (h < 1 || h > 5 || !(fpr > 0.0 && fpr < 1.0))
        refuse("hash functions " + std::to_string(h) + " / false-positive rate " + std::to_string(fpr) + " out of range");
    ExtendPlan plan;
    plan.fills.resize(n_ibf);
    for (uint64_t i = 0; i < n_ibf; ++i)
    {
        if (rows[i] == 0)
            refuse("IBF " + std::to_string(i) + " has no rows");
        if (popcounts[i].size() < bins[i])
            refuse("IBF " + std::to_string(i) + ": " + std::to_string(bins[i]) + " bins, but " + std::to_string(popcounts[i].size()) + " bit counts");
        for (uint64_t b = 0; b < bins[i]; ++b)
            if (popcounts[i][b] > rows[i])
                refuse("IBF " + std::to_string(i) + " bin " + std::to_string(b) + ": " + std::to_string(popcounts[i][b]) + " bits set in " +
                       std::to_string(rows[i]) + " rows");
        plan.fills[i].assign(popcounts[i].begin(), popcounts[i].begin() + bins[i]);
    }
    std::vector<std::vector<int64_t>> touched_at(n_ibf); // index into plan.touched, or -1
    for (uint64_t i = 0; i < n_ibf; ++i)
        touched_at[i].assign(bins[i], -1);
    std::vector<bool> seen(n_user, false);
    for (size_t x = 0; x < ext.size(); ++x)
    {
        const ExtendInput& in = ext[x];
        if (in.user_bin >= n_user || seen[in.user_bin])
            refuse("extension " + std::to_string(x) + ": user bin " + std::to_string(in.user_bin) + " of " + std::to_string(n_user) + ", or named twice");
        seen[in.user_bin] = true;
        if (in.lost_at.size() != old.depth || in.hashes == 0 || in.hashes > kUpdateMaxCount)
            refuse("extension " + std::to_string(x) + ": " + std::to_string(in.hashes) + " hashes, " + std::to_string(in.lost_at.size()) + " counts for a path of " +
                   std::to_string(old.depth));
        const gn_path_entry* p = &old.entries[(size_t)in.user_bin * old.depth];
        for (uint32_t d = 0; d < old.depth; ++d)
            if (in.lost_at[d] > in.hashes || (p[d].n_bins == 0 && in.lost_at[d] != 0) || (p[d].n_bins && (p[d].ibf >= n_ibf || (uint64_t)p[d].first_bin + p[d].n_bins > bins[p[d].ibf])))
                refuse("extension " + std::to_string(x) + ": entry " + std::to_string(d) + " of its path");
        // the run
        const uint64_t        m = rows[p[0].ibf];
        std::vector<uint64_t> t(popcounts[p[0].ibf].begin() + p[0].first_bin, popcounts[p[0].ibf].begin() + p[0].first_bin + p[0].n_bins);
        plan.quotas.push_back(deal_run(t, m, h, in.lost_at[0]));
        const double run_bound = std::pow(1.0 - std::exp(std::log(1.0 - fpr) / p[0].n_bins), 1.0 / h) * m;
        for (uint32_t j = 0; j < p[0].n_bins; ++j)
        {
            const double fill = update_predict((double)t[j], plan.quotas.back()[j], m, h);
            plan.run.push_back(ExtendRunBin{ p[0].ibf, p[0].first_bin + j, plan.quotas.back()[j], t[j], fill });
            plan.fills[p[0].ibf][p[0].first_bin + j] = fill;
            if (!(fill <= run_bound))
                plan.over.push_back(ExtendOver{ (uint32_t)x, p[0].ibf, p[0].first_bin + j, fill, run_bound });
        }
        // the merged bins above it
        for (uint32_t d = 1; d < old.depth && p[d].n_bins; ++d)
        {
            const uint32_t i = p[d].ibf, b = p[d].first_bin;
            const double   bound = std::pow(fpr, 1.0 / h) * rows[i];
            const double   fill  = update_predict(plan.fills[i][b], in.lost_at[d], rows[i], h);
            if (touched_at[i][b] < 0)
            {
                touched_at[i][b] = (int64_t)plan.touched.size();
                plan.touched.push_back(UpdateTouched{ i, b, popcounts[i][b], 0 });
            }
            plan.fills[i][b]                               = fill;
            plan.touched[touched_at[i][b]].bits_predicted = fill;
            if (!(fill <= bound))
                plan.over.push_back(ExtendOver{ (uint32_t)x, i, b, fill, bound });
        }
    }
    return plan;
}

inline UpdatePlan plan_update(const std::vector<uint64_t>& bins, const std::vector<uint64_t>& rows, const std::vector<std::vector<int64_t>>& next_ibf_id,
                              const std::vector<std::vector<int64_t>>& bin_to_user, uint64_t n_user_old, uint8_t h, double fpr,
                              const std::vector<std::vector<uint64_t>>& popcounts, const std::vector<uint64_t>& new_counts,
                              const std::vector<std::vector<double>>* fills = nullptr) // the fills to start from: ExtendPlan::fills
{
    auto refuse = [](const std::string& m) -> void { throw std::runtime_error("HIBF update: " + m); };
    const Paths    old   = derive_paths(bins, next_ibf_id, bin_to_user, n_user_old); // (refuses malformed tables)
    const uint64_t n_ibf = bins.size();
    if (rows.size() != n_ibf || popcounts.size() != n_ibf)
        refuse("rows / bit counts do not have one entry per IBF");
    if (h < 1 || h > 5 || !(fpr > 0.0 && fpr < 1.0))
        refuse("hash functions " + std::to_string(h) + " / false-positive rate " + std::to_string(fpr) + " out of range");
    if (n_user_old + new_counts.size() > 0x7FFFFFFFFFFFFFFFull || new_counts.size() > 0xFFFFFFFFull)
        refuse("too many user bins");
    for (uint64_t i = 0; i < n_ibf; ++i)
    {
        if (rows[i] == 0)
            refuse("IBF " + std::to_string(i) + " has no rows");
        if (popcounts[i].size() < bins[i])
            refuse("IBF " + std::to_string(i) + ": " + std::to_string(bins[i]) + " bins, but " + std::to_string(popcounts[i].size()) + " bit counts");
        for (uint64_t b = 0; b < bins[i]; ++b)
            if (popcounts[i][b] > rows[i])
                refuse("IBF " + std::to_string(i) + " bin " + std::to_string(b) + ": " + std::to_string(popcounts[i][b]) + " bits set in " +
                       std::to_string(rows[i]) + " rows");
    }
    for (size_t k = 0; k < new_counts.size(); ++k)
        if (new_counts[k] == 0 || new_counts[k] > kUpdateMaxCount)
            refuse("new user bin " + std::to_string(k) + ": " + std::to_string(new_counts[k]) + " distinct hashes (1.." + std::to_string(kUpdateMaxCount) + ")");

    UpdatePlan plan;
    plan.bins        = bins;
    plan.next_ibf_id = next_ibf_id;
    plan.bin_to_user = bin_to_user;
    for (uint64_t i = 0; i < n_ibf; ++i) // (the tables may be longer than the IBF has bins)
        plan.next_ibf_id[i].resize(bins[i]), plan.bin_to_user[i].resize(bins[i]);
    plan.n_user_bins = n_user_old + new_counts.size();
    plan.paths.depth = old.depth;
    plan.paths.entries.assign(new_counts.size() * (size_t)old.depth, gn_path_entry{ 0, 0, 0, 0, 0 });

    std::vector<std::vector<double>> t_now(n_ibf);
    for (uint64_t i = 0; i < n_ibf; ++i)
    {
        if (fills && (fills->size() != n_ibf || (*fills)[i].size() < bins[i]))
            refuse("the starting fills do not have one entry per bin");
        if (fills)
            t_now[i].assign((*fills)[i].begin(), (*fills)[i].begin() + bins[i]);
        else
            t_now[i].assign(popcounts[i].begin(), popcounts[i].begin() + bins[i]);
    }
    std::vector<std::vector<int64_t>> touched_at(n_ibf); // index into plan.touched, or -1
    for (uint64_t i = 0; i < n_ibf; ++i)
        touched_at[i].assign(bins[i], -1);

    std::vector<uint32_t> order(new_counts.size());
    std::iota(order.begin(), order.end(), 0u);
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return new_counts[a] > new_counts[b]; });

    auto fits = [&](uint64_t n, uint64_t s, uint64_t i) { return gnbuild::hibf_run_bits(n, s, fpr, h) <= rows[i]; };
    std::vector<gn_path_entry> down; // the merged bins taken, from the root
    for (const uint32_t k : order)
    {
        const uint64_t n = new_counts[k];
        down.clear();
        uint64_t i = 0;
        for (;;)
        {
            const double bound    = std::pow(fpr, 1.0 / h) * rows[i];
            int64_t      best     = -1;
            double       best_fill = 0;
            for (uint64_t b = 0; b < bins[i]; ++b) // (the bins the file had: a new run is never merged)
            {
                if (bin_to_user[i][b] >= 0)
                    continue;
                const double fill = update_predict(t_now[i][b], n, rows[i], h);
                if (!(fill <= bound) || !fits(n, 1, (uint64_t)next_ibf_id[i][b]))
                    continue;
                if (best < 0 || fill < best_fill)
                    best = (int64_t)b, best_fill = fill;
            }
            if (best < 0)
                break;
            if (touched_at[i][best] < 0)
            {
                touched_at[i][best] = (int64_t)plan.touched.size();
                plan.touched.push_back(UpdateTouched{ (uint32_t)i, (uint32_t)best, popcounts[i][best], 0 });
            }
            t_now[i][best]                                       = best_fill;
            plan.touched[touched_at[i][best]].bits_predicted = best_fill;
            down.push_back(gn_path_entry{ (uint32_t)i, (uint32_t)best, 1, 0, 1 });
            i = (uint64_t)next_ibf_id[i][best];
            if (down.size() >= old.depth) // (cannot happen: derive_paths found no chain longer than depth - 1)
                refuse("the descent is deeper than the tree");
        }
        uint64_t s = 1;
        while (s <= kUpdateMaxSplit && s <= n && !fits(n, s, i))
            ++s;
        if (s > kUpdateMaxSplit || s > n)
            refuse("new user bin " + std::to_string(k) + " (" + std::to_string(n) + " distinct hashes) fits no run of up to " +
                   std::to_string(std::min(n, kUpdateMaxSplit)) + " bins of IBF " + std::to_string(i) + " (" + std::to_string(rows[i]) + " rows): rebuild the index");
        if (plan.bins[i] + s > 0xFFFFFFF0ull)
            refuse("IBF " + std::to_string(i) + " would have more than 2^32 - 16 bins");
        gn_path_entry* p = &plan.paths.entries[(size_t)k * old.depth];
        *p++             = gn_path_entry{ (uint32_t)i, (uint32_t)plan.bins[i], (uint32_t)s, 0, (n + s - 1) / s };
        for (size_t d = down.size(); d-- > 0;)
            *p++ = down[d];
        plan.bins[i] += s;
        plan.next_ibf_id[i].insert(plan.next_ibf_id[i].end(), s, (int64_t)i);
        plan.bin_to_user[i].insert(plan.bin_to_user[i].end(), s, (int64_t)(n_user_old + k));
    }
    return plan;
}

} // namespace gnhibf
