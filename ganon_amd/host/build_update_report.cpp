// build_update_report.cpp -- what `ganon-build --hibf --update` says on stdout once the file is written: the index line, a line per
// new, removed and extended target with its path, the IBFs and merged bins that changed with their fill before and after, the merged
// bins a fold made, and the result line.  No device call and no file in here: everything comes in one UpdateReport.
#include "build_update.hpp"

#include <algorithm>
#include <cmath>
#include <iomanip>
#include <numeric>

namespace gnbuild
{

namespace
{

uint32_t used_entries(const gn_path_entry* p, uint32_t depth)
{
    uint32_t used = 0;
    while (used < depth && p[used].n_bins)
        ++used;
    return used;
}

// a path from the root down, `ibf:first_bin` per entry
void print_path(std::ostream& os, const gn_path_entry* p, uint32_t depth)
{
    for (uint32_t d = used_entries(p, depth); d-- > 0;)
        os << p[d].ibf << ":" << p[d].first_bin << (d ? " " : "");
}

void print_removed(std::ostream& os, const UpdateReport& r)
{
    // (old numbers: what left is named as the index given knows it; `stale` speaks of the file written)
    auto estimate = [](uint64_t hashes, bool full) { return full ? std::string("full") : std::to_string(hashes); };
    const gnhibf::Paths was = gnhibf::derive_paths(r.bins_a, r.nx_a, r.bu_a, r.n_old);
    os << "#removed\ttarget\tuser_bin\tleaf_ibf\tfirst_bin\tbins\tbits\testimated_hashes\tpath\n";
    for (size_t j = 0; j < r.gone.removed.size(); ++j)
    {
        const gnhibf::RemovedRun& run = r.gone.removed[j];
        os << "removed\t" << (j < r.remove_name.size() ? r.remove_name[j] : std::string("?")) << "\t" << run.user_bin << "\t" << run.ibf << "\t" << run.first_bin << "\t"
           << run.n_bins << "\t" << run.bits << "\t" << estimate(run.hashes, run.full) << "\t";
        print_path(os, &was.entries[(size_t)run.user_bin * was.depth], was.depth);
        os << "\n";
    }
    os << "#dropped\tibf\tparent_ibf\tparent_bin\n";
    for (const gnhibf::RemoveDropped& d : r.gone.dropped)
        os << "dropped\t" << d.ibf << "\t" << d.parent_ibf << "\t" << d.parent_bin << "\n";
    os << "#stale\tibf\tbin\tbits\testimated_stale_hashes\n";
    for (const gnhibf::RemoveStale& st : r.gone.stale)
    {
        const auto [i, b] = r.final.now(st.ibf, st.bin);
        os << "stale\t" << i << "\t" << b << "\t" << r.pop_b[i][b] << "\t" << estimate(st.hashes, st.full) << "\n";
    }
}

void print_extended(std::ostream& os, const UpdateReport& r)
{
    const uint32_t depth = r.final.depth;
    os << "#extended\ttarget\tuser_bin\thashes\talready_present\tinserted\tleaf_ibf\tfirst_bin\tbins\tpath\n";
    for (size_t j = 0; j < r.ext_name.size(); ++j)
    {
        const gn_path_entry* p        = &r.old_paths.entries[(size_t)r.ext_user_b[j] * depth];
        const uint64_t       n        = r.ext_counts[j];
        const uint64_t       inserted = std::accumulate(r.ex.quotas[j].begin(), r.ex.quotas[j].end(), uint64_t(0));
        os << "extended\t" << r.ext_name[j] << "\t" << r.ext_user_b[j] << "\t" << n << "\t" << n - inserted << "\t" << inserted << "\t" << p[0].ibf << "\t" << p[0].first_bin
           << "\t" << p[0].n_bins << "\t";
        print_path(os, p, depth);
        os << "\n";
    }
    os << "#run\tibf\tbin\tdealt\tbits_before\tbits_predicted\tbits_after\n";
    for (const gnhibf::ExtendRunBin& run : r.ex.run)
    {
        const auto [i, b] = r.final.now(run.ibf, run.bin);
        os << "run\t" << i << "\t" << b << "\t" << run.dealt << "\t" << run.bits_before << "\t" << std::fixed << std::setprecision(1) << run.bits_predicted << "\t"
           << r.pop_b[i][b] << "\n";
    }
}

// the `ibf` lines: every IBF that gained or lost bins or lies on a path this command wrote along
void print_ibfs(std::ostream& os, const UpdateReport& r)
{
    const uint64_t n_ibf_b = r.bins.size();
    os << "#ibf\trows\tbins_before\tbins_after\tmax_fill_before\tmax_fill_after\n" << std::fixed << std::setprecision(6);
    for (uint64_t i = 0; i < n_ibf_b; ++i)
        if (r.shown[i])
            os << "ibf\t" << i << "\t" << r.rows[i] << "\t" << (r.removing ? r.bins_a[r.gone.old_ibf[i]] : r.bins[i]) << "\t" << r.final.bins[i] << "\t"
               << *std::max_element(r.pop[i].begin(), r.pop[i].end()) / (double)r.rows[i] << "\t"
               << *std::max_element(r.pop_b[i].begin(), r.pop_b[i].end()) / (double)r.rows[i] << "\n";
    for (uint64_t i = n_ibf_b; i < r.final.bins.size(); ++i) // (--fold: an IBF it creates had no bin before)
        os << "ibf\t" << i << "\t" << r.final.rows[i] << "\t0\t" << r.final.bins[i] << "\t" << 0.0 << "\t"
           << *std::max_element(r.pop_b[i].begin(), r.pop_b[i].end()) / (double)r.final.rows[i] << "\n";
}

struct Fullest // the fullest merged bin among those touched: its bits and its IBF's rows
{
    uint64_t bits = 0, rows = 1;
    bool     any = false;
};

Fullest print_merged(std::ostream& os, const UpdateReport& r, double bound_fill)
{
    os << "#merged\tibf\tbin\tbits_before\tbits_predicted\tbits_after\n";
    Fullest                            f;
    std::vector<gnhibf::UpdateTouched> touched = r.ex.touched; // the extensions' merged bins, then the new user bins'; a bin of both once,
    for (const gnhibf::UpdateTouched& t : r.plan.touched)      // with the later prediction (which starts from the earlier)
    {
        auto at = std::find_if(touched.begin(), touched.end(), [&](const gnhibf::UpdateTouched& x) { return x.ibf == t.ibf && x.bin == t.bin; });
        if (at == touched.end())
            touched.push_back(t);
        else
            at->bits_predicted = t.bits_predicted;
    }
    for (const gnhibf::UpdateTouched& t : touched)
    {
        const auto [ti, tb]  = r.final.now(t.ibf, t.bin); // (a merged bin stays in its IBF; a fold may move it to the left)
        const uint64_t after = r.pop_b[ti][tb];
        os << "merged\t" << ti << "\t" << tb << "\t" << t.bits_before << "\t" << std::setprecision(1) << t.bits_predicted << std::setprecision(6) << "\t" << after
           << (after > bound_fill * r.rows[t.ibf] ? "\tWARN fill" : "") << "\n";
        if (!f.any || after * (double)f.rows > f.bits * (double)r.rows[t.ibf])
            f.bits = after, f.rows = r.rows[t.ibf];
        f.any = true;
    }
    return f;
}

} // namespace

void print_update_report(std::ostream& os, const UpdateReport& r)
{
    const uint32_t depth      = r.final.depth;
    const double   bound_fill = std::pow(r.fpr, 1.0 / r.h);
    os << "index\t" << r.update << "\t->\t" << r.output_file << "\tk=" << r.kmer_size << " w=" << r.window_size << " h=" << r.h << " ibfs=" << r.bins_a.size();
    if (r.removing || r.folding)
        os << "->" << r.final.bins.size();
    os << " levels=" << depth << " user_bins=" << r.n_old << "->" << r.plan.n_user_bins << " fpr=" << r.fpr << "\n";
    os << "#target\tuser_bin\tdistinct_hashes\tleaf_ibf\tfirst_bin\tbins\tdepth\tpath\n";
    uint64_t bins_added = 0;
    for (size_t j = 0; j < r.fresh_name.size(); ++j)
    {
        const gn_path_entry* p = &r.new_paths.entries[j * depth];
        os << "target\t" << r.fresh_name[j] << "\t" << r.n_base + j << "\t" << r.fresh_counts[j] << "\t" << p[0].ibf << "\t" << p[0].first_bin << "\t" << p[0].n_bins << "\t"
           << used_entries(p, depth) << "\t";
        print_path(os, p, depth);
        os << "\n";
        bins_added += p[0].n_bins;
    }
    if (r.removing)
        print_removed(os, r);
    if (r.extending)
        print_extended(os, r);
    print_ibfs(os, r);
    const Fullest f = print_merged(os, r, bound_fill);
    if (r.folding)
    {
        // (a merged bin that holds new user bins was predicted with their fills; one an extension passes through may end above it)
        os << "#folded\tparent_ibf\tmerged_bin\tnew_ibf\truns\tbins\tbits_predicted\tbits_found\n";
        for (const gnhibf::FoldGroup& g : r.fold.groups)
        {
            const uint64_t found = r.pop_b[g.parent][g.merged_bin];
            os << "folded\t" << g.parent << "\t" << g.merged_bin << "\t" << g.new_ibf << "\t" << g.runs << "\t" << g.bins << "\t" << std::setprecision(1) << g.bits_predicted
               << std::setprecision(6) << "\t" << found << (found > bound_fill * r.final.rows[g.parent] ? "\tWARN fill" : "") << "\n";
        }
    }
    os << "result\tok\t";
    if (r.removing)
        os << r.gone.removed.size() << " user bin(s) removed, " << r.gone.dropped.size() << " IBF(s) dropped, ";
    if (r.folding)
        os << r.fold.groups.size() << " IBF(s) created under " << r.fold.folded.size() << " folded, ";
    if (r.extending)
        os << r.ext_name.size() << " user bin(s) extended, ";
    os << r.fresh_name.size() << " user bin(s) added, " << bins_added << " bin(s) added, " << r.bytes_before << " -> " << r.bytes_after
       << " bytes, fullest touched merged bin ";
    if (!f.any)
        os << "n/a";
    else if (f.bits >= f.rows)
        os << "full";
    else
        os << std::setprecision(0) << -((double)f.rows / r.h) * std::log(1.0 - (double)f.bits / f.rows) << " estimated hashes at fill " << std::setprecision(6)
           << (double)f.bits / f.rows;
    os << std::endl;
}

} // namespace gnbuild
