// build_update.cpp -- `ganon-build --hibf --update F` (this project's extension).
// Adds the inputs' targets to an index without its genomes: the file into filter A, how full every bin is off A's bits
// (gn_filter_bin_popcounts), the placement (hibf_update.hpp), filter B with the new bins, every IBF moved over (gn_filter_copy_ibf),
// the new sets along their paths, B written with the file's own header fields and strings and the new names behind them.
// With `--remove NAMES` targets leave on the way: the tables after the removal (hibf_remove.hpp) are what the placement works on, B is
// created without the dropped bins and IBFs, and the move compacts the columns (gn_filter_copy_ibf_spans) -- every row is read and
// written once either way.  A name in both NAMES and the inputs is replaced: the old user bin goes, the inputs enter as a new one.
// With `--fold N` the IBFs of the result are held to N bins (hibf_fold.hpp): the plan runs last, on the tables and fills the others leave,
// B is created with the new IBFs, every surviving and every new IBF takes its columns from A (gn_filter_copy_ibf_spans), the new merged
// bins are the OR of their groups' columns (gn_filter_fold_ibf), and the inserts go along the rewritten paths.
// Which calls move A into B is a plan of its own (hibf_transfer.hpp); run_update is the steps below in their order, each of which
// fills in its part of the UpdateReport (build_update.hpp) that build_update_report.cpp prints at the end.
#include "build_common.hpp"
#include "build_update.hpp"
#include "hibf_pool.hpp"
#include "hibf_transfer.hpp"

#include <algorithm>
#include <fstream>
#include <iomanip>
#include <memory>
#include <set>
#include <sstream>

namespace gnbuild
{

namespace
{

struct Stopwatch
{
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    double lap() // seconds since the last lap
    {
        const double s = since(t0);
        t0             = std::chrono::steady_clock::now();
        return s;
    }
};

struct Inputs // what every input is to the index, by its name
{
    std::vector<uint32_t> fresh_target; // the new targets, in input order: new user bin n_base + position
    std::vector<uint32_t> ext_target;   // --extend: the targets the index holds, in input order, and their user bins as A numbers them
    std::vector<uint64_t> ext_user;
    std::vector<uint64_t> remove_user;  // --remove: the user bins that leave, ascending
};

struct Loaded // the index given: its header and strings, and filter A on the device until every IBF is moved
{
    gnhost::FilterMeta                  meta;
    std::unique_ptr<gnhost::DeviceSink> sink;
};

// --remove: the names listed -> the user bins that leave and the name each of them carries
bool resolve_removal(const Config& c, const gnhost::FilterMeta& names, std::set<std::string>& leaving, Inputs& in, UpdateReport& r)
{
    std::vector<std::string> listed;
    std::ifstream            file(c.remove);
    for (std::string line; std::getline(file, line);)
    {
        if (!line.empty() && line.back() == '\r')
            line.pop_back();
        if (!line.empty() && leaving.insert(name_as_read(line)).second)
            listed.push_back(name_as_read(line));
    }
    const gnhibf::RemoveNames found = gnhibf::resolve_remove(names.targets, names.target_bins, names.bin_count, listed);
    if (!found.unknown.empty())
    {
        std::string m = "--remove: " + std::to_string(found.unknown.size()) + " name(s) are not in the index; nothing written:";
        for (const std::string& n : found.unknown)
            m += "\n  " + n;
        return fail(m);
    }
    if (!found.shared.empty())
    {
        std::string m = "--remove: a user bin that leaves also names a target that stays; nothing written:";
        for (const auto& [u, n] : found.shared)
            m += "\n  user bin " + std::to_string(u) + " also names " + n;
        return fail(m);
    }
    in.remove_user = found.user_bins;
    for (const uint64_t u : in.remove_user)
        for (size_t i = 0; i < names.targets.size() && i < names.target_bins.size(); ++i)
            if (std::find(names.target_bins[i].begin(), names.target_bins[i].end(), u) != names.target_bins[i].end())
            {
                r.remove_name.push_back(names.targets[i]);
                break;
            }
    return true;
}

// the names of the file against --remove's list and the inputs (`hashed`: the targets with a hash): what leaves, and per input whether
// it is new, replaced (it leaves and comes: a new user bin) or an extension
bool resolve_inputs(const Config& c, const std::vector<Target>& targets, const std::vector<uint32_t>& hashed, Inputs& in, UpdateReport& r)
{
    gnhost::FilterMeta names;
    gnhost::read_hibf_meta(c.update, names);
    std::set<std::string> leaving;
    if (c.remove_given && !resolve_removal(c, names, leaving, in, r))
        return false;
    const std::set<std::string> have(names.targets.begin(), names.targets.end());
    for (uint32_t t : hashed)
    {
        const std::string name = name_as_read(targets[t].name);
        if (!have.count(name) || leaving.count(name))
        {
            in.fresh_target.push_back(t);
            continue;
        }
        if (!c.extend)
            return fail("--update: target " + targets[t].name + " is already in the index (adding sequences to an existing user bin is not supported); nothing written");
        uint64_t held = 0, user = 0;
        for (size_t i = 0; i < names.targets.size(); ++i)
            if (names.targets[i] == name)
            {
                held += i < names.target_bins.size() ? names.target_bins[i].size() : 1;
                user = i < names.target_bins.size() && !names.target_bins[i].empty() ? names.target_bins[i][0] : i;
            }
        if (held != 1)
            return fail("--update --extend: " + std::to_string(held) + " user bins of the index are named " + targets[t].name + "; nothing written");
        in.ext_target.push_back(t), in.ext_user.push_back(user);
        r.ext_name.push_back(targets[t].name), r.ext_counts.push_back(targets[t].hashes.size());
    }
    for (uint32_t t : in.fresh_target)
        r.fresh_name.push_back(targets[t].name), r.fresh_counts.push_back(targets[t].hashes.size());
    r.ext_user_b = in.ext_user;
    return true;
}

std::vector<uint64_t> count_bits(const gn_filter* f, uint64_t ibf, uint64_t bins)
{
    std::vector<uint64_t> pop(bins, 0);
    if (gn_filter_bin_popcounts(f, (uint32_t)ibf, pop.data()) != GN_OK)
        throw std::runtime_error(gn_last_error());
    return pop;
}

// the file into filter A; its shape into the report
bool load_index(const Config& c, Loaded& a, UpdateReport& r)
{
    a.sink = std::make_unique<gnhost::DeviceSink>(c.device);
    gnhost::load_filter_file(c.update, true, a.meta, *a.sink);
    r.n_old = a.meta.n_user_bins;
    r.h     = (uint8_t)a.meta.shapes.at(0).hash_funs;
    r.fpr   = a.meta.ibf_config.max_fp;
    if (a.meta.raw_bin_path.size() != r.n_old || a.meta.raw_user_bin_filenames.size() != r.n_old)
        return fail("--update: the index names " + std::to_string(a.meta.raw_bin_path.size()) + " file lists for " + std::to_string(r.n_old) + " user bins");
    for (const gnhost::IbfShape& m : a.meta.shapes)
    {
        r.bins_a.push_back(m.bins), r.rows.push_back(m.bin_size);
        if (m.hash_funs != r.h)
            return fail("--update: the IBFs of the index differ in their hash functions");
    }
    r.bins = r.bins_a;
    return true;
}

// --remove: the tables the rest works on are those after the removal, with A's bit counts carried to the new places
void plan_removal(const Inputs& in, const gnhost::FilterMeta& meta, UpdateReport& r)
{
    r.n_base = r.n_old;
    if (!r.removing)
        return;
    r.gone = gnhibf::plan_remove(r.bins_a, meta.next_ibf_id, meta.bin_to_user, r.n_old, in.remove_user, r.rows, (uint8_t)r.h, &r.pop);
    std::vector<uint64_t> kept_rows;
    for (const uint32_t i : r.gone.old_ibf)
        kept_rows.push_back(r.rows[i]);
    r.rows.swap(kept_rows);
    r.bins = r.gone.bins, r.pop = r.gone.popcounts, r.n_base = r.gone.n_user_bins;
    r.nx_a = meta.next_ibf_id, r.bu_a = meta.bin_to_user;
}

// --extend probes A, along the paths of the file's own tables (left in r.old_paths): what every extension set's path lacks
bool probe_extensions(const std::vector<Target>& targets, const Inputs& in, const Loaded& a, UpdateReport& r, std::vector<gnhibf::ExtendInput>& ext)
{
    if (in.ext_target.empty())
        return true;
    r.old_paths       = gnhibf::derive_paths(r.bins_a, a.meta.next_ibf_id, a.meta.bin_to_user, r.n_old);
    const uint32_t d0 = r.old_paths.depth;
    ext.resize(in.ext_target.size());
    for (size_t j = 0; j < ext.size(); ++j)
    {
        if (in.ext_user[j] >= r.n_old)
            return fail("--update --extend: the index names user bin " + std::to_string(in.ext_user[j]) + " of " + std::to_string(r.n_old));
        ext[j].user_bin = in.ext_user[j], ext[j].hashes = targets[in.ext_target[j]].hashes.size();
        ext[j].lost_at.assign(d0, 0);
    }
    gnhibf::for_each_pooled(
        ext.size(), [&](size_t j) { return hash_set(targets[in.ext_target[j]]); }, [&](size_t j) { return &r.old_paths.entries[(size_t)in.ext_user[j] * d0]; }, d0,
        [&](const uint64_t* hashes, const uint64_t* off, size_t n, const gn_path_entry* p, const std::vector<size_t>& ids) {
            std::vector<uint64_t> found(n), first(n), lost(n * d0);
            if (gn_filter_probe_path(a.sink->filter(), hashes, off, (uint32_t)n, p, d0, found.data(), lost.data(), first.data()) != GN_OK)
                throw std::runtime_error(gn_last_error());
            for (size_t k = 0; k < n; ++k)
                ext[ids[k]].lost_at.assign(lost.begin() + k * d0, lost.begin() + (k + 1) * d0);
        });
    return true;
}

// --extend: the quotas of every extended run and the fills the new user bins start from, or the refusal of a bin over its bound
bool plan_extensions(const std::vector<std::vector<int64_t>>& nx, const std::vector<std::vector<int64_t>>& bu, std::vector<gnhibf::ExtendInput>& ext, UpdateReport& r)
{
    if (r.removing)
    {
        // a removal changes no bit of a surviving bin and no surviving path but for its numbers: what A lacks, B lacks.  The tree
        // may have lost levels; a surviving path is as long as it was, so what is cut off lost_at are unused entries
        r.old_paths = gnhibf::derive_paths(r.bins, nx, bu, r.n_base);
        for (size_t j = 0; j < ext.size(); ++j)
        {
            ext[j].user_bin = r.ext_user_b[j] = (uint64_t)r.gone.user_map[ext[j].user_bin];
            ext[j].lost_at.resize(r.old_paths.depth);
        }
    }
    r.ex = gnhibf::plan_extend(r.old_paths, r.bins, r.rows, (uint8_t)r.h, r.fpr, r.pop, ext);
    if (r.ex.over.empty())
        return true;
    std::ostringstream m;
    m << "--update --extend: " << r.ex.over.size() << " bin(s) would be over their bound; nothing written:";
    for (const gnhibf::ExtendOver& o : r.ex.over)
        m << "\n  target " << r.ext_name[o.extension] << ": IBF " << o.ibf << " bin " << o.bin << " predicted " << std::fixed << std::setprecision(1) << o.bits_predicted
          << " bits, bound " << o.bound;
    m << "\na run is never moved or widened: leave it out or rebuild";
    return fail(m.str());
}

// --fold: the rule runs last, on the tables the plans before it leave and on a fill per bin: the bit count A shows (or the extension's
// prediction), the prediction for a merged bin the new user bins touch, and for a bin of a new run what its share of hashes sets
bool plan_folding(const Config& c, UpdateReport& r)
{
    std::vector<std::vector<double>> fills(r.bins.size());
    for (uint64_t i = 0; i < r.bins.size(); ++i)
    {
        if (!r.ext_name.empty())
            fills[i] = r.ex.fills[i];
        else
            fills[i].assign(r.pop[i].begin(), r.pop[i].begin() + r.bins[i]);
        fills[i].resize(r.plan.bins[i], 0.0);
    }
    for (const gnhibf::UpdateTouched& t : r.plan.touched)
        fills[t.ibf][t.bin] = t.bits_predicted;
    for (size_t j = 0; j < r.fresh_name.size(); ++j)
    {
        const gn_path_entry& run = r.plan.paths.entries[j * r.plan.paths.depth];
        for (uint32_t b = run.first_bin; b < run.first_bin + run.n_bins; ++b)
            fills[run.ibf][b] = gnhibf::update_predict(0.0, run.hashes_per_bin, r.rows[run.ibf], (uint8_t)r.h); // (ceil(count / bins of the run))
    }
    try
    {
        r.fold = gnhibf::plan_fold(r.plan.bins, r.rows, r.plan.next_ibf_id, r.plan.bin_to_user, r.plan.n_user_bins, (uint8_t)r.h, r.fpr, fills, c.fold);
    }
    catch (const gnhibf::FoldUnreachable& e)
    {
        return fail(std::string("--fold: ") + e.what() + "; nothing written");
    }
    r.new_paths = gnhibf::fold_paths(r.plan.paths, r.fold);
    if (!r.ext_name.empty())
        r.old_paths = gnhibf::fold_paths(r.old_paths, r.fold);
    return true;
}

// the plans on the tables B starts from, in their order: the extensions, the placement of the new user bins, the fold; then the
// tables of the file written
bool make_plans(const Config& c, const gnhost::FilterMeta& meta, std::vector<gnhibf::ExtendInput>& ext, UpdateReport& r)
{
    const std::vector<std::vector<int64_t>>& nx = r.removing ? r.gone.next_ibf_id : meta.next_ibf_id;
    const std::vector<std::vector<int64_t>>& bu = r.removing ? r.gone.bin_to_user : meta.bin_to_user;
    if (!ext.empty() && !plan_extensions(nx, bu, ext, r))
        return false;
    r.plan      = gnhibf::plan_update(r.bins, r.rows, nx, bu, r.n_base, (uint8_t)r.h, r.fpr, r.pop, r.fresh_counts, ext.empty() ? nullptr : &r.ex.fills);
    r.new_paths = r.plan.paths;
    if (r.folding && !plan_folding(c, r))
        return false;
    r.final = r.folding ? FinalTables{ r.fold.bins, r.fold.rows, r.fold.next_ibf_id, r.fold.bin_to_user, r.fold.depth, r.fold.where }
                        : FinalTables{ r.plan.bins, r.rows, r.plan.next_ibf_id, r.plan.bin_to_user, r.plan.paths.depth, {} };
    return true;
}

// filter B: the same rows, the new bins.  A and B are on the device together until every IBF is moved
bool create_b(const Config& c, const gnhost::FilterMeta& meta, const UpdateReport& r, std::vector<HibfShape>& ibfs, gnhost::OwnedFilter& b)
{
    const FinalTables& f = r.final;
    ibfs.resize(f.bins.size());
    uint64_t a_bytes = 0, b_bytes = 0;
    for (uint64_t i = 0; i < r.bins_a.size(); ++i)
        a_bytes += meta.shapes[i].bin_size * gn_hibf_row_stride_words((r.bins_a[i] + 63) >> 6) * 8;
    for (uint64_t i = 0; i < ibfs.size(); ++i)
    {
        ibfs[i].bins = f.bins[i], ibfs[i].rows = f.rows[i];
        ibfs[i].next_ibf_id = f.next_ibf_id[i], ibfs[i].bin_to_user = f.bin_to_user[i];
        b_bytes += f.rows[i] * gn_hibf_row_stride_words((f.bins[i] + 63) >> 6) * 8;
    }
    uint64_t free_b = 0, total_b = 0;
    if (gn_device_memory(c.device, &free_b, &total_b) != GN_OK)
        throw std::runtime_error(gn_last_error());
    // (free_b is what is left beside A.  The 256 MiB on top of B are for what is still to come on this device: the staging buffer
    // of the inserts (32 M hashes, 256 MiB at most, usually far less), their item and path tables, the bit counts, and whatever
    // the hasher streams of the counting phase have not yet given back)
    if (b_bytes + (256ull << 20) > free_b)
        return fail("--update: the index (" + std::to_string(a_bytes) + " bytes on the device) and the updated one (" + std::to_string(b_bytes) +
                    " bytes) do not fit device " + std::to_string(c.device) + " together (" + std::to_string(free_b) + " bytes free beside the index)");
    gnhost::HibfDescs descs;
    for (const HibfShape& s : ibfs)
        descs.add(s.bins, s.rows, (uint8_t)r.h, s.next_ibf_id, s.bin_to_user);
    b = descs.upload(c.device, r.plan.n_user_bins);
    if (!b)
        throw std::runtime_error(gn_last_error());
    return true;
}

// A into B, call by call as the transfer lists them -> the seconds the fold calls took
double execute_transfer(const gnhibf::Transfer& t, gn_filter* b, const gn_filter* a)
{
    for (const gnhibf::TransferMove& m : t.moves)
    {
        const int rc = m.whole ? gn_filter_copy_ibf(b, m.dst_ibf, a, m.src_ibf)
                               : gn_filter_copy_ibf_spans(b, m.dst_ibf, a, m.src_ibf, m.spans.data(), (uint32_t)m.spans.size());
        if (rc != GN_OK)
            throw std::runtime_error(gn_last_error());
    }
    const auto t_fold = std::chrono::steady_clock::now();
    for (const gnhibf::TransferFold& f : t.folds)
        if (gn_filter_fold_ibf(b, f.parent, f.merged_bin, f.n_groups, a, f.src_ibf, f.members.data(), (uint32_t)f.members.size()) != GN_OK)
            throw std::runtime_error(gn_last_error());
    return since(t_fold);
}

// the new sets along their paths, pooled as run_hibf pools them; before them the extensions, by their quotas
// (the pooler may cut the extensions into several calls.  A later call takes presence against B after the earlier ORs, not against A,
// where lost_at was counted; the counts still agree, because presence is a matter of the run's own columns and only the run's own set
// writes them -- one extension per user bin, and the new targets are inserted afterwards)
void insert_sets(const std::vector<Target>& targets, const Inputs& in, const UpdateReport& r, gn_filter* b)
{
    const uint32_t depth = r.final.depth;
    gnhibf::for_each_pooled(
        in.ext_target.size(), [&](size_t j) { return hash_set(targets[in.ext_target[j]]); }, [&](size_t j) { return &r.old_paths.entries[(size_t)r.ext_user_b[j] * depth]; }, depth,
        [&](const uint64_t* hashes, const uint64_t* off, size_t n, const gn_path_entry* p, const std::vector<size_t>& ids) {
            std::vector<uint64_t> deal_off{ 0 }, deal;
            for (size_t k = 0; k < n; ++k)
            {
                deal.insert(deal.end(), r.ex.quotas[ids[k]].begin(), r.ex.quotas[ids[k]].end());
                deal_off.push_back(deal.size());
            }
            if (gn_filter_extend_path(b, hashes, off, (uint32_t)n, p, depth, deal_off.data(), deal.data()) != GN_OK)
                throw std::runtime_error(gn_last_error());
        });
    gnhibf::for_each_pooled(
        in.fresh_target.size(), [&](size_t j) { return hash_set(targets[in.fresh_target[j]]); }, [&](size_t j) { return &r.new_paths.entries[j * depth]; }, depth,
        [&](const uint64_t* hashes, const uint64_t* off, size_t n, const gn_path_entry* p, const std::vector<size_t>&) {
            if (gn_filter_emplace_path(b, hashes, off, (uint32_t)n, p, depth) != GN_OK)
                throw std::runtime_error(gn_last_error());
        });
}

// B's bit counts, for the IBFs the report speaks of: those that gained or lost bins or lie on a path this command wrote along
void count_b(const gn_filter* b, UpdateReport& r)
{
    const uint64_t n_ibf_b = r.bins.size(), n_final = r.final.bins.size();
    const uint32_t depth   = r.final.depth;
    r.shown.assign(n_final, false);
    for (uint64_t i = 0; i < n_ibf_b; ++i)
        r.shown[i] = r.final.bins[i] != r.bins[i] || (r.removing && r.bins[i] != r.bins_a[r.gone.old_ibf[i]]);
    for (uint64_t i = n_ibf_b; i < n_final; ++i) // (--fold: the IBFs it creates)
        r.shown[i] = true;
    for (const uint32_t i : r.fold.folded)
        r.shown[i] = true;
    for (const gnhibf::RemoveStale& st : r.gone.stale)
        r.shown[st.ibf] = true;
    for (const gn_path_entry& e : r.new_paths.entries)
        if (e.n_bins)
            r.shown[e.ibf] = true;
    for (const uint64_t u : r.ext_user_b)
        for (uint32_t d = 0; d < depth && r.old_paths.entries[(size_t)u * depth + d].n_bins; ++d)
            r.shown[r.old_paths.entries[(size_t)u * depth + d].ibf] = true;
    r.pop_b.assign(n_final, {});
    for (uint64_t i = 0; i < n_final; ++i)
        if (r.shown[i])
            r.pop_b[i] = count_bits(b, i, r.final.bins[i]);
}

// the file: its header fields and strings as they are, the new names behind them in the form run_hibf writes
bool write_index(const Config& c, const gnhost::FilterMeta& meta, const std::vector<HibfShape>& ibfs, gnhost::OwnedFilter& b, UpdateReport& r)
{
    std::vector<std::vector<std::string>> bin_path   = meta.raw_bin_path;
    std::vector<std::string>              user_files = meta.raw_user_bin_filenames;
    if (r.removing) // the removed user bins' entries go; the others stay verbatim and in order
    {
        size_t kept = 0;
        for (uint64_t u = 0; u < r.n_old; ++u)
            if (r.gone.user_map[u] >= 0)
            {
                if (kept != u) // (a self-move would empty the entry)
                    bin_path[kept] = std::move(bin_path[u]), user_files[kept] = std::move(user_files[u]);
                ++kept;
            }
        bin_path.resize(kept), user_files.resize(kept);
    }
    const std::string dir = output_folder(c);
    for (const std::string& name : r.fresh_name)
    {
        const std::string f = dir + "/" + user_bin_file_name(name) + ".minimiser";
        bin_path.push_back({ f });
        user_files.push_back(f);
    }
    std::string err;
    const bool  saved = save_hibf(c, b.get(), ibfs, (uint8_t)r.h, bin_path, user_files, err); // (c holds the file's k, w and fpr: validate())
    b.reset();
    if (!saved)
        return fail(err);
    std::error_code ec;
    r.bytes_before = fs::file_size(c.update, ec), r.bytes_after = fs::file_size(c.output_file, ec);
    return true;
}

} // namespace

bool run_update(const Config& c, std::vector<Target>& targets, const Lap& counting)
{
    Stopwatch             watch;
    std::vector<uint32_t> hashed; // the targets with a hash, in input order
    for (uint32_t t = 0; t < targets.size(); ++t)
    {
        if (targets[t].hashes.empty())
            continue;
        if (!unite_files(c, targets[t]))
            return fail(gn_last_error());
        hashed.push_back(t);
    }
    if (hashed.empty() && !((c.remove_given || c.fold_given) && c.input_file.empty())) // (without inputs only where targets leave or move and none comes)
        return fail("No valid sequences to build");
    const double hash_s = counting.seconds() + watch.lap();
    try
    {
        UpdateReport r;
        r.update = c.update, r.output_file = c.output_file, r.kmer_size = c.kmer_size, r.window_size = c.window_size;
        r.removing = c.remove_given, r.extending = c.extend, r.folding = c.fold_given;
        Inputs in;
        if (!resolve_inputs(c, targets, hashed, in, r))
            return false;
        watch.lap();
        Loaded a;
        if (!load_index(c, a, r))
            return false;
        const double load_s = watch.lap();
        for (uint64_t i = 0; i < r.bins_a.size(); ++i)
            r.pop.push_back(count_bits(a.sink->filter(), i, r.bins_a[i]));
        double count_s = watch.lap();
        plan_removal(in, a.meta, r);
        double                           plan_s = watch.lap();
        std::vector<gnhibf::ExtendInput> ext;
        if (!probe_extensions(targets, in, a, r, ext))
            return false;
        count_s += watch.lap();
        if (!make_plans(c, a.meta, ext, r))
            return false;
        const gnhibf::Transfer transfer = gnhibf::plan_transfer(r.bins_a, r.removing ? &r.gone : nullptr, r.plan, r.folding ? &r.fold : nullptr);
        plan_s += watch.lap();

        std::vector<HibfShape> ibfs;
        gnhost::OwnedFilter    b;
        if (!create_b(c, a.meta, r, ibfs, b))
            return false;
        const double fold_s = execute_transfer(transfer, b.get(), a.sink->filter());
        a.sink.reset(); // (frees A)
        const double copy_s = watch.lap() - fold_s;
        insert_sets(targets, in, r, b.get());
        const double emplace_s = watch.lap();
        count_b(b.get(), r);
        count_s += watch.lap();
        if (!write_index(c, a.meta, ibfs, b, r))
            return false;
        const double write_s = watch.lap();

        print_update_report(std::cout, r);
        if (c.verbose && !c.quiet)
            std::cerr << std::setprecision(6) << " - seconds: hash " << hash_s << " load " << load_s << " count " << count_s << " plan " << plan_s << " copy " << copy_s
                      << (r.folding ? " fold " + std::to_string(fold_s) : std::string()) << " emplace " << emplace_s << " write " << write_s << std::endl;
        return true;
    }
    catch (const std::exception& e)
    {
        return fail(std::string("ERROR: ") + e.what());
    }
}

} // namespace gnbuild
