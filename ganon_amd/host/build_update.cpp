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
#include "build_common.hpp"
#include "hibf_fold.hpp"
#include "hibf_pool.hpp"
#include "hibf_remove.hpp"
#include "hibf_update.hpp"

#include <algorithm>
#include <cmath>
#include <fstream>
#include <iomanip>
#include <memory>
#include <numeric>
#include <set>
#include <sstream>

namespace gnbuild
{

bool run_update(const Config& c, std::vector<Target>& targets, const Lap& counting)
{
    auto t0 = std::chrono::steady_clock::now();
    std::vector<uint32_t> fresh_target; // the new targets with a hash, in input order: new user bin n_user_old + position
    std::vector<uint64_t> fresh_counts;
    std::vector<uint32_t> ext_target;   // --extend: the targets the index holds, in input order, and their user bins
    std::vector<uint64_t> ext_user;
    for (uint32_t t = 0; t < targets.size(); ++t)
    {
        if (targets[t].hashes.empty())
            continue;
        if (!unite_files(c, targets[t]))
            return fail(gn_last_error());
        fresh_target.push_back(t);
    }
    if (fresh_target.empty() && !((c.remove_given || c.fold_given) && c.input_file.empty())) // (without inputs only where targets leave or move and none comes)
        return fail("No valid sequences to build");
    const double hash_s = counting.seconds() + since(t0);
    std::vector<uint64_t>    remove_user;  // --remove: the user bins that leave, ascending, and the name each of them carries
    std::vector<std::string> remove_name;
    try
    {
        {
            gnhost::FilterMeta names;
            gnhost::read_hibf_meta(c.update, names);
            std::set<std::string> leaving;
            if (c.remove_given)
            {
                std::vector<std::string> listed;
                std::ifstream            in(c.remove);
                for (std::string line; std::getline(in, line);)
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
                remove_user = found.user_bins;
                for (const uint64_t u : remove_user)
                    for (size_t i = 0; i < names.targets.size() && i < names.target_bins.size(); ++i)
                        if (std::find(names.target_bins[i].begin(), names.target_bins[i].end(), u) != names.target_bins[i].end())
                        {
                            remove_name.push_back(names.targets[i]);
                            break;
                        }
            }
            const std::set<std::string> have(names.targets.begin(), names.targets.end());
            std::vector<uint32_t>       added;
            for (uint32_t t : fresh_target)
            {
                const std::string name = name_as_read(targets[t].name);
                if (!have.count(name) || leaving.count(name)) // (a name that leaves and comes is replaced: a new user bin)
                {
                    added.push_back(t);
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
                ext_target.push_back(t), ext_user.push_back(user);
            }
            fresh_target.swap(added);
            for (uint32_t t : fresh_target)
                fresh_counts.push_back(targets[t].hashes.size());
        }
        t0 = std::chrono::steady_clock::now();
        gnhost::FilterMeta meta;
        auto               sink = std::make_unique<gnhost::DeviceSink>(c.device);
        gnhost::load_filter_file(c.update, true, meta, *sink);
        const double load_s = since(t0);
        const uint64_t n_ibf = meta.shapes.size(), n_old = meta.n_user_bins;
        const uint8_t  h   = (uint8_t)meta.shapes.at(0).hash_funs;
        const double   fpr = meta.ibf_config.max_fp;
        if (meta.raw_bin_path.size() != n_old || meta.raw_user_bin_filenames.size() != n_old)
            return fail("--update: the index names " + std::to_string(meta.raw_bin_path.size()) + " file lists for " + std::to_string(n_old) + " user bins");
        std::vector<uint64_t> bins, rows;
        for (const gnhost::IbfShape& m : meta.shapes)
        {
            bins.push_back(m.bins), rows.push_back(m.bin_size);
            if (m.hash_funs != h)
                return fail("--update: the IBFs of the index differ in their hash functions");
        }

        t0 = std::chrono::steady_clock::now();
        std::vector<std::vector<uint64_t>> pop(n_ibf);
        for (uint64_t i = 0; i < n_ibf; ++i)
        {
            pop[i].assign(bins[i], 0);
            if (gn_filter_bin_popcounts(sink->filter(), (uint32_t)i, pop[i].data()) != GN_OK)
                throw std::runtime_error(gn_last_error());
        }
        const double count_s = since(t0);

        t0 = std::chrono::steady_clock::now();
        // --extend probes A, along the paths of the file's own tables
        gnhibf::Paths a_paths;
        if (!ext_target.empty())
            a_paths = gnhibf::derive_paths(bins, meta.next_ibf_id, meta.bin_to_user, n_old);
        // --remove: the tables the rest works on are those after the removal, with A's bit counts carried to the new places
        const bool                  removing = c.remove_given;
        const std::vector<uint64_t> bins_a   = bins; // per IBF of the file
        std::vector<std::vector<int64_t>> loaded_next_ibf_id, loaded_bin_to_user; // the file's tables (--remove: for the report)
        gnhibf::RemovePlan          gone;
        if (removing)
        {
            gone = gnhibf::plan_remove(bins, meta.next_ibf_id, meta.bin_to_user, n_old, remove_user, rows, h, &pop);
            std::vector<uint64_t> kept_rows;
            for (const uint32_t i : gone.old_ibf)
                kept_rows.push_back(rows[i]);
            rows.swap(kept_rows);
            bins = gone.bins, pop = gone.popcounts;
            loaded_next_ibf_id.swap(meta.next_ibf_id), loaded_bin_to_user.swap(meta.bin_to_user);
            meta.next_ibf_id = gone.next_ibf_id, meta.bin_to_user = gone.bin_to_user;
        }
        const uint64_t n_ibf_b = bins.size(), n_base = removing ? gone.n_user_bins : n_old; // what B starts from
        // --extend: what every extension set's path lacks (A's bits), the quotas of its run and the fills the new user bins start from
        gnhibf::Paths         old_paths;            // of the tables B starts from
        std::vector<uint64_t> ext_user_b = ext_user; // the extended user bins as B numbers them
        gnhibf::ExtendPlan    ex;
        double                probe_s = 0;
        if (!ext_target.empty())
        {
            const uint32_t                   d0 = a_paths.depth;
            std::vector<gnhibf::ExtendInput> in(ext_target.size());
            for (size_t j = 0; j < in.size(); ++j)
            {
                if (ext_user[j] >= n_old)
                    return fail("--update --extend: the index names user bin " + std::to_string(ext_user[j]) + " of " + std::to_string(n_old));
                in[j].user_bin = ext_user[j], in[j].hashes = targets[ext_target[j]].hashes.size();
                in[j].lost_at.assign(d0, 0);
            }
            gnhibf::for_each_pooled(
                in.size(), [&](size_t j) { return hash_set(targets[ext_target[j]]); }, [&](size_t j) { return &a_paths.entries[(size_t)ext_user[j] * d0]; }, d0,
                [&](const uint64_t* hashes, const uint64_t* off, size_t n, const gn_path_entry* p, const std::vector<size_t>& ids) {
                    std::vector<uint64_t> found(n), first(n), lost(n * d0);
                    if (gn_filter_probe_path(sink->filter(), hashes, off, (uint32_t)n, p, d0, found.data(), lost.data(), first.data()) != GN_OK)
                        throw std::runtime_error(gn_last_error());
                    for (size_t k = 0; k < n; ++k)
                        in[ids[k]].lost_at.assign(lost.begin() + k * d0, lost.begin() + (k + 1) * d0);
                });
            probe_s = since(t0);
            if (!removing)
                old_paths = a_paths;
            else
            {
                // a removal changes no bit of a surviving bin and no surviving path but for its numbers: what A lacks, B lacks.  The tree
                // may have lost levels; a surviving path is as long as it was, so what is cut off lost_at are unused entries
                old_paths = gnhibf::derive_paths(bins, meta.next_ibf_id, meta.bin_to_user, n_base);
                for (size_t j = 0; j < in.size(); ++j)
                {
                    in[j].user_bin = ext_user_b[j] = (uint64_t)gone.user_map[ext_user[j]];
                    in[j].lost_at.resize(old_paths.depth);
                }
            }
            ex = gnhibf::plan_extend(old_paths, bins, rows, h, fpr, pop, in);
            if (!ex.over.empty())
            {
                std::ostringstream m;
                m << "--update --extend: " << ex.over.size() << " bin(s) would be over their bound; nothing written:";
                for (const gnhibf::ExtendOver& o : ex.over)
                    m << "\n  target " << targets[ext_target[o.extension]].name << ": IBF " << o.ibf << " bin " << o.bin << " predicted " << std::fixed << std::setprecision(1)
                      << o.bits_predicted << " bits, bound " << o.bound;
                m << "\na run is never moved or widened: leave it out or rebuild";
                return fail(m.str());
            }
        }
        const gnhibf::UpdatePlan plan =
            gnhibf::plan_update(bins, rows, meta.next_ibf_id, meta.bin_to_user, n_base, h, fpr, pop, fresh_counts, ext_target.empty() ? nullptr : &ex.fills);
        // --fold: the rule runs last, on the tables the plans above leave and on a fill per bin: the bit count A shows (or the extension's
        // prediction), the prediction for a merged bin the new user bins touch, and for a bin of a new run what its share of hashes sets
        const bool        folding = c.fold_given;
        gnhibf::FoldPlan  fold;
        gnhibf::Paths     new_paths = plan.paths; // of the new user bins, along the tables written
        if (folding)
        {
            std::vector<std::vector<double>> fills(n_ibf_b);
            for (uint64_t i = 0; i < n_ibf_b; ++i)
            {
                if (!ext_target.empty())
                    fills[i] = ex.fills[i];
                else
                    fills[i].assign(pop[i].begin(), pop[i].begin() + bins[i]);
                fills[i].resize(plan.bins[i], 0.0);
            }
            for (const gnhibf::UpdateTouched& t : plan.touched)
                fills[t.ibf][t.bin] = t.bits_predicted;
            for (size_t j = 0; j < fresh_target.size(); ++j)
            {
                const gn_path_entry& run = plan.paths.entries[j * plan.paths.depth];
                for (uint32_t b = run.first_bin; b < run.first_bin + run.n_bins; ++b)
                    fills[run.ibf][b] = gnhibf::update_predict(0.0, run.hashes_per_bin, rows[run.ibf], h); // (ceil(count / bins of the run))
            }
            try
            {
                fold = gnhibf::plan_fold(plan.bins, rows, plan.next_ibf_id, plan.bin_to_user, plan.n_user_bins, h, fpr, fills, c.fold);
            }
            catch (const gnhibf::FoldUnreachable& e)
            {
                return fail(std::string("--fold: ") + e.what() + "; nothing written");
            }
            new_paths = gnhibf::fold_paths(plan.paths, fold);
            if (!ext_target.empty())
                old_paths = gnhibf::fold_paths(old_paths, fold);
        }
        const std::vector<uint64_t>&             final_bins = folding ? fold.bins : plan.bins;
        const std::vector<uint64_t>&             final_rows = folding ? fold.rows : rows;
        const std::vector<std::vector<int64_t>>& final_nx   = folding ? fold.next_ibf_id : plan.next_ibf_id;
        const std::vector<std::vector<int64_t>>& final_bu   = folding ? fold.bin_to_user : plan.bin_to_user;
        const uint64_t n_final = final_bins.size();
        const uint32_t depth   = folding ? fold.depth : plan.paths.depth;
        // where a bin of the tables the plans worked on is in the file written
        auto now = [&](uint32_t i, uint32_t b) { return folding ? std::pair<uint32_t, uint32_t>(fold.where[i][b].ibf, fold.where[i][b].bin) : std::pair<uint32_t, uint32_t>(i, b); };
        const double   plan_s = since(t0) - probe_s;

        // filter B: the same rows, the new bins.  A and B are on the device together until every IBF is moved
        t0 = std::chrono::steady_clock::now();
        std::vector<HibfShape> ibfs(n_final);
        uint64_t               a_bytes = 0, b_bytes = 0;
        for (uint64_t i = 0; i < n_ibf; ++i)
            a_bytes += meta.shapes[i].bin_size * gn_hibf_row_stride_words((bins_a[i] + 63) >> 6) * 8;
        for (uint64_t i = 0; i < n_final; ++i)
        {
            ibfs[i].bins = final_bins[i], ibfs[i].rows = final_rows[i];
            ibfs[i].next_ibf_id = final_nx[i], ibfs[i].bin_to_user = final_bu[i];
            b_bytes += final_rows[i] * gn_hibf_row_stride_words((final_bins[i] + 63) >> 6) * 8;
        }
        {
            uint64_t free_b = 0, total_b = 0;
            if (gn_device_memory(c.device, &free_b, &total_b) != GN_OK)
                throw std::runtime_error(gn_last_error());
            // (free_b is what is left beside A.  The 256 MiB on top of B are for what is still to come on this device: the staging buffer
            // of the inserts (32 M hashes, 256 MiB at most, usually far less), their item and path tables, the bit counts, and whatever
            // the hasher streams of the counting phase have not yet given back)
            if (b_bytes + (256ull << 20) > free_b)
                return fail("--update: the index (" + std::to_string(a_bytes) + " bytes on the device) and the updated one (" + std::to_string(b_bytes) +
                            " bytes) do not fit device " + std::to_string(c.device) + " together (" + std::to_string(free_b) + " bytes free beside the index)");
        }
        gnhost::HibfDescs descs;
        for (const HibfShape& s : ibfs)
            descs.add(s.bins, s.rows, h, s.next_ibf_id, s.bin_to_user);
        gnhost::OwnedFilter b_flt = descs.upload(c.device, plan.n_user_bins);
        if (!b_flt)
            throw std::runtime_error(gn_last_error());
        double fold_s = 0;
        if (!folding)
        {
            for (uint64_t i = 0; i < n_ibf_b; ++i)
                if ((removing ? gn_filter_copy_ibf_spans(b_flt.get(), (uint32_t)i, sink->filter(), gone.old_ibf[i], gone.spans[i].data(), (uint32_t)gone.spans[i].size())
                              : gn_filter_copy_ibf(b_flt.get(), (uint32_t)i, sink->filter(), (uint32_t)i)) != GN_OK)
                    throw std::runtime_error(gn_last_error());
        }
        else
        {
            // the bin of A that holds the column of bin b of IBF i of the tables the fold worked on, or -1: a bin this command adds
            std::vector<std::vector<int64_t>> a_bin(n_ibf_b);
            for (uint64_t i = 0; i < n_ibf_b; ++i)
            {
                a_bin[i].assign(plan.bins[i], -1);
                if (!removing)
                    std::iota(a_bin[i].begin(), a_bin[i].begin() + bins[i], int64_t(0));
                else
                    for (const gn_bin_span& s : gone.spans[i])
                        std::iota(a_bin[i].begin() + s.dst_first, a_bin[i].begin() + s.dst_first + s.n_bins, (int64_t)s.src_first);
            }
            auto a_ibf = [&](uint32_t i) { return removing ? gone.old_ibf[i] : i; };
            // every surviving IBF and every child: its columns out of A, one span per maximal run that is one in A too
            for (uint64_t f = 0; f < n_final; ++f)
            {
                const uint32_t           si = fold.src_ibf[f];
                std::vector<gn_bin_span> spans;
                for (const gn_bin_span& s : fold.spans[f])
                    for (uint32_t j = 0; j < s.n_bins; ++j)
                    {
                        const int64_t from = a_bin[si][s.src_first + j];
                        if (from < 0)
                            continue;
                        if (!spans.empty() && spans.back().src_first + spans.back().n_bins == (uint64_t)from && spans.back().dst_first + spans.back().n_bins == s.dst_first + j)
                            ++spans.back().n_bins;
                        else
                            spans.push_back(gn_bin_span{ (uint32_t)from, s.dst_first + j, 1, 0 });
                    }
                if (gn_filter_copy_ibf_spans(b_flt.get(), (uint32_t)f, sink->filter(), a_ibf(si), spans.data(), (uint32_t)spans.size()) != GN_OK)
                    throw std::runtime_error(gn_last_error());
            }
            // the new merged bins: per folded parent the OR of every group's columns of A.  A group of new user bins alone has no column
            // there yet (the inserts below fill its merged bin); the groups on either side of it go in calls of their own
            const auto t_fold = std::chrono::steady_clock::now();
            for (size_t g0 = 0; g0 < fold.groups.size();)
            {
                const uint32_t              parent = fold.groups[g0].parent;
                std::vector<gn_fold_member> members;
                size_t                      g = g0;
                for (; g < fold.groups.size() && fold.groups[g].parent == parent; ++g)
                {
                    const size_t had = members.size();
                    for (size_t k = 0; k < fold.groups[g].run_first.size(); ++k)
                        for (uint32_t b = fold.groups[g].run_first[k]; b < fold.groups[g].run_first[k] + fold.groups[g].run_bins[k]; ++b)
                            if (a_bin[parent][b] >= 0)
                                members.push_back(gn_fold_member{ (uint32_t)a_bin[parent][b], 1, (uint32_t)(g - g0), 0 });
                    if (members.size() == had)
                        break;
                }
                if (!members.empty())
                {
                    std::sort(members.begin(), members.end(), [](const gn_fold_member& x, const gn_fold_member& y) { return x.src_first < y.src_first; });
                    std::vector<gn_fold_member> joined; // neighbouring bins of one group are one member
                    for (const gn_fold_member& m : members)
                        if (!joined.empty() && joined.back().group == m.group && joined.back().src_first + joined.back().n_bins == m.src_first)
                            ++joined.back().n_bins;
                        else
                            joined.push_back(m);
                    if (gn_filter_fold_ibf(b_flt.get(), parent, fold.groups[g0].merged_bin, (uint32_t)(g - g0), sink->filter(), a_ibf(parent), joined.data(),
                                           (uint32_t)joined.size()) != GN_OK)
                        throw std::runtime_error(gn_last_error());
                }
                g0 = g > g0 ? g : g0 + 1; // (g == g0: the group at g0 has no column in A)
            }
            fold_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_fold).count();
        }
        sink.reset(); // (frees A)
        const double copy_s = since(t0) - fold_s;

        // the new sets along their paths, pooled as run_hibf pools them; before them the extensions, by their quotas
        // (the pooler may cut the extensions into several calls.  A later call takes presence against B after the earlier ORs, not against A,
        // where lost_at was counted; the counts still agree, because presence is a matter of the run's own columns and only the run's own set
        // writes them -- one extension per user bin, and the new targets are inserted afterwards)
        t0 = std::chrono::steady_clock::now();
        gnhibf::for_each_pooled(
            ext_target.size(), [&](size_t j) { return hash_set(targets[ext_target[j]]); }, [&](size_t j) { return &old_paths.entries[(size_t)ext_user_b[j] * depth]; }, depth,
            [&](const uint64_t* hashes, const uint64_t* off, size_t n, const gn_path_entry* p, const std::vector<size_t>& ids) {
                std::vector<uint64_t> deal_off{ 0 }, deal;
                for (size_t k = 0; k < n; ++k)
                {
                    deal.insert(deal.end(), ex.quotas[ids[k]].begin(), ex.quotas[ids[k]].end());
                    deal_off.push_back(deal.size());
                }
                if (gn_filter_extend_path(b_flt.get(), hashes, off, (uint32_t)n, p, depth, deal_off.data(), deal.data()) != GN_OK)
                    throw std::runtime_error(gn_last_error());
            });
        gnhibf::for_each_pooled(
            fresh_target.size(),
            [&](size_t j) { return hash_set(targets[fresh_target[j]]); },
            [&](size_t j) { return &new_paths.entries[j * depth]; }, depth,
            [&](const uint64_t* hashes, const uint64_t* off, size_t n, const gn_path_entry* p, const std::vector<size_t>&) {
                if (gn_filter_emplace_path(b_flt.get(), hashes, off, (uint32_t)n, p, depth) != GN_OK)
                    throw std::runtime_error(gn_last_error());
            });
        const double emplace_s = since(t0);

        // B's bit counts, for the IBFs the report speaks of: those that gained bins or lie on a new path
        t0 = std::chrono::steady_clock::now();
        std::vector<bool> shown(n_final, false);
        for (uint64_t i = 0; i < n_ibf_b; ++i)
            shown[i] = final_bins[i] != bins[i] || (removing && bins[i] != bins_a[gone.old_ibf[i]]);
        for (uint64_t i = n_ibf_b; i < n_final; ++i) // (--fold: the IBFs it creates)
            shown[i] = true;
        for (const uint32_t i : fold.folded)
            shown[i] = true;
        for (const gnhibf::RemoveStale& st : gone.stale)
            shown[st.ibf] = true;
        for (const gn_path_entry& e : new_paths.entries)
            if (e.n_bins)
                shown[e.ibf] = true;
        for (const uint64_t u : ext_user_b)
            for (uint32_t d = 0; d < depth && old_paths.entries[(size_t)u * depth + d].n_bins; ++d)
                shown[old_paths.entries[(size_t)u * depth + d].ibf] = true;
        std::vector<std::vector<uint64_t>> pop_b(n_final);
        for (uint64_t i = 0; i < n_final; ++i)
            if (shown[i])
            {
                pop_b[i].assign(final_bins[i], 0);
                if (gn_filter_bin_popcounts(b_flt.get(), (uint32_t)i, pop_b[i].data()) != GN_OK)
                    throw std::runtime_error(gn_last_error());
            }
        const double count_b_s = since(t0);

        // the file: its header fields and strings as they are, the new names behind them in the form run_hibf writes
        t0 = std::chrono::steady_clock::now();
        std::vector<std::vector<std::string>> bin_path   = meta.raw_bin_path;
        std::vector<std::string>              user_files = meta.raw_user_bin_filenames;
        if (removing) // the removed user bins' entries go; the others stay verbatim and in order
        {
            size_t kept = 0;
            for (uint64_t u = 0; u < n_old; ++u)
                if (gone.user_map[u] >= 0)
                {
                    if (kept != u) // (a self-move would empty the entry)
                        bin_path[kept] = std::move(bin_path[u]), user_files[kept] = std::move(user_files[u]);
                    ++kept;
                }
            bin_path.resize(kept), user_files.resize(kept);
        }
        const std::string dir = output_folder(c);
        for (uint32_t t : fresh_target)
        {
            const std::string f = dir + "/" + user_bin_file_name(targets[t].name) + ".minimiser";
            bin_path.push_back({ f });
            user_files.push_back(f);
        }
        std::string err;
        const bool  saved = save_hibf(c, b_flt.get(), ibfs, h, bin_path, user_files, err); // (c holds the file's k, w and fpr: validate())
        b_flt.reset();
        if (!saved)
            return fail(err);
        const double write_s = since(t0);

        // the report
        const double bound_fill = std::pow(fpr, 1.0 / h);
        std::cout << "index\t" << c.update << "\t->\t" << c.output_file << "\tk=" << unsigned(c.kmer_size) << " w=" << c.window_size << " h=" << unsigned(h)
                  << " ibfs=" << n_ibf;
        if (removing || folding)
            std::cout << "->" << n_final;
        std::cout << " levels=" << depth << " user_bins=" << n_old << "->" << plan.n_user_bins << " fpr=" << fpr << "\n";
        std::cout << "#target\tuser_bin\tdistinct_hashes\tleaf_ibf\tfirst_bin\tbins\tdepth\tpath\n";
        uint64_t bins_added = 0;
        for (size_t j = 0; j < fresh_target.size(); ++j)
        {
            const gn_path_entry* p    = &new_paths.entries[j * depth];
            uint32_t             used = 0;
            while (used < depth && p[used].n_bins)
                ++used;
            std::cout << "target\t" << targets[fresh_target[j]].name << "\t" << n_base + j << "\t" << fresh_counts[j] << "\t" << p[0].ibf << "\t" << p[0].first_bin << "\t"
                      << p[0].n_bins << "\t" << used << "\t";
            for (uint32_t d = used; d-- > 0;)
                std::cout << p[d].ibf << ":" << p[d].first_bin << (d ? " " : "");
            std::cout << "\n";
            bins_added += p[0].n_bins;
        }
        if (removing)
        {
            // (old numbers: what left is named as the index given knows it; `stale` speaks of the file written)
            auto estimate = [](uint64_t hashes, bool full) { return full ? std::string("full") : std::to_string(hashes); };
            const gnhibf::Paths was = gnhibf::derive_paths(bins_a, loaded_next_ibf_id, loaded_bin_to_user, n_old);
            std::cout << "#removed\ttarget\tuser_bin\tleaf_ibf\tfirst_bin\tbins\tbits\testimated_hashes\tpath\n";
            for (size_t j = 0; j < gone.removed.size(); ++j)
            {
                const gnhibf::RemovedRun& r = gone.removed[j];
                const gn_path_entry*      p = &was.entries[(size_t)r.user_bin * was.depth];
                uint32_t                  used = 0;
                while (used < was.depth && p[used].n_bins)
                    ++used;
                std::cout << "removed\t" << (j < remove_name.size() ? remove_name[j] : std::string("?")) << "\t" << r.user_bin << "\t" << r.ibf << "\t" << r.first_bin << "\t" << r.n_bins
                          << "\t" << r.bits << "\t" << estimate(r.hashes, r.full) << "\t";
                for (uint32_t d = used; d-- > 0;)
                    std::cout << p[d].ibf << ":" << p[d].first_bin << (d ? " " : "");
                std::cout << "\n";
            }
            std::cout << "#dropped\tibf\tparent_ibf\tparent_bin\n";
            for (const gnhibf::RemoveDropped& d : gone.dropped)
                std::cout << "dropped\t" << d.ibf << "\t" << d.parent_ibf << "\t" << d.parent_bin << "\n";
            std::cout << "#stale\tibf\tbin\tbits\testimated_stale_hashes\n";
            for (const gnhibf::RemoveStale& st : gone.stale)
            {
                const auto [i, b] = now(st.ibf, st.bin);
                std::cout << "stale\t" << i << "\t" << b << "\t" << pop_b[i][b] << "\t" << estimate(st.hashes, st.full) << "\n";
            }
        }
        if (c.extend)
        {
            std::cout << "#extended\ttarget\tuser_bin\thashes\talready_present\tinserted\tleaf_ibf\tfirst_bin\tbins\tpath\n";
            for (size_t j = 0; j < ext_target.size(); ++j)
            {
                const gn_path_entry* p        = &old_paths.entries[(size_t)ext_user_b[j] * depth];
                const uint64_t       n        = targets[ext_target[j]].hashes.size();
                const uint64_t       inserted = std::accumulate(ex.quotas[j].begin(), ex.quotas[j].end(), uint64_t(0));
                uint32_t             used     = 0;
                while (used < depth && p[used].n_bins)
                    ++used;
                std::cout << "extended\t" << targets[ext_target[j]].name << "\t" << ext_user_b[j] << "\t" << n << "\t" << n - inserted << "\t" << inserted << "\t" << p[0].ibf
                          << "\t" << p[0].first_bin << "\t" << p[0].n_bins << "\t";
                for (uint32_t d = used; d-- > 0;)
                    std::cout << p[d].ibf << ":" << p[d].first_bin << (d ? " " : "");
                std::cout << "\n";
            }
            std::cout << "#run\tibf\tbin\tdealt\tbits_before\tbits_predicted\tbits_after\n";
            for (const gnhibf::ExtendRunBin& r : ex.run)
            {
                const auto [i, b] = now(r.ibf, r.bin);
                std::cout << "run\t" << i << "\t" << b << "\t" << r.dealt << "\t" << r.bits_before << "\t" << std::fixed << std::setprecision(1) << r.bits_predicted << "\t"
                          << pop_b[i][b] << "\n";
            }
        }
        std::cout << "#ibf\trows\tbins_before\tbins_after\tmax_fill_before\tmax_fill_after\n" << std::fixed << std::setprecision(6);
        for (uint64_t i = 0; i < n_ibf_b; ++i)
            if (shown[i])
                std::cout << "ibf\t" << i << "\t" << rows[i] << "\t" << (removing ? bins_a[gone.old_ibf[i]] : bins[i]) << "\t" << final_bins[i] << "\t"
                          << *std::max_element(pop[i].begin(), pop[i].end()) / (double)rows[i] << "\t"
                          << *std::max_element(pop_b[i].begin(), pop_b[i].end()) / (double)rows[i] << "\n";
        for (uint64_t i = n_ibf_b; i < n_final; ++i) // (--fold: an IBF it creates had no bin before)
            std::cout << "ibf\t" << i << "\t" << final_rows[i] << "\t0\t" << final_bins[i] << "\t" << 0.0 << "\t"
                      << *std::max_element(pop_b[i].begin(), pop_b[i].end()) / (double)final_rows[i] << "\n";
        std::cout << "#merged\tibf\tbin\tbits_before\tbits_predicted\tbits_after\n";
        uint64_t fullest = 0, fullest_rows = 1;
        bool     any_touched = false;
        std::vector<gnhibf::UpdateTouched> touched = ex.touched; // the extensions' merged bins, then the new user bins'; a bin of both once,
        for (const gnhibf::UpdateTouched& t : plan.touched)      // with the later prediction (which starts from the earlier)
        {
            auto at = std::find_if(touched.begin(), touched.end(), [&](const gnhibf::UpdateTouched& x) { return x.ibf == t.ibf && x.bin == t.bin; });
            if (at == touched.end())
                touched.push_back(t);
            else
                at->bits_predicted = t.bits_predicted;
        }
        for (const gnhibf::UpdateTouched& t : touched)
        {
            const auto [ti, tb]  = now(t.ibf, t.bin); // (a merged bin stays in its IBF; a fold may move it to the left)
            const uint64_t after = pop_b[ti][tb];
            std::cout << "merged\t" << ti << "\t" << tb << "\t" << t.bits_before << "\t" << std::setprecision(1) << t.bits_predicted << std::setprecision(6) << "\t"
                      << after << (after > bound_fill * rows[t.ibf] ? "\tWARN fill" : "") << "\n";
            if (!any_touched || after * (double)fullest_rows > fullest * (double)rows[t.ibf])
                fullest = after, fullest_rows = rows[t.ibf];
            any_touched = true;
        }
        if (folding)
        {
            // (a merged bin that holds new user bins was predicted with their fills; one an extension passes through may end above it)
            std::cout << "#folded\tparent_ibf\tmerged_bin\tnew_ibf\truns\tbins\tbits_predicted\tbits_found\n";
            for (const gnhibf::FoldGroup& g : fold.groups)
            {
                const uint64_t found = pop_b[g.parent][g.merged_bin];
                std::cout << "folded\t" << g.parent << "\t" << g.merged_bin << "\t" << g.new_ibf << "\t" << g.runs << "\t" << g.bins << "\t" << std::setprecision(1) << g.bits_predicted
                          << std::setprecision(6) << "\t" << found << (found > bound_fill * final_rows[g.parent] ? "\tWARN fill" : "") << "\n";
            }
        }
        std::error_code ec;
        std::cout << "result\tok\t";
        if (removing)
            std::cout << gone.removed.size() << " user bin(s) removed, " << gone.dropped.size() << " IBF(s) dropped, ";
        if (folding)
            std::cout << fold.groups.size() << " IBF(s) created under " << fold.folded.size() << " folded, ";
        if (c.extend)
            std::cout << ext_target.size() << " user bin(s) extended, ";
        std::cout << fresh_target.size() << " user bin(s) added, " << bins_added << " bin(s) added, " << fs::file_size(c.update, ec) << " -> "
                  << fs::file_size(c.output_file, ec) << " bytes, fullest touched merged bin ";
        if (!any_touched)
            std::cout << "n/a";
        else if (fullest >= fullest_rows)
            std::cout << "full";
        else
            std::cout << std::setprecision(0) << -((double)fullest_rows / h) * std::log(1.0 - (double)fullest / fullest_rows) << " estimated hashes at fill " << std::setprecision(6)
                      << (double)fullest / fullest_rows;
        std::cout << std::endl;
        if (c.verbose && !c.quiet)
            std::cerr << std::setprecision(6) << " - seconds: hash " << hash_s << " load " << load_s << " count " << count_s + count_b_s + probe_s << " plan " << plan_s << " copy " << copy_s
                      << (folding ? " fold " + std::to_string(fold_s) : std::string()) << " emplace " << emplace_s << " write " << write_s << std::endl;
        return true;
    }
    catch (const std::exception& e)
    {
        return fail(std::string("ERROR: ") + e.what());
    }
}

} // namespace gnbuild
