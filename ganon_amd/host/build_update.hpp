// build_update.hpp -- what build_update.cpp (the run) and build_update_report.cpp (its report on stdout) share: the facts of one
// `ganon-build --hibf --update`, which the steps of the run fill in as they go and the report prints.
#pragma once

#include "hibf_fold.hpp"
#include "hibf_remove.hpp"
#include "hibf_update.hpp"

#include <ostream>
#include <string>
#include <utility>

namespace gnbuild
{

// the tables of the file written: the fold's where there is one, else the placement's.  Built once, after the plans
struct FinalTables
{
    std::vector<uint64_t>                       bins, rows; // per IBF
    std::vector<std::vector<int64_t>>           next_ibf_id, bin_to_user;
    uint32_t                                    depth = 0;
    std::vector<std::vector<gnhibf::FoldWhere>> where; // --fold: per IBF and bin of the tables the plans worked on
    // where a bin of the tables the plans worked on is in the file written
    std::pair<uint32_t, uint32_t> now(uint32_t i, uint32_t b) const
    {
        return where.empty() ? std::pair<uint32_t, uint32_t>(i, b) : std::pair<uint32_t, uint32_t>(where[i][b].ibf, where[i][b].bin);
    }
};

struct UpdateReport // plain data: no device, no file
{
    // the command
    std::string update, output_file;
    unsigned    kmer_size = 0, window_size = 0;
    bool        removing = false, extending = false, folding = false; // --remove, --extend, --fold given
    // the file given (A)
    unsigned                          h = 0;
    double                            fpr = 0;
    uint64_t                          n_old = 0, bytes_before = 0;
    std::vector<uint64_t>             bins_a;     // per IBF
    std::vector<std::vector<int64_t>> nx_a, bu_a; // its tables (--remove only: what left is named as the file knows it)
    // the tables B starts from: the file's, or those after the removal, with A's bit counts carried to the new places
    std::vector<uint64_t>              bins, rows;
    std::vector<std::vector<uint64_t>> pop;
    uint64_t                           n_base = 0;
    // the plans, the paths along the tables written (of the new user bins; of the old ones, where a target is extended), the result
    gnhibf::RemovePlan gone;
    gnhibf::ExtendPlan ex;
    gnhibf::UpdatePlan plan;
    gnhibf::FoldPlan   fold;
    gnhibf::Paths      new_paths, old_paths;
    FinalTables        final;
    // the file written (B): its bit counts, for the IBFs the report speaks of
    std::vector<bool>                  shown;
    std::vector<std::vector<uint64_t>> pop_b;
    uint64_t                           bytes_after = 0;
    // the targets: new user bin n_base + j; extended user bin ext_user_b[j] of B; removed[j] of the plan
    std::vector<std::string> fresh_name, ext_name, remove_name;
    std::vector<uint64_t>    fresh_counts, ext_counts, ext_user_b;
};

void print_update_report(std::ostream& os, const UpdateReport& r); // build_update_report.cpp

} // namespace gnbuild
