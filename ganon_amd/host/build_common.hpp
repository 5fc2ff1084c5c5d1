// build_common.hpp -- what the modes of `ganon-build` share: build.cpp (arguments, hashing, the flat .ibf), build_hibf.cpp (--hibf),
// build_verify.cpp (--hibf --verify-index), build_update.cpp (--hibf --update; its report is build_update_report.cpp, what the two share
// build_update.hpp), build_slabs.cpp and build_hibf_parts.cpp (a filter larger than a device, flat in row slabs and hierarchical in
// parts) and build_write.cpp (the two file writers).
#pragma once

#include "build_params.hpp"
#include "device_sink.hpp"
#include "hibf_build_parts.hpp"
#include "hibf_paths.hpp"
#include "set_arena.hpp"

#include "../csrc/gn_packed_set.h"

#include "ganon_hip.h"

#include <chrono>
#include <cstdint>
#include <ctime>
#include <filesystem>
#include <iostream>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

namespace gnbuild
{

namespace fs = std::filesystem;

constexpr int kVersionTuple[3] = { 2, 1, 1 };

struct Config // Config.hpp:10-27
{
    std::string input_file, output_file, tmp_output_folder, mode = "avg";
    double      max_fp = 0.05, filter_size = 0;
    uint8_t     kmer_size = 19;
    uint16_t    window_size = 31;
    uint8_t     hash_functions = 0; // (parsed into an int first: 0..255)
    uint64_t    min_length = 0;
    uint16_t    threads = 1;
    bool        verbose = false, quiet = false;
    int         device = 0; // (not in the reference: which GPU; the first entry of `devices`)
    std::vector<int> devices = { 0 }; // (--device a,b,...: the flat build deals row slabs to the entries; an entry may repeat)
    uint64_t    device_memory = 0;    // (--device-memory: most bytes of filter rows on a list entry at one time; 0 = from what is free)
    bool        device_memory_given = false;
    std::string hash_sets = "raw";    // (--hash-sets: how the flat build keeps the hash sets between hashing and filling -- raw: 8 bytes a hash in
                                      //  memory; packed: csrc/gn_packed_set.h in memory; spilled: the same in files of output_folder())
    std::string hibf_hash_sets = "raw"; // (--hibf-hash-sets: the same three ways for the hash sets of a --hibf build -- its unions, sketches and
                                        //  insert have packed twins; --update and --verify-index read raw sets)
    bool        hibf_hash_sets_given = false;
    std::string parse = "host";       // (--parse: who finds the records of the input genomes -- host: the sequential reader; device: FASTA files travel
                                      //  as text and are tokenised there, hasher.hpp hash_text_file, with the host reader as the fallback)
    bool        hibf = false;   // (not in the reference: write a raptor 3.0.1 HIBF index instead of a flat .ibf)
    uint64_t    hibf_memory = 0; // (--hibf-memory: most device bytes of IBF rows on an entry of hibf_devices at one time; 0 = from what is free)
    bool        hibf_memory_given = false, hibf_devices_given = false;
    std::vector<int> hibf_devices; // (--hibf-devices a,b,...: the entries the parts of a tree are dealt to; empty = the single --device)
    uint64_t    tmax = 0;       // (--hibf only: most technical bins of an IBF; 0 = ceil(sqrt(user bins) / 64) * 64)
    bool        tmax_given = false, filter_size_given = false;
    std::string layout = "rule"; // (--hibf only: rule = hibf_layout.hpp, sketch = hibf_layout_sketch.hpp on HyperLogLog union estimates,
                                 //  similarity = hibf_layout_similarity.hpp: sketch over an order that groups related targets)
    bool        layout_given = false;
    std::string verify_index;    // (--hibf only: check this index against the inputs instead of building one)
    uint64_t    verify_memory = 0; // (--verify-memory: most device bytes of IBF rows on an entry of verify_devices at one time; 0 = from what is free)
    bool        verify_memory_given = false, verify_devices_given = false;
    std::vector<int> verify_devices; // (--verify-devices a,b,...: the entries the parts of an index are dealt to; empty = the single --device)
    std::string update;          // (--hibf only: add the inputs' targets to this index and write the result to --output-file)
    bool        update_given = false, max_fp_given = false, mode_given = false;
    bool        extend = false;  // (--update only: a target the index holds gains the inputs' sequences)
    std::string remove;          // (--update only: a file of target names, one per line, that leave the index)
    bool        remove_given = false;
    uint64_t    fold = 0;        // (--update only: hold every IBF of the updated index to this many bins by folding runs of user bins)
    bool        fold_given = false;
    bool        verify_given = false, kmer_given = false, window_given = false, hashes_given = false, output_given = false;
};

struct Target
{
    std::string              name;
    std::vector<std::string> files;
    std::vector<uint64_t>    hashes; // per file: its distinct hashes, ascending; files behind each other (:236-238)
    std::vector<uint64_t>    file_ends; // where each file's hashes end in `hashes` (--hibf unites the files of a target)
    // --hash-sets / --hibf-hash-sets packed|spilled: `hashes` stays empty; the target keeps its count and the blocks of its files' packed sets behind each
    // other, whose word_at count from the start of arena `arena` (the one of the thread that hashed the target; --hibf moves a target of
    // several files to the arena of the unions, build_hibf.cpp)
    uint64_t                   count = 0;
    std::vector<GnPackedBlock> blocks;
    uint32_t                   arena = 0;
};

// how many hashes a target has, however its sets are kept
inline uint64_t n_hashes(const Target& t)
{
    return t.blocks.empty() ? t.hashes.size() : t.count;
}

// a target's hashes as the pooler (hibf_pool.hpp) asks for a set
inline std::pair<const uint64_t*, uint64_t> hash_set(const Target& t)
{
    return { t.hashes.data(), t.hashes.size() };
}

struct Totals // :52-59
{
    uint64_t files = 0, invalid_files = 0, sequences = 0, skipped_sequences = 0, length_bp = 0;
};

struct HibfShape // IBF i of the tree as it is created and written
{
    uint64_t             bins = 0, rows = 0;
    std::vector<int64_t> next_ibf_id, bin_to_user;
};

inline std::string stamp(std::chrono::system_clock::time_point t)
{
    const std::time_t tt = std::chrono::system_clock::to_time_t(t);
    char              b[64];
    std::strftime(b, sizeof(b), "%Y-%m-%d %H:%M:%S", std::localtime(&tt));
    return b;
}

struct Lap
{
    std::chrono::system_clock::time_point b, e;
    void   start() { b = std::chrono::system_clock::now(); }
    void   stop() { e = std::chrono::system_clock::now(); }
    double seconds() const { return std::chrono::duration<double>(e - b).count(); }
};

inline double since(std::chrono::steady_clock::time_point t)
{
    return std::chrono::duration<double>(std::chrono::steady_clock::now() - t).count();
}

inline bool fail(const std::string& m)
{
    std::cerr << m << std::endl;
    return false;
}

// where the user bins' files are said to lie: --tmp-output-folder, else the folder of --output-file
inline std::string output_folder(const Config& c)
{
    return !c.tmp_output_folder.empty()                  ? c.tmp_output_folder
           : fs::path(c.output_file).has_parent_path() ? fs::path(c.output_file).parent_path().string()
                                                       : std::string(".");
}

// the name of a target's user bin as an index file gives it back: written as <folder>/<name, "---" for a space>.minimiser by this
// builder (and by `ganon build`, build_update.py:411-518), read as filter_io.cpp:parse_hibf reads it (GanonClassify.cpp:908-935)
inline std::string user_bin_file_name(const std::string& target)
{
    std::string name = target;
    for (size_t p = 0; (p = name.find(' ', p)) != std::string::npos; p += 3)
        name.replace(p, 1, "---");
    return name;
}

// the loader's own reading of the name this builder would write for a target (filter_io.cpp:parse_hibf)
inline std::string name_as_read(const std::string& target)
{
    std::string f     = fs::path(user_bin_file_name(target) + ".minimiser").filename().string();
    size_t      found = f.find(".minimiser");
    if (found != std::string::npos)
        f = f.substr(0, found);
    for (const auto& [from, to] : { std::pair<std::string, std::string>{ "|||", "." }, { "---", " " } })
        for (size_t p = 0; (p = f.find(from, p)) != std::string::npos; p += to.size())
            f.replace(p, from.size(), to);
    return f;
}

// a target's set = the union of its files' sets, ascending
inline bool unite_files(const Config& c, Target& tg)
{
    if (tg.file_ends.size() <= 1)
        return true;
    std::vector<const uint64_t*> sets;
    std::vector<uint64_t>        sizes;
    uint64_t                     a = 0;
    for (uint64_t e : tg.file_ends)
    {
        sets.push_back(tg.hashes.data() + a);
        sizes.push_back(e - a);
        a = e;
    }
    std::vector<uint64_t> all(tg.hashes.size());
    uint64_t              n = 0;
    if (gn_hashes_union(c.device, sets.data(), sizes.data(), (uint32_t)sets.size(), all.data(), all.size(), &n) != GN_OK)
        return false;
    all.resize(n);
    tg.hashes.swap(all);
    tg.file_ends.assign(1, n);
    return true;
}

// the end of a build: with --verbose the five laps (print_stats_verbose, :730-757; `second` and its label are the mode's: sizing
// or layout), then what was processed and what was skipped (print_stats, :706-728).  The lines that follow are the mode's.
inline void print_stats(const Config& c, const Totals& totals, const Lap& counting, const char* second_label, const Lap& second, const Lap& filling,
                        const Lap& writing, const Lap& whole)
{
    if (c.verbose)
    {
        auto block = [](const char* a, const Lap& l) {
            const char* pad = "                ";
            std::cerr << a << stamp(l.b) << '\n' << pad << "    end: " << stamp(l.e) << '\n' << pad << "elapsed (s): " << l.seconds() << '\n';
        };
        block("Count/save hashes start: ", counting);
        block(second_label, second);
        block("Building filter   start: ", filling);
        block("Saving filer      start: ", writing);
        block("ganon-build       start: ", whole);
        std::cerr << std::endl;
    }
    const double elapsed = whole.seconds();
    std::cerr << "ganon-build processed " << totals.sequences << " sequences / " << totals.files << " files ("
              << totals.length_bp / 1000000.0 << " Mbp) in " << elapsed << " seconds ("
              << (totals.length_bp / 1000000.0) / (elapsed / 60.0) << " Mbp/m)" << std::endl;
    if (totals.invalid_files > 0)
        std::cerr << " - " << totals.invalid_files << " invalid files skipped" << std::endl;
    if (totals.skipped_sequences > 0)
        std::cerr << " - " << totals.skipped_sequences << " sequences skipped" << std::endl;
}

// build_write.cpp: header from the host, the bit matrices streamed out of HBM
bool save_filter(const Config& c, gn_filter* flt, const IbfParams& p, const std::vector<Target>& targets, const std::vector<BinSpan>& bins,
                 std::string& err);
bool save_hibf(const Config& c, gn_filter* flt, const std::vector<HibfShape>& ibfs, uint8_t hash_functions,
               const std::vector<std::vector<std::string>>& bin_path, const std::vector<std::string>& user_files, std::string& err);
// the flat .ibf in pieces, for a build in row slabs: the header and a file of full size, whose descriptor (>= 0; the caller closes it) and
// payload offset come back; then rows [0, n_rows) of a slab filter to byte `at` of the file
int  open_filter(const Config& c, const IbfParams& p, const std::vector<Target>& targets, const std::vector<BinSpan>& bins, uint64_t& payload_at,
                 std::string& err);
bool save_slab(int fd, gn_filter* flt, uint64_t n_rows, uint64_t row_bytes, uint64_t at, gnhost::PinnedBlock& stage, std::string& err);

// build_slabs.cpp: the bit matrix of a flat filter, filled slab by slab over c.devices and written as it goes
struct FlatFill
{
    const Config&               c;
    const IbfParams&            p;
    const std::vector<Target>&  targets;
    const std::vector<BinSpan>& bins;
    const std::vector<uint64_t>& shares; // hashes per bin of each target (lay_out_bins)
    const std::vector<const uint64_t*>* arenas = nullptr; // --hash-sets packed|spilled: the arenas' words (Target::arena); null: raw sets
};
bool fill_and_save_flat(const FlatFill& w, Lap& filling, Lap& writing);
// (build_slabs.cpp) most bytes of rows on a list entry at one time when the user names none: the smallest share of free memory over the
// entries -- what gn_device_memory reports free now, less the staging of the fills that run there and a reserve, divided by how often
// the device is named.  The rule of the flat build in row slabs and of the hierarchical build in parts.
bool budget_from_free_memory(const std::vector<int>& devices, uint64_t& budget, std::string& err);

// The raptor index in pieces, for a build in parts (build_write.cpp): everything but the payloads -- the header, every IBF's own header
// at its offset, the tables behind the last payload -- and a file of full size, whose descriptor (>= 0; the caller closes it) and
// payload offsets (one per IBF) come back; then rows [0, n_rows) of IBF `ibf` of a part's filter to byte `at` of the file.
int  open_hibf(const Config& c, const std::vector<HibfShape>& ibfs, uint8_t hash_functions, const std::vector<std::vector<std::string>>& bin_path,
               const std::vector<std::string>& user_files, std::vector<uint64_t>& payload_at, std::string& err);
bool save_piece(int fd, gn_filter* flt, uint32_t ibf, uint64_t n_rows, uint64_t row_bytes, uint64_t at, gnhost::PinnedBlock& stage, std::string& err);

// the user bins' sets of a --hibf build from packed sets, as the library's calls for packed runs take them: per user bin its blocks and
// the words of the arena their word_at count in; `bytes` is what one pass over all of them uploads (payload words and block tables)
struct PackedSets
{
    std::vector<const gn_packed_block*> blocks;
    std::vector<uint64_t>               n_blocks;
    std::vector<const uint64_t*>        payload;
    std::vector<uint64_t>               bytes; // per user bin
};
inline uint64_t packed_pass_bytes(const std::vector<GnPackedBlock>& blocks)
{
    uint64_t b = 0;
    for (const GnPackedBlock& x : blocks)
        b += 8ull * gn_packed_words(x.cnt, x.width) + sizeof(GnPackedItem);
    return b;
}

// build_hibf_parts.cpp: the tree of a hierarchical filter, filled part by part over `devices` (one worker an entry) and written as it
// goes; any failure removes the output file.  hash_bytes_uploaded: what the parts' passes over the hash sets sent to the devices.
struct HibfPartsFill
{
    const Config&                                        c;
    const std::vector<HibfShape>&                        ibfs;
    uint8_t                                              hash_functions;
    const HibfPartPlan&                                  plan;
    const std::vector<int>&                              devices;
    const gnhibf::Paths&                                 paths;
    const std::vector<std::pair<const uint64_t*, uint64_t>>& sets; // per user bin (packed: no pointer, the size alone)
    const std::vector<std::vector<std::string>>&         bin_path;
    const std::vector<std::string>&                      user_files;
    const PackedSets*                                    packed = nullptr; // --hibf-hash-sets packed|spilled: the sets; null: raw sets
};
bool fill_and_save_hibf_parts(const HibfPartsFill& w, uint64_t& hash_bytes_uploaded);

// the modes, after the inputs are hashed (build.cpp: run)
// (arenas: --hibf-hash-sets packed|spilled -- the hashing threads' arenas, by Target::arena; empty: raw sets)
bool run_hibf(const Config& c, std::vector<Target>& targets, const Totals& totals, Lap& whole, const Lap& counting,
              const std::vector<std::unique_ptr<SetArena>>& arenas);                                                   // build_hibf.cpp
// build_verify_parts.cpp: the same check of an index that does not fit what an entry of `devices` may hold at one time, part by part
// (hibf_build_parts.hpp: the plan; hibf_verify_parts.hpp: what is carried from part to part); the same report on stdout
bool run_verify_parts(const Config& c, std::vector<Target>& targets, const gnhost::FilterMeta& meta, const std::vector<uint64_t>& payload_at,
                      const HibfPartPlan& plan, const std::vector<int>& devices, double hash_s);
bool run_verify(const Config& c, std::vector<Target>& targets, const Lap& counting);                                  // build_verify.cpp
bool run_update(const Config& c, std::vector<Target>& targets, const Lap& counting);                                  // build_update.cpp

} // namespace gnbuild
