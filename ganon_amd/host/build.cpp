// build.cpp -- `ganon-build` on MI355X: the flat-IBF builder behind the reference's own command line
// (/root/reference/src/ganon-build/CommandLineParser.cpp:14-33, Config.hpp, GanonBuild.cpp).
//
//   input file (file [<tab> target]) -> per target: distinct minimiser hashes of its files   (count_hashes :184-249)
//                                    -> bin capacity / filter size / hash functions          (optimal_hashes :427-616)
//                                    -> technical bins, equal shares per target              (create_bin_map_hash :619-653)
//                                    -> bits set                                             (build :655-698)
//                                    -> .ibf                                                 (save_filter :251-288)
//
// The device does what is data-parallel: sequences are cut into overlapping pieces (every window of a sequence lies in one
// piece), the classify-side minimiser kernels hash them, a radix sort + unique gives the file's hash SET
// (gn_stream_distinct_hashes), the filter is created empty in HBM, filled by an atomic-OR scatter
// (gn_filter_emplace_split) and streamed to the file.  The host parses FASTA, keeps the hash sets (RAM, not `.min` files:
// --tmp-output-folder is accepted and validated, nothing is written there) and does the sizing arithmetic.
// There is no CPU implementation of the hashing or the filter: without a HIP device the program fails.
//
// --hibf (this project's extension, like --device): the same hash sets go into a hierarchical filter instead, written as the
// raptor 3.0.1 index `ganon build --filter-type hibf` gets from `raptor prepare / layout / build`
// (/root/reference/src/ganon/build_update.py:411-518; read at src/ganon-classify/GanonClassify.cpp:875-938):
//   one user bin per target -> tree of IBFs (hibf_layout.hpp) -> exact cardinalities of the merged bins (gn_hashes_union)
//   -> rows per IBF (gnbuild::hibf_run_bits) -> zero-filled HIBF in HBM -> every user bin ORed in along its whole path
//   (gn_filter_emplace_path) -> IBF after IBF streamed into the file (save_hibf: the twin of ganon_amd/ibf_file.py:save_hibf).
//
// --hibf --verify-index F (this project's extension): nothing is built.  The inputs are hashed as for a build, the file's bits are
// streamed into HBM, and per user bin the device answers two questions: is every distinct minimiser of the target found in every
// IBF on the user bin's root-to-leaf path (gn_filter_probe_path along hibf_paths.hpp:derive_paths -- the paths come from the
// FILE's tables, whoever wrote it), and how often does the user bin answer to values that are no target's minimiser
// (gn_filter_probe_paths_shared).
//
// Differences from the reference that cannot be avoided here: targets are laid out in the order of
// their first appearance in the input file and a target's hashes in ascending order -- the reference uses the iteration
// order of robin_hood maps/sets, which is not reproducible without that library; which bin of a split target holds
// which hash therefore differs, the set of hashes per target, the sizing and every IBFConfig value do not.
// Sequences shorter than the window (but at least one k-mer long) yield the minimum over all their k-mers, which is what
// seqan3::views::minimiser does when the range is shorter than its window (recollection of SeqAn3 3.3.0, unpinned).
#include "build_params.hpp"
#include "filter_io.hpp"
#include "hasher.hpp"
#include "hibf_layout.hpp"
#include "hibf_paths.hpp"
#include "hibf_update.hpp"
#include "hibf_layout_similarity.hpp"
#include "hibf_layout_sketch.hpp"
#include "hostmem.hpp"
#include "seq_io.hpp"
#include "tunables.hpp"

#include "ganon_hip.h"

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstring>
#include <fcntl.h>
#include <filesystem>
#include <fstream>
#include <iomanip>
#include <iostream>
#include <map>
#include <memory>
#include <mutex>
#include <set>
#include <sstream>
#include <thread>
#include <unistd.h>

namespace fs = std::filesystem;
using gnbuild::IbfParams;

namespace
{

constexpr const char* kVersion = "2.1.1-mi355x"; // as ganon-classify of this build (config.hpp)
constexpr int         kVersionTuple[3] = { 2, 1, 1 };

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
    int         device = 0; // (not in the reference: which GPU)
    bool        hibf = false;   // (not in the reference: write a raptor 3.0.1 HIBF index instead of a flat .ibf)
    uint64_t    tmax = 0;       // (--hibf only: most technical bins of an IBF; 0 = ceil(sqrt(user bins) / 64) * 64)
    bool        tmax_given = false, filter_size_given = false;
    std::string layout = "rule"; // (--hibf only: rule = hibf_layout.hpp, sketch = hibf_layout_sketch.hpp on HyperLogLog union estimates,
                                 //  similarity = hibf_layout_similarity.hpp: sketch over an order that groups related targets)
    bool        layout_given = false;
    std::string verify_index;    // (--hibf only: check this index against the inputs instead of building one)
    std::string update;          // (--hibf only: add the inputs' targets to this index and write the result to --output-file)
    bool        update_given = false, max_fp_given = false, mode_given = false;
    bool        verify_given = false, kmer_given = false, window_given = false, hashes_given = false, output_given = false;
};

bool validate(Config& c) // Config.hpp:29-107, same messages
{
    auto say = [&](const char* m) {
        if (!c.quiet)
            std::cerr << m << std::endl;
        return false;
    };
    if (c.tmax_given && !c.hibf)
        return say("--tmax needs --hibf");
    if (c.layout_given && !c.hibf)
        return say("--layout needs --hibf");
    if (c.layout_given && c.layout != "rule" && c.layout != "sketch" && c.layout != "similarity")
        return say("--layout has to be rule, sketch or similarity");
    if (c.update_given)
    {
        if (!c.hibf)
            return say("--update needs --hibf (it adds targets to a hierarchical index; a flat .ibf is rebuilt)");
        if (!c.output_given || c.output_file.empty())
            return say("--update needs --output-file (the updated index is written there; the index given is left as it is)");
        if (c.verify_given)
            return say("--update cannot be used with --verify-index (update first, then check the file written)");
        if (c.layout_given)
            return say("--update cannot be used with --layout (the tree of the index is kept)");
        if (c.tmax_given)
            return say("--update cannot be used with --tmax (the tree of the index is kept; an updated IBF is not held to a tmax)");
        if (c.filter_size_given)
            return say("--update cannot be used with --filter-size (the IBFs keep their rows)");
        if (c.mode_given)
            return say("--update cannot be used with --mode");
        if (c.update.empty() || !fs::exists(c.update))
        {
            if (!c.quiet)
                std::cerr << "--update not found: " << c.update << std::endl;
            return false;
        }
        {
            std::error_code ec;
            if (fs::exists(c.output_file) && fs::equivalent(c.update, c.output_file, ec))
                return say("--update: --output-file is the index itself (it is read while the new one is written: give another file)");
        }
        // k, w, the number of hash functions and the false-positive rate are the file's; a value given on the command line has to agree
        try
        {
            gnhost::FilterMeta meta;
            gnhost::read_hibf_meta(c.update, meta);
            const unsigned k = meta.ibf_config.kmer_size, w = meta.ibf_config.window_size, h = (unsigned)meta.shapes.at(0).hash_funs;
            const double   fpr = meta.ibf_config.max_fp;
            auto differs = [&](const char* opt, double given, double file) {
                if (!c.quiet)
                    std::cerr << "--update: " << opt << " " << given << " differs from the index, which was built with " << file << std::endl;
                return false;
            };
            if (c.kmer_given && c.kmer_size != k)
                return differs("--kmer-size", c.kmer_size, k);
            if (c.window_given && c.window_size != w)
                return differs("--window-size", c.window_size, w);
            if (c.hashes_given && c.hash_functions != h)
                return differs("--hash-functions", c.hash_functions, h);
            if (c.max_fp_given && c.max_fp != fpr)
                return differs("--max-fp", c.max_fp, fpr);
            c.kmer_size = (uint8_t)k, c.window_size = (uint16_t)w, c.hash_functions = (uint8_t)h, c.max_fp = fpr;
        }
        catch (const std::exception& e)
        {
            if (!c.quiet)
                std::cerr << "--update: " << e.what() << std::endl;
            return false;
        }
    }
    if (c.verify_given)
    {
        if (!c.hibf)
            return say("--verify-index needs --hibf (it checks a hierarchical index; a flat .ibf is checked by ganon-classify --verify-filter)");
        if (c.output_given)
            return say("--verify-index cannot be used with --output-file (nothing is built and nothing is written)");
        if (c.verify_index.empty() || !fs::exists(c.verify_index))
        {
            if (!c.quiet)
                std::cerr << "--verify-index not found: " << c.verify_index << std::endl;
            return false;
        }
        // k, w and the number of hash functions are the file's; a value given on the command line has to agree
        try
        {
            gnhost::FilterMeta meta;
            gnhost::read_hibf_meta(c.verify_index, meta);
            const unsigned k = meta.ibf_config.kmer_size, w = meta.ibf_config.window_size, h = (unsigned)meta.shapes.at(0).hash_funs;
            auto differs = [&](const char* opt, unsigned given, unsigned file) {
                if (!c.quiet)
                    std::cerr << "--verify-index: " << opt << " " << given << " differs from the index, which was built with " << file << std::endl;
                return false;
            };
            if (c.kmer_given && c.kmer_size != k)
                return differs("--kmer-size", c.kmer_size, k);
            if (c.window_given && c.window_size != w)
                return differs("--window-size", c.window_size, w);
            if (c.hashes_given && c.hash_functions != h)
                return differs("--hash-functions", c.hash_functions, h);
            c.kmer_size = (uint8_t)k, c.window_size = (uint16_t)w, c.hash_functions = (uint8_t)h;
        }
        catch (const std::exception& e)
        {
            if (!c.quiet)
                std::cerr << "--verify-index: " << e.what() << std::endl;
            return false;
        }
    }
    if (c.hibf)
    {
        if (c.filter_size_given)
            return say("--filter-size cannot be used with --hibf (the IBFs are sized from --max-fp)");
        if (c.mode != "avg")
            return say("--mode cannot be used with --hibf");
        if (c.tmax_given && (c.tmax < 2 || c.tmax > 0xFFFFFFFFull))
            return say("--tmax has to be >= 2");
        if (!(c.max_fp > 0 && c.max_fp < 1))
            return say("--max-fp has to be above 0 and below 1 with --hibf");
    }
    if (c.input_file.empty())
        return say("--input-file is mandatory");
    if (!fs::exists(c.input_file))
    {
        if (!c.quiet)
            std::cerr << "--input-file not found: " << c.input_file << std::endl;
        return false;
    }
    if (fs::file_size(c.input_file) == 0)
    {
        if (!c.quiet)
            std::cerr << "--input-file is empty: " << c.input_file << std::endl;
        return false;
    }
    if (c.output_file.empty() && !c.verify_given)
        return say("--output-file is mandatory");
    if (c.tmp_output_folder != "" && !fs::exists(c.tmp_output_folder))
        return say("--tmp-output-folder not found");
    if (c.hash_functions > gnbuild::kMaxHashFunctions)
        return say("--hash-functions must be <=5");
    if (c.filter_size == 0 && c.max_fp == 0)
        return say("--max-fp or --filter-size is mandatory");
    if (c.filter_size > 0)
        c.max_fp = 0;
    if (c.window_size < c.kmer_size)
        return say("--window-size has to be >= --kmer-size");
    if (c.mode != "avg" && c.mode != "smaller" && c.mode != "smallest" && c.mode != "faster" && c.mode != "fastest")
        return say("Invalid --mode");
    if (c.kmer_size > 32)
        return say("--kmer-size has to be <= 32");
    return true;
}

void print_config(const Config& c) // Config.hpp:110-133
{
    const char* sep = "----------------------------------------------------------------------";
    std::cerr << sep << '\n'
              << "--input-file        " << c.input_file << '\n'
              << "--output-file       " << c.output_file << '\n'
              << "--tmp-output-folder " << c.tmp_output_folder << '\n'
              << "--max-fp            " << c.max_fp << '\n'
              << "--filter-size       " << c.filter_size << '\n'
              << "--kmer-size         " << unsigned(c.kmer_size) << '\n'
              << "--window-size       " << c.window_size << '\n'
              << "--hash-functions    " << unsigned(c.hash_functions) << '\n'
              << "--mode              " << c.mode << '\n'
              << "--min-length        " << c.min_length << '\n'
              << "--threads           " << c.threads << '\n'
              << "--verbose           " << c.verbose << '\n'
              << "--quiet             " << c.quiet << '\n';
    if (c.hibf)
        std::cerr << "--hibf              " << c.hibf << '\n' << "--tmax              " << c.tmax << '\n';
    if (c.layout_given)
        std::cerr << "--layout            " << c.layout << '\n';
    if (c.verify_given)
        std::cerr << "--verify-index      " << c.verify_index << '\n';
    if (c.update_given)
        std::cerr << "--update            " << c.update << '\n';
    std::cerr << sep << '\n';
}

const char* kHelp =
    "Ganon builder (MI355X)\n"
    "Usage:\n"
    "  ganon-build [OPTION...]\n\n"
    "  -i, --input-file arg         Define sequences to use. Tabular file with the fields: file [<tab> target]\n"
    "  -o, --output-file arg        Filter output file\n"
    "  -k, --kmer-size arg          k-mer size. Default: 19\n"
    "  -w, --window-size arg        window size. Default: 31\n"
    "  -s, --hash-functions arg     number of hash functions. 0 to auto-detect. Default: 0\n"
    "  -p, --max-fp arg             Maximum false positive rate per target. Used to define filter size [mutually exclusive\n"
    "                               --filter-size]. Default: 0.05\n"
    "  -f, --filter-size arg        Filter size (MB) [mutually exclusive --max-fp]\n"
    "  -j, --mode arg               mode to build filter [avg, smaller, smallest, faster, fastest]. Default: avg\n"
    "  -y, --min-length arg         min. sequence length (bp) to keep. 0 to keep all. Default: 0\n"
    "  -m, --tmp-output-folder arg  Folder to write temporary files (accepted; this build keeps the hashes in memory)\n"
    "  -t, --threads arg            Number of threads (parser threads, one device stream each)\n"
    "      --device arg             HIP device index. Default: 0\n"
    "      --hibf                   Write a hierarchical filter (raptor 3.0.1 index, one user bin per target) sized from\n"
    "                               --max-fp; --hash-functions 0 means 4. Not with --filter-size or a --mode other than avg\n"
    "      --tmax arg               [--hibf] most technical bins of one IBF of the tree (>= 2).\n"
    "                               Default: ceil(sqrt(targets) / 64) * 64\n"
    "      --layout arg             [--hibf] how the tree is chosen: rule (from the targets' hash counts alone), sketch (by size,\n"
    "                               from HyperLogLog estimates of the unions of neighbouring targets) or similarity (as sketch,\n"
    "                               with targets of comparable size reordered so that related ones are neighbours; the\n"
    "                               smaller of the two trees is kept). Default: rule\n"
    "      --verify-index arg       [--hibf] build nothing: check the index `arg` against the --input-file it was built from.\n"
    "                               Per target: is every distinct minimiser found in every IBF on its user bin's path (FAIL\n"
    "                               otherwise, with the first false negative), and how many of 65536 values that are no\n"
    "                               target's minimiser the user bin answers to (WARN fp when clearly above the index's fpr;\n"
    "                               a warning does not fail).  k, w and the hash functions come from the index; give the\n"
    "                               --min-length of the build.  Not with --output-file\n"
    "      --update arg             [--hibf] add the targets of --input-file to the index `arg` and write the result to\n"
    "                               --output-file; `arg` is left as it is.  The old genomes are not needed: how full every bin is\n"
    "                               is read off the index's bits.  The tree is kept: a new target goes below a merged bin that\n"
    "                               has room for it, otherwise it widens the IBF it reached (the root at worst) -- no IBF is\n"
    "                               created or resized in its rows, and --tmax does not bound an updated IBF; the report says\n"
    "                               how many bins each IBF gained, so that one sees when a rebuild is due.  k, w, the hash\n"
    "                               functions and the false-positive rate come from the index.  A target the index holds\n"
    "                               already is refused.  Not with --verify-index, --layout, --tmax, --filter-size, --mode\n"
    "      --verbose                Verbose output mode\n"
    "      --quiet                  Quiet output mode\n"
    "  -h, --help                   Show help commands\n"
    "  -v, --version                Show current version\n";

// returns 0 = run, 1 = exit success, 2 = exit failure
int parse_args(int argc, char** argv, Config& c)
{
    if (argc == 1)
    {
        std::cerr << "Try 'ganon-build -h/--help' for more information." << std::endl;
        return 2;
    }
    static const std::map<std::string, std::string> shorts = {
        { "-i", "--input-file" },  { "-o", "--output-file" }, { "-k", "--kmer-size" },  { "-w", "--window-size" },
        { "-s", "--hash-functions" }, { "-p", "--max-fp" },    { "-f", "--filter-size" }, { "-j", "--mode" },
        { "-y", "--min-length" },  { "-m", "--tmp-output-folder" }, { "-t", "--threads" }, { "-h", "--help" }, { "-v", "--version" }
    };
    std::map<std::string, std::string> vals;
    for (int i = 1; i < argc; ++i)
    {
        std::string a = argv[i], v;
        bool        has = false;
        if (a.size() > 2 && a[0] == '-' && a[1] != '-') // attached short form, -k19 (what cxxopts takes as well)
        {
            v   = a.substr(a[2] == '=' ? 3 : 2);
            a   = a.substr(0, 2);
            has = true;
        }
        if (a.rfind("--", 0) == 0)
        {
            const size_t eq = a.find('=');
            if (eq != std::string::npos)
            {
                v   = a.substr(eq + 1);
                a   = a.substr(0, eq);
                has = true;
            }
        }
        auto s = shorts.find(a);
        if (s != shorts.end())
            a = s->second;
        if (a == "--help" || a == "--version" || a == "--verbose" || a == "--quiet" || a == "--hibf")
        {
            vals[a] = has ? v : "true";
            continue;
        }
        static const std::set<std::string> known = { "--input-file", "--output-file", "--kmer-size", "--window-size",
                                                     "--hash-functions", "--max-fp", "--filter-size", "--mode", "--min-length",
                                                     "--tmp-output-folder", "--threads", "--device", "--tmax", "--layout", "--verify-index", "--update" };
        if (!known.count(a))
        {
            std::cerr << "Option '" << a << "' does not exist" << std::endl;
            return 2;
        }
        if (!has)
        {
            if (i + 1 >= argc)
            {
                std::cerr << "Option '" << a << "' is missing an argument" << std::endl;
                return 2;
            }
            v = argv[++i];
        }
        vals[a] = v;
    }
    if (vals.count("--help"))
    {
        std::cerr << kHelp << std::endl;
        return 1;
    }
    if (vals.count("--version"))
    {
        std::cerr << "version: " << kVersion << std::endl;
        return 1;
    }
    try
    {
        auto u = [&](const char* k, uint64_t hi) -> uint64_t {
            size_t             pos = 0;
            const std::string& s   = vals.at(k);
            const uint64_t     x   = std::stoull(s, &pos);
            if (pos != s.size() || s[0] == '-' || x > hi)
                throw std::invalid_argument(k);
            return x;
        };
        auto d = [&](const char* k) -> double {
            size_t             pos = 0;
            const std::string& s   = vals.at(k);
            const double       x   = std::stod(s, &pos);
            if (pos != s.size())
                throw std::invalid_argument(k);
            return x;
        };
        if (vals.count("--input-file"))
            c.input_file = vals["--input-file"];
        if (vals.count("--output-file"))
            c.output_file = vals["--output-file"], c.output_given = true;
        if (vals.count("--kmer-size"))
            c.kmer_size = (uint8_t)u("--kmer-size", 255), c.kmer_given = true;
        if (vals.count("--window-size"))
            c.window_size = (uint16_t)u("--window-size", 65535), c.window_given = true;
        if (vals.count("--hash-functions"))
            c.hash_functions = (uint8_t)u("--hash-functions", 255), c.hashes_given = true;
        if (vals.count("--verify-index"))
            c.verify_index = vals["--verify-index"], c.verify_given = true;
        if (vals.count("--update"))
            c.update = vals["--update"], c.update_given = true;
        if (vals.count("--max-fp"))
            c.max_fp = d("--max-fp"), c.max_fp_given = true;
        if (vals.count("--filter-size"))
            c.filter_size = d("--filter-size"), c.filter_size_given = true;
        if (vals.count("--tmax"))
            c.tmax = u("--tmax", ~0ull), c.tmax_given = true;
        if (vals.count("--layout"))
            c.layout = vals["--layout"], c.layout_given = true;
        c.hibf = vals.count("--hibf") && vals["--hibf"] != "false";
        if (vals.count("--mode"))
            c.mode = vals["--mode"], c.mode_given = true;
        if (vals.count("--min-length"))
            c.min_length = u("--min-length", ~0ull);
        if (vals.count("--tmp-output-folder"))
            c.tmp_output_folder = vals["--tmp-output-folder"];
        if (vals.count("--threads"))
            c.threads = (uint16_t)u("--threads", 65535);
        if (vals.count("--device"))
            c.device = (int)u("--device", 1 << 20);
        c.verbose = vals.count("--verbose") && vals["--verbose"] != "false";
        c.quiet   = vals.count("--quiet") && vals["--quiet"] != "false";
    }
    catch (const std::exception& e)
    {
        std::cerr << "Argument '" << e.what() << "' failed to parse" << std::endl;
        return 2;
    }
    return 0;
}

struct Target
{
    std::string              name;
    std::vector<std::string> files;
    std::vector<uint64_t>    hashes; // per file: its distinct hashes, ascending; files behind each other (:236-238)
    std::vector<uint64_t>    file_ends; // where each file's hashes end in `hashes` (--hibf unites the files of a target)
};

struct Totals // :52-59
{
    uint64_t files = 0, invalid_files = 0, sequences = 0, skipped_sequences = 0, length_bp = 0;
};

// parse_input_file (:88-140); targets in first-appearance order
std::vector<Target> read_input_file(const Config& c, Totals& totals)
{
    std::vector<Target>           targets;
    std::map<std::string, size_t> index;
    std::set<std::string>         files;
    std::ifstream                 in(c.input_file);
    std::string                   line;
    while (std::getline(in, line, '\n'))
    {
        if (line.empty())
            continue;
        std::vector<std::string> fields;
        std::istringstream       ls(line);
        std::string              f;
        while (std::getline(ls, f, '\t'))
            fields.push_back(f);
        if (fields.empty())
            continue;
        const std::string& file = fields[0];
        files.insert(file);
        std::error_code ec;
        if (!fs::exists(file, ec) || fs::file_size(file, ec) == 0)
        {
            if (!c.quiet)
                std::cerr << "WARNING: input file not found/empty: " << file << std::endl;
            totals.invalid_files++;
            continue;
        }
        std::string target;
        if (fields.size() == 1)
            target = fs::path(file).filename().string();
        else if (fields.size() == 2)
            target = fields[1];
        else
            continue; // (the reference handles one or two columns only)
        auto it = index.find(target);
        if (it == index.end())
        {
            it = index.emplace(target, targets.size()).first;
            targets.push_back(Target{ target, {}, {} });
        }
        targets[it->second].files.push_back(file);
    }
    totals.files = files.size();
    return targets;
}

// count_hashes (:184-249) for the targets this thread draws from the shared cursor
void hash_targets(const Config& c, std::vector<Target>& targets, std::atomic<size_t>& next, Totals& totals, std::string& fatal,
                  std::mutex& log_mutex)
{
    try
    {
        gnhost::Hasher    hasher(c.device, c.kmer_size, c.window_size);
        std::string       ids;
        gnhost::ByteBuf   seq;
        for (;;)
        {
            const size_t t = next.fetch_add(1);
            if (t >= targets.size())
                break;
            Target& tg = targets[t];
            for (const std::string& file : tg.files)
            {
                std::vector<uint64_t> file_hashes;
                unsigned              flushes = 0;
                try
                {
                    gnhost::SeqReader reader(file);
                    for (;;)
                    {
                        ids.clear();
                        seq.clear();
                        if (!reader.next(ids, seq))
                            break;
                        if (seq.size() < c.min_length)
                        {
                            totals.skipped_sequences++;
                            continue;
                        }
                        totals.sequences++;
                        totals.length_bp += seq.size();
                        hasher.add(seq.data(), seq.size(), file_hashes, flushes);
                    }
                    hasher.flush(file_hashes, flushes);
                    hasher.flush_short(file_hashes, flushes);
                }
                catch (const gnhost::ParseError& e)
                {
                    // the reference's catch (:242-246): the file contributes nothing, the next file goes on
                    std::lock_guard<std::mutex> lk(log_mutex);
                    std::cerr << "Error parsing file [" << file << "]. " << e.what() << std::endl;
                    unsigned dummy = 0;
                    std::vector<uint64_t> discard;
                    hasher.flush(discard, dummy);
                    hasher.flush_short(discard, dummy);
                    continue;
                }
                if (flushes > 1) // several device batches: their sets still have to be united
                {
                    std::sort(file_hashes.begin(), file_hashes.end());
                    file_hashes.erase(std::unique(file_hashes.begin(), file_hashes.end()), file_hashes.end());
                }
                tg.hashes.insert(tg.hashes.end(), file_hashes.begin(), file_hashes.end());
                tg.file_ends.push_back(tg.hashes.size());
            }
        }
    }
    catch (const std::exception& e)
    {
        std::lock_guard<std::mutex> lk(log_mutex);
        fatal = e.what();
    }
}

// cereal BinaryOutputArchive encodings
struct Writer
{
    std::string buf;
    template <typename T>
    void raw(const T& v)
    {
        buf.append(reinterpret_cast<const char*>(&v), sizeof(T));
    }
    void str(const std::string& s)
    {
        raw<uint64_t>(s.size());
        buf.append(s);
    }
};

bool pwrite_all(int fd, const void* p, size_t n, uint64_t at)
{
    const char* c = static_cast<const char*>(p);
    while (n)
    {
        const ssize_t w = ::pwrite(fd, c, n, (off_t)at);
        if (w <= 0)
            return false;
        c += w;
        n -= (size_t)w;
        at += (uint64_t)w;
    }
    return true;
}

// save_filter (:251-288): header from the host, the bit matrix streamed out of HBM
bool save_filter(const Config& c, gn_filter* flt, const IbfParams& p, const std::vector<Target>& targets,
                 const std::vector<gnbuild::BinSpan>& bins, std::string& err)
{
    const uint64_t W = (p.n_bins + 63) >> 6;
    Writer         w;
    for (int v : kVersionTuple)
        w.raw<int32_t>(v);
    w.raw<uint64_t>(p.n_bins);
    w.raw<uint64_t>(p.max_hashes_bin);
    w.raw<uint8_t>(p.hash_functions);
    w.raw<uint8_t>(p.kmer_size);
    w.raw<uint16_t>(p.window_size);
    w.raw<uint64_t>(p.bin_size_bits);
    w.raw<double>(p.max_fp);
    w.raw<double>(p.true_max_fp);
    w.raw<double>(p.true_avg_fp);
    w.raw<uint64_t>(targets.size()); // hashes_count_std
    for (const Target& t : targets)
    {
        w.str(t.name);
        w.raw<uint64_t>(t.hashes.size());
    }
    w.raw<uint64_t>(bins.size()); // bin_map
    for (uint64_t b = 0; b < bins.size(); ++b)
    {
        w.raw<uint64_t>(b);
        w.str(targets[bins[b].target].name);
    }
    // seqan3::interleaved_bloom_filter: bins, technical_bins, bin_size, hash_shift, bin_words, hash_funs, sdsl bit_vector
    w.raw<uint64_t>(p.n_bins);
    w.raw<uint64_t>(W * 64);
    w.raw<uint64_t>(p.bin_size_bits);
    w.raw<uint64_t>((uint64_t)__builtin_clzll(p.bin_size_bits));
    w.raw<uint64_t>(W);
    w.raw<uint64_t>(p.hash_functions);
    w.raw<uint8_t>(1);      // sdsl int_vector<1>: width
    w.raw<float>(1.5f);     //                    growth factor
    w.raw<uint64_t>(W * 64 * p.bin_size_bits); // size in bits
    const int fd = ::open(c.output_file.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0644);
    if (fd < 0)
    {
        err = "cannot write " + c.output_file;
        return false;
    }
    bool ok = pwrite_all(fd, w.buf.data(), w.buf.size(), 0);
    const uint64_t payload_at = w.buf.size();
    const uint64_t row_bytes  = W * 8;
    const uint64_t per        = std::max<uint64_t>(1, std::min<uint64_t>(256ull << 20, p.bin_size_bits * row_bytes) / row_bytes);
    void*          stage      = nullptr;
    if (ok && gn_pinned_alloc(per * row_bytes, &stage) != GN_OK)
    {
        err = gnhost::hip_error();
        ok  = false;
    }
    for (uint64_t row = 0; ok && row < p.bin_size_bits; row += per)
    {
        const uint64_t n = std::min<uint64_t>(per, p.bin_size_bits - row);
        if (gn_filter_download_rows(flt, 0, row, n, static_cast<uint64_t*>(stage)) != GN_OK)
        {
            err = gnhost::hip_error();
            ok  = false;
            break;
        }
        // a few writers per chunk: one pwrite stream does not fill a fast disk
        const unsigned           nt = (unsigned)std::min<uint64_t>(8, std::max<uint64_t>(1, n * row_bytes >> 24));
        std::vector<std::thread> th;
        std::atomic<bool>        good{ true };
        const uint64_t           bytes = n * row_bytes, share = (bytes + nt - 1) / nt;
        for (unsigned i = 0; i < nt; ++i)
            th.emplace_back([&, i] {
                const uint64_t lo = std::min<uint64_t>(bytes, i * share), hi = std::min<uint64_t>(bytes, lo + share);
                if (hi > lo && !pwrite_all(fd, static_cast<const char*>(stage) + lo, hi - lo, payload_at + row * row_bytes + lo))
                    good = false;
            });
        for (auto& t : th)
            t.join();
        if (!good)
        {
            err = "write error on " + c.output_file;
            ok  = false;
        }
    }
    if (stage)
        gn_pinned_free(stage);
    ::close(fd);
    return ok;
}

std::string stamp(std::chrono::system_clock::time_point t)
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

// ---- --hibf ----------------------------------------------------------------------------------------------------------------------

struct HibfShape // IBF i of the tree as it is created and written
{
    uint64_t             bins = 0, rows = 0;
    std::vector<int64_t> next_ibf_id, bin_to_user;
};

// The raptor 3.0.1 index (reader: GanonClassify.cpp:875-938 with hibf.hpp:163-169,293-298), field for field what
// ganon_amd/ibf_file.py:save_hibf writes; the matrices streamed IBF after IBF out of HBM.
// bin_path: the files of every user bin (this builder writes one each; a raptor file that `--update` carries over may list several);
// user_files: user_bin_filenames, one per user bin.
bool save_hibf(const Config& c, gn_filter* flt, const std::vector<HibfShape>& ibfs, uint8_t hash_functions,
               const std::vector<std::vector<std::string>>& bin_path, const std::vector<std::string>& user_files, std::string& err)
{
    const int fd = ::open(c.output_file.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0644);
    if (fd < 0)
    {
        err = "cannot write " + c.output_file;
        return false;
    }
    uint64_t at    = 0;
    bool     ok    = true;
    auto     flush = [&](Writer& w) {
        ok = ok && pwrite_all(fd, w.buf.data(), w.buf.size(), at);
        at += w.buf.size();
        w.buf.clear();
    };
    Writer w;
    w.raw<uint32_t>(1);                                     // raptor index version
    w.raw<uint64_t>(c.window_size);
    w.raw<uint64_t>(c.kmer_size);                           // seqan3::shape: size, bits
    w.raw<uint64_t>(c.kmer_size >= 64 ? ~0ull : (1ull << c.kmer_size) - 1);
    w.raw<uint8_t>(1);                                      // parts
    w.raw<uint8_t>(0);                                      // compressed
    w.raw<uint64_t>(bin_path.size());                       // bin_path
    for (const std::vector<std::string>& lst : bin_path)
    {
        w.raw<uint64_t>(lst.size());
        for (const std::string& f : lst)
            w.str(f);
    }
    w.raw<double>(c.max_fp);                                // fpr
    w.raw<uint8_t>(1);                                      // is_hibf
    w.raw<uint64_t>(ibfs.size());                           // ibf_vector
    flush(w);
    constexpr uint64_t kChunk = 256ull << 20;
    uint64_t           stage_bytes = 0;
    for (const HibfShape& s : ibfs)
        stage_bytes = std::max(stage_bytes, std::max<uint64_t>(1, std::min<uint64_t>(kChunk, s.rows * ((s.bins + 63) >> 6) * 8) / (((s.bins + 63) >> 6) * 8)) *
                                                (((s.bins + 63) >> 6) * 8));
    void* stage = nullptr;
    if (ok && gn_pinned_alloc(stage_bytes, &stage) != GN_OK)
    {
        err = gnhost::hip_error();
        ok  = false;
    }
    for (uint32_t i = 0; ok && i < ibfs.size(); ++i)
    {
        const HibfShape& s = ibfs[i];
        const uint64_t   W = (s.bins + 63) >> 6, row_bytes = W * 8;
        // seqan3::interleaved_bloom_filter: bins, technical_bins, bin_size, hash_shift, bin_words, hash_funs, sdsl bit_vector
        w.raw<uint64_t>(s.bins);
        w.raw<uint64_t>(W * 64);
        w.raw<uint64_t>(s.rows);
        w.raw<uint64_t>((uint64_t)__builtin_clzll(s.rows));
        w.raw<uint64_t>(W);
        w.raw<uint64_t>(hash_functions);
        w.raw<uint8_t>(1);
        w.raw<float>(1.5f);
        w.raw<uint64_t>(W * 64 * s.rows);
        flush(w);
        const uint64_t per = std::max<uint64_t>(1, std::min<uint64_t>(kChunk, s.rows * row_bytes) / row_bytes);
        for (uint64_t row = 0; ok && row < s.rows; row += per)
        {
            const uint64_t n = std::min<uint64_t>(per, s.rows - row);
            if (gn_filter_download_rows(flt, i, row, n, static_cast<uint64_t*>(stage)) != GN_OK)
            {
                err = gnhost::hip_error();
                ok  = false;
                break;
            }
            if (!pwrite_all(fd, stage, n * row_bytes, at))
                ok = false;
            at += n * row_bytes;
        }
    }
    auto tables = [&](bool next) {
        w.raw<uint64_t>(ibfs.size());
        for (const HibfShape& s : ibfs)
        {
            const std::vector<int64_t>& v = next ? s.next_ibf_id : s.bin_to_user;
            w.raw<uint64_t>(v.size());
            w.buf.append(reinterpret_cast<const char*>(v.data()), v.size() * 8);
        }
    };
    tables(true);                                           // next_ibf_id
    w.raw<uint64_t>(user_files.size());                     // user_bins: user_bin_filenames
    for (const std::string& f : user_files)
        w.str(f);
    tables(false);                                          //            ibf_bin_to_filename_position
    flush(w);
    if (stage)
        gn_pinned_free(stage);
    ::close(fd);
    if (!ok && err.empty())
        err = "write error on " + c.output_file;
    return ok;
}

// --layout sketch | similarity: one HyperLogLog sketch per user bin on the device, the estimated unions of up to `width` neighbours
// in an order for every start (tiled over the starts: gn_sketches_union_table bounds a call), then the search of
// hibf_layout_sketch.hpp.  similarity (hibf_layout_similarity.hpp) asks for that table twice, one after the other -- the size order's
// and the similarity order's -- and in between for one gn_sketches_pair_table per interval of the size order.
struct SketchLaps // seconds inside the `layout` lap: the rest of it is the host's ordering and searches
{
    double sketches = 0, tables = 0, pairs = 0;
};

bool lay_out_by_sketches(const Config& c, const std::vector<Target>& targets, const std::vector<uint32_t>& user_target, const std::vector<uint64_t>& counts,
                         uint32_t tmax, uint8_t h, gnhibf::Layout& lay, SketchLaps& laps, std::string& err)
{
    constexpr uint64_t kTableBytes = 4ull << 30; // the most host memory a union table may take
    const uint64_t     n = counts.size(), width = gnhibf::sketch_width(n, tmax);
    const bool         similarity = c.layout == "similarity";
    gn_sketches*       sk = nullptr;
    auto               since = [](std::chrono::steady_clock::time_point t) { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t).count(); };
    if (width >= 2) // (width 1: one IBF, no union is asked for)
    {
        if (n * width > kTableBytes / 8)
        {
            err = "--layout " + c.layout + ": the union estimates of " + std::to_string(n) + " user bins, " + std::to_string(width) +
                  " neighbours each, take " + std::to_string(n * width * 8) + " bytes of host memory, more than " + std::to_string(kTableBytes) +
                  "; use another --tmax (which sets how many neighbours a merged bin may hold) or --layout rule";
            return false;
        }
        const auto                   t0 = std::chrono::steady_clock::now();
        std::vector<const uint64_t*> sets(n);
        for (uint64_t u = 0; u < n; ++u)
            sets[u] = targets[user_target[u]].hashes.data();
        if (gn_sketches_create(c.device, sets.data(), counts.data(), (uint32_t)n, &sk) != GN_OK)
        {
            err = gn_last_error();
            return false;
        }
        laps.sketches = since(t0);
    }
    struct DeviceError // a device call inside a callback failed: the search ends there
    {
        std::string what;
    };
    // the union table of an order, held by the estimate that reads it
    const gnhibf::OrderUnions unions = [&](const std::vector<uint32_t>& order) -> gnhibf::UnionEstimate {
        const auto t0    = std::chrono::steady_clock::now();
        auto       table = std::make_shared<std::vector<uint64_t>>(n * width, 0);
        const uint64_t per = std::max<uint64_t>(1, GN_SKETCH_TABLE_MAX / width);
        for (uint64_t j = 0; j < n; j += per)
            if (gn_sketches_union_table(sk, order.data(), (uint32_t)n, (uint32_t)j, (uint32_t)std::min(n, j + per), (uint32_t)width,
                                        table->data() + j * width) != GN_OK)
                throw DeviceError{ gn_last_error() };
        laps.tables += since(t0);
        return [table, width](uint64_t j, uint64_t l) { return (*table)[j * width + l - 1]; };
    };
    const std::vector<uint32_t> size_order = gnhibf::sketch_order(counts);
    // the pair table of one interval of the size order, held likewise
    const gnhibf::IntervalPairs pairs = [&](uint64_t a, uint64_t b) -> gnhibf::PairEstimate {
        const auto     t0    = std::chrono::steady_clock::now();
        const uint64_t m     = b - a;
        auto           table = std::make_shared<std::vector<uint64_t>>(m * m, 0);
        if (gn_sketches_pair_table(sk, size_order.data() + a, (uint32_t)m, table->data()) != GN_OK)
            throw DeviceError{ gn_last_error() };
        laps.pairs += since(t0);
        return [table, m](uint64_t p, uint64_t q) { return (*table)[p * m + q]; };
    };
    bool ok = true;
    try
    {
        if (similarity)
        {
            gnhibf::SimilarityLayout got = gnhibf::lay_out_similarity(counts, tmax, c.max_fp, h, unions, pairs);
            lay                          = std::move(got.layout);
            if (c.verbose)
                std::cerr << "layout similarity: " << got.intervals << " intervals, " << got.moved << " of " << n << " user bins moved, kept " << got.kept
                          << std::endl;
        }
        else if (width >= 2)
            lay = gnhibf::lay_out_sketch(counts, tmax, c.max_fp, h, unions(size_order));
        else
            lay = gnhibf::lay_out_sketch(counts, tmax, c.max_fp, h, [](uint64_t, uint64_t) -> uint64_t { return 0; });
    }
    catch (const DeviceError& e)
    {
        err = e.what;
        ok  = false;
    }
    if (sk)
        gn_sketches_free(sk);
    return ok;
}

// a target's set = the union of its files' sets, ascending
bool unite_files(const Config& c, Target& tg)
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

// the name of a target's user bin as an index file gives it back: written as <folder>/<name, "---" for a space>.minimiser by this
// builder (and by `ganon build`, build_update.py:411-518), read as filter_io.cpp:parse_hibf reads it (GanonClassify.cpp:908-935)
std::string user_bin_file_name(const std::string& target)
{
    std::string name = target;
    for (size_t p = 0; (p = name.find(' ', p)) != std::string::npos; p += 3)
        name.replace(p, 1, "---");
    return name;
}

// the loader's own reading of the name this builder would write for a target (filter_io.cpp:parse_hibf)
std::string name_as_read(const std::string& target)
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

bool run_hibf(const Config& c, std::vector<Target>& targets, const Totals& totals, Lap& whole, const Lap& counting)
{
    Lap            uniting, laying, filling, writing;
    const uint8_t  h = c.hash_functions == 0 ? 4 : c.hash_functions; // (what `ganon build` passes to raptor, config.py:138-145)
    auto           fail = [](const std::string& m) {
        std::cerr << m << std::endl;
        return false;
    };

    // one user bin per target with a hash, in first-appearance order; its set = the union of its files' sets
    uniting.start();
    std::vector<uint32_t>    user_target;
    std::vector<uint64_t>    counts;
    std::vector<std::string> files;
    const std::string        dir = !c.tmp_output_folder.empty() ? c.tmp_output_folder
                                   : fs::path(c.output_file).has_parent_path() ? fs::path(c.output_file).parent_path().string()
                                                                               : std::string(".");
    for (uint32_t t = 0; t < targets.size(); ++t)
    {
        Target& tg = targets[t];
        if (tg.hashes.empty())
            continue;
        if (!unite_files(c, tg))
            return fail(gn_last_error());
        user_target.push_back(t);
        counts.push_back(tg.hashes.size());
        files.push_back(dir + "/" + user_bin_file_name(tg.name) + ".minimiser");
    }
    if (counts.empty())
        return fail("No valid sequences to build");
    const uint64_t n_user = counts.size();
    uint64_t       tmax   = c.tmax;
    if (!c.tmax_given)
        tmax = (uint64_t)std::ceil(std::sqrt((double)n_user) / 64.0) * 64; // build_update.py:487
    laying.start();
    gnhibf::Layout lay;
    SketchLaps     sketch_laps;
    if (c.layout == "sketch" || c.layout == "similarity")
    {
        std::string err;
        if (!lay_out_by_sketches(c, targets, user_target, counts, (uint32_t)tmax, h, lay, sketch_laps, err))
            return fail(err);
    }
    else
        lay = gnhibf::lay_out(counts, (uint32_t)tmax);
    laying.stop();

    // rows per IBF: the largest need of its runs; a merged bin holds the union of the sets below it
    std::vector<HibfShape> ibfs(lay.ibfs.size());
    uint64_t               device_bits = 0;
    for (uint32_t i = 0; i < lay.ibfs.size(); ++i)
    {
        const gnhibf::Ibf& f = lay.ibfs[i];
        uint64_t           rows = 0;
        for (const gnhibf::Run& r : f.runs)
        {
            uint64_t n = 0;
            if (r.user >= 0)
                n = counts[r.user];
            else
            {
                std::vector<const uint64_t*> sets;
                std::vector<uint64_t>        sizes;
                for (uint32_t u : lay.ibfs[r.child].members)
                {
                    sets.push_back(targets[user_target[u]].hashes.data());
                    sizes.push_back(counts[u]);
                }
                if (gn_hashes_union(c.device, sets.data(), sizes.data(), (uint32_t)sets.size(), nullptr, 0, &n) != GN_OK)
                    return fail(gn_last_error());
            }
            rows = std::max(rows, gnbuild::hibf_run_bits(n, r.n_bins, c.max_fp, h));
        }
        ibfs[i].bins = f.bins;
        ibfs[i].rows = rows;
        gnhibf::tables_of(lay, i, ibfs[i].next_ibf_id, ibfs[i].bin_to_user);
        device_bits += rows * gn_hibf_row_stride_words((f.bins + 63) >> 6) * 64;
    }
    uniting.stop();
    if (c.verbose)
    {
        std::cerr << "hibf_config:" << '\n'
                  << "user_bins      " << n_user << '\n'
                  << "tmax           " << tmax << '\n'
                  << "ibfs           " << ibfs.size() << '\n'
                  << "levels         " << lay.levels << '\n'
                  << "layout         " << c.layout << '\n'
                  << "hash_functions " << unsigned(h) << '\n'
                  << "max_fp         " << c.max_fp << '\n';
        std::cerr << "Filter size: " << device_bits << " Bits (" << device_bits / static_cast<double>(8388608u) << " Megabytes)" << std::endl;
    }

    filling.start();
    gn_filter* flt = nullptr;
    {
        std::vector<gn_ibf_desc>    descs(ibfs.size());
        std::vector<const int64_t*> nx(ibfs.size()), bu(ibfs.size());
        for (uint32_t i = 0; i < ibfs.size(); ++i)
        {
            gn_ibf_desc& d = descs[i];
            d.rows = nullptr, d.bins = ibfs[i].bins, d.bin_words = (ibfs[i].bins + 63) >> 6, d.bin_size = ibfs[i].rows, d.hash_funs = h;
            d.hash_shift = (uint32_t)__builtin_clzll(ibfs[i].rows);
            nx[i] = ibfs[i].next_ibf_id.data(), bu[i] = ibfs[i].bin_to_user.data();
        }
        if (gn_filter_upload_hibf(c.device, (uint32_t)ibfs.size(), descs.data(), nx.data(), bu.data(), n_user, &flt) != GN_OK)
            return fail(gn_last_error());
    }
    {
        // every user bin's path: its run in its leaf IBF, then the merged bin that leads there in each IBF above
        const gnhibf::Paths               all_paths = gnhibf::paths_of(lay, counts);
        const uint32_t                    depth     = all_paths.depth;
        const std::vector<gn_path_entry>& path_of   = all_paths.entries;
        // large sets go as they lie; small ones are gathered so that a launch has enough of them
        constexpr uint64_t         kBatch = 16ull << 20, kAlone = 4ull << 20;
        std::vector<uint64_t>      pool, off{ 0 };
        std::vector<gn_path_entry> paths;
        bool                       ok    = true;
        auto                       flush = [&] {
            if (off.size() > 1 && gn_filter_emplace_path(flt, pool.data(), off.data(), (uint32_t)off.size() - 1, paths.data(), depth) != GN_OK)
                ok = false;
            pool.clear(), paths.clear(), off.assign(1, 0);
        };
        for (uint64_t u = 0; ok && u < n_user; ++u)
        {
            const std::vector<uint64_t>& hs = targets[user_target[u]].hashes;
            if (hs.size() >= kAlone)
            {
                const uint64_t one[2] = { 0, hs.size() };
                ok = gn_filter_emplace_path(flt, hs.data(), one, 1, &path_of[u * depth], depth) == GN_OK;
                continue;
            }
            pool.insert(pool.end(), hs.begin(), hs.end());
            off.push_back(pool.size());
            paths.insert(paths.end(), path_of.begin() + u * depth, path_of.begin() + (u + 1) * depth);
            if (pool.size() >= kBatch)
                flush();
        }
        if (ok)
            flush();
        if (!ok)
        {
            const std::string m = gn_last_error();
            gn_filter_free(flt);
            return fail(m);
        }
    }
    filling.stop();

    writing.start();
    std::string err;
    std::vector<std::vector<std::string>> bin_path; // one file per user bin
    for (const std::string& f : files)
        bin_path.push_back({ f });
    const bool saved = save_hibf(c, flt, ibfs, h, bin_path, files, err);
    gn_filter_free(flt);
    if (!saved)
        return fail(err);
    writing.stop();
    whole.stop();

    if (!c.quiet)
    {
        if (c.verbose)
        {
            auto block = [](const char* a, const char* pad, const Lap& l) {
                std::cerr << a << stamp(l.b) << '\n' << pad << "    end: " << stamp(l.e) << '\n' << pad << "elapsed (s): " << l.seconds() << '\n';
            };
            block("Count/save hashes start: ", "                ", counting);
            block("Layout and unions start: ", "                ", uniting);
            block("Building filter   start: ", "                ", filling);
            block("Saving filer      start: ", "                ", writing);
            block("ganon-build       start: ", "                ", whole);
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
        std::cerr << " - hibf: " << n_user << " user bins in " << ibfs.size() << " IBFs on " << lay.levels << " level(s), tmax " << tmax << std::endl;
        std::cerr << std::fixed << std::setprecision(2) << " - filter size: " << device_bits / static_cast<double>(8388608u) << "MB" << std::endl;
        // (one line a caller can parse: where the time went)
        std::cerr << std::setprecision(6) << " - seconds: hash " << counting.seconds() << " union " << uniting.seconds() << " emplace " << filling.seconds()
                  << " write " << writing.seconds();
        if (c.layout == "sketch" || c.layout == "similarity") // (part of `union`: sketches, union table and search)
            std::cerr << " layout " << laying.seconds();
        std::cerr << std::endl;
        if (c.layout == "similarity") // (where the layout lap went; host = the ordering and the searches)
            std::cerr << " - layout seconds: sketches " << sketch_laps.sketches << " tables " << sketch_laps.tables << " pairs " << sketch_laps.pairs << " host "
                      << laying.seconds() - sketch_laps.sketches - sketch_laps.tables - sketch_laps.pairs << std::endl;
    }
    return true;
}

// ---- --hibf --verify-index -------------------------------------------------------------------------------------------------------

// the index's bits into HBM of one device through the streaming loader (as verify.cpp's OneDeviceSink does for a flat filter)
class HibfDeviceSink final : public gnhost::FilterSink
{
public:
    explicit HibfDeviceSink(int device) : device_(device) {}
    ~HibfDeviceSink() override
    {
        if (f_)
            gn_filter_free(f_);
        for (auto& s : stage_)
            if (s.ptr)
                gn_pinned_free(s.ptr);
    }
    bool begin(const gnhost::FilterMeta& f, std::string& err) override
    {
        std::vector<gn_ibf_desc>    descs(f.shapes.size());
        std::vector<const int64_t*> nx(f.shapes.size()), bu(f.shapes.size());
        words_.resize(f.shapes.size());
        for (size_t i = 0; i < f.shapes.size(); ++i)
        {
            const gnhost::IbfShape& m = f.shapes[i];
            descs[i] = gn_ibf_desc{ nullptr, m.bin_size, m.bin_words, m.bins, (uint32_t)m.hash_funs, (uint32_t)m.hash_shift };
            nx[i] = f.next_ibf_id[i].data(), bu[i] = f.bin_to_user[i].data();
            words_[i] = m.bin_words;
        }
        if (gn_filter_upload_hibf(device_, (uint32_t)descs.size(), descs.data(), nx.data(), bu.data(), f.n_user_bins, &f_) != GN_OK)
        {
            err = gn_last_error();
            return false;
        }
        return true;
    }
    uint64_t* staging(int which, size_t bytes) override
    {
        Stage& s = stage_[which & 1];
        if (s.bytes < bytes)
        {
            if (s.ptr)
                gn_pinned_free(s.ptr);
            s = Stage{};
            void* p = nullptr;
            if (gn_pinned_alloc(bytes, &p) != GN_OK)
                return nullptr;
            s.ptr = p, s.bytes = bytes;
        }
        return static_cast<uint64_t*>(s.ptr);
    }
    bool rows(uint32_t ibf, uint64_t row_begin, uint64_t n_rows, const uint64_t* src, std::string& err) override
    {
        if (gn_filter_write_rows(f_, ibf, row_begin, n_rows, src, words_.at(ibf), 0) == GN_OK)
            return true;
        err = gn_last_error();
        return false;
    }
    bool drain(std::string& err) override
    {
        if (gn_filter_write_sync(f_) == GN_OK)
            return true;
        err = gn_last_error();
        return false;
    }
    bool end(std::string& err) override
    {
        if (gn_filter_finalize(f_) == GN_OK)
            return true;
        err = gn_last_error();
        return false;
    }
    gn_filter* filter() const { return f_; }

private:
    struct Stage
    {
        void*  ptr   = nullptr;
        size_t bytes = 0;
    };
    int                   device_;
    std::vector<uint64_t> words_;
    gn_filter*            f_ = nullptr;
    Stage                 stage_[2];
};

constexpr uint64_t kVerifyProbes = 65536; // P of the false-positive pass

// probe i of the false-positive pass (include/ganon_hip.h states the generator): splitmix64 of i + 1 with bit 63 set -- a
// (k,w)-minimiser hash is below 4^k, so for k <= 31 no target holds such a value
uint64_t verify_probe(uint64_t i)
{
    uint64_t z = (i + 1) * 0x9E3779B97F4A7C15ull;
    z          = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z          = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    return z | (1ull << 63);
}

bool run_verify(const Config& c, std::vector<Target>& targets, const Lap& counting)
{
    auto fail = [](const std::string& m) {
        std::cerr << m << std::endl;
        return false;
    };
    auto since = [](std::chrono::steady_clock::time_point t) { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t).count(); };
    auto t0 = std::chrono::steady_clock::now();
    for (Target& tg : targets)
        if (!unite_files(c, tg))
            return fail(gn_last_error());
    const double hash_s = counting.seconds() + since(t0);
    try
    {
        t0 = std::chrono::steady_clock::now();
        gnhost::FilterMeta meta;
        HibfDeviceSink     sink(c.device);
        gnhost::load_filter_file(c.verify_index, true, meta, sink);
        gn_filter* const flt    = sink.filter();
        const double     load_s = since(t0);
        std::vector<uint64_t> bins;
        for (const gnhost::IbfShape& m : meta.shapes)
            bins.push_back(m.bins);
        const gnhibf::Paths paths  = gnhibf::derive_paths(bins, meta.next_ibf_id, meta.bin_to_user, meta.n_user_bins);
        const uint32_t      depth  = paths.depth;
        const uint64_t      n_user = meta.n_user_bins;
        const unsigned      k = meta.ibf_config.kmer_size, h = (unsigned)meta.shapes.at(0).hash_funs;
        const double        fpr = meta.ibf_config.max_fp;
        std::map<std::string, uint64_t> user_of; // names as the loader recovers them -> user bin
        for (size_t t = 0; t < meta.targets.size(); ++t)
            user_of[meta.targets[t]] = meta.target_bins[t].at(0);
        auto as_read = [](const std::string& target) { return name_as_read(target); };

        // membership: every target's set along its user bin's path, pooled as run_hibf pools its inserts
        t0 = std::chrono::steady_clock::now();
        constexpr uint64_t    none = ~0ull;
        std::vector<uint64_t> user(targets.size(), none), found(targets.size(), 0), first_lost(targets.size(), none);
        std::vector<uint64_t> lost_at(targets.size() * (size_t)depth, 0);
        uint64_t              looked_up = 0;
        {
            constexpr uint64_t         kBatch = 16ull << 20, kAlone = 4ull << 20;
            std::vector<uint64_t>      pool, off{ 0 }, r_found, r_lost, r_first;
            std::vector<gn_path_entry> pp;
            std::vector<size_t>        who;
            auto probe = [&](const uint64_t* hashes, const uint64_t* set_off, const gn_path_entry* p, const std::vector<size_t>& ts) {
                r_found.assign(ts.size(), 0), r_first.assign(ts.size(), none), r_lost.assign(ts.size() * (size_t)depth, 0);
                if (gn_filter_probe_path(flt, hashes, set_off, (uint32_t)ts.size(), p, depth, r_found.data(), r_lost.data(), r_first.data()) != GN_OK)
                    throw std::runtime_error(gn_last_error());
                for (size_t j = 0; j < ts.size(); ++j)
                {
                    found[ts[j]] = r_found[j], first_lost[ts[j]] = r_first[j];
                    std::copy(r_lost.begin() + j * depth, r_lost.begin() + (j + 1) * depth, lost_at.begin() + ts[j] * depth);
                }
            };
            auto flush = [&] {
                if (!who.empty())
                    probe(pool.data(), off.data(), pp.data(), who);
                pool.clear(), pp.clear(), who.clear(), off.assign(1, 0);
            };
            for (size_t t = 0; t < targets.size(); ++t)
            {
                const std::vector<uint64_t>& hs = targets[t].hashes;
                auto                         it = user_of.find(as_read(targets[t].name));
                if (it == user_of.end() || hs.empty())
                {
                    user[t] = it == user_of.end() ? none : it->second;
                    continue;
                }
                user[t] = it->second;
                looked_up += hs.size();
                const gn_path_entry* p = &paths.entries[user[t] * depth];
                if (hs.size() >= kAlone)
                {
                    const uint64_t one[2] = { 0, hs.size() };
                    probe(hs.data(), one, p, { t });
                    continue;
                }
                pool.insert(pool.end(), hs.begin(), hs.end());
                off.push_back(pool.size());
                pp.insert(pp.end(), p, p + depth);
                who.push_back(t);
                if (pool.size() >= kBatch)
                    flush();
            }
            flush();
        }
        const double member_s = since(t0);

        // false positives: the same P probes against every user bin of the file, paths sorted by (leaf ibf, first bin)
        t0 = std::chrono::steady_clock::now();
        const bool            fp_pass = k <= 31; // (k = 32: a hash can take any 64-bit value, no probe is a certain negative)
        std::vector<uint64_t> false_hits(n_user, 0);
        if (fp_pass && n_user)
        {
            std::vector<uint64_t> probes(kVerifyProbes), order(n_user), got(n_user, 0);
            for (uint64_t i = 0; i < kVerifyProbes; ++i)
                probes[i] = verify_probe(i);
            for (uint64_t u = 0; u < n_user; ++u)
                order[u] = u;
            std::sort(order.begin(), order.end(), [&](uint64_t a, uint64_t b) {
                const gn_path_entry &x = paths.entries[a * depth], &y = paths.entries[b * depth];
                return std::make_pair(x.ibf, x.first_bin) < std::make_pair(y.ibf, y.first_bin);
            });
            std::vector<gn_path_entry> sorted;
            for (uint64_t u : order)
                sorted.insert(sorted.end(), paths.entries.begin() + u * depth, paths.entries.begin() + (u + 1) * depth);
            if (gn_filter_probe_paths_shared(flt, probes.data(), probes.size(), sorted.data(), (uint32_t)n_user, depth, got.data()) != GN_OK)
                throw std::runtime_error(gn_last_error());
            for (uint64_t j = 0; j < n_user; ++j)
                false_hits[order[j]] = got[j];
        }
        const double fp_s = since(t0);
        const double P = (double)kVerifyProbes;
        const uint64_t warn_above = (uint64_t)std::ceil(P * fpr + 4.0 * std::sqrt(P * fpr * (1.0 - fpr)));

        std::cout << "index\t" << c.verify_index << "\tk=" << k << " w=" << meta.ibf_config.window_size << " h=" << h << " ibfs=" << meta.shapes.size()
                  << " levels=" << depth << " user_bins=" << n_user << " fpr=" << fpr << "\n";
        std::cout << "#target\tuser_bin\tleaf_ibf\tbins\tdepth\tdistinct_hashes\tmissing\tfalse_hits\tobserved_fp\tverdict\n";
        uint64_t          n_checked = 0, n_bad = 0, fp_sum = 0, fp_max = 0;
        std::vector<bool> named(n_user, false);
        std::cout << std::fixed << std::setprecision(6);
        for (size_t t = 0; t < targets.size(); ++t)
        {
            const std::vector<uint64_t>& hs = targets[t].hashes;
            if (user[t] == none)
            {
                // a target without a hash has no user bin in an index built from these inputs: nothing to look for
                std::cout << targets[t].name << "\t-\t-\t0\t0\t" << hs.size() << "\t0\t" << (fp_pass ? "0" : "n/a") << "\t" << (fp_pass ? "0.000000" : "n/a") << "\t"
                          << (hs.empty() ? "ok" : "FAIL: no such user bin") << "\n";
                n_bad += !hs.empty();
                continue;
            }
            const gn_path_entry* p = &paths.entries[user[t] * depth];
            uint32_t             used = 0;
            while (used < depth && p[used].n_bins)
                ++used;
            const uint64_t missing = hs.size() - found[t], hits = false_hits[user[t]];
            const bool     warn    = fp_pass && hits > warn_above;
            ++n_checked;
            named[user[t]] = true;
            n_bad += missing != 0;
            fp_sum += hits, fp_max = std::max(fp_max, hits);
            std::cout << targets[t].name << "\t" << user[t] << "\t" << p[0].ibf << "\t" << p[0].n_bins << "\t" << used << "\t" << hs.size() << "\t" << missing << "\t";
            if (fp_pass)
                std::cout << hits << "\t" << hits / P;
            else
                std::cout << "n/a\tn/a";
            std::cout << "\t" << (missing ? "FAIL" : warn ? "WARN fp" : "ok") << "\n";
            if (missing)
            {
                // the first false negative: its hash, the first entry of the path that lacks it, its h rows there and the bits found
                const uint64_t        v = hs[first_lost[t]], one[2] = { 0, 1 };
                uint64_t              f1 = 0, fl = 0;
                std::vector<uint64_t> l1(depth, 0);
                if (gn_filter_probe_path(flt, &v, one, 1, p, depth, &f1, l1.data(), &fl) != GN_OK)
                    throw std::runtime_error(gn_last_error());
                uint32_t d = 0;
                while (d + 1 < used && l1[d] == 0)
                    ++d;
                const gnhost::IbfShape& m = meta.shapes.at(p[d].ibf);
                std::vector<uint64_t>   rows(m.hash_funs), words(m.hash_funs * m.bin_words);
                for (unsigned i = 0; i < m.hash_funs; ++i)
                    rows[i] = gnhost::ibf_row(v, i, m);
                if (gn_filter_download_row_list(flt, p[d].ibf, rows.data(), rows.size(), words.data()) != GN_OK)
                    throw std::runtime_error(gn_last_error());
                std::cout << "  first false negative: hash " << v << " (index " << first_lost[t] << " of the sorted distinct hashes); lost at level " << d << ", ibf "
                          << p[d].ibf << ", bins " << p[d].first_bin << ".." << p[d].first_bin + p[d].n_bins - 1 << "; rows";
                for (auto r : rows)
                    std::cout << " " << r;
                std::cout << "; bits [bin: one per hash function]";
                for (uint32_t b = p[d].first_bin; b < p[d].first_bin + p[d].n_bins && b < p[d].first_bin + 8; ++b)
                {
                    std::cout << " [" << b << ":";
                    for (unsigned i = 0; i < m.hash_funs; ++i)
                        std::cout << " " << ((words[i * m.bin_words + (b >> 6)] >> (b & 63)) & 1);
                    std::cout << "]";
                }
                std::cout << "\n";
            }
        }
        uint64_t unnamed = 0;
        for (uint64_t u = 0; u < n_user; ++u)
            unnamed += !named[u];
        std::cout << "result\t" << (n_bad ? "FAIL" : "ok") << "\t" << n_checked << " target(s) checked, " << n_bad << " failing, " << unnamed
                  << " user bin(s) of the index not named by the input, " << looked_up << " distinct minimisers looked up, max_observed_fp ";
        if (fp_pass)
            std::cout << fp_max / P << ", mean_observed_fp " << (n_checked ? fp_sum / P / (double)n_checked : 0.0);
        else
            std::cout << "n/a, mean_observed_fp n/a";
        std::cout << std::endl;
        if (c.verbose && !c.quiet)
            std::cerr << std::setprecision(6) << " - seconds: hash " << hash_s << " load " << load_s << " membership " << member_s << " fp " << fp_s << std::endl;
        return n_bad == 0 && n_checked > 0;
    }
    catch (const std::exception& e)
    {
        return fail(std::string("ERROR: ") + e.what());
    }
}

// ---- --hibf --update -------------------------------------------------------------------------------------------------------------
// Adds the inputs' targets to an index without its genomes: the file into filter A, how full every bin is off A's bits
// (gn_filter_bin_popcounts), the placement (hibf_update.hpp), filter B with the new bins, every IBF moved over (gn_filter_copy_ibf),
// the new sets along their paths, B written with the file's own header fields and strings and the new names behind them.
bool run_update(const Config& c, std::vector<Target>& targets, const Lap& counting)
{
    auto fail = [](const std::string& m) {
        std::cerr << m << std::endl;
        return false;
    };
    auto since = [](std::chrono::steady_clock::time_point t) { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t).count(); };
    auto t0 = std::chrono::steady_clock::now();
    std::vector<uint32_t> fresh_target; // targets with a hash, in input order: new user bin n_user_old + position
    std::vector<uint64_t> fresh_counts;
    for (uint32_t t = 0; t < targets.size(); ++t)
    {
        if (targets[t].hashes.empty())
            continue;
        if (!unite_files(c, targets[t]))
            return fail(gn_last_error());
        fresh_target.push_back(t);
        fresh_counts.push_back(targets[t].hashes.size());
    }
    if (fresh_counts.empty())
        return fail("No valid sequences to build");
    const double hash_s = counting.seconds() + since(t0);
    gn_filter*   b_flt  = nullptr;
    try
    {
        {
            gnhost::FilterMeta names;
            gnhost::read_hibf_meta(c.update, names);
            const std::set<std::string> have(names.targets.begin(), names.targets.end());
            for (uint32_t t : fresh_target)
                if (have.count(name_as_read(targets[t].name)))
                    return fail("--update: target " + targets[t].name + " is already in the index (adding sequences to an existing user bin is not supported); nothing written");
        }
        t0 = std::chrono::steady_clock::now();
        gnhost::FilterMeta meta;
        auto               sink = std::make_unique<HibfDeviceSink>(c.device);
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
        const gnhibf::UpdatePlan plan = gnhibf::plan_update(bins, rows, meta.next_ibf_id, meta.bin_to_user, n_old, h, fpr, pop, fresh_counts);
        const uint32_t           depth = plan.paths.depth;
        const double             plan_s = since(t0);

        // filter B: the same rows, the new bins.  A and B are on the device together until every IBF is moved
        t0 = std::chrono::steady_clock::now();
        std::vector<HibfShape> ibfs(n_ibf);
        uint64_t               a_bytes = 0, b_bytes = 0;
        for (uint64_t i = 0; i < n_ibf; ++i)
        {
            ibfs[i].bins = plan.bins[i], ibfs[i].rows = rows[i];
            ibfs[i].next_ibf_id = plan.next_ibf_id[i], ibfs[i].bin_to_user = plan.bin_to_user[i];
            a_bytes += rows[i] * gn_hibf_row_stride_words((bins[i] + 63) >> 6) * 8;
            b_bytes += rows[i] * gn_hibf_row_stride_words((plan.bins[i] + 63) >> 6) * 8;
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
        {
            std::vector<gn_ibf_desc>    descs(n_ibf);
            std::vector<const int64_t*> nx(n_ibf), bu(n_ibf);
            for (uint64_t i = 0; i < n_ibf; ++i)
            {
                descs[i] = gn_ibf_desc{ nullptr, rows[i], (ibfs[i].bins + 63) >> 6, ibfs[i].bins, h, (uint32_t)__builtin_clzll(rows[i]) };
                nx[i] = ibfs[i].next_ibf_id.data(), bu[i] = ibfs[i].bin_to_user.data();
            }
            if (gn_filter_upload_hibf(c.device, (uint32_t)n_ibf, descs.data(), nx.data(), bu.data(), plan.n_user_bins, &b_flt) != GN_OK)
                throw std::runtime_error(gn_last_error());
        }
        for (uint64_t i = 0; i < n_ibf; ++i)
            if (gn_filter_copy_ibf(b_flt, (uint32_t)i, sink->filter(), (uint32_t)i) != GN_OK)
                throw std::runtime_error(gn_last_error());
        sink.reset(); // (frees A)
        const double copy_s = since(t0);

        // the new sets along their paths, pooled as run_hibf pools them
        t0 = std::chrono::steady_clock::now();
        {
            constexpr uint64_t         kBatch = 16ull << 20, kAlone = 4ull << 20;
            std::vector<uint64_t>      pool, off{ 0 };
            std::vector<gn_path_entry> pp;
            auto                       flush = [&] {
                if (off.size() > 1 && gn_filter_emplace_path(b_flt, pool.data(), off.data(), (uint32_t)off.size() - 1, pp.data(), depth) != GN_OK)
                    throw std::runtime_error(gn_last_error());
                pool.clear(), pp.clear(), off.assign(1, 0);
            };
            for (size_t j = 0; j < fresh_target.size(); ++j)
            {
                const std::vector<uint64_t>& hs = targets[fresh_target[j]].hashes;
                const gn_path_entry*         p  = &plan.paths.entries[j * depth];
                if (hs.size() >= kAlone)
                {
                    const uint64_t one[2] = { 0, hs.size() };
                    if (gn_filter_emplace_path(b_flt, hs.data(), one, 1, p, depth) != GN_OK)
                        throw std::runtime_error(gn_last_error());
                    continue;
                }
                pool.insert(pool.end(), hs.begin(), hs.end());
                off.push_back(pool.size());
                pp.insert(pp.end(), p, p + depth);
                if (pool.size() >= kBatch)
                    flush();
            }
            flush();
        }
        const double emplace_s = since(t0);

        // B's bit counts, for the IBFs the report speaks of: those that gained bins or lie on a new path
        t0 = std::chrono::steady_clock::now();
        std::vector<bool> shown(n_ibf, false);
        for (uint64_t i = 0; i < n_ibf; ++i)
            shown[i] = plan.bins[i] != bins[i];
        for (const gn_path_entry& e : plan.paths.entries)
            if (e.n_bins)
                shown[e.ibf] = true;
        std::vector<std::vector<uint64_t>> pop_b(n_ibf);
        for (uint64_t i = 0; i < n_ibf; ++i)
            if (shown[i])
            {
                pop_b[i].assign(plan.bins[i], 0);
                if (gn_filter_bin_popcounts(b_flt, (uint32_t)i, pop_b[i].data()) != GN_OK)
                    throw std::runtime_error(gn_last_error());
            }
        const double count_b_s = since(t0);

        // the file: its header fields and strings as they are, the new names behind them in the form run_hibf writes
        t0 = std::chrono::steady_clock::now();
        std::vector<std::vector<std::string>> bin_path   = meta.raw_bin_path;
        std::vector<std::string>              user_files = meta.raw_user_bin_filenames;
        const std::string dir = !c.tmp_output_folder.empty() ? c.tmp_output_folder
                                : fs::path(c.output_file).has_parent_path() ? fs::path(c.output_file).parent_path().string()
                                                                            : std::string(".");
        for (uint32_t t : fresh_target)
        {
            const std::string f = dir + "/" + user_bin_file_name(targets[t].name) + ".minimiser";
            bin_path.push_back({ f });
            user_files.push_back(f);
        }
        std::string err;
        const bool  saved = save_hibf(c, b_flt, ibfs, h, bin_path, user_files, err); // (c holds the file's k, w and fpr: validate())
        gn_filter_free(b_flt);
        b_flt = nullptr;
        if (!saved)
            return fail(err);
        const double write_s = since(t0);

        // the report
        const double bound_fill = std::pow(fpr, 1.0 / h);
        std::cout << "index\t" << c.update << "\t->\t" << c.output_file << "\tk=" << unsigned(c.kmer_size) << " w=" << c.window_size << " h=" << unsigned(h)
                  << " ibfs=" << n_ibf << " levels=" << depth << " user_bins=" << n_old << "->" << plan.n_user_bins << " fpr=" << fpr << "\n";
        std::cout << "#target\tuser_bin\tdistinct_hashes\tleaf_ibf\tfirst_bin\tbins\tdepth\tpath\n";
        uint64_t bins_added = 0;
        for (size_t j = 0; j < fresh_target.size(); ++j)
        {
            const gn_path_entry* p    = &plan.paths.entries[j * depth];
            uint32_t             used = 0;
            while (used < depth && p[used].n_bins)
                ++used;
            std::cout << "target\t" << targets[fresh_target[j]].name << "\t" << n_old + j << "\t" << fresh_counts[j] << "\t" << p[0].ibf << "\t" << p[0].first_bin << "\t"
                      << p[0].n_bins << "\t" << used << "\t";
            for (uint32_t d = used; d-- > 0;)
                std::cout << p[d].ibf << ":" << p[d].first_bin << (d ? " " : "");
            std::cout << "\n";
            bins_added += p[0].n_bins;
        }
        std::cout << "#ibf\trows\tbins_before\tbins_after\tmax_fill_before\tmax_fill_after\n" << std::fixed << std::setprecision(6);
        for (uint64_t i = 0; i < n_ibf; ++i)
            if (shown[i])
                std::cout << "ibf\t" << i << "\t" << rows[i] << "\t" << bins[i] << "\t" << plan.bins[i] << "\t"
                          << *std::max_element(pop[i].begin(), pop[i].end()) / (double)rows[i] << "\t"
                          << *std::max_element(pop_b[i].begin(), pop_b[i].end()) / (double)rows[i] << "\n";
        std::cout << "#merged\tibf\tbin\tbits_before\tbits_predicted\tbits_after\n";
        uint64_t fullest = 0, fullest_rows = 1;
        bool     any_touched = false;
        for (const gnhibf::UpdateTouched& t : plan.touched)
        {
            const uint64_t after = pop_b[t.ibf][t.bin];
            std::cout << "merged\t" << t.ibf << "\t" << t.bin << "\t" << t.bits_before << "\t" << std::setprecision(1) << t.bits_predicted << std::setprecision(6) << "\t"
                      << after << (after > bound_fill * rows[t.ibf] ? "\tWARN fill" : "") << "\n";
            if (!any_touched || after * (double)fullest_rows > fullest * (double)rows[t.ibf])
                fullest = after, fullest_rows = rows[t.ibf];
            any_touched = true;
        }
        std::error_code ec;
        std::cout << "result\tok\t" << fresh_target.size() << " user bin(s) added, " << bins_added << " bin(s) added, " << fs::file_size(c.update, ec) << " -> "
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
            std::cerr << std::setprecision(6) << " - seconds: hash " << hash_s << " load " << load_s << " count " << count_s + count_b_s << " plan " << plan_s << " copy " << copy_s
                      << " emplace " << emplace_s << " write " << write_s << std::endl;
        return true;
    }
    catch (const std::exception& e)
    {
        if (b_flt)
            gn_filter_free(b_flt);
        return fail(std::string("ERROR: ") + e.what());
    }
}

bool run(Config c)
{
    if (!validate(c))
        return false;
    if (c.verbose)
        print_config(c);
    Lap whole, counting, sizing, filling, writing;
    whole.start();

    int n_dev = 0;
    if (gn_device_count(&n_dev) != GN_OK || n_dev <= 0)
    {
        std::cerr << "no usable MI355X/HIP device (" << gn_last_error() << "); ganon-build has no CPU fallback" << std::endl;
        return false;
    }
    if (c.device >= n_dev)
    {
        std::cerr << "--device " << c.device << " does not exist (" << n_dev << " visible)" << std::endl;
        return false;
    }

    Totals              totals;
    std::vector<Target> targets = read_input_file(c, totals);
    if (targets.empty())
    {
        std::cerr << "No valid input files" << std::endl;
        return false;
    }

    counting.start();
    {
        // every hasher page-locks 64 MiB and owns a device stream with GBs of hash and sort buffers: --threads (the wrapper
        // forwards 64 or 128 gladly) buys parser threads only up to what eight such streams keep busy
        const unsigned           nt = std::max<unsigned>(1, std::min<unsigned>(std::min<unsigned>(c.threads, 8u), (unsigned)targets.size()));
        std::vector<Totals>      per(nt);
        std::vector<std::thread> th;
        std::atomic<size_t>      next{ 0 };
        std::string              fatal;
        std::mutex               log_mutex;
        for (unsigned i = 0; i < nt; ++i)
            th.emplace_back(hash_targets, std::cref(c), std::ref(targets), std::ref(next), std::ref(per[i]), std::ref(fatal),
                            std::ref(log_mutex));
        for (auto& t : th)
            t.join();
        if (!fatal.empty())
        {
            std::cerr << fatal << std::endl;
            return false;
        }
        for (const Totals& t : per)
        {
            totals.sequences += t.sequences;
            totals.skipped_sequences += t.skipped_sequences;
            totals.length_bp += t.length_bp;
        }
    }
    counting.stop();

    if (c.verify_given)
        return run_verify(c, targets, counting);
    if (c.update_given)
        return run_update(c, targets, counting);
    if (c.hibf)
        return run_hibf(c, targets, totals, whole, counting);

    sizing.start();
    IbfParams p;
    p.kmer_size   = c.kmer_size;
    p.window_size = c.window_size;
    std::vector<uint64_t> counts;
    for (const Target& t : targets)
        counts.push_back(t.hashes.size());
    gnbuild::choose_capacity(c.max_fp, c.filter_size, counts, c.hash_functions, c.mode, p);
    if (p.n_bins != 0)
        gnbuild::true_fp(counts, p);
    sizing.stop();

    if (c.verbose) // :793-802
    {
        const char* sep = "----------------------------------------------------------------------";
        std::cerr << "ibf_config:" << '\n'
                  << "n_bins         " << p.n_bins << '\n'
                  << "max_hashes_bin " << p.max_hashes_bin << '\n'
                  << "hash_functions " << unsigned(p.hash_functions) << '\n'
                  << "kmer_size      " << unsigned(p.kmer_size) << '\n'
                  << "window_size    " << p.window_size << '\n'
                  << "bin_size_bits  " << p.bin_size_bits << '\n'
                  << "max_fp         " << p.max_fp << '\n'
                  << "true_max_fp    " << p.true_max_fp << '\n'
                  << "true_avg_fp    " << p.true_avg_fp << '\n'
                  << sep << '\n';
        std::cerr << "Filter size: " << (gnbuild::padded_bins(p.n_bins) * p.bin_size_bits) << " Bits";
        std::cerr << " (" << (gnbuild::padded_bins(p.n_bins) * p.bin_size_bits) / static_cast<double>(8388608u) << " Megabytes)"
                  << std::endl;
    }
    if (p.n_bins == 0)
    {
        std::cerr << "No valid sequences to build" << std::endl;
        return false;
    }

    std::vector<uint64_t>             shares;
    const std::vector<gnbuild::BinSpan> bins = gnbuild::lay_out_bins(p, counts, &shares);
    if (bins.size() != p.n_bins)
    {
        std::cerr << "internal error: " << bins.size() << " bins laid out, " << p.n_bins << " expected" << std::endl;
        return false;
    }

    if (p.bin_size_bits == 0 || p.hash_functions < 1 || p.hash_functions > 5)
    {
        // (the reference fails in the seqan3 IBF constructor: "The size of a bin must be > 0" / "hash functions must be > 0 and <= 5")
        std::cerr << "ERROR: the parameters leave a filter of " << p.bin_size_bits << " bits per bin with " << (unsigned)p.hash_functions
                  << " hash function(s): --filter-size / --max-fp do not fit " << targets.size() << " target(s)" << std::endl;
        return false;
    }
    filling.start();
    gn_filter*  flt = nullptr;
    gn_ibf_desc d{};
    d.bins = p.n_bins, d.bin_words = (p.n_bins + 63) >> 6, d.bin_size = p.bin_size_bits, d.hash_funs = p.hash_functions, d.rows = nullptr;
    d.hash_shift = (uint32_t)__builtin_clzll(p.bin_size_bits);
    if (gn_filter_upload_ibf(c.device, &d, nullptr, 0, &flt) != GN_OK) // storage only: no bin map
    {
        std::cerr << gn_last_error() << std::endl;
        return false;
    }
    {
        uint32_t first_bin = 0;
        for (size_t t = 0; t < targets.size(); ++t)
        {
            const uint64_t n = targets[t].hashes.size();
            if (n == 0)
                continue;
            if (gn_filter_emplace_split(flt, targets[t].hashes.data(), n, first_bin, shares[t]) != GN_OK)
            {
                std::cerr << gn_last_error() << std::endl;
                gn_filter_free(flt);
                return false;
            }
            first_bin += (uint32_t)((n + shares[t] - 1) / shares[t]);
        }
    }
    filling.stop();

    writing.start();
    std::string err;
    const bool  saved = save_filter(c, flt, p, targets, bins, err);
    gn_filter_free(flt);
    if (!saved)
    {
        std::cerr << err << std::endl;
        return false;
    }
    writing.stop();
    whole.stop();

    if (!c.quiet)
    {
        if (c.verbose) // print_stats_verbose (:730-757)
        {
            auto block = [](const char* a, const char* pad, const Lap& l) {
                std::cerr << a << stamp(l.b) << '\n' << pad << "    end: " << stamp(l.e) << '\n' << pad << "elapsed (s): " << l.seconds() << '\n';
            };
            block("Count/save hashes start: ", "                ", counting);
            block("Estimate params   start: ", "                ", sizing);
            block("Building filter   start: ", "                ", filling);
            block("Saving filer      start: ", "                ", writing);
            block("ganon-build       start: ", "                ", whole);
            std::cerr << std::endl;
        }
        const double elapsed = whole.seconds(); // print_stats (:706-728)
        std::cerr << "ganon-build processed " << totals.sequences << " sequences / " << totals.files << " files ("
                  << totals.length_bp / 1000000.0 << " Mbp) in " << elapsed << " seconds ("
                  << (totals.length_bp / 1000000.0) / (elapsed / 60.0) << " Mbp/m)" << std::endl;
        if (totals.invalid_files > 0)
            std::cerr << " - " << totals.invalid_files << " invalid files skipped" << std::endl;
        if (totals.skipped_sequences > 0)
            std::cerr << " - " << totals.skipped_sequences << " sequences skipped" << std::endl;
        std::cerr << std::fixed << std::setprecision(4) << " - max. false positive: " << p.true_max_fp;
        std::cerr << std::fixed << std::setprecision(4) << " (avg.: " << p.true_avg_fp << ")" << std::endl;
        std::cerr << std::fixed << std::setprecision(2)
                  << " - filter size: " << (gnbuild::padded_bins(p.n_bins) * p.bin_size_bits) / static_cast<double>(8388608u) << "MB"
                  << std::endl;
    }
    return true;
}

} // namespace

int main(int argc, char** argv)
{
    gnhost::HostTunables::init();
    Config    c;
    const int r = parse_args(argc, argv, c);
    if (r == 1)
        return EXIT_SUCCESS;
    if (r == 2)
        return EXIT_FAILURE;
    return run(c) ? EXIT_SUCCESS : EXIT_FAILURE;
}
