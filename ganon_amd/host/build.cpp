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
// (gn_filter_emplace_runs_window) and streamed to the file -- whole when it fits what a device may hold, otherwise in slabs of rows
// over the entries of --device (build_slabs.cpp).  The host parses FASTA (with --parse device the text travels and the device finds the
// records and cuts the pieces, csrc/gn_genome.hip; the host reader stays the fallback), keeps the hash sets and does the sizing arithmetic.  The sets
// are held in RAM at 8 bytes a hash (--hash-sets raw, the default; not `.min` files), or packed by the device as deltas of fixed width
// (csrc/gn_packed_set.h) in RAM (packed) or in files of --tmp-output-folder that live as long as the command (spilled).
// There is no CPU implementation of the hashing or the filter: without a HIP device the program fails.
//
// The hierarchical modes (this project's extensions, like --device) take the same hash sets: --hibf (build_hibf.cpp; with --hibf-hash-sets
// packed|spilled it takes them packed, from the same arenas),
// --hibf --verify-index (build_verify.cpp; in parts build_verify_parts.cpp), --hibf --update (build_update.cpp).  The files are written by build_write.cpp.
//
// Differences from the reference that cannot be avoided here: targets are laid out in the order of
// their first appearance in the input file and a target's hashes in ascending order -- the reference uses the iteration
// order of robin_hood maps/sets, which is not reproducible without that library; which bin of a split target holds
// which hash therefore differs, the set of hashes per target, the sizing and every IBFConfig value do not.
// Sequences shorter than the window (but at least one k-mer long) yield the minimum over all their k-mers, which is what
// seqan3::views::minimiser does when the range is shorter than its window (recollection of SeqAn3 3.3.0, unpinned).
#include "build_common.hpp"
#include "filter_io.hpp"
#include "hasher.hpp"
#include "hostmem.hpp"
#include "seq_io.hpp"
#include "tunables.hpp"

#include <algorithm>
#include <atomic>
#include <fstream>
#include <iomanip>
#include <map>
#include <memory>
#include <mutex>
#include <set>
#include <sstream>
#include <thread>
#include <unistd.h>

using namespace gnbuild;

namespace
{

constexpr const char* kVersion = "2.1.1-mi355x"; // as ganon-classify of this build (config.hpp)

// k, w and the number of hash functions -- for --update the false-positive rate as well -- are those of the index `opt` names; a
// value given on the command line has to agree.  Num: how the two values of a refusal are printed (--update prints doubles)
template <typename Num>
bool take_from_index(Config& c, const char* opt, const std::string& path, bool with_fp)
{
    try
    {
        gnhost::FilterMeta meta;
        gnhost::read_hibf_meta(path, meta);
        const unsigned k = meta.ibf_config.kmer_size, w = meta.ibf_config.window_size, h = (unsigned)meta.shapes.at(0).hash_funs;
        const double   fpr = meta.ibf_config.max_fp;
        auto differs = [&](const char* what, Num given, Num file) {
            if (!c.quiet)
                std::cerr << opt << ": " << what << " " << given << " differs from the index, which was built with " << file << std::endl;
            return false;
        };
        if (c.kmer_given && c.kmer_size != k)
            return differs("--kmer-size", c.kmer_size, k);
        if (c.window_given && c.window_size != w)
            return differs("--window-size", c.window_size, w);
        if (c.hashes_given && c.hash_functions != h)
            return differs("--hash-functions", c.hash_functions, h);
        if (with_fp && c.max_fp_given && c.max_fp != fpr)
            return differs("--max-fp", (Num)c.max_fp, (Num)fpr);
        c.kmer_size = (uint8_t)k, c.window_size = (uint16_t)w, c.hash_functions = (uint8_t)h;
        if (with_fp)
            c.max_fp = fpr;
        return true;
    }
    catch (const std::exception& e)
    {
        if (!c.quiet)
            std::cerr << opt << ": " << e.what() << std::endl;
        return false;
    }
}

bool parse_mode_ok(const Config& c)
{
    return c.parse == "host" || c.parse == "device";
}

bool validate(Config& c) // Config.hpp:29-107, same messages
{
    auto say = [&](const std::string& m) {
        if (!c.quiet)
            std::cerr << m << std::endl;
        return false;
    };
    // a build in row slabs or over several devices is the flat build's: refused here, before any device call
    for (const auto& [on, mode] : { std::pair<bool, const char*>{ c.update_given, "--update" }, { c.verify_given, "--verify-index" }, { c.hibf, "--hibf" } })
    {
        if (on && c.device_memory_given)
            return say(std::string("--device-memory cannot be used with ") + mode + " (only a flat .ibf is built in row slabs)");
        if (on && c.devices.size() > 1)
            return say(std::string("--device takes one device with ") + mode + " (only a flat .ibf is built over a device list)");
    }
    if (c.hash_sets != "raw" && c.hash_sets != "packed" && c.hash_sets != "spilled")
        return say("--hash-sets has to be raw, packed or spilled");
    for (const auto& [on, mode] : { std::pair<bool, const char*>{ c.update_given, "--update" }, { c.verify_given, "--verify-index" }, { c.hibf, "--hibf" } })
        if (on && c.hash_sets != "raw")
            return say(std::string("--hash-sets ") + c.hash_sets + " cannot be used with " + mode + " (unions, sketches and probes read raw sets; only a flat .ibf is built from packed ones)" +
                       (c.update_given || c.verify_given ? "" : "; use --hibf-hash-sets"));
    // the hierarchical build keeps packed sets by a switch of its own (its unions, sketches and insert have packed twins; the probes and
    // deals of --update and --verify-index read raw sets)
    if (c.hibf_hash_sets != "raw" && c.hibf_hash_sets != "packed" && c.hibf_hash_sets != "spilled")
        return say("--hibf-hash-sets has to be raw, packed or spilled");
    if (c.hibf_hash_sets_given && !c.hibf)
        return say("--hibf-hash-sets needs --hibf (a flat .ibf is built from packed sets with --hash-sets)");
    for (const auto& [on, mode] : { std::pair<bool, const char*>{ c.update_given, "--update" }, { c.verify_given, "--verify-index" } })
        if (on && c.hibf_hash_sets_given)
            return say(std::string("--hibf-hash-sets ") + c.hibf_hash_sets + " cannot be used with " + mode + " (its probes and deals read raw sets)");
    if (!parse_mode_ok(c))
        return say("--parse has to be host or device");
    if (c.device_memory_given && c.device_memory == 0)
        return say("--device-memory has to be > 0");
    // the hierarchical build in parts has switches of its own (a tree is cut by IBF and by padded device rows, not by file rows)
    for (const auto& [given, name] : { std::pair<bool, const char*>{ c.hibf_memory_given, "--hibf-memory" }, { c.hibf_devices_given, "--hibf-devices" } })
    {
        if (given && !c.hibf)
            return say(std::string(name) + " needs --hibf (a flat .ibf is built in row slabs with --device-memory and a --device list)");
        if (given && c.update_given)
            return say(std::string(name) + " cannot be used with --update (an index is updated on one device)");
        if (given && c.verify_given)
            return say(std::string(name) + " cannot be used with --verify-index (an index is checked on one device)");
    }
    if (c.hibf_memory_given && c.hibf_memory == 0)
        return say("--hibf-memory has to be > 0");
    // ... and so has the check of an index in parts (--hibf-memory and --hibf-devices stay the build's)
    for (const auto& [given, name] : { std::pair<bool, const char*>{ c.verify_memory_given, "--verify-memory" }, { c.verify_devices_given, "--verify-devices" } })
        if (given && !c.verify_given)
            return say(std::string(name) + " needs --verify-index (it says in what parts an index is checked; a build in parts takes --hibf-memory and --hibf-devices)");
    if (c.verify_memory_given && c.verify_memory == 0)
        return say("--verify-memory has to be > 0");
    if (c.tmax_given && !c.hibf)
        return say("--tmax needs --hibf");
    if (c.layout_given && !c.hibf)
        return say("--layout needs --hibf");
    if (c.layout_given && c.layout != "rule" && c.layout != "sketch" && c.layout != "similarity")
        return say("--layout has to be rule, sketch or similarity");
    if (c.extend && !c.update_given)
        return say("--extend needs --update (it adds the inputs' sequences to targets of the index --update names)");
    if (c.remove_given && !c.update_given)
        return say("--remove needs --update (it takes targets out of the index --update names)");
    if (c.fold_given && c.verify_given)
        return say("--fold cannot be used with --verify-index (fold first, then check the file written)");
    if (c.fold_given && !c.update_given)
        return say("--fold needs --update (it holds the IBFs of the index --update names to a number of bins)");
    if (c.fold_given && c.fold < 2)
        return say("--fold has to be >= 2");
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
            return say("--update not found: " + c.update);
        if (c.remove_given && (c.remove.empty() || !fs::is_regular_file(c.remove)))
            return say("--remove not found: " + c.remove);
        {
            std::error_code ec;
            if (fs::exists(c.output_file) && fs::equivalent(c.update, c.output_file, ec))
                return say("--update: --output-file is the index itself (it is read while the new one is written: give another file)");
        }
        if (!take_from_index<double>(c, "--update", c.update, true))
            return false;
    }
    if (c.verify_given)
    {
        if (!c.hibf)
            return say("--verify-index needs --hibf (it checks a hierarchical index; a flat .ibf is checked by ganon-classify --verify-filter)");
        if (c.output_given)
            return say("--verify-index cannot be used with --output-file (nothing is built and nothing is written)");
        if (c.verify_index.empty() || !fs::exists(c.verify_index))
            return say("--verify-index not found: " + c.verify_index);
        if (!take_from_index<unsigned>(c, "--verify-index", c.verify_index, false))
            return false;
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
    const bool remove_only = (c.remove_given || c.fold_given) && c.input_file.empty(); // (without inputs: targets leave or move, none comes)
    if (c.input_file.empty() && !remove_only)
        return say("--input-file is mandatory");
    if (!remove_only && !fs::exists(c.input_file))
        return say("--input-file not found: " + c.input_file);
    if (!remove_only && fs::file_size(c.input_file) == 0)
        return say("--input-file is empty: " + c.input_file);
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
    if (c.devices.size() > 1)
    {
        std::cerr << "--device            ";
        for (size_t i = 0; i < c.devices.size(); ++i)
            std::cerr << (i ? "," : "") << c.devices[i];
        std::cerr << '\n';
    }
    if (c.device_memory_given)
        std::cerr << "--device-memory     " << c.device_memory << '\n';
    if (c.hash_sets != "raw")
        std::cerr << "--hash-sets         " << c.hash_sets << '\n';
    if (c.hibf)
        std::cerr << "--hibf              " << c.hibf << '\n' << "--tmax              " << c.tmax << '\n';
    if (c.hibf_hash_sets_given)
        std::cerr << "--hibf-hash-sets    " << c.hibf_hash_sets << '\n';
    if (c.parse != "host")
        std::cerr << "--parse             " << c.parse << '\n';
    if (c.hibf_memory_given)
        std::cerr << "--hibf-memory       " << c.hibf_memory << '\n';
    if (c.hibf_devices_given)
    {
        std::cerr << "--hibf-devices      ";
        for (size_t i = 0; i < c.hibf_devices.size(); ++i)
            std::cerr << (i ? "," : "") << c.hibf_devices[i];
        std::cerr << '\n';
    }
    if (c.layout_given)
        std::cerr << "--layout            " << c.layout << '\n';
    if (c.verify_given)
        std::cerr << "--verify-index      " << c.verify_index << '\n';
    if (c.verify_memory_given)
        std::cerr << "--verify-memory     " << c.verify_memory << '\n';
    if (c.verify_devices_given)
    {
        std::cerr << "--verify-devices    ";
        for (size_t i = 0; i < c.verify_devices.size(); ++i)
            std::cerr << (i ? "," : "") << c.verify_devices[i];
        std::cerr << '\n';
    }
    if (c.update_given)
        std::cerr << "--update            " << c.update << '\n';
    if (c.extend)
        std::cerr << "--extend            " << c.extend << '\n';
    if (c.remove_given)
        std::cerr << "--remove            " << c.remove << '\n';
    if (c.fold_given)
        std::cerr << "--fold              " << c.fold << '\n';
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
    "  -m, --tmp-output-folder arg  Folder to write temporary files (only --hash-sets spilled writes there; otherwise the hashes\n"
    "                               stay in memory)\n"
    "  -t, --threads arg            Number of threads (parser threads, one device stream each)\n"
    "      --device arg             HIP device index. Default: 0.  A list a,b,... (an index may repeat) deals the row slabs of a flat\n"
    "                               filter to its entries, one worker each, and the hashing threads to the devices; not with --hibf\n"
    "      --device-memory arg      most bytes of filter rows held on an entry of --device at one time.  A flat filter larger than\n"
    "                               that is filled in slabs of rows, each one more pass over the hash sets (which stay in host\n"
    "                               memory), and written slab by slab: the same file.  Default: what the device has free when\n"
    "                               filling starts, less staging and a reserve, shared among the entries that name it; not with --hibf\n"
    "      --hash-sets arg          how a flat build keeps the targets' hash sets between hashing and filling: raw (8 bytes a hash in\n"
    "                               host memory), packed (deltas of fixed width in blocks of 512 hashes, packed by the device where\n"
    "                               a set is born and decoded inside the insert; in host memory) or spilled (packed, in one file per\n"
    "                               hashing thread in --tmp-output-folder, else the output's folder: appended to while hashing,\n"
    "                               mapped for the passes, removed when the command ends).  The same file.  Default: raw; not with\n"
    "                               --hibf, --update or --verify-index\n"
    "      --parse arg              who finds the records of the input genomes: host (the sequential reader, on the hashing threads) or\n"
    "                               device (a FASTA file, plain or .gz, travels as text in large chunks and is tokenised and cut into\n"
    "                               pieces there; .bz2, blocked gzip and FASTQ names stay with the host reader, and so does any file\n"
    "                               the device does not take whole: an illegal letter, a missing header, a record cut too short --\n"
    "                               it is read again from its start, so messages, totals and the file written are those of host).\n"
    "                               Applies wherever inputs are hashed: the flat build, --hibf, --update, --verify-index.  Default:\n"
    "                               host.  $GANON_BUILD_PARSE_CHUNK: bytes of text per device chunk (default: what fills a batch)\n"
    "      --hibf                   Write a hierarchical filter (raptor 3.0.1 index, one user bin per target) sized from\n"
    "                               --max-fp; --hash-functions 0 means 4. Not with --filter-size or a --mode other than avg\n"
    "      --tmax arg               [--hibf] most technical bins of one IBF of the tree (>= 2).\n"
    "                               Default: ceil(sqrt(targets) / 64) * 64\n"
    "      --hibf-memory arg        [--hibf] most device bytes of IBF rows held on an entry of --hibf-devices at one time (rows as the\n"
    "                               device pads them, not as the file holds them).  A tree larger than that is filled in parts --\n"
    "                               whole IBFs grouped in file order, an IBF over the budget in slabs of rows -- each from the\n"
    "                               hash sets that reach it (which stay in host memory), and written part by part: the same file.\n"
    "                               Default: what the device has free when filling starts, less staging and a reserve, shared\n"
    "                               among the entries that name it.  Not with --update or --verify-index\n"
    "      --hibf-devices arg       [--hibf] a list a,b,... (an index may repeat): the parts are dealt to its entries, one worker\n"
    "                               each.  Default: the single --device, where hashing, unions and sketches stay.  Two families of\n"
    "                               switches because --device-memory counts file rows of one matrix and a --device list also deals\n"
    "                               the hashing threads; with --hibf both stay refused.  Not with --update or --verify-index\n"
    "      --hibf-hash-sets arg     [--hibf] how the hierarchical build keeps the targets' hash sets: raw, packed or spilled, as\n"
    "                               --hash-sets keeps a flat build's.  Packed sets stay packed from hashing to the insert: a target\n"
    "                               of several files is united on the packed bytes (into one more arena, or one more file\n"
    "                               <output>.hashsets.<pid>.united), the sketches and the merged bins' sizes are taken from them, and\n"
    "                               the insert decodes a block in registers.  The same file.  Two families here too: --hash-sets\n"
    "                               stays refused with --hibf.  Default: raw.  Not with --update or --verify-index\n"
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
    "      --verify-memory arg      [--verify-index] most device bytes of IBF rows held on an entry of --verify-devices at one time\n"
    "                               (rows as the device pads them).  An index larger than that is checked in parts -- whole IBFs\n"
    "                               grouped in file order, an IBF over the budget in slabs of rows -- and what a hash's rows in\n"
    "                               other parts said is carried along in host memory: the same report.  Default: what the device\n"
    "                               has free when loading starts, less staging and a reserve, shared among the entries that name it\n"
    "      --verify-devices arg     [--verify-index] a list a,b,... (an index may repeat): the parts are dealt to its entries, one\n"
    "                               worker each.  Default: the single --device\n"
    "      --update arg             [--hibf] add the targets of --input-file to the index `arg` and write the result to\n"
    "                               --output-file; `arg` is left as it is.  The old genomes are not needed: how full every bin is\n"
    "                               is read off the index's bits.  The tree is kept: a new target goes below a merged bin that\n"
    "                               has room for it, otherwise it widens the IBF it reached (the root at worst) -- no IBF is\n"
    "                               created or resized in its rows, and --tmax does not bound an updated IBF; the report says\n"
    "                               how many bins each IBF gained, so that one sees when a rebuild is due.  k, w, the hash\n"
    "                               functions and the false-positive rate come from the index.  A target the index holds\n"
    "                               already is refused.  Not with --verify-index, --layout, --tmax, --filter-size, --mode\n"
    "      --extend                 [--update] a target whose name the index holds once is not refused: its user bin gains the\n"
    "                               hashes of the target's input files that it does not hold yet, dealt to the bins of its run by\n"
    "                               how full the bits show them; the merged bins above take all of them.  A run is never moved or\n"
    "                               widened: when a bin is predicted over its bound nothing is written and the targets are named\n"
    "                               (leave them out or rebuild).  Unknown names are added as new targets, as without the flag\n"
    "      --remove arg             [--update] take targets out of the index: `arg` is a file of target names, one per line, as in\n"
    "                               column 2 of an input file (empty lines and repeats are ignored).  The removed user bins'\n"
    "                               technical bins are dropped, the bins behind them move left, user bins and IBFs are renumbered,\n"
    "                               and an IBF left without a bin goes together with the merged bin that led to it; the file written\n"
    "                               is an ordinary index.  --input-file may then be left out.  A name in both --remove and\n"
    "                               --input-file is REPLACED: its old user bin goes, the input's sequences enter as a new one.  A\n"
    "                               name the index does not hold, or the removal of every target, ends the command with nothing\n"
    "                               written.  Merged bins above a removed target keep its hashes (`stale` lines of the report say\n"
    "                               how many, estimated); rows never shrink\n"
    "      --fold arg               [--update] hold every IBF of the updated index to `arg` bins (>= 2) without the genomes: runs of\n"
    "                               user bins of a wider IBF, the emptiest first, move into new IBFs one level down, and one merged\n"
    "                               bin per group -- the OR of the group's columns -- stays behind.  User bins, names and columns are\n"
    "                               unchanged; a folded target is found one level deeper.  Merged bins are not folded, a new IBF has\n"
    "                               its parent's rows, and one level is added per command: an IBF that cannot reach `arg` this way\n"
    "                               ends the command with nothing written (rebuild or give a larger --fold).  --input-file may\n"
    "                               then be left out.  Not with --verify-index\n"
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
        if (a == "--help" || a == "--version" || a == "--verbose" || a == "--quiet" || a == "--hibf" || a == "--extend")
        {
            vals[a] = has ? v : "true";
            continue;
        }
        static const std::set<std::string> known = { "--input-file", "--output-file", "--kmer-size", "--window-size",
                                                     "--hash-functions", "--max-fp", "--filter-size", "--mode", "--min-length",
                                                     "--tmp-output-folder", "--threads", "--device", "--device-memory", "--hash-sets", "--hibf-hash-sets", "--parse", "--hibf-memory", "--hibf-devices", "--tmax", "--layout", "--verify-index", "--verify-memory", "--verify-devices", "--update", "--remove", "--fold" };
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
        if (vals.count("--remove"))
            c.remove = vals["--remove"], c.remove_given = true;
        if (vals.count("--fold"))
            c.fold = u("--fold", 0xFFFFFFFFull), c.fold_given = true;
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
        auto device_list = [&](const char* k) { // one index, or a list a,b,...
            std::vector<int>   out;
            std::istringstream list(vals[k]);
            for (std::string e; std::getline(list, e, ',');)
            {
                size_t pos = 0;
                if (e.empty() || e[0] == '-' || e[0] == '+')
                    throw std::invalid_argument(k);
                const uint64_t x = std::stoull(e, &pos);
                if (pos != e.size() || x > (1u << 20))
                    throw std::invalid_argument(k);
                out.push_back((int)x);
            }
            if (out.empty() || vals[k].back() == ',')
                throw std::invalid_argument(k);
            return out;
        };
        if (vals.count("--device"))
            c.devices = device_list("--device"), c.device = c.devices[0];
        if (vals.count("--device-memory"))
            c.device_memory = u("--device-memory", ~0ull), c.device_memory_given = true;
        if (vals.count("--hash-sets"))
            c.hash_sets = vals["--hash-sets"];
        if (vals.count("--hibf-hash-sets"))
            c.hibf_hash_sets = vals["--hibf-hash-sets"], c.hibf_hash_sets_given = true;
        if (vals.count("--parse"))
            c.parse = vals["--parse"];
        if (vals.count("--hibf-devices"))
            c.hibf_devices = device_list("--hibf-devices"), c.hibf_devices_given = true;
        if (vals.count("--hibf-memory"))
            c.hibf_memory = u("--hibf-memory", ~0ull), c.hibf_memory_given = true;
        if (vals.count("--verify-devices"))
            c.verify_devices = device_list("--verify-devices"), c.verify_devices_given = true;
        if (vals.count("--verify-memory"))
            c.verify_memory = u("--verify-memory", ~0ull), c.verify_memory_given = true;
        c.verbose = vals.count("--verbose") && vals["--verbose"] != "false";
        c.quiet   = vals.count("--quiet") && vals["--quiet"] != "false";
        c.extend  = vals.count("--extend") && vals["--extend"] != "false";
    }
    catch (const std::exception& e)
    {
        std::cerr << "Argument '" << e.what() << "' failed to parse" << std::endl;
        return 2;
    }
    return 0;
}

// the process's anonymous resident memory as /proc/self/status gives it (0 where it does not)
uint64_t rss_anon_kb()
{
    std::ifstream in("/proc/self/status");
    for (std::string line; std::getline(in, line);)
        if (line.rfind("RssAnon:", 0) == 0)
            return std::stoull(line.substr(8));
    return 0;
}

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

// --parse device, over all hashing threads: files tokenised on the device, files it did not take whole (read again by the host reader),
// files that never travel as text (.bz2, blocked gzip, FASTQ names), text bytes uploaded
struct ParseCounters
{
    std::atomic<uint64_t> device{ 0 }, fell_back{ 0 }, host_only{ 0 }, bytes{ 0 };
} g_parse;

// count_hashes (:184-249) for the targets this thread draws from the shared cursor
// (arena: --hash-sets / --hibf-hash-sets packed|spilled -- this thread's, number arena_no; the files' sets are packed and their payload goes there)
void hash_targets(const Config& c, int device, std::vector<Target>& targets, std::atomic<size_t>& next, Totals& totals, std::string& fatal,
                  std::mutex& log_mutex, SetArena* arena, uint32_t arena_no)
{
    try
    {
        gnhost::Hasher    hasher(device, c.kmer_size, c.window_size);
        std::string       ids;
        gnhost::ByteBuf   seq;
        gnhost::PackedFile packed;
        for (;;)
        {
            const size_t t = next.fetch_add(1);
            if (t >= targets.size())
                break;
            Target& tg = targets[t];
            tg.arena   = arena_no;
            for (const std::string& file : tg.files)
            {
                if (arena)
                    packed.clear();
                std::vector<uint64_t> file_hashes;
                unsigned              flushes = 0;
                // --parse device: the file's text goes to the device; the totals of a file are committed only when it finished there,
                // and a file the device does not take whole is read again from its start by the sequential reader, as with --parse host
                bool on_device = false;
                if (c.parse == "device")
                {
                    gnhost::Hasher::TextTotals tt;
                    if (!gnhost::genome_text_eligible(file))
                        g_parse.host_only++;
                    else if (arena ? hasher.hash_text_file(file, c.min_length, packed, tt) : hasher.hash_text_file(file, c.min_length, file_hashes, flushes, tt))
                    {
                        on_device = true;
                        totals.sequences += tt.sequences;
                        totals.skipped_sequences += tt.skipped;
                        totals.length_bp += tt.length_bp;
                        g_parse.device++;
                        g_parse.bytes += tt.bytes;
                    }
                    else
                    {
                        g_parse.fell_back++;
                        hasher.discard();
                        packed.clear();
                        file_hashes.clear();
                        flushes = 0;
                    }
                }
                try
                {
                    for (std::unique_ptr<gnhost::SeqReader> reader(on_device ? nullptr : new gnhost::SeqReader(file)); reader;)
                    {
                        ids.clear();
                        seq.clear();
                        if (!reader->next(ids, seq))
                            break;
                        if (seq.size() < c.min_length)
                        {
                            totals.skipped_sequences++;
                            continue;
                        }
                        totals.sequences++;
                        totals.length_bp += seq.size();
                        if (arena)
                            hasher.add(seq.data(), seq.size(), packed);
                        else
                            hasher.add(seq.data(), seq.size(), file_hashes, flushes);
                    }
                    if (arena)
                        hasher.flush(packed), hasher.flush_short(packed);
                    else
                    {
                        hasher.flush(file_hashes, flushes);
                        hasher.flush_short(file_hashes, flushes);
                    }
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
                if (arena) // the file's blocks behind the target's, its payload behind the arena's words
                {
                    packed.finish();
                    const uint64_t base = arena->words();
                    arena->append(packed.payload.data(), packed.payload.size());
                    for (GnPackedBlock b : packed.blocks)
                        b.word_at += base, tg.blocks.push_back(b);
                    tg.count += packed.hashes;
                    tg.file_ends.push_back(tg.count);
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
        return fail(std::string("no usable MI355X/HIP device (") + gn_last_error() + "); ganon-build has no CPU fallback");
    for (int d : c.devices)
        if (d >= n_dev)
            return fail("--device " + std::to_string(d) + " does not exist (" + std::to_string(n_dev) + " visible)");
    for (int d : c.hibf_devices)
        if (d >= n_dev)
            return fail("--hibf-devices " + std::to_string(d) + " does not exist (" + std::to_string(n_dev) + " visible)");
    for (int d : c.verify_devices)
        if (d >= n_dev)
            return fail("--verify-devices " + std::to_string(d) + " does not exist (" + std::to_string(n_dev) + " visible)");

    Totals              totals;
    const bool          remove_only = (c.remove_given || c.fold_given) && c.input_file.empty();
    std::vector<Target> targets;
    if (!remove_only)
        targets = read_input_file(c, totals);
    if (targets.empty() && !remove_only)
        return fail("No valid input files");

    // --hash-sets packed|spilled, and --hibf-hash-sets with --hibf: one arena per hashing thread; they live until the command ends (a
    // spilled one's file goes with it)
    const std::string&                     sets_mode   = c.hibf ? c.hibf_hash_sets : c.hash_sets;
    const bool                             packed_sets = sets_mode != "raw";
    std::vector<std::unique_ptr<SetArena>> arenas;

    counting.start();
    if (!targets.empty())
    {
        // every hasher page-locks 64 MiB and owns a device stream with GBs of hash and sort buffers: --threads (the wrapper
        // forwards 64 or 128 gladly) buys parser threads only up to what eight such streams keep busy
        const unsigned           nt = std::max<unsigned>(1, std::min<unsigned>(std::min<unsigned>(c.threads, 8u), (unsigned)targets.size()));
        std::vector<Totals>      per(nt);
        std::vector<std::thread> th;
        std::atomic<size_t>      next{ 0 };
        std::string              fatal;
        std::mutex               log_mutex;
        try
        {
            for (unsigned i = 0; packed_sets && i < nt; ++i)
                arenas.emplace_back(sets_mode == "spilled" ? new SetArena((fs::path(output_folder(c)) / (fs::path(c.output_file).filename().string() + ".hashsets." +
                                                                                                         std::to_string(::getpid()) + "." + std::to_string(i) + ".tmp"))
                                                                                .string())
                                                             : new SetArena());
        }
        catch (const std::exception& e)
        {
            return fail(e.what());
        }
        for (unsigned i = 0; i < nt; ++i)
            th.emplace_back(hash_targets, std::cref(c), c.devices[i % c.devices.size()], std::ref(targets), std::ref(next), std::ref(per[i]), std::ref(fatal),
                            std::ref(log_mutex), packed_sets ? arenas[i].get() : nullptr, i);
        for (auto& t : th)
            t.join();
        if (!fatal.empty())
            return fail(fatal);
        for (const Totals& t : per)
        {
            totals.sequences += t.sequences;
            totals.skipped_sequences += t.skipped_sequences;
            totals.length_bp += t.length_bp;
        }
    }
    counting.stop();
    if (c.verbose && c.parse == "device")
        std::cerr << "parse device: " << g_parse.device << " files tokenised on the device, " << g_parse.fell_back << " fell back to the host reader, "
                  << g_parse.host_only << " not eligible, " << g_parse.bytes << " text bytes uploaded" << std::endl;

    if (c.verify_given)
        return run_verify(c, targets, counting);
    if (c.update_given)
        return run_update(c, targets, counting);
    if (c.hibf)
        return run_hibf(c, targets, totals, whole, counting, arenas);

    std::vector<const uint64_t*> arena_words;
    if (c.verbose || packed_sets)
    {
        uint64_t hashes = 0, blocks = 0, words = 0;
        for (const Target& t : targets)
            hashes += n_hashes(t), blocks += t.blocks.size();
        try
        {
            for (auto& a : arenas)
                arena_words.push_back(a->data()), words += a->words();
        }
        catch (const std::exception& e)
        {
            return fail(e.what());
        }
        if (c.verbose)
        {
            std::cerr << "hash sets: " << hashes << " hashes held " << c.hash_sets << " in " << (packed_sets ? gn_packed_bytes(blocks, words) : hashes * 8)
                      << " bytes (8 x hashes = " << hashes * 8 << " bytes)";
            if (c.hash_sets == "spilled")
                std::cerr << ", " << arenas.size() << " files in " << output_folder(c);
            std::cerr << '\n' << "RssAnon after hashing: " << rss_anon_kb() << " kB" << std::endl;
        }
    }

    sizing.start();
    IbfParams p;
    p.kmer_size   = c.kmer_size;
    p.window_size = c.window_size;
    std::vector<uint64_t> counts;
    for (const Target& t : targets)
        counts.push_back(n_hashes(t));
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
        return fail("No valid sequences to build");

    std::vector<uint64_t>             shares;
    const std::vector<gnbuild::BinSpan> bins = gnbuild::lay_out_bins(p, counts, &shares);
    if (bins.size() != p.n_bins)
        return fail("internal error: " + std::to_string(bins.size()) + " bins laid out, " + std::to_string(p.n_bins) + " expected");

    if (p.bin_size_bits == 0 || p.hash_functions < 1 || p.hash_functions > 5)
    {
        // (the reference fails in the seqan3 IBF constructor: "The size of a bin must be > 0" / "hash functions must be > 0 and <= 5")
        std::cerr << "ERROR: the parameters leave a filter of " << p.bin_size_bits << " bits per bin with " << (unsigned)p.hash_functions
                  << " hash function(s): --filter-size / --max-fp do not fit " << targets.size() << " target(s)" << std::endl;
        return false;
    }
    if (!fill_and_save_flat(FlatFill{ c, p, targets, bins, shares, packed_sets ? &arena_words : nullptr }, filling, writing))
        return false;
    whole.stop();

    if (!c.quiet)
    {
        print_stats(c, totals, counting, "Estimate params   start: ", sizing, filling, writing, whole);
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
    if (run(c))
        return EXIT_SUCCESS;
    return parse_mode_ok(c) ? EXIT_FAILURE : 2; // (an unusable --parse is refused like a usage error, with status 2)
}
