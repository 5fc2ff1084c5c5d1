// build_hibf.cpp -- `ganon-build --hibf` (this project's extension, like --device): the hash sets of the targets go into a hierarchical
// filter, written as the raptor 3.0.1 index `ganon build --filter-type hibf` gets from `raptor prepare / layout / build`
// (/root/reference/src/ganon/build_update.py:411-518; read at src/ganon-classify/GanonClassify.cpp:875-938):
//   one user bin per target -> tree of IBFs (hibf_layout.hpp) -> exact cardinalities of the merged bins (gn_hashes_union)
//   -> rows per IBF (gnbuild::hibf_run_bits) -> zero-filled HIBF in HBM -> every user bin ORed in along its whole path
//   (gn_filter_emplace_path) -> IBF after IBF streamed into the file (save_hibf: the twin of ganon_amd/ibf_file.py:save_hibf).
// A tree that does not fit what a device may hold at one time (--hibf-memory, or what is free) is filled in parts over --hibf-devices
// instead (hibf_build_parts.hpp: the plan; build_hibf_parts.cpp: the workers) and gives the same file.
// --hibf-hash-sets packed|spilled: the targets' sets stay packed (csrc/gn_packed_set.h) from hashing to the insert, in the hashing
// threads' arenas and one more for the unions of targets of several files; the unions (gn_packed_union), the sketches
// (gn_sketches_create_packed) and the insert (gn_filter_emplace_path_packed_window) take packed runs: the same tree, rows and bits, so
// the same file.
#include "build_common.hpp"
#include "hibf_layout.hpp"
#include "hibf_layout_similarity.hpp"
#include "hibf_layout_sketch.hpp"
#include "hibf_paths.hpp"
#include "hibf_pool.hpp"

#include <cmath>
#include <iomanip>
#include <memory>
#include <unistd.h>

namespace gnbuild
{

namespace
{

// --layout sketch | similarity: one HyperLogLog sketch per user bin on the device, the estimated unions of up to `width` neighbours
// in an order for every start (tiled over the starts: gn_sketches_union_table bounds a call), then the search of
// hibf_layout_sketch.hpp.  similarity (hibf_layout_similarity.hpp) asks for that table twice, one after the other -- the size order's
// and the similarity order's -- and in between for one gn_sketches_pair_table per interval of the size order.
struct SketchLaps // seconds inside the `layout` lap: the rest of it is the host's ordering and searches
{
    double sketches = 0, tables = 0, pairs = 0;
};

bool lay_out_by_sketches(const Config& c, const std::vector<Target>& targets, const std::vector<uint32_t>& user_target, const std::vector<uint64_t>& counts,
                         const PackedSets* packed, uint32_t tmax, uint8_t h, gnhibf::Layout& lay, SketchLaps& laps, std::string& err)
{
    constexpr uint64_t kTableBytes = 4ull << 30; // the most host memory a union table may take
    const uint64_t     n = counts.size(), width = gnhibf::sketch_width(n, tmax);
    const bool         similarity = c.layout == "similarity";
    gn_sketches*       sk = nullptr;
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
        const int rc = packed ? gn_sketches_create_packed(c.device, packed->blocks.data(), packed->n_blocks.data(), packed->payload.data(), (uint32_t)n, &sk)
                              : gn_sketches_create(c.device, sets.data(), counts.data(), (uint32_t)n, &sk);
        if (rc != GN_OK)
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

} // namespace

namespace
{

// --hibf-hash-sets packed|spilled: a target of several files becomes one packed set, the union of its files' sets, whose payload goes
// behind the words of `united` (the hashing arena keeps the files' words: they are dead from here on, and not reclaimed)
bool unite_files_packed(const Config& c, Target& tg, const uint64_t* words, SetArena& united, uint32_t united_no)
{
    const gn_packed_block*     run = reinterpret_cast<const gn_packed_block*>(tg.blocks.data());
    const uint64_t             n_blocks = tg.blocks.size();
    std::vector<GnPackedBlock> out(gn_packed_max_blocks(tg.count));
    std::vector<uint64_t>      payload(gn_packed_max_words(tg.count));
    uint64_t                   n = 0, nb = 0, nw = 0;
    if (gn_packed_union(c.device, &run, &n_blocks, &words, 1, reinterpret_cast<gn_packed_block*>(out.data()), out.size(), payload.data(), payload.size(), &n,
                        &nb, &nw) != GN_OK)
        return false;
    out.resize(nb);
    const uint64_t base = united.words();
    united.append(payload.data(), nw);
    for (GnPackedBlock& b : out)
        b.word_at += base;
    tg.blocks.swap(out);
    tg.count = n;
    tg.arena = united_no;
    tg.file_ends.assign(1, n);
    return true;
}

} // namespace

bool run_hibf(const Config& c, std::vector<Target>& targets, const Totals& totals, Lap& whole, const Lap& counting,
              const std::vector<std::unique_ptr<SetArena>>& arenas)
{
    Lap            uniting, laying, filling, writing;
    const uint8_t  h = c.hash_functions == 0 ? 4 : c.hash_functions; // (what `ganon build` passes to raptor, config.py:138-145)

    // one user bin per target with a hash, in first-appearance order; its set = the union of its files' sets
    uniting.start();
    std::vector<uint32_t>    user_target;
    std::vector<uint64_t>    counts;
    std::vector<std::string> files;
    const std::string        dir = output_folder(c);
    const bool               packed_sets = c.hibf_hash_sets != "raw";
    // packed sets: the words of every arena by Target::arena -- the hashing threads' (complete: they may be mapped) and, behind them, the
    // one the unions are appended to, which is mapped only when the last union is in it; it goes, with its file, when this function returns
    std::vector<const uint64_t*> arena_words;
    std::unique_ptr<SetArena>    united;
    uint64_t                     n_united = 0;
    try
    {
        if (packed_sets)
        {
            for (const auto& a : arenas)
                arena_words.push_back(a->data());
            united.reset(c.hibf_hash_sets == "spilled"
                             ? new SetArena((fs::path(dir) / (fs::path(c.output_file).filename().string() + ".hashsets." + std::to_string(::getpid()) + ".united")).string())
                             : new SetArena());
        }
        for (uint32_t t = 0; t < targets.size(); ++t)
        {
            Target& tg = targets[t];
            if (n_hashes(tg) == 0)
                continue;
            if (packed_sets && tg.file_ends.size() > 1)
            {
                if (!unite_files_packed(c, tg, arena_words[tg.arena], *united, (uint32_t)arenas.size()))
                    return fail(gn_last_error());
                ++n_united;
            }
            else if (!packed_sets && !unite_files(c, tg))
                return fail(gn_last_error());
            user_target.push_back(t);
            counts.push_back(n_hashes(tg));
            files.push_back(dir + "/" + user_bin_file_name(tg.name) + ".minimiser");
        }
        if (packed_sets)
            arena_words.push_back(united->data());
    }
    catch (const std::exception& e) // (an arena: a file that cannot be created, written or mapped)
    {
        return fail(e.what());
    }
    if (counts.empty())
        return fail("No valid sequences to build");
    const uint64_t n_user = counts.size();
    PackedSets     packed;
    uint64_t       one_pass_bytes = 0; // what the one-pass build uploads: every user bin's set once
    for (uint64_t u = 0; packed_sets && u < n_user; ++u)
    {
        const Target& tg = targets[user_target[u]];
        packed.blocks.push_back(reinterpret_cast<const gn_packed_block*>(tg.blocks.data())), packed.n_blocks.push_back(tg.blocks.size());
        packed.payload.push_back(arena_words[tg.arena]), packed.bytes.push_back(packed_pass_bytes(tg.blocks));
        one_pass_bytes += packed.bytes.back();
    }
    if (packed_sets && (c.verbose || !c.quiet))
    {
        uint64_t hashes = 0, held = 0;
        for (uint64_t u = 0; u < n_user; ++u)
            hashes += counts[u], held += packed.bytes[u] - packed.n_blocks[u] * (sizeof(GnPackedItem) - sizeof(GnPackedBlock));
        std::cerr << "hibf hash sets: " << hashes << " hashes held " << c.hibf_hash_sets << " in " << held << " bytes, " << n_united << " targets united" << std::endl;
    }
    uint64_t       tmax   = c.tmax;
    if (!c.tmax_given)
        tmax = (uint64_t)std::ceil(std::sqrt((double)n_user) / 64.0) * 64; // build_update.py:487
    laying.start();
    gnhibf::Layout lay;
    SketchLaps     sketch_laps;
    if (c.layout == "sketch" || c.layout == "similarity")
    {
        std::string err;
        if (!lay_out_by_sketches(c, targets, user_target, counts, packed_sets ? &packed : nullptr, (uint32_t)tmax, h, lay, sketch_laps, err))
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
                std::vector<const gn_packed_block*> blocks;
                for (uint32_t u : lay.ibfs[r.child].members)
                {
                    sets.push_back(packed_sets ? packed.payload[u] : targets[user_target[u]].hashes.data());
                    sizes.push_back(packed_sets ? packed.n_blocks[u] : counts[u]);
                    if (packed_sets)
                        blocks.push_back(packed.blocks[u]);
                }
                uint64_t  nb = 0, nw = 0;
                const int rc = packed_sets ? gn_packed_union(c.device, blocks.data(), sizes.data(), sets.data(), (uint32_t)sets.size(), nullptr, 0, nullptr, 0, &n, &nb, &nw)
                                           : gn_hashes_union(c.device, sets.data(), sizes.data(), (uint32_t)sets.size(), nullptr, 0, &n);
                if (rc != GN_OK)
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

    // the end of either build: the laps and what was built
    auto report = [&]() {
        whole.stop();
        if (c.quiet)
            return;
        print_stats(c, totals, counting, "Layout and unions start: ", uniting, filling, writing, whole);
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
    };

    filling.start();
    // the parts the tree is filled in: one when it fits what an entry of the list may hold at one time
    const std::vector<int> entries = c.hibf_devices.empty() ? std::vector<int>{ c.device } : c.hibf_devices;
    uint64_t               budget  = c.hibf_memory;
    if (!c.hibf_memory_given)
    {
        std::string why;
        if (!budget_from_free_memory(entries, budget, why))
            return fail(why);
    }
    HibfPartPlan plan;
    try
    {
        std::vector<uint64_t> rows, row_bytes;
        for (const HibfShape& s : ibfs)
            rows.push_back(s.rows), row_bytes.push_back(gn_hibf_row_stride_words((s.bins + 63) >> 6) * 8);
        plan = plan_hibf_parts(rows, row_bytes, budget, (uint32_t)entries.size());
    }
    catch (const std::exception& e)
    {
        return fail(std::string(c.hibf_memory_given ? "--hibf-memory: " : "--hibf-devices: ") + e.what());
    }
    // every user bin's path: its run in its leaf IBF, then the merged bin that leads there in each IBF above
    const gnhibf::Paths paths = gnhibf::paths_of(lay, counts);
    std::vector<std::vector<std::string>> bin_path; // one file per user bin
    for (const std::string& f : files)
        bin_path.push_back({ f });
    for (uint64_t n : counts)
        if (!packed_sets)
            one_pass_bytes += n * 8;
    if (c.verbose && plan.n_parts <= 100000) // (a plan is a rule: a budget of a few rows makes more parts than anyone reads)
        for (uint64_t p = 0; p < plan.n_parts; ++p)
            for (const HibfPiece& x : plan.part(p))
                std::cerr << "part " << p << " device " << entries[plan.entry_of(p)] << ": ibf " << x.ibf << " rows [" << x.row_begin << ", "
                          << x.row_begin + x.n_rows << ")\n";
    if (plan.n_parts > 1)
    {
        std::vector<std::pair<const uint64_t*, uint64_t>> sets;
        for (uint64_t u = 0; u < n_user; ++u)
            sets.push_back(packed_sets ? std::pair<const uint64_t*, uint64_t>{ nullptr, counts[u] } : hash_set(targets[user_target[u]]));
        uint64_t uploaded = 0;
        if (!fill_and_save_hibf_parts(HibfPartsFill{ c, ibfs, h, plan, entries, paths, sets, bin_path, files, packed_sets ? &packed : nullptr }, uploaded))
            return false;
        filling.stop();
        writing.start(), writing.stop(); // (the rows went out piece by piece, inside the fill)
        if (c.verbose)
            std::cerr << "filled in " << plan.n_parts << " parts, " << uploaded << " hash bytes uploaded (one pass: " << one_pass_bytes << ")" << std::endl;
        report();
        return true;
    }
    gnhost::HibfDescs descs;
    for (const HibfShape& s : ibfs)
        descs.add(s.bins, s.rows, h, s.next_ibf_id, s.bin_to_user);
    gnhost::OwnedFilter flt = descs.upload(entries[0], n_user);
    if (!flt)
        return fail(gn_last_error());
    try
    {
        if (packed_sets) // one call over all user bins: it streams, nothing is pooled
        {
            std::vector<uint64_t> total_rows, row_begin(ibfs.size(), 0);
            for (const HibfShape& s : ibfs)
                total_rows.push_back(s.rows);
            if (gn_filter_emplace_path_packed_window(flt.get(), packed.blocks.data(), packed.n_blocks.data(), packed.payload.data(), (uint32_t)n_user,
                                                     paths.entries.data(), paths.depth, total_rows.data(), row_begin.data(), 0) != GN_OK)
                throw std::runtime_error(gn_last_error());
        }
        else
            gnhibf::for_each_pooled(
                n_user,
                [&](size_t u) { return hash_set(targets[user_target[u]]); },
                [&](size_t u) { return &paths.entries[u * paths.depth]; }, paths.depth,
                [&](const uint64_t* hashes, const uint64_t* off, size_t n, const gn_path_entry* p, const std::vector<size_t>&) {
                    if (gn_filter_emplace_path(flt.get(), hashes, off, (uint32_t)n, p, paths.depth) != GN_OK)
                        throw std::runtime_error(gn_last_error());
                });
    }
    catch (const std::exception& e)
    {
        return fail(e.what());
    }
    filling.stop();

    writing.start();
    std::string err;
    const bool  saved = save_hibf(c, flt.get(), ibfs, h, bin_path, files, err);
    flt.reset();
    if (!saved)
        return fail(err);
    writing.stop();
    if (c.verbose)
        std::cerr << "filled in 1 part, " << one_pass_bytes << " hash bytes uploaded" << std::endl;
    report();
    return true;
}

} // namespace gnbuild
