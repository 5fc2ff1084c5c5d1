// build_hibf_packed_driver.cpp -- test harness: a host model of gn_emplace_path_packed_window_kernel (ganon_amd/csrc/gn_build_hibf.hip) and
// of gn_packed_union (gn_build.hip) built from the PRODUCT's own functions -- the encoder, the decoder, the bit-extract and the item builder
// of ganon_amd/csrc/gn_packed_set.h, the path arithmetic of gn_path_window.h, the window test of gn_emplace_window.h -- so that
// tests/test_build_hibf_packed_cpu.py can check them.  One case per line of stdin; a run is `<n_files> { <size> <hash in hex> per hash }
// per file`, and is packed here as the builder packs it: every file's set on its own, the files behind each other.
//   window <h> <cap_words> <n_ibf> { <bins> <total_rows> <row_begin> <n_rows> } per IBF <depth> <n_sets>
//          { { <ibf> <first_bin> <n_bins> <per_bin> } per entry <run> } per set
//   union <n_runs> <run> per run
// stdout:
//   window:  per IBF `ibf <j>` and n_rows lines of ceil(bins / 64) words in hex: the pieces after the model -- per staging chunk
//            (gn_packed_next_chunk) the payload gathered into a buffer of EXACTLY the chunk's words, per item the decode as a wave makes
//            it (lane L: deltas 8L .. 8L + 7 through gn_packed_delta, an inclusive scan of the lane sums, hash 8L = first + scan - own
//            sum), per entry of the item's path, per hash, per hash function: the row of the WHOLE IBF, the window test, the bit -- into
//            buffers of EXACTLY n_rows * ceil(bins / 64) words (a read or a write outside is a heap overflow the sanitizer sees)
//   union:   `union <hashes> <blocks> <words>`, `block <first in hex> <word_at> <cnt> <width>` per block, `payload <word in hex> ...`:
//            gn_packed_encode of the sorted distinct hashes gn_packed_decode gives for the runs
#include "../ganon_amd/csrc/gn_packed_set.h"
#include "../ganon_amd/csrc/gn_path_window.h"
#include "../include/ganon_ibf_hash.h"

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <iostream>
#include <memory>
#include <sstream>
#include <stdexcept>
#include <string>

static const uint64_t kSeeds[GN_IBF_MAX_HASH_FUNS] = GN_IBF_SEED_LIST;

// gn_build_row (ganon_amd/csrc/gn_build_row.h) on the host
static uint32_t build_row(uint64_t v, uint32_t i, uint32_t shift, uint64_t S)
{
    uint64_t x = v * kSeeds[i];
    x ^= x >> shift;
    x *= GN_IBF_MULTIPLIER;
    return (uint32_t)(((unsigned __int128)x * S) >> 64);
}

static void unreadable(bool bad)
{
    if (bad)
        throw std::runtime_error("driver: unreadable case");
}

// a run as the builder holds it: blocks whose word_at count from words[0], and exactly the words there are
struct Run
{
    std::vector<GnPackedBlock>  blocks;
    std::unique_ptr<uint64_t[]> words;
    uint64_t                    n_words = 0, hashes = 0;
};

static void read_run(std::istringstream& in, Run& r)
{
    uint64_t n_files = 0;
    in >> std::dec >> n_files;
    unreadable(!in || n_files > 1000);
    std::vector<uint64_t> payload;
    for (uint64_t f = 0; f < n_files; ++f)
    {
        uint64_t n = 0;
        in >> std::dec >> n;
        unreadable(!in || n > 10000000);
        std::unique_ptr<uint64_t[]> v(new uint64_t[n]);
        in >> std::hex;
        for (uint64_t i = 0; i < n; ++i)
            in >> v[i];
        unreadable(!in);
        gn_packed_encode(v.get(), n, r.blocks, payload);
        r.hashes += n;
    }
    in >> std::dec;
    r.n_words = payload.size();
    r.words.reset(new uint64_t[r.n_words]);
    if (r.n_words)
        memcpy(r.words.get(), payload.data(), r.n_words * 8);
}

static void window_case(std::istringstream& in)
{
    uint64_t h = 0, cap_words = 0, n_ibf = 0, depth = 0, n_sets = 0;
    in >> h >> cap_words >> n_ibf;
    unreadable(!in || h < 1 || h > GN_IBF_MAX_HASH_FUNS || cap_words < GN_PACKED_MAX_WORDS || n_ibf == 0 || n_ibf > 1000);
    std::vector<uint64_t>                    bins(n_ibf), total(n_ibf), begin(n_ibf), n_rows(n_ibf), W(n_ibf);
    std::vector<std::unique_ptr<uint64_t[]>> piece(n_ibf);
    for (uint64_t j = 0; j < n_ibf; ++j)
    {
        in >> bins[j] >> total[j] >> begin[j] >> n_rows[j];
        unreadable(!in || bins[j] == 0 || bins[j] > 1000000 || total[j] == 0 || total[j] > 0xFFFFFFFFull || n_rows[j] == 0 || begin[j] + n_rows[j] > total[j] ||
                   n_rows[j] > 10000000);
        W[j] = (bins[j] + 63) / 64;
        piece[j].reset(new uint64_t[n_rows[j] * W[j]]()); // (exactly as many words as the piece has)
    }
    in >> depth >> n_sets;
    unreadable(!in || depth == 0 || depth > 64 || n_sets > 100000);
    std::vector<GnPathWinDev> paths(n_sets * depth, GnPathWinDev{ nullptr, 1, 1, 1, 0, 0, 0, 0, 0 });
    std::vector<Run>          runs(n_sets);
    for (uint64_t s = 0; s < n_sets; ++s)
    {
        for (uint64_t d = 0; d < depth; ++d)
        {
            uint64_t      ibf = 0;
            GnPathWinDev& e   = paths[s * depth + d];
            in >> std::dec >> ibf >> e.first_bin >> e.n_bins >> e.per_bin;
            unreadable(!in || ibf >= n_ibf || (uint64_t)e.first_bin + e.n_bins > bins[ibf] || (e.n_bins > 1 && e.per_bin == 0));
            // what the library's host resolves: the piece and the WHOLE IBF's geometry
            e.rows    = piece[ibf].get();
            e.S_total = total[ibf], e.shift = (uint32_t)__builtin_clzll(total[ibf]);
            e.Ws      = (uint32_t)W[ibf]; // (no padding on the host: the model's rows are the file's)
            e.row_begin = (uint32_t)begin[ibf], e.n_rows = (uint32_t)n_rows[ibf];
        }
        read_run(in, runs[s]);
        for (uint64_t d = 0; d < depth && paths[s * depth + d].n_bins; ++d)
            if (paths[s * depth + d].n_bins > 1 && runs[s].hashes && (runs[s].hashes - 1) / paths[s * depth + d].per_bin >= paths[s * depth + d].n_bins)
                throw std::runtime_error("driver: the hashes do not fit the run");
    }
    std::vector<const GnPackedBlock*> blocks(n_sets);
    std::unique_ptr<uint64_t[]>       n_blocks(new uint64_t[n_sets]);
    uint64_t                          total_blocks = 0;
    for (uint64_t s = 0; s < n_sets; ++s)
        blocks[s] = runs[s].blocks.data(), n_blocks[s] = runs[s].blocks.size(), total_blocks += n_blocks[s];
    std::vector<GnPackedItem> items;
    GnPackedCursor            cur;
    for (;;)
    {
        uint64_t       words = 0;
        const uint64_t taken = gn_packed_next_chunk(blocks.data(), n_blocks.get(), (uint32_t)n_sets, cur, cap_words, std::min<uint64_t>(cap_words / 16 + 16, total_blocks),
                                                    items, &words);
        if (taken == 0)
            break;
        std::unique_ptr<uint64_t[]> stage(new uint64_t[words]); // (exactly the chunk's words)
        for (const GnPackedItem& it : items)                     // the host's gather into the staging chunk
            if (const uint32_t w = gn_packed_words(it.cnt, it.width))
                memcpy(stage.get() + it.stage_at, runs[it.run].words.get() + blocks[it.run][it.block].word_at, (size_t)w * 8);
        for (const GnPackedItem& it : items) // the kernel: one wave per item
        {
            // the decode of a wave: lane L extracts deltas 8L .. 8L + 7 and sums them, the inclusive scan of the sums less the lane's own
            // is what leads from `first` to hash 8L
            uint64_t v[GN_WIN_ITEM], d[GN_WIN_ITEM], incl = 0;
            for (uint32_t lane = 0; lane < 64; ++lane)
            {
                uint64_t sum = 0;
                for (uint32_t j = 0; j < GN_WIN_PER_LANE; ++j)
                {
                    const uint32_t e = lane * GN_WIN_PER_LANE + j;
                    d[e]             = e + 1 < it.cnt ? gn_packed_delta(stage.get() + it.stage_at, e, it.width) : 0;
                    sum += d[e];
                }
                incl += sum;
                uint64_t x = it.first + (incl - sum);
                for (uint32_t j = 0; j < GN_WIN_PER_LANE; ++j)
                    v[lane * GN_WIN_PER_LANE + j] = x, x += d[lane * GN_WIN_PER_LANE + j];
            }
            for (uint64_t dd = 0; dd < depth; ++dd)
            {
                const GnPathWinDev& e = paths[it.run * depth + dd];
                if (e.n_bins == 0)
                    break;
                uint32_t bin0;
                uint64_t r0;
                gn_path_window_start(e.first_bin, e.n_bins, e.per_bin, it.begin, &bin0, &r0);
                for (uint32_t q = 0; q < it.cnt; ++q)
                {
                    const uint32_t bin = gn_path_window_bin(bin0, r0, q, e.n_bins, e.per_bin);
                    if (bin != (e.n_bins == 1 ? e.first_bin : gn_window_bin(e.first_bin, it.begin + q, e.per_bin)))
                        throw std::runtime_error("driver: the item's bin differs from the rule's");
                    for (uint32_t i = 0; i < h; ++i)
                    {
                        uint32_t local;
                        if (gn_window_local(build_row(v[q], i, e.shift, e.S_total), e.row_begin, e.n_rows, &local))
                            e.rows[(uint64_t)local * e.Ws + (bin >> 6)] |= 1ULL << (bin & 63);
                    }
                }
            }
        }
    }
    for (uint64_t j = 0; j < n_ibf; ++j)
    {
        std::printf("ibf %llu\n", (unsigned long long)j);
        for (uint64_t r = 0; r < n_rows[j]; ++r)
        {
            for (uint64_t w = 0; w < W[j]; ++w)
                std::printf("%s%llx", w ? " " : "", (unsigned long long)piece[j][r * W[j] + w]);
            std::printf("\n");
        }
    }
}

static void union_case(std::istringstream& in)
{
    uint64_t n_runs = 0;
    in >> n_runs;
    unreadable(!in || n_runs > 100000);
    std::vector<uint64_t> all;
    for (uint64_t r = 0; r < n_runs; ++r)
    {
        Run run;
        read_run(in, run);
        gn_packed_decode(run.blocks.data(), run.blocks.size(), run.words.get(), all);
    }
    std::sort(all.begin(), all.end());
    all.erase(std::unique(all.begin(), all.end()), all.end());
    std::vector<GnPackedBlock> blocks;
    std::vector<uint64_t>      payload;
    gn_packed_encode(all.data(), all.size(), blocks, payload);
    if (blocks.size() > gn_packed_max_blocks(all.size()) || (all.size() && payload.size() > gn_packed_max_words(all.size())))
        throw std::runtime_error("driver: the union exceeds the bounds of the format");
    std::printf("union %zu %zu %zu\n", all.size(), blocks.size(), payload.size());
    for (const GnPackedBlock& b : blocks)
        std::printf("block %llx %llu %u %u\n", (unsigned long long)b.first, (unsigned long long)b.word_at, b.cnt, b.width);
    std::printf("payload");
    for (uint64_t w : payload)
        std::printf(" %llx", (unsigned long long)w);
    std::printf("\n");
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
            if (what == "window")
                window_case(in);
            else if (what == "union")
                union_case(in);
        }
        catch (const std::exception& e)
        {
            std::printf("refused %s\n", e.what());
        }
    }
    return 0;
}
