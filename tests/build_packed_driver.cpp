// build_packed_driver.cpp -- test harness: runs the PRODUCT's packed hash sets (ganon_amd/csrc/gn_packed_set.h: the host encoder and
// decoder, the bit-extract, the bounds, the item builder -- the very functions the kernels and their host call) so that
// tests/test_build_packed_cpu.py can check them.  One case per line of stdin; a run is `<n_files> { <size> <hash in hex> per hash } per
// file`, every file strictly ascending:
//   encode <n_runs> { run }
//   items <cap_words> <cap_items> <n_runs> { run }
//   window <total_rows> <bins> <h> <row_begin> <n_rows> <cap_words> <n_runs> { <first_bin> <per_bin> run }
// stdout:
//   encode: per run `run <hashes> <blocks> <words>`, `block <first hex> <word_at> <cnt> <width>` per block, `payload <word in hex> ...`,
//           `decoded <hash in hex> ...` -- decoded from copies of EXACTLY the blocks and words there are (a read past the payload is a
//           heap overflow the sanitizer sees); `refused ...` when the bounds do not hold
//   items:  per chunk `chunk <items> <words>`, then `item <run> <cnt> <width> <first hex> <begin> <stage_at> <block>` per item
//   window: n_rows lines of ceil(bins / 64) words in hex: the slab after a host model of gn_emplace_packed_window_kernel -- per chunk the
//           host's gather into a staging buffer of exactly the chunk's words, per item 64 lanes: lane L extracts deltas 8L .. 8L + 7 (none
//           past the block's last), sums them, an inclusive scan of the lane sums less the lane's own plus `first` is hash 8L, the deltas
//           lead on to 8L + 1 .. 8L + 7; then per hash function the row of the WHOLE filter, the window test, the bit -- into a buffer of
//           EXACTLY n_rows * ceil(bins / 64) words
#include "../ganon_amd/csrc/gn_packed_set.h"
#include "../include/ganon_ibf_hash.h"

#include <cstdio>
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

struct PackedRun
{
    std::vector<GnPackedBlock> blocks;
    std::vector<uint64_t>      payload;
    uint64_t                   hashes = 0;
};

// a run from the case's text, file by file through the product's encoder; the bounds are checked per file
static PackedRun read_run(std::istringstream& in)
{
    PackedRun r;
    uint64_t  n_files = 0;
    in >> std::dec >> n_files;
    if (!in || n_files > 1000)
        throw std::runtime_error("driver: unreadable run");
    for (uint64_t f = 0; f < n_files; ++f)
    {
        uint64_t n = 0;
        in >> std::dec >> n;
        if (!in || n > 10000000)
            throw std::runtime_error("driver: unreadable file");
        std::unique_ptr<uint64_t[]> v(new uint64_t[n]);
        in >> std::hex;
        for (uint64_t i = 0; i < n; ++i)
            in >> v[i];
        if (!in)
            throw std::runtime_error("driver: unreadable hashes");
        const size_t b0 = r.blocks.size(), w0 = r.payload.size();
        gn_packed_encode(v.get(), n, r.blocks, r.payload);
        if (r.blocks.size() - b0 != gn_packed_max_blocks(n) || r.payload.size() - w0 > gn_packed_max_words(n))
            throw std::runtime_error("the bounds on blocks and words do not hold");
        r.hashes += n;
    }
    return r;
}

static void encode_case(std::istringstream& in)
{
    uint64_t n_runs = 0;
    in >> n_runs;
    if (!in || n_runs > 100000)
        throw std::runtime_error("driver: unreadable case");
    for (uint64_t k = 0; k < n_runs; ++k)
    {
        const PackedRun r = read_run(in);
        std::printf("run %llu %zu %zu\n", (unsigned long long)r.hashes, r.blocks.size(), r.payload.size());
        for (const GnPackedBlock& b : r.blocks)
            std::printf("block %llx %llu %u %u\n", (unsigned long long)b.first, (unsigned long long)b.word_at, b.cnt, b.width);
        std::printf("payload");
        for (uint64_t w : r.payload)
            std::printf(" %llx", (unsigned long long)w);
        // (new[], not the vectors: exactly as many blocks and words as there are, with the sanitizer's red zone right behind them)
        std::unique_ptr<GnPackedBlock[]> blocks(new GnPackedBlock[r.blocks.size()]);
        std::unique_ptr<uint64_t[]>      words(new uint64_t[r.payload.size()]);
        std::copy(r.blocks.begin(), r.blocks.end(), blocks.get());
        std::copy(r.payload.begin(), r.payload.end(), words.get());
        std::vector<uint64_t> out;
        gn_packed_decode(blocks.get(), r.blocks.size(), words.get(), out);
        std::printf("\ndecoded");
        for (uint64_t v : out)
            std::printf(" %llx", (unsigned long long)v);
        std::printf("\n");
    }
}

struct Runs
{
    std::vector<PackedRun>            runs;
    std::vector<const GnPackedBlock*> blocks;
    std::vector<uint64_t>             n_blocks;
};

static void items_case(std::istringstream& in)
{
    uint64_t cap_words = 0, cap_items = 0, n_runs = 0;
    in >> cap_words >> cap_items >> n_runs;
    if (!in || cap_words < GN_PACKED_MAX_WORDS || cap_items == 0 || n_runs > 100000)
        throw std::runtime_error("driver: unreadable case");
    Runs r;
    for (uint64_t k = 0; k < n_runs; ++k)
        r.runs.push_back(read_run(in));
    for (const PackedRun& p : r.runs)
        r.blocks.push_back(p.blocks.data()), r.n_blocks.push_back(p.blocks.size());
    std::vector<GnPackedItem> items;
    GnPackedCursor            cur;
    for (uint64_t words = 0; gn_packed_next_chunk(r.blocks.data(), r.n_blocks.data(), (uint32_t)n_runs, cur, cap_words, cap_items, items, &words);)
    {
        std::printf("chunk %zu %llu\n", items.size(), (unsigned long long)words);
        for (const GnPackedItem& it : items)
            std::printf("item %u %u %u %llx %llu %llu %llu\n", it.run, it.cnt, it.width, (unsigned long long)it.first, (unsigned long long)it.begin,
                        (unsigned long long)it.stage_at, (unsigned long long)it.block);
    }
}

static void window_case(std::istringstream& in)
{
    uint64_t total_rows = 0, bins = 0, h = 0, row_begin = 0, n_rows = 0, cap_words = 0, n_runs = 0;
    in >> total_rows >> bins >> h >> row_begin >> n_rows >> cap_words >> n_runs;
    if (!in || total_rows == 0 || total_rows > 0xFFFFFFFFull || bins == 0 || bins > 1000000 || h < 1 || h > GN_IBF_MAX_HASH_FUNS || n_rows == 0 ||
        row_begin + n_rows > total_rows || cap_words < GN_PACKED_MAX_WORDS || n_runs > 100000)
        throw std::runtime_error("driver: unreadable case");
    Runs                        r;
    std::unique_ptr<uint64_t[]> per_bin(new uint64_t[n_runs]);
    std::unique_ptr<uint32_t[]> first_bin(new uint32_t[n_runs]);
    for (uint64_t k = 0; k < n_runs; ++k)
    {
        in >> std::dec >> first_bin[k] >> per_bin[k];
        if (!in || per_bin[k] == 0)
            throw std::runtime_error("driver: unreadable run");
        r.runs.push_back(read_run(in));
        if (r.runs[k].hashes && first_bin[k] + (r.runs[k].hashes - 1) / per_bin[k] >= bins)
            throw std::runtime_error("driver: a run leaves the filter's bins");
    }
    for (const PackedRun& p : r.runs)
        r.blocks.push_back(p.blocks.data()), r.n_blocks.push_back(p.blocks.size());
    const uint64_t              W     = (bins + 63) / 64;
    const uint32_t              shift = (uint32_t)__builtin_clzll(total_rows);
    std::unique_ptr<uint64_t[]> slab(new uint64_t[n_rows * W]());
    std::vector<GnPackedItem>   items;
    GnPackedCursor              cur;
    for (uint64_t words = 0; gn_packed_next_chunk(r.blocks.data(), r.n_blocks.data(), (uint32_t)n_runs, cur, cap_words, cap_words / 16 + 16, items, &words);)
    {
        std::unique_ptr<uint64_t[]> stage(new uint64_t[words]); // exactly the chunk's words
        for (const GnPackedItem& it : items)                    // the host's gather
            for (uint32_t w = 0; w < gn_packed_words(it.cnt, it.width); ++w)
                stage[it.stage_at + w] = r.runs[it.run].payload[r.runs[it.run].blocks[it.block].word_at + w];
        for (const GnPackedItem& it : items) // the kernel: one wave per item
        {
            const uint64_t* words_at = stage.get() + it.stage_at;
            uint64_t        d[64][GN_WIN_PER_LANE], sum[64], incl[64];
            for (uint32_t lane = 0; lane < 64; ++lane)
            {
                sum[lane] = 0;
                for (uint32_t j = 0; j < GN_WIN_PER_LANE; ++j)
                {
                    const uint32_t e = lane * GN_WIN_PER_LANE + j;
                    d[lane][j]       = e + 1 < it.cnt ? gn_packed_delta(words_at, e, it.width) : 0;
                    sum[lane] += d[lane][j];
                }
                incl[lane] = sum[lane] + (lane ? incl[lane - 1] : 0);
            }
            const uint64_t b0 = it.begin / per_bin[it.run], r0 = it.begin - b0 * per_bin[it.run];
            const uint32_t bin0 = first_bin[it.run] + (uint32_t)b0;
            for (uint32_t lane = 0; lane < 64; ++lane)
            {
                uint64_t v = it.first + (incl[lane] - sum[lane]);
                for (uint32_t j = 0; j < GN_WIN_PER_LANE; ++j)
                {
                    const uint32_t q = lane * GN_WIN_PER_LANE + j;
                    if (q < it.cnt)
                    {
                        const uint32_t bin = gn_window_item_bin(bin0, r0, q, per_bin[it.run]);
                        if (bin != gn_window_bin(first_bin[it.run], it.begin + q, per_bin[it.run]))
                            throw std::runtime_error("driver: the item's bin differs from the rule's");
                        for (uint32_t i = 0; i < h; ++i)
                        {
                            uint32_t local;
                            if (gn_window_local(build_row(v, i, shift, total_rows), (uint32_t)row_begin, (uint32_t)n_rows, &local))
                                slab[(uint64_t)local * W + (bin >> 6)] |= 1ULL << (bin & 63);
                        }
                    }
                    v += d[lane][j];
                }
            }
        }
    }
    for (uint64_t row = 0; row < n_rows; ++row)
    {
        for (uint64_t w = 0; w < W; ++w)
            std::printf("%s%llx", w ? " " : "", (unsigned long long)slab[row * W + w]);
        std::printf("\n");
    }
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
            if (what == "encode")
                encode_case(in);
            else if (what == "items")
                items_case(in);
            else if (what == "window")
                window_case(in);
        }
        catch (const std::exception& e)
        {
            std::printf("refused %s\n", e.what());
        }
    }
    return 0;
}
