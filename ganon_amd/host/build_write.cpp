// build_write.cpp -- the files `ganon-build` writes: the flat .ibf (save_filter; in row slabs open_filter + save_slab) and the raptor
// 3.0.1 index (save_hibf; in parts open_hibf + save_piece).  The header comes from the host; the bit matrices are streamed out of HBM
// through one page-locked stage (write_rows).
#include "build_common.hpp"
#include "hasher.hpp"

#include <algorithm>
#include <atomic>
#include <fcntl.h>
#include <thread>
#include <unistd.h>

namespace gnbuild
{

namespace
{

using gnhost::PinnedBlock;

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

uint64_t row_bytes_of(uint64_t bins)
{
    return ((bins + 63) >> 6) * 8;
}

// seqan3::interleaved_bloom_filter: bins, technical_bins, bin_size, hash_shift, bin_words, hash_funs, sdsl bit_vector
void ibf_header(Writer& w, uint64_t bins, uint64_t rows, uint64_t hash_functions)
{
    const uint64_t W = (bins + 63) >> 6;
    w.raw<uint64_t>(bins);
    w.raw<uint64_t>(W * 64);
    w.raw<uint64_t>(rows);
    w.raw<uint64_t>((uint64_t)__builtin_clzll(rows));
    w.raw<uint64_t>(W);
    w.raw<uint64_t>(hash_functions);
    w.raw<uint8_t>(1);      // sdsl int_vector<1>: width
    w.raw<float>(1.5f);     //                    growth factor
    w.raw<uint64_t>(W * 64 * rows); // size in bits
}

// rows per download: what 256 MiB hold, one at least
uint64_t chunk_rows(uint64_t n_rows, uint64_t row_bytes)
{
    return std::max<uint64_t>(1, std::min<uint64_t>(256ull << 20, n_rows * row_bytes) / row_bytes);
}

// rows [0, n_rows) of IBF `ibf` out of HBM into the file from offset `at` on, chunk after chunk through `stage` (which holds
// chunk_rows(n_rows, row_bytes) rows), a chunk written by up to `writers` threads.  false: `err` says what the device refused, or is
// left as it was when a write failed.
bool write_rows(int fd, gn_filter* flt, uint32_t ibf, uint64_t n_rows, uint64_t row_bytes, uint64_t at, void* stage, unsigned writers,
                std::string& err)
{
    const uint64_t per = chunk_rows(n_rows, row_bytes);
    for (uint64_t row = 0; row < n_rows; row += per)
    {
        const uint64_t n = std::min<uint64_t>(per, n_rows - row);
        if (gn_filter_download_rows(flt, ibf, row, n, static_cast<uint64_t*>(stage)) != GN_OK)
        {
            err = gnhost::hip_error();
            return false;
        }
        const unsigned           nt = (unsigned)std::min<uint64_t>(writers, std::max<uint64_t>(1, n * row_bytes >> 24));
        std::vector<std::thread> th;
        std::atomic<bool>        good{ true };
        const uint64_t           bytes = n * row_bytes, share = (bytes + nt - 1) / nt;
        for (unsigned i = 0; i < nt; ++i)
            th.emplace_back([&, i] {
                const uint64_t lo = std::min<uint64_t>(bytes, i * share), hi = std::min<uint64_t>(bytes, lo + share);
                if (hi > lo && !pwrite_all(fd, static_cast<const char*>(stage) + lo, hi - lo, at + row * row_bytes + lo))
                    good = false;
            });
        for (auto& t : th)
            t.join();
        if (!good)
            return false;
    }
    return true;
}

} // namespace

// the flat file's header: IBFConfig, hashes_count_std, bin_map, then the IBF's own fields up to the bit vector's size
static void filter_header(Writer& w, const IbfParams& p, const std::vector<Target>& targets, const std::vector<BinSpan>& bins)
{
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
        w.raw<uint64_t>(n_hashes(t));
    }
    w.raw<uint64_t>(bins.size()); // bin_map
    for (uint64_t b = 0; b < bins.size(); ++b)
    {
        w.raw<uint64_t>(b);
        w.str(targets[bins[b].target].name);
    }
    ibf_header(w, p.n_bins, p.bin_size_bits, p.hash_functions);
}

// save_filter (:251-288): header from the host, the bit matrix streamed out of HBM
bool save_filter(const Config& c, gn_filter* flt, const IbfParams& p, const std::vector<Target>& targets, const std::vector<BinSpan>& bins,
                 std::string& err)
{
    Writer w;
    filter_header(w, p, targets, bins);
    const int fd = ::open(c.output_file.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0644);
    if (fd < 0)
    {
        err = "cannot write " + c.output_file;
        return false;
    }
    bool           ok = pwrite_all(fd, w.buf.data(), w.buf.size(), 0);
    const uint64_t row_bytes = row_bytes_of(p.n_bins);
    PinnedBlock    stage;
    if (ok && !stage.reserve(chunk_rows(p.bin_size_bits, row_bytes) * row_bytes))
    {
        err = gnhost::hip_error();
        ok  = false;
    }
    // a few writers per chunk: one pwrite stream does not fill a fast disk
    if (ok && !write_rows(fd, flt, 0, p.bin_size_bits, row_bytes, w.buf.size(), stage.get(), 8, err))
    {
        if (err.empty())
            err = "write error on " + c.output_file;
        ok = false;
    }
    ::close(fd);
    return ok;
}

// The same file for a build in row slabs: the header, and the file extended to its full size so that every slab's rows have their
// place (payload_at + row_begin * row_bytes) whichever slab is written first.  -1: `err` says why.
int open_filter(const Config& c, const IbfParams& p, const std::vector<Target>& targets, const std::vector<BinSpan>& bins, uint64_t& payload_at,
                std::string& err)
{
    Writer w;
    filter_header(w, p, targets, bins);
    payload_at   = w.buf.size();
    const int fd = ::open(c.output_file.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0644);
    if (fd < 0)
    {
        err = "cannot write " + c.output_file;
        return -1;
    }
    if (!pwrite_all(fd, w.buf.data(), w.buf.size(), 0) || ::ftruncate(fd, (off_t)(payload_at + p.bin_size_bits * row_bytes_of(p.n_bins))) != 0)
    {
        err = "write error on " + c.output_file;
        ::close(fd);
        return -1;
    }
    return fd;
}

// rows [0, n_rows) of a slab's filter to byte `at` of the file; `stage` is the caller's (one per worker) and grows to a chunk
bool save_slab(int fd, gn_filter* flt, uint64_t n_rows, uint64_t row_bytes, uint64_t at, PinnedBlock& stage, std::string& err)
{
    if (!stage.reserve(chunk_rows(n_rows, row_bytes) * row_bytes))
    {
        err = gnhost::hip_error();
        return false;
    }
    if (!write_rows(fd, flt, 0, n_rows, row_bytes, at, stage.get(), 8, err))
    {
        if (err.empty())
            err = "write error on the output file";
        return false;
    }
    return true;
}

// The raptor 3.0.1 index (reader: GanonClassify.cpp:875-938 with hibf.hpp:163-169,293-298), field for field what
// ganon_amd/ibf_file.py:save_hibf writes.  The fields before the first IBF and those behind the last one, for the two writers below.
// bin_path: the files of every user bin (this builder writes one each; a raptor file that `--update` carries over may list several);
// user_files: user_bin_filenames, one per user bin.
static void hibf_front(Writer& w, const Config& c, const std::vector<std::vector<std::string>>& bin_path, uint64_t n_ibf)
{
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
    w.raw<uint64_t>(n_ibf);                                 // ibf_vector
}

static void hibf_back(Writer& w, const std::vector<HibfShape>& ibfs, const std::vector<std::string>& user_files)
{
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
}

// the matrices streamed IBF after IBF out of HBM
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
    hibf_front(w, c, bin_path, ibfs.size());
    flush(w);
    uint64_t stage_bytes = 0; // the largest chunk of any IBF
    for (const HibfShape& s : ibfs)
        stage_bytes = std::max(stage_bytes, chunk_rows(s.rows, row_bytes_of(s.bins)) * row_bytes_of(s.bins));
    PinnedBlock stage;
    if (ok && !stage.reserve(stage_bytes))
    {
        err = gnhost::hip_error();
        ok  = false;
    }
    for (uint32_t i = 0; ok && i < ibfs.size(); ++i)
    {
        const HibfShape& s = ibfs[i];
        ibf_header(w, s.bins, s.rows, hash_functions);
        flush(w);
        // (one writer, as ever: measured on an index of 0.97 GB, 2, 4 and 8 writers a chunk were 2 .. 29 % slower, on a tmpfs and on a disk)
        ok = ok && write_rows(fd, flt, i, s.rows, row_bytes_of(s.bins), at, stage.get(), 1, err);
        at += s.rows * row_bytes_of(s.bins);
    }
    hibf_back(w, ibfs, user_files);
    flush(w);
    ::close(fd);
    if (!ok && err.empty())
        err = "write error on " + c.output_file;
    return ok;
}

// The same file for a build in parts: everything but the payloads, and the file extended to its full size, so that every piece's rows
// have their place (payload_at[ibf] + row_begin * row bytes) whichever part is written first.  -1: `err` says why.
int open_hibf(const Config& c, const std::vector<HibfShape>& ibfs, uint8_t hash_functions, const std::vector<std::vector<std::string>>& bin_path,
              const std::vector<std::string>& user_files, std::vector<uint64_t>& payload_at, std::string& err)
{
    const int fd = ::open(c.output_file.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0644);
    if (fd < 0)
    {
        err = "cannot write " + c.output_file;
        return -1;
    }
    uint64_t at    = 0;
    bool     ok    = true;
    auto     flush = [&](Writer& w) {
        ok = ok && pwrite_all(fd, w.buf.data(), w.buf.size(), at);
        at += w.buf.size();
        w.buf.clear();
    };
    Writer w;
    hibf_front(w, c, bin_path, ibfs.size());
    flush(w);
    payload_at.assign(ibfs.size(), 0);
    for (uint32_t i = 0; i < ibfs.size(); ++i)
    {
        ibf_header(w, ibfs[i].bins, ibfs[i].rows, hash_functions);
        flush(w);
        payload_at[i] = at;
        at += ibfs[i].rows * row_bytes_of(ibfs[i].bins);
    }
    hibf_back(w, ibfs, user_files);
    flush(w); // (behind the last payload: the file has its full size, the payloads in between read as zeros until they are written)
    if (!ok || ::ftruncate(fd, (off_t)at) != 0)
    {
        err = "write error on " + c.output_file;
        ::close(fd);
        return -1;
    }
    return fd;
}

// rows [0, n_rows) of IBF `ibf` of a part's filter to byte `at` of the file; `stage` is the caller's (one per worker) and grows to a chunk
bool save_piece(int fd, gn_filter* flt, uint32_t ibf, uint64_t n_rows, uint64_t row_bytes, uint64_t at, PinnedBlock& stage, std::string& err)
{
    if (!stage.reserve(chunk_rows(n_rows, row_bytes) * row_bytes))
    {
        err = gnhost::hip_error();
        return false;
    }
    // (one writer a chunk, as save_hibf: the workers of a build in parts write side by side already)
    if (!write_rows(fd, flt, ibf, n_rows, row_bytes, at, stage.get(), 1, err))
    {
        if (err.empty())
            err = "write error on the output file";
        return false;
    }
    return true;
}

} // namespace gnbuild
