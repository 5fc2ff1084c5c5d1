// hasher.hpp -- the distinct minimiser hashes of whole sequences, computed on the device (count_hashes,
// /root/reference/src/ganon-build/GanonBuild.cpp:184-249).  Shared by ganon-build (which inserts them) and
// `ganon-classify --verify-filter` (which looks them up again, tests/ganon-build/GanonBuild.test.cpp:53-98).
#pragma once

#include "ganon_hip.h"

#include "genome_chunks.hpp"
#include "tunables.hpp"

#include "../csrc/gn_packed_set.h"

#include <zlib.h>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <map>
#include <stdexcept>
#include <string>
#include <vector>

namespace gnhost
{

inline std::string hip_error()
{
    return gn_last_error();
}

// One file's set in packed form (csrc/gn_packed_set.h; `ganon-build --hash-sets packed|spilled`): what the hasher leaves when the file
// is done.  A file hashed in one flush -- the common case -- is packed by the device and only the packed bytes are downloaded; a second
// flush unpacks the first into `raw`, the later ones append to it as without packing, and finish() unites them on the host and packs
// the result with the header's encoder.  word_at of the blocks counts from payload[0].
struct PackedFile
{
    std::vector<GnPackedBlock> blocks;
    std::vector<uint64_t>      payload, raw;
    uint64_t                   hashes  = 0;
    unsigned                   flushes = 0;
    void clear()
    {
        blocks.clear(), payload.clear(), raw.clear();
        hashes = 0, flushes = 0;
    }
    void finish()
    {
        if (flushes <= 1)
            return;
        std::sort(raw.begin(), raw.end());
        raw.erase(std::unique(raw.begin(), raw.end()), raw.end());
        blocks.clear(), payload.clear();
        gn_packed_encode(raw.data(), raw.size(), blocks, payload);
        hashes = raw.size();
        raw.clear();
    }
};

// One parser thread's device side: a stream on a placeholder filter (hashing does not look at the filter)
class Hasher
{
public:
    Hasher(int device, uint32_t k, uint32_t w) : k_(k), w_(w)
    {
        // pieces of `stride_` window starts; short enough for the lane-per-read minimiser kernel where it applies
        stride_ = w <= 128 ? 512 : 4096;
        gn_ibf_desc d{};
        d.bins = 64, d.bin_words = 1, d.bin_size = 64, d.hash_shift = 57, d.hash_funs = 1, d.rows = nullptr;
        std::vector<uint32_t> identity(64);
        for (uint32_t b = 0; b < 64; ++b)
            identity[b] = b;
        if (gn_filter_upload_ibf(device, &d, identity.data(), 64, &flt_) != GN_OK)
            throw std::runtime_error(hip_error());
        if (gn_stream_create(flt_, kMaxPieces, kMaxBases, 1, &st_) != GN_OK)
            throw std::runtime_error(hip_error());
        void* p = nullptr;
        if (gn_pinned_alloc(kMaxBases, &p) != GN_OK)
            throw std::runtime_error(hip_error());
        bases_ = static_cast<uint8_t*>(p);
        off_.reserve(kMaxPieces + 1);
        off_.push_back(0);
    }
    ~Hasher()
    {
        if (st_)
            gn_stream_destroy(st_);
        if (flt_)
            gn_filter_free(flt_);
        if (bases_)
            gn_pinned_free(bases_);
    }

    // add one sequence; `out` receives the distinct hashes of everything flushed so far for the current file
    void add(const uint8_t* seq, uint64_t len, std::vector<uint64_t>& out, unsigned& flushes) { add(seq, len, Sink{ &out, &flushes, nullptr }); }
    void flush(std::vector<uint64_t>& out, unsigned& flushes) { flush(Sink{ &out, &flushes, nullptr }); }
    void flush_short(std::vector<uint64_t>& out, unsigned& flushes) { flush_short(Sink{ &out, &flushes, nullptr }); }
    // the same with a packed output (call out.finish() behind the file's last flush)
    void add(const uint8_t* seq, uint64_t len, PackedFile& out) { add(seq, len, Sink{ &out.raw, &out.flushes, &out }); }
    void flush(PackedFile& out) { flush(Sink{ &out.raw, &out.flushes, &out }); }
    void flush_short(PackedFile& out) { flush_short(Sink{ &out.raw, &out.flushes, &out }); }

    // `--parse device`: what a file that went through hash_text_file adds to the build's totals
    struct TextTotals
    {
        uint64_t sequences = 0, skipped = 0, length_bp = 0, bytes = 0; // bytes: text uploaded
    };
    // A whole FASTA file as text: read in large blocks into the pinned buffer (gzopen serves plain and .gz alike), cut into chunks at
    // record or line boundaries (genome_chunks.hpp), tokenised and cut into pieces on the device (gn_stream_upload_genome_text), hashed as
    // after add().  Every chunk is one flush; records shorter than the window go to flush_short, so call it (and flush) behind the file as
    // after add().  false: the file is the sequential reader's -- an illegal letter, a line that is no header before the first one, no
    // newline in a buffer, a read error, or a record cut with fewer than max(w, min_length) letters so far; what went into `out` by then
    // is the caller's to discard, `tot` is only to be used after a true.
    bool hash_text_file(const std::string& path, uint64_t min_length, std::vector<uint64_t>& out, unsigned& flushes, TextTotals& tot)
    {
        return hash_text_file(path, min_length, Sink{ &out, &flushes, nullptr }, tot);
    }
    bool hash_text_file(const std::string& path, uint64_t min_length, PackedFile& out, TextTotals& tot)
    {
        return hash_text_file(path, min_length, Sink{ &out.raw, &out.flushes, &out }, tot);
    }
    // forget what add() and hash_text_file() have queued (a file that is read again from its start)
    void discard()
    {
        short_.clear();
        fill_ = 0;
        off_.assign(1, 0);
    }

private:
    struct Sink // where a device batch's set goes: appended to *raw, or -- a packed file's first batch -- into *packed
    {
        std::vector<uint64_t>* raw;
        unsigned*              flushes;
        PackedFile*            packed;
    };

    void add(const uint8_t* seq, uint64_t len, const Sink& to)
    {
        if (len < k_)
            return;
        if (len < w_)
        {
            short_[(uint32_t)len].append(reinterpret_cast<const char*>(seq), len);
            return;
        }
        for (uint64_t at = 0; at + w_ <= len; at += stride_)
        {
            const uint64_t n = std::min<uint64_t>(len - at, (uint64_t)stride_ + w_ - 1);
            if (fill_ + n > kMaxBases || off_.size() > kMaxPieces)
                flush(to);
            std::memcpy(bases_ + fill_, seq + at, n);
            fill_ += n;
            off_.push_back(fill_);
        }
    }

    void flush(const Sink& to)
    {
        if (off_.size() > 1)
            run(w_, to);
        fill_ = 0;
        off_.assign(1, 0);
    }

    // sequences shorter than the window: one launch per length, the window being the whole sequence
    void flush_short(const Sink& to)
    {
        for (auto& [len, cat] : short_)
        {
            for (size_t at = 0; at < cat.size();)
            {
                const size_t n_seq = std::min<size_t>((cat.size() - at) / len, std::min<size_t>(kMaxPieces, kMaxBases / len));
                std::memcpy(bases_, cat.data() + at, n_seq * len);
                off_.assign(1, 0);
                for (size_t i = 1; i <= n_seq; ++i)
                    off_.push_back(i * len);
                fill_ = n_seq * len;
                run(len, to);
                at += n_seq * len;
            }
        }
        short_.clear();
        fill_ = 0;
        off_.assign(1, 0);
    }

    // one device batch: enough for a bacterial genome in one go; every parser thread has its own (page-locked) copy, so the
    // size is also what start-up pays per thread
    static constexpr uint64_t kMaxBases  = 64ull << 20;
    static constexpr uint32_t kMaxPieces = 1u << 18;

    bool hash_text_file(const std::string& path, uint64_t min_length, const Sink& to, TextTotals& tot)
    {
        struct Gz
        {
            gzFile f;
            ~Gz()
            {
                if (f)
                    gzclose(f);
            }
        } gz{ gzopen(path.c_str(), "rb") };
        if (!gz.f)
            return false;
        gzbuffer(gz.f, 1 << 20);
        // a chunk's pieces repeat w - 1 letters every stride: chunk x (1 + (w - 1) / stride) plus slack has to fit a batch (where it does
        // not after all -- many short records -- the device takes a prefix and the rest is sent again)
        const uint64_t fit   = (kMaxBases - (1u << 20)) / (stride_ + w_ - 1) * stride_;
        const uint64_t chunk = std::clamp<uint64_t>(tun().size(Knob::build_parse_chunk, fit), 64, fit);
        tot                  = TextTotals{};
        uint64_t              fill = 0;
        bool                  eof = false, continues = false;
        std::vector<uint64_t> rec_at, rec_letters;
        std::vector<uint8_t>  rec_state;
        std::string           letters;
        while (!eof || fill)
        {
            while (!eof && fill < chunk)
            {
                const int n = gzread(gz.f, bases_ + fill, (unsigned)std::min<uint64_t>(chunk - fill, 1u << 30));
                if (n < 0)
                    return false;
                if (n == 0)
                    eof = true;
                fill += (uint64_t)n;
            }
            if (fill == 0)
                break;
            const GenomeCut cut = genome_cut(bases_, fill, eof);
            if (!cut.ok)
                return false;
            for (uint64_t at = 0; at < cut.cut;) // one upload, unless the device takes a prefix of the records
            {
                const uint32_t flags = (continues && at == 0 ? GN_GENOME_CONTINUES : 0u) | (cut.open ? GN_GENOME_OPEN_END : 0u);
                uint32_t       n_rec = 0, n_pieces = 0;
                uint64_t       n_bases = 0, parsed = 0, bad_at = 0, open_letters = 0;
                int            status = 0;
                if (gn_stream_upload_genome_text(st_, bases_ + at, cut.cut - at, w_, stride_, min_length, flags) != GN_OK)
                    throw std::runtime_error(hip_error());
                const int rc = gn_stream_genome_index(st_, &n_rec, &n_pieces, &n_bases, &parsed, &status, &bad_at, &open_letters);
                if (rc == GN_ERANGE || (rc == GN_OK && (status != 0 || parsed == 0)))
                    return false;
                if (rc != GN_OK)
                    throw std::runtime_error(hip_error());
                tot.bytes += cut.cut - at;
                rec_at.resize(n_rec), rec_letters.resize(n_rec), rec_state.resize(n_rec);
                if (gn_stream_genome_records(st_, rec_at.data(), rec_letters.data(), rec_state.data()) != GN_OK)
                    throw std::runtime_error(hip_error());
                for (uint32_t r = 0; r < n_rec; ++r) // a record is counted where it ends
                {
                    if (rec_state[r] == 3)
                    {
                        // the host path is the authority on a record that may still turn out shorter than --min-length or the window
                        if (open_letters < std::max<uint64_t>(w_, min_length))
                            return false;
                        continue;
                    }
                    if (rec_state[r] == 1)
                    {
                        tot.skipped++;
                        continue;
                    }
                    tot.sequences++;
                    tot.length_bp += rec_letters[r];
                    if (rec_state[r] == 2) // shorter than the window: its letters from the text, hashed by flush_short
                    {
                        if (r == 0 && (flags & GN_GENOME_CONTINUES))
                            return false; // (cannot be: an open record that short ended the device path at its cut)
                        const uint64_t end = r + 1 < n_rec ? rec_at[r + 1] : parsed;
                        if (!genome_record_letters(bases_ + at + rec_at[r], end - rec_at[r], letters))
                            return false;
                        add(reinterpret_cast<const uint8_t*>(letters.data()), letters.size(), to);
                    }
                }
                if (n_pieces)
                {
                    if (gn_stream_minimisers(st_, k_, w_) != GN_OK)
                        throw std::runtime_error(hip_error());
                    collect(to);
                }
                at += parsed;
            }
            continues = cut.open;
            std::memmove(bases_, bases_ + cut.cut, fill - cut.cut);
            fill -= cut.cut;
        }
        return true;
    }

    void run(uint32_t w, const Sink& to)
    {
        const uint32_t n = (uint32_t)off_.size() - 1;
        if (gn_stream_upload_reads(st_, bases_, fill_, off_.data(), nullptr, n) != GN_OK || gn_stream_minimisers(st_, k_, w) != GN_OK)
            throw std::runtime_error(hip_error());
        collect(to);
    }

    // the distinct hashes of the batch the stream has just hashed, into the sink
    void collect(const Sink& to)
    {
        const unsigned before = (*to.flushes)++;
        if (to.packed && before == 0) // the file's first batch: packed where it lies, only the packed bytes come back
        {
            PackedFile& pk = *to.packed;
            uint64_t    nb = 0, nw = 0;
            if (gn_stream_distinct_hashes_packed(st_, nullptr, 0, nullptr, 0, &pk.hashes, &nb, &nw) != GN_OK)
                throw std::runtime_error(hip_error());
            pk.blocks.resize(nb), pk.payload.resize(nw);
            if (nb && gn_stream_distinct_hashes_packed(st_, reinterpret_cast<gn_packed_block*>(pk.blocks.data()), nb, pk.payload.data(), nw, &pk.hashes, &nb,
                                                       &nw) != GN_OK)
                throw std::runtime_error(hip_error());
            return;
        }
        if (to.packed && before == 1) // a second batch after all: the first one's set joins the raw hashes, to be united at the end
            gn_packed_decode(to.packed->blocks.data(), to.packed->blocks.size(), to.packed->payload.data(), *to.raw);
        std::vector<uint64_t>& out = *to.raw;
        uint64_t               nd  = 0;
        if (gn_stream_distinct_hashes(st_, nullptr, 0, &nd) != GN_OK)
            throw std::runtime_error(hip_error());
        const size_t at = out.size();
        out.resize(at + nd);
        if (nd && gn_stream_distinct_hashes(st_, out.data() + at, nd, &nd) != GN_OK)
            throw std::runtime_error(hip_error());
    }

    uint32_t                        k_, w_, stride_;
    gn_filter*                      flt_ = nullptr;
    gn_stream*                      st_  = nullptr;
    uint8_t*                        bases_ = nullptr;
    uint64_t                        fill_  = 0;
    std::vector<uint64_t>           off_;
    std::map<uint32_t, std::string> short_;
};

} // namespace gnhost
