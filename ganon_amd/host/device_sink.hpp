// device_sink.hpp -- a filter file's bits into HBM of one device through the streaming loader (filter_io.hpp), for the tools that
// look things up in a file on one device: `ganon-classify --verify-filter` (a flat .ibf), `ganon-build --hibf --verify-index` and
// `--update` (a .hibf).  DeviceSet (placement.hpp) does the same for a replica that classify workers share.
// Also here, for them and for the builds: the owners of the two library handles a tool holds by hand -- whoever leaves a scope early,
// by return or by exception, gives the device filter and the page-locked block back -- and the one place that fills a gn_ibf_desc.
#pragma once

#include "filter_io.hpp"

#include "ganon_hip.h"

#include <memory>
#include <string>
#include <vector>

namespace gnhost
{

struct FilterFree
{
    void operator()(gn_filter* f) const { gn_filter_free(f); }
};
using OwnedFilter = std::unique_ptr<gn_filter, FilterFree>; // reset() frees the device memory at once

// page-locked host memory from gn_pinned_alloc
class PinnedBlock
{
public:
    // makes get() a block of at least `bytes`: the one held when it is large enough, otherwise a new one in its place (the contents
    // are not kept; nothing is asked for 0 bytes).  false when the library has none to give (gn_last_error says why)
    bool reserve(size_t bytes)
    {
        if (bytes_ < bytes)
        {
            ptr_.reset(), bytes_ = 0;
            void* p = nullptr;
            if (gn_pinned_alloc(bytes, &p) != GN_OK)
                return false;
            ptr_.reset(p), bytes_ = bytes;
        }
        return true;
    }
    void* get() const { return ptr_.get(); }

private:
    struct Free
    {
        void operator()(void* p) const { gn_pinned_free(p); }
    };
    std::unique_ptr<void, Free> ptr_;
    size_t                      bytes_ = 0;
};

// an IBF of `bins` bins and `rows` rows, its storage allocated zero-filled on the device
inline gn_ibf_desc ibf_desc(uint64_t bins, uint64_t rows, uint64_t hash_funs)
{
    gn_ibf_desc d{};
    d.rows       = nullptr;
    d.bin_size   = rows;
    d.bin_words  = (bins + 63) >> 6;
    d.bins       = bins;
    d.hash_funs  = (uint32_t)hash_funs;
    d.hash_shift = (uint32_t)__builtin_clzll(rows);
    return d;
}

// the IBFs of a hierarchical filter as gn_filter_upload_hibf takes them; the tables stay the caller's
struct HibfDescs
{
    std::vector<gn_ibf_desc>    descs;
    std::vector<const int64_t*> next_ibf_id, bin_to_user;
    void add(uint64_t bins, uint64_t rows, uint64_t hash_funs, const std::vector<int64_t>& next, const std::vector<int64_t>& user)
    {
        descs.push_back(ibf_desc(bins, rows, hash_funs));
        next_ibf_id.push_back(next.data()), bin_to_user.push_back(user.data());
    }
    OwnedFilter upload(int device, uint64_t n_user_bins) const // null: gn_last_error says why
    {
        gn_filter* f  = nullptr;
        const int  rc = gn_filter_upload_hibf(device, (uint32_t)descs.size(), descs.data(), next_ibf_id.data(), bin_to_user.data(), n_user_bins, &f);
        return OwnedFilter(rc == GN_OK ? f : nullptr);
    }
};

// a flat IBF, likewise; bin2target == nullptr: storage only, no bin map (the builder's)
inline OwnedFilter upload_ibf(int device, uint64_t bins, uint64_t rows, uint64_t hash_funs, const uint32_t* bin2target, uint32_t n_targets)
{
    const gn_ibf_desc d = ibf_desc(bins, rows, hash_funs);
    gn_filter*        f = nullptr;
    const int         rc = gn_filter_upload_ibf(device, &d, bin2target, n_targets, &f);
    return OwnedFilter(rc == GN_OK ? f : nullptr);
}

class DeviceSink final : public FilterSink
{
public:
    explicit DeviceSink(int device) : device_(device) {}
    bool begin(const FilterMeta& f, std::string& err) override
    {
        words_.clear();
        for (const IbfShape& m : f.shapes) // (the loader has checked bin_words and hash_shift against bins and bin_size)
            words_.push_back(m.bin_words);
        if (f.is_hibf)
        {
            HibfDescs d;
            for (size_t i = 0; i < f.shapes.size(); ++i)
                d.add(f.shapes[i].bins, f.shapes[i].bin_size, f.shapes[i].hash_funs, f.next_ibf_id[i], f.bin_to_user[i]);
            f_ = d.upload(device_, f.n_user_bins);
        }
        else
        {
            const IbfShape&       m = f.shapes.at(0);
            std::vector<uint32_t> bin2target(m.bins, 0xFFFFFFFFu);
            for (size_t t = 0; t < f.targets.size(); ++t)
                for (uint64_t b : f.target_bins[t])
                    bin2target[b] = (uint32_t)t;
            f_ = upload_ibf(device_, m.bins, m.bin_size, m.hash_funs, bin2target.data(), (uint32_t)f.targets.size());
        }
        return f_ || failed(err);
    }
    uint64_t* staging(int which, size_t bytes) override
    {
        PinnedBlock& s = stage_[which & 1];
        return s.reserve(bytes) ? static_cast<uint64_t*>(s.get()) : nullptr;
    }
    bool rows(uint32_t ibf, uint64_t row_begin, uint64_t n_rows, const uint64_t* src, std::string& err) override
    {
        return gn_filter_write_rows(f_.get(), ibf, row_begin, n_rows, src, words_.at(ibf), 0) == GN_OK || failed(err);
    }
    bool drain(std::string& err) override { return gn_filter_write_sync(f_.get()) == GN_OK || failed(err); }
    bool end(std::string& err) override { return gn_filter_finalize(f_.get()) == GN_OK || failed(err); }
    gn_filter* filter() const { return f_.get(); }

private:
    static bool failed(std::string& err)
    {
        err = gn_last_error();
        return false;
    }
    int                   device_;
    std::vector<uint64_t> words_;
    PinnedBlock           stage_[2];
    OwnedFilter           f_; // (freed before the stages)
};

} // namespace gnhost
