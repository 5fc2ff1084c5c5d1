// hibf_verify_parts.hpp -- the state `ganon-build --hibf --verify-index` carries from part to part when the index is checked in parts
// (--verify-memory / --verify-devices; the plan is hibf_build_parts.hpp's, the workers are build_verify_parts.cpp).  An insert could be
// cut freely, an OR does not care; a lookup does: a hash is in a run of bins only if ONE bin has its bit in all h rows, the rows may lie
// in different row slabs of a cut IBF, and "missing" counts distinct hashes over all levels, which lie in different parts.  So, per unit
// (a target with its sorted distinct hashes in the membership pass, a user bin with the 65 536 probes in the false-positive pass):
//   alive     one bit per hash: word q / 64, bit q % 64 for hash q.  Valid bits start as 1, the padding bits of the last word as 0.
//             A bit goes when some entry of the unit's path does not contain the hash.
//   lost_at   per path entry: the hashes that entry does not contain, each entry counted on its own.
//   planes    per path entry whose IBF is cut into slabs: n_bins bitmaps of the same length, plane b = "every row of hash q seen so far
//             has the bit of bin first_bin + b".  They start as all ones, every slab's answer is ANDed in, and when the IBF's last slab
//             is through the entry is CLOSED:  hit = OR over b of plane[b];  lost_at += popcount(valid & ~hit);  alive &= hit;  the planes
//             are freed.  An entry whose IBF is whole in its part needs none: its answer per hash is final.
// After the last part found = popcount(alive) and first_lost = the index of the first zero valid bit -- the three numbers the report
// prints.  A hash lost at two levels, or in two slabs of one level, is one zero bit: it is counted once.
// Memory: 1 bit per hash, and for a unit with a run in a cut IBF another n_bins bits per hash while that IBF's group of parts runs.  A
// worker answers a part into bitmaps of its own (the same figures, for the units of the part in flight only) and ANDs them in here
// under the owner's lock: two calls never AND into the same words at the same time.
// Pure host code, no device call: the test driver (tests/build_verify_parts_driver.cpp) compiles it on its own.
#pragma once

#include <cstdint>
#include <map>
#include <stdexcept>
#include <utility>
#include <vector>

namespace gnbuild
{

inline uint64_t bitmap_words(uint64_t n)
{
    return (n + 63) / 64;
}

// the bits of word w of a bitmap of n bits that stand for a hash
inline uint64_t bitmap_valid(uint64_t n, uint64_t w)
{
    if (w * 64 >= n)
        return 0;
    const uint64_t left = n - w * 64;
    return left >= 64 ? ~0ull : (1ull << left) - 1;
}

// a bitmap of n bits, every valid bit set
inline std::vector<uint64_t> bitmap_ones(uint64_t n)
{
    std::vector<uint64_t> m(bitmap_words(n));
    for (uint64_t w = 0; w < m.size(); ++w)
        m[w] = bitmap_valid(n, w);
    return m;
}

inline uint64_t bitmap_count(const uint64_t* m, uint64_t n)
{
    uint64_t c = 0;
    for (uint64_t w = 0; w < bitmap_words(n); ++w)
        c += (uint64_t)__builtin_popcountll(m[w] & bitmap_valid(n, w));
    return c;
}

// the index of the first zero valid bit, ~0 when there is none
inline uint64_t bitmap_first_zero(const uint64_t* m, uint64_t n)
{
    for (uint64_t w = 0; w < bitmap_words(n); ++w)
    {
        const uint64_t z = ~m[w] & bitmap_valid(n, w);
        if (z)
            return w * 64 + (uint64_t)__builtin_ctzll(z);
    }
    return ~0ull;
}

// The closing rule on bare words: n_bins planes of bitmap_words(n) words behind each other; returns popcount(valid & ~hit) and ANDs hit
// into alive.
inline uint64_t close_planes(const uint64_t* planes, uint32_t n_bins, uint64_t n, uint64_t* alive)
{
    const uint64_t words = bitmap_words(n);
    uint64_t       lost  = 0;
    for (uint64_t w = 0; w < words; ++w)
    {
        uint64_t hit = 0;
        for (uint32_t b = 0; b < n_bins; ++b)
            hit |= planes[(uint64_t)b * words + w];
        lost += (uint64_t)__builtin_popcountll(bitmap_valid(n, w) & ~hit);
        alive[w] &= hit;
    }
    return lost;
}

class VerifyCarry
{
public:
    VerifyCarry(std::vector<uint64_t> sizes, uint32_t depth) : sizes_(std::move(sizes)), depth_(depth), lost_at_(sizes_.size() * (size_t)depth, 0)
    {
        for (uint64_t n : sizes_)
            alive_.push_back(bitmap_ones(n));
    }
    size_t   units() const { return sizes_.size(); }
    uint32_t depth() const { return depth_; }
    uint64_t size(size_t u) const { return sizes_.at(u); }

    // what a part answered for unit u, ANDed in.  `src`: bitmap_words(size(u)) words
    void and_alive(size_t u, const uint64_t* src)
    {
        std::vector<uint64_t>& a = alive_.at(u);
        for (size_t w = 0; w < a.size(); ++w)
            a[w] &= src[w];
    }
    void add_lost(size_t u, uint32_t d, uint64_t n) { lost_at_.at(u * depth_ + d) += n; }
    // a slab's answer for entry d of unit u: n_bins planes behind each other; the first one finds planes of all ones
    void and_planes(size_t u, uint32_t d, uint32_t n_bins, const uint64_t* src)
    {
        if (d >= depth_ || n_bins == 0)
            throw std::invalid_argument("VerifyCarry: no such entry");
        const size_t            words = bitmap_words(sizes_.at(u)) * n_bins;
        auto                    at = planes_.find({ u, d });
        if (at == planes_.end())
            at = planes_.emplace(std::make_pair(u, d), Planes{ n_bins, std::vector<uint64_t>(words, ~0ull) }).first;
        if (at->second.n_bins != n_bins)
            throw std::invalid_argument("VerifyCarry: an entry's slabs disagree on its bins");
        for (size_t w = 0; w < words; ++w)
            at->second.words[w] &= src[w];
    }
    // the last slab of the entry's IBF is through.  An entry that no slab answered has nothing to close.
    void close(size_t u, uint32_t d)
    {
        auto at = planes_.find({ u, d });
        if (at == planes_.end())
            return;
        lost_at_[u * depth_ + d] += close_planes(at->second.words.data(), at->second.n_bins, sizes_[u], alive_[u].data());
        planes_.erase(at);
    }

    const uint64_t* alive(size_t u) const { return alive_.at(u).data(); }
    uint64_t        found(size_t u) const { return bitmap_count(alive_.at(u).data(), sizes_[u]); }
    uint64_t        first_lost(size_t u) const { return bitmap_first_zero(alive_.at(u).data(), sizes_[u]); }
    uint64_t        lost_at(size_t u, uint32_t d) const { return lost_at_.at(u * depth_ + d); }
    size_t          open_entries() const { return planes_.size(); }
    uint64_t        plane_words() const // the planes alive now
    {
        uint64_t n = 0;
        for (const auto& kv : planes_)
            n += kv.second.words.size();
        return n;
    }

private:
    struct Planes
    {
        uint32_t              n_bins;
        std::vector<uint64_t> words;
    };
    std::vector<uint64_t>                                 sizes_;
    uint32_t                                              depth_;
    std::vector<std::vector<uint64_t>>                    alive_;
    std::vector<uint64_t>                                 lost_at_;
    std::map<std::pair<size_t, uint32_t>, Planes>         planes_;
};

} // namespace gnbuild
