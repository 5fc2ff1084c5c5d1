// build_verify_parts_driver.cpp -- test harness: runs the PRODUCT's carried state of a `--verify-index` in parts
// (ganon_amd/host/hibf_verify_parts.hpp, the very class the workers of build_verify_parts.cpp AND their answers into) so that
// tests/test_build_verify_parts_cpu.py can check it against a per-hash evaluation of its own.  One command per line of stdin; a bitmap is
// a string of '0' and '1', hash 0 first, or "-" for no hash:
//   new DEPTH N_UNITS SIZE...                 a fresh state
//   whole U D BITS                            a part that holds entry D's IBF whole answered: BITS = the hash is contained.  What the
//                                             worker does with the device's answer: alive ANDed, the lost ones counted
//   slab U D N_BINS BITS...                   a slab of entry D's IBF answered: per bin, "every row of the hash in this slab has the bit"
//   slabs2 U D N_BINS BITS... | BITS...       two workers' slabs, ANDed into planes of their own first and merged then (and_planes twice)
//   close U D                                 the IBF's last slab is through
//   report                                    per unit: "unit U found FIRST_LOST open_entries plane_words alive=BITS lost=L0,L1,..."
// Buffers are exactly as long as the words there are, and the program runs under AddressSanitizer and UBSan.
#include "../ganon_amd/host/hibf_verify_parts.hpp"

#include <iostream>
#include <memory>
#include <sstream>
#include <string>

using namespace gnbuild;

static std::vector<uint64_t> bitmap_of(const std::string& bits, uint64_t n, bool pad_ones)
{
    if ((bits == "-" ? 0 : bits.size()) != n)
        throw std::runtime_error("a bitmap of the wrong length");
    // (padding as the device leaves it: a plane's padding bits are whatever the lanes without a hash answered)
    std::vector<uint64_t> m(bitmap_words(n), pad_ones ? ~0ull : 0);
    for (uint64_t q = 0; q < n; ++q)
        m[q / 64] = (m[q / 64] & ~(1ull << (q % 64))) | ((uint64_t)(bits[q] == '1') << (q % 64));
    return m;
}

static std::vector<uint64_t> planes_of(std::istringstream& in, uint32_t n_bins, uint64_t n, bool pad_ones)
{
    std::vector<uint64_t> out;
    for (uint32_t b = 0; b < n_bins; ++b)
    {
        std::string bits;
        in >> bits;
        const std::vector<uint64_t> m = bitmap_of(bits, n, pad_ones);
        out.insert(out.end(), m.begin(), m.end());
    }
    return out;
}

int main()
{
    std::unique_ptr<VerifyCarry> st;
    for (std::string line; std::getline(std::cin, line);)
    {
        std::istringstream in(line);
        std::string        cmd;
        if (!(in >> cmd))
            continue;
        if (cmd == "new")
        {
            uint32_t depth = 0;
            size_t   n     = 0;
            in >> depth >> n;
            std::vector<uint64_t> sizes(n);
            for (uint64_t& s : sizes)
                in >> s;
            st.reset(new VerifyCarry(sizes, depth));
        }
        else if (cmd == "whole")
        {
            size_t      u;
            uint32_t    d;
            std::string bits;
            in >> u >> d >> bits;
            const uint64_t              n   = st->size(u);
            const std::vector<uint64_t> hit = bitmap_of(bits, n, true);
            std::vector<uint64_t>       alive = bitmap_ones(n);
            uint64_t                    lost = 0;
            for (uint64_t w = 0; w < alive.size(); ++w)
            {
                lost += (uint64_t)__builtin_popcountll(bitmap_valid(n, w) & ~hit[w]);
                alive[w] &= hit[w];
            }
            st->and_alive(u, alive.data());
            st->add_lost(u, d, lost);
        }
        else if (cmd == "slab" || cmd == "slabs2")
        {
            size_t   u;
            uint32_t d, n_bins;
            in >> u >> d >> n_bins;
            const uint64_t        n = st->size(u);
            std::vector<uint64_t> a = planes_of(in, n_bins, n, true);
            st->and_planes(u, d, n_bins, a.data());
            if (cmd == "slabs2")
            {
                std::string bar;
                in >> bar;
                std::vector<uint64_t> b = planes_of(in, n_bins, n, false);
                st->and_planes(u, d, n_bins, b.data());
            }
        }
        else if (cmd == "close")
        {
            size_t   u;
            uint32_t d;
            in >> u >> d;
            st->close(u, d);
        }
        else if (cmd == "report")
        {
            for (size_t u = 0; u < st->units(); ++u)
            {
                std::cout << "unit " << u << " " << st->found(u) << " " << (long long)st->first_lost(u) << " " << st->open_entries() << " " << st->plane_words()
                          << " alive=";
                for (uint64_t q = 0; q < st->size(u); ++q)
                    std::cout << ((st->alive(u)[q / 64] >> (q % 64)) & 1);
                if (st->size(u) == 0)
                    std::cout << "-";
                std::cout << " lost=";
                for (uint32_t d = 0; d < st->depth(); ++d)
                    std::cout << (d ? "," : "") << st->lost_at(u, d);
                std::cout << "\n";
            }
        }
        else
        {
            std::cerr << "unknown command " << cmd << "\n";
            return 2;
        }
        if (!in)
        {
            std::cerr << "short line: " << line.substr(0, 80) << "\n";
            return 2;
        }
    }
    return 0;
}
