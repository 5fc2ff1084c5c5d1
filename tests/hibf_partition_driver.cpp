// hibf_partition_driver.cpp -- stand-alone program around host/hibf_partition.hpp (tests/test_hibf_partition_cpu.py builds it with
// -fsanitize=address,undefined and runs it directly; no device, no library).
//
// stdin, any number of cases:   n_ibf n_user_bins
//                               per IBF: bins bin_size, then `bins` pairs  next_ibf_id bin_to_user
//                               n_budgets, then the budgets
// stdout per case:              "refusal <text>"  or
//                               "parts K units U", per part "part slot unit_lo unit_hi bin_lo bin_hi word_lo word_hi bytes n_ibf n_user",
//                               "ibfs ...", "users ...", per local IBF "ibf bins bin_words bin_size" + "next ..." + "user ..."
#include "../ganon_amd/host/hibf_partition.hpp"

#include <iostream>

// the row stride libganon_hip gives an IBF of an HIBF (gn_hibf_row_stride_words): whole 128-byte lines
static uint64_t stride(uint64_t w)
{
    if (w >= 16)
        return (w + 15) & ~15ull;
    uint64_t p = 1;
    while (p < w)
        p <<= 1;
    return p;
}

int main()
{
    std::ios::sync_with_stdio(false);
    size_t n_ibf;
    while (std::cin >> n_ibf)
    {
        gnhost::FilterMeta f;
        f.is_hibf = true;
        std::cin >> f.n_user_bins;
        f.shapes.resize(n_ibf);
        f.next_ibf_id.resize(n_ibf);
        f.bin_to_user.resize(n_ibf);
        for (size_t i = 0; i < n_ibf; ++i)
        {
            gnhost::IbfShape& m = f.shapes[i];
            std::cin >> m.bins >> m.bin_size;
            m.bin_words      = (m.bins + 63) >> 6;
            m.technical_bins = m.bin_words * 64;
            m.hash_funs      = 2;
            m.hash_shift     = m.bin_size ? (uint64_t)__builtin_clzll(m.bin_size) : 0;
            f.next_ibf_id[i].resize(m.bins);
            f.bin_to_user[i].resize(m.bins);
            for (uint64_t b = 0; b < m.bins; ++b)
                std::cin >> f.next_ibf_id[i][b] >> f.bin_to_user[i][b];
        }
        size_t nb;
        std::cin >> nb;
        std::vector<uint64_t> budgets(nb);
        for (auto& b : budgets)
            std::cin >> b;
        if (!std::cin)
        {
            std::cerr << "truncated case\n";
            return 2;
        }
        const gnhost::HibfPlan plan = gnhost::plan_hibf_partition(f, budgets, stride);
        if (!plan.refusal.empty())
        {
            std::cout << "refusal " << plan.refusal << "\n";
            continue;
        }
        std::cout << "parts " << plan.parts.size() << " units " << plan.n_units << "\n";
        for (auto const& p : plan.parts)
        {
            std::cout << "part " << p.slot << ' ' << p.unit_lo << ' ' << p.unit_hi << ' ' << p.bin_lo << ' ' << p.bin_hi << ' ' << p.word_lo << ' '
                      << p.word_hi << ' ' << p.bytes << ' ' << p.ibf_global.size() << ' ' << p.user_global.size() << "\n";
            std::cout << "ibfs";
            for (uint32_t g : p.ibf_global)
                std::cout << ' ' << g;
            std::cout << "\nusers";
            for (uint32_t u : p.user_global)
                std::cout << ' ' << u;
            std::cout << "\n";
            for (size_t i = 0; i < p.shapes.size(); ++i)
            {
                std::cout << "ibf " << p.shapes[i].bins << ' ' << p.shapes[i].bin_words << ' ' << p.shapes[i].bin_size << "\nnext";
                for (int64_t x : p.next_ibf_id[i])
                    std::cout << ' ' << x;
                std::cout << "\nuser";
                for (int64_t x : p.bin_to_user[i])
                    std::cout << ' ' << x;
                std::cout << "\n";
            }
        }
    }
    return 0;
}
