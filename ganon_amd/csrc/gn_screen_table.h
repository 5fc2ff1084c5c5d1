// gn_screen_table.h -- how many hashes of a read the fast count kernel screens on rows 0 and 1 alone (host side, no device code).
//
// The kernel's screened flow (gn_kernels.hip) fetches, for the first ds hashes of a read, only two of the h rows, counts per bin the
// hashes whose two rows both have the bin's bit (c2 >= the true count c4), and then keeps the bins with c2 >= T - (n - ds): the
// others cannot reach the cutoff count T any more.  No bin left: the read is done after 2 ds row fetches.  A few left: their exact
// counts are fetched word by word.  Too many: the read starts again in the unscreened flow.  The table only chooses ds, so it
// decides speed, never results.
//
// Model: every bit of a row is set with probability 1/2, independently -- the density a Bloom filter sized for its false-positive
// rate sits at or below.  A bin that holds nothing of the read then passes both rows of a hash with probability 1/4, and
//     surv(n, d) = bins * P[Bin(d, 1/4) >= T - (n - d)]
// bins of the unit are expected to be left after d hashes.  ds[n] is the smallest d <= n with surv(n, d) <= 1/2, if under the same
// model the screened flow asks for fewer 128-byte lines than the unscreened one:
//     screened   = 2 ds rows + surv(n, ds) * 2 ds word loads (a stray bin's finish probes rows 2 and 3 of the screened hashes and drops it)
//     unscreened = (the first of its check points at which bins * P[Bin(d, 1/16) >= T - (n - d)] <= 1/2 -- all h rows of a hash hit
//                  a stray bin with probability 1/16 -- plus the iteration in flight there) * h rows; every row when it has none
// with rows of unit_bins / 1024 lines.  Otherwise, and for T = 1 (nothing can be ruled out) and h != 4, ds[n] = 0.
// (h = 5 stays unscreened: the screen's register sets and wait counts are those of four loads an iteration.)
#pragma once
#include <cmath>
#include <cstdint>

#define GN_SCREEN_NMAX 127u // reads with more minimisers never reach the fast kernel's main loop

// T of a read with n minimisers, computed as the kernels do (GanonClassify.cpp:492-495, 720-724)
inline uint32_t gn_screen_cutoff_count(uint32_t n, double rel_cutoff)
{
    volatile double prod = (double)n * rel_cutoff; // (one rounded product, as __dmul_rn on the device)
    const uint32_t  T    = (uint32_t)(uint64_t)std::ceil(prod);
    return T ? T : 1u;
}

// t[d][k] = P[Bin(d, p) >= k] for d <= 127, from pmf(d, k) = (1 - p) pmf(d - 1, k) + p pmf(d - 1, k - 1)
struct GnScreenTail
{
    double t[GN_SCREEN_NMAX + 1][GN_SCREEN_NMAX + 2];
    explicit GnScreenTail(double p)
    {
        double pmf[2][GN_SCREEN_NMAX + 2] = {};
        pmf[0][0] = 1.0;
        for (uint32_t d = 0; d <= GN_SCREEN_NMAX; ++d)
        {
            double* cur = pmf[d & 1];
            if (d)
                for (uint32_t k = 0; k <= d; ++k)
                    cur[k] = (1.0 - p) * (k < d ? pmf[(d - 1) & 1][k] : 0.0) + p * (k ? pmf[(d - 1) & 1][k - 1] : 0.0);
            t[d][d + 1] = 0.0;
            for (uint32_t k = d + 1; k-- > 0;)
                t[d][k] = t[d][k + 1] + cur[k];
        }
    }
};

inline void gn_screen_table(double rel_cutoff, uint32_t hash_funs, uint32_t unit_bins, uint8_t ds[GN_SCREEN_NMAX + 1])
{
    for (uint32_t n = 0; n <= GN_SCREEN_NMAX; ++n)
        ds[n] = 0;
    if (hash_funs != 4 || unit_bins == 0)
        return;
    static const GnScreenTail two(0.25), all(0.0625); // (built once, by whichever thread comes first)
    const double row_lines = unit_bins > 1024u ? (double)unit_bins / 1024.0 : 1.0;
    for (uint32_t n = 1; n <= GN_SCREEN_NMAX; ++n)
    {
        const uint32_t T = gn_screen_cutoff_count(n, rel_cutoff);
        if (T < 2 || T > n)
            continue;
        // the unscreened flow's check points, as the kernel sets them with one hash an iteration: from one before the half-way bound
        // to two after it, if that leaves an iteration to save
        uint32_t       its = n;
        const uint32_t c   = 2 * (n - T + 1);
        if (c + 2 <= n)
            for (uint32_t d = c - 1; d <= c + 2 && d + 1 < n; ++d)
                if (d + T > n && (double)unit_bins * all.t[d][T - (n - d)] <= 0.5)
                {
                    its = d + 1;
                    break;
                }
        for (uint32_t d = n - T + 1; d <= n; ++d) // (the bound T - (n - d) is at least 1 from here on)
        {
            const double surv = (double)unit_bins * two.t[d][T - (n - d)];
            if (surv > 0.5)
                continue;
            const double screened   = 2.0 * d * row_lines + surv * 2.0 * d;
            const double unscreened = (double)its * hash_funs * row_lines;
            if (screened < unscreened)
                ds[n] = (uint8_t)d;
            break;
        }
    }
}
