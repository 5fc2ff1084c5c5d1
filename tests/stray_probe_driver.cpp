// Stand-alone driver of tests/test_stray_probe_cpu.py: the drop tests of ganon_amd/csrc/gn_stray_probe.h -- the very functions both
// finish sites of the fast count kernel call -- against brute force, and the screen table the restatement in stray_probe_model.py
// must reproduce.  Built with -fsanitize=address,undefined as a program of its own; nothing is preloaded.
//   bound          n <= 12: every T, ds, hit pattern of rows 0 AND 1 over the screened hashes, every e: stage 1 drops exactly when no
//                  completion of the bits it has not seen reaches T; stage 2 never drops a bin that some completion lets reach T
//   counts         n <= 127, by counts: the same for stage 1; stage 2 drops whatever the one-stage rule dropped on the same words
//   table c h bins ds[n] and T[n], n = 1 .. 127
#include "gn_screen_table.h"
#include "gn_stray_probe.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>

static unsigned long long g_checked = 0;

static void fail(const char* what, uint32_t n, uint32_t T, uint32_t ds, uint32_t a, uint32_t b, uint32_t c)
{
    printf("FAIL %s: n %u T %u ds %u | %u %u %u\n", what, n, T, ds, a, b, c);
    exit(1);
}

static uint32_t popc(uint32_t x)
{
    return (uint32_t)__builtin_popcount(x);
}

static void bound(uint32_t nmax, uint32_t F)
{
    for (uint32_t n = 1; n <= nmax; ++n)
        for (uint32_t ds = 1; ds <= n; ++ds)
        {
            const uint32_t Fp = gn_probe_first(F, ds);
            if (Fp != (F < ds ? F : ds))
                fail("first", n, 0, ds, Fp, F, 0);
            for (uint32_t P = 0; P < (1u << ds); ++P) // bit q: rows 0 and 1 of hash q both have the bin's bit
            {
                const uint32_t c2 = popc(P), M = P & ((1u << Fp) - 1u), m = popc(M), rest = P >> Fp;
                // the most the hashes stage 1 has not looked at can add, by trying every completion: rows 2 AND 3 of the hashes
                // Fp <= q < ds (X; a hash counts only with its bit in P), every row of the hashes q >= ds (Y)
                uint32_t best_x = 0, best_y = 0;
                for (uint32_t X = 0; X < (1u << (ds - Fp)); ++X)
                    if (popc(X & rest) > best_x)
                        best_x = popc(X & rest);
                for (uint32_t Y = 0; Y < (1u << (n - ds)); ++Y)
                    if (popc(Y) > best_y)
                        best_y = popc(Y);
                for (uint32_t T = 1; T <= n; ++T)
                    for (uint32_t e = 0; e <= m; ++e) // hashes of M whose rows 2 and 3 have the bit too: the exact count over q < Fp
                    {
                        const bool drop = gn_probe_drop1(n, T, ds, c2, m, e), can = e + best_x + best_y >= T;
                        if (drop == can)
                            fail("stage 1", n, T, ds, P, e, drop);
                        ++g_checked;
                        if (drop || n > 10) // (stage 2 by patterns up to n = 10: the words it sees multiply the cases)
                            continue;
                        // stage 2 sees X but not which of those hashes are in P: what it drops, no P of the same c2 - m lets reach T
                        for (uint32_t X = 0; X < (1u << (ds - Fp)); ++X)
                        {
                            const uint32_t add = e + popc(X);
                            if (gn_probe_drop2(n, T, ds, add) && e + popc(X & rest) + best_y >= T)
                                fail("stage 2", n, T, ds, P, X, e);
                            // ... and the one-stage rule on the same words (y = hashes below Fp with rows 2 and 3, at least e) dropped no more
                            for (uint32_t y = e; y <= Fp - (m - e); ++y)
                                if (gn_probe_drop2(n, T, ds, y + popc(X)) && !gn_probe_drop2(n, T, ds, add))
                                    fail("stage 2 against one stage", n, T, ds, P, X, y);
                            ++g_checked;
                        }
                    }
            }
        }
}

static void counts(uint32_t F)
{
    for (uint32_t ds = 1; ds <= GN_SCREEN_NMAX; ++ds)
    {
        const uint32_t Fp = gn_probe_first(F, ds);
        const uint32_t rs[2] = {0u, GN_SCREEN_NMAX - ds};
        for (uint32_t ri = 0; ri < 2; ++ri)
        {
            const uint32_t r = rs[ri], n = ds + r; // hashes beyond the screen
            for (uint32_t T = 1; T <= n; ++T)
            {
                for (uint32_t c2 = 0; c2 <= ds; ++c2)
                    for (uint32_t m = 0; m <= Fp && m <= c2; ++m)
                    {
                        if (c2 - m > ds - Fp)
                            continue; // (more hits than hashes left)
                        for (uint32_t e = 0; e <= m; ++e)
                        {
                            const uint32_t most = e + (c2 - m) + r; // every hit hash not yet looked at passes, and every hash beyond ds
                            if (gn_probe_drop1(n, T, ds, c2, m, e) != (most < T))
                                fail("stage 1 by counts", n, T, ds, c2, m, e);
                            ++g_checked;
                        }
                    }
                for (uint32_t e = 0; e <= Fp; ++e)
                    for (uint32_t y = e; y <= Fp; ++y)
                        for (uint32_t x = 0; x <= ds - Fp; ++x)
                        {
                            const bool old_drop = gn_probe_drop2(n, T, ds, y + x), new_drop = gn_probe_drop2(n, T, ds, e + x);
                            if (new_drop != (e + x + r < T))
                                fail("stage 2 by counts", n, T, ds, e, x, 0);
                            if (old_drop && !new_drop)
                                fail("stage 2 against one stage by counts", n, T, ds, e, y, x);
                            ++g_checked;
                        }
            }
        }
    }
}

int main(int argc, char** argv)
{
    if (argc >= 2 && !strcmp(argv[1], "bound"))
    {
        bound(12, GN_PROBE_HASHES);
        bound(9, 0); // the one-stage probe: stage 1 sees nothing and never drops a bin the survey kept
        bound(9, 2);
    }
    else if (argc >= 2 && !strcmp(argv[1], "counts"))
    {
        counts(GN_PROBE_HASHES);
        counts(0);
    }
    else if (argc >= 5 && !strcmp(argv[1], "table"))
    {
        uint8_t ds[GN_SCREEN_NMAX + 1];
        gn_screen_table(atof(argv[2]), (uint32_t)atoi(argv[3]), (uint32_t)atoi(argv[4]), ds);
        for (uint32_t n = 1; n <= GN_SCREEN_NMAX; ++n)
            printf("%u %u\n", (unsigned)ds[n], gn_screen_cutoff_count(n, atof(argv[2])));
        return 0;
    }
    else
        return 2;
    printf("ok %llu F %u\n", g_checked, (unsigned)GN_PROBE_HASHES);
    return 0;
}
