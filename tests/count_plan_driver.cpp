// Stand-alone driver of tests/test_count_plan_cpu.py: ganon_amd/csrc/gn_count_plan.h -- the very function gn_run_count_range calls -- on
// cases read from stdin.  Built with -fsanitize=address,undefined as a program of its own; nothing is preloaded.
//   (no argument)          one case per stdin line, `key=value` tokens over the defaults of GnCountPlanIn (switches: sw=name,name), one plan
//                          per stdout line as JSON
//   screen c h unit_bins   how many n in 1 .. 127 gn_screen_table gives a screen
#include "gn_count_plan.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

static bool set_field(GnCountPlanIn& in, const std::string& k, const char* v)
{
    const unsigned long long u = strtoull(v, nullptr, 0);
#define B(name) if (k == #name) { in.name = u != 0; return true; }
#define U(name) if (k == #name) { in.name = (decltype(in.name))u; return true; }
    B(is_hibf) B(identity) B(split_table) B(csr_identity) B(run_ok) B(unit_list) B(long_reads) B(pf_on) B(pf_merge) B(pf_joint) B(pf_segmin)
    U(h) U(W) U(S) U(lw) U(wpr) U(gp_log2) U(rpb) U(block) U(lds_bytes) U(split_lds_bytes) U(n_cu) U(split_bpc) U(uniform_nb)
    U(stream_rows_min_bytes) U(pf_segmin_cap) U(lo) U(hi) U(n_reads)
#undef B
#undef U
    if (k == "prev_count_deferred" || k == "prev_unit_deferred")
    {
        (k == "prev_count_deferred" ? in.prev_count_deferred : in.prev_unit_deferred) = !strcmp(v, "unknown") ? ~0ull : u;
        return true;
    }
    if (k == "rel_cutoff" || k == "pf_rel_filter")
    {
        (k == "rel_cutoff" ? in.rel_cutoff : in.pf_rel_filter) = atof(v);
        return true;
    }
    if (k == "emit_probe")
    {
        in.sw.emit_probe = (uint32_t)u;
        return true;
    }
    return false;
}

static bool set_switch(GnCountPlanSw& sw, const std::string& k)
{
#define S(name) if (k == #name) { sw.name = true; return true; }
    S(early_exit) S(row_screen) S(lean_screen) S(stream_rows) S(stray_masks) S(cand_select) S(csr_identity) S(uniform_select) S(run_select)
    S(max_first) S(const_nb) S(split_kernel) S(predrop) S(deferred_grids) S(on_demand) S(fake_count)
#undef S
    return false;
}

int main(int argc, char** argv)
{
    if (argc >= 5 && !strcmp(argv[1], "screen"))
    {
        uint8_t  ds[GN_SCREEN_NMAX + 1];
        uint32_t n_screened = 0;
        gn_screen_table(atof(argv[2]), (uint32_t)atoi(argv[3]), (uint32_t)atoi(argv[4]), ds);
        for (uint32_t n = 1; n <= GN_SCREEN_NMAX; ++n)
            n_screened += ds[n] != 0;
        printf("%u\n", n_screened);
        return 0;
    }
    static const char* const family[] = {"split", "lean", "fast", "generic", "long"};
    static const char* const list[]   = {"none", "deferred", "units"};
    static const char* const clear[]  = {"skipped", "pre", "segmin", "deferred", "unit_cursor", "units_left", "long"};
    char line[4096];
    while (fgets(line, sizeof line, stdin))
    {
        GnCountPlanIn in;
        for (char* tok = strtok(line, " \n"); tok; tok = strtok(nullptr, " \n"))
        {
            char* eq = strchr(tok, '=');
            if (!eq)
                return 2;
            const std::string k(tok, eq);
            bool              ok = true;
            if (k == "sw")
                for (std::string rest(eq + 1); ok && !rest.empty();)
                {
                    const size_t c = rest.find(',');
                    ok   = set_switch(in.sw, rest.substr(0, c));
                    rest = c == std::string::npos ? "" : rest.substr(c + 1);
                }
            else
                ok = set_field(in, k, eq + 1);
            if (!ok)
            {
                fprintf(stderr, "unknown token %s\n", tok);
                return 2;
            }
        }
        GnCountPlan pl;
        gn_count_plan(in, &pl);
        if (pl.n_launches > GN_COUNT_MAX_LAUNCHES)
            return 3;
        printf("{\"launches\": [");
        for (uint32_t i = 0; i < pl.n_launches; ++i)
        {
            const GnCountLaunch& L = pl.launch[i];
            printf("%s{\"family\": \"%s\", \"key\": [%u, %u, %u, %u, %u], \"stream\": %u, \"blocks\": %u, \"lds\": %llu, \"in\": \"%s\", \"out\": \"%s\", \"grab\": %u}",
                   i ? ", " : "", family[L.family], (unsigned)L.HF, (unsigned)L.LW, (unsigned)L.EE, (unsigned)L.WIDE, (unsigned)L.SCRN, (unsigned)L.stream,
                   L.blocks, (unsigned long long)L.lds_bytes, list[L.list_in], list[L.list_out], (unsigned)L.grab);
        }
        uint32_t n_screened = 0;
        for (uint32_t n = 0; n <= GN_SCREEN_NMAX; ++n)
            n_screened += pl.screen[n] != 0;
        printf("], \"early_exit\": %u, \"probe_hashes\": %u, \"emit_probe\": %u, \"csr_identity\": %u, \"uniform_nb\": %u, \"run_select\": %u, \"max_first\": %u, "
               "\"const_nb\": %u, \"pre_mode\": %u, \"bin_nb2\": %u, \"screen_filled\": %u, \"screen_unit_bins\": %u, \"n_screened\": %u, \"predrop\": %u, "
               "\"fake_count\": %u, \"streamed\": %u, \"clear\": [",
               pl.early_exit, pl.probe_hashes, pl.emit_probe, pl.csr_identity, pl.uniform_nb, pl.run_select, pl.max_first, pl.const_nb, pl.pre_mode,
               (unsigned)pl.bin_nb2, (unsigned)pl.screen_filled, pl.screen_unit_bins, n_screened, (unsigned)pl.predrop, (unsigned)pl.fake_count, (unsigned)pl.streamed);
        bool first = true;
        for (uint32_t b = 0; b < 7; ++b)
            if (pl.clear & (1u << b))
            {
                printf("%s\"%s\"", first ? "" : ", ", clear[b]);
                first = false;
            }
        printf("]}\n");
    }
    return 0;
}
