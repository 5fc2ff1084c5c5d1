    extern __shared__ __attribute__((aligned(16))) uint32_t gn_lds[];
    constexpr int      HF   = 4;
    constexpr int      ND   = 2;
    constexpr uint32_t NMAX = 127;

    const int      lane   = threadIdx.x & (GN_WAVE - 1);
    const int      wave   = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint32_t wpr    = p.wpr;
    uint32_t*      rowtab = gn_lds + (size_t)wave * 128 * HF;
    // hit masks of the first GN_PROBE_HASHES screened hashes, dword (q * ND + d) * 64 + lane: in LDS (2 KiB a wave), there is no register for them
    uint32_t*      pmask  = gn_lds + (size_t)(blockDim.x >> 6) * 128 * HF + (size_t)wave * (GN_PROBE_HASHES * ND * GN_WAVE);

    // units are handed out as in gn_ibf_count_fast_kernel
    const uint64_t n_units = (uint64_t)(p.n_reads - p.read_begin) * wpr;
    const uint64_t stride  = (uint64_t)gridDim.x * (blockDim.x >> 6);
    uint64_t       unit    = (uint64_t)blockIdx.x * (blockDim.x >> 6) + wave;
    if (unit >= n_units)
        return;
    const bool     dyn      = p.grab != nullptr && n_units >= 64u * stride;
    const uint64_t dyn_from = stride * 16u;
    uint64_t       chunk_end = unit + 1;
    if (dyn)
    {
        unit *= 16u;
        chunk_end = unit + 16u;
    }
    unsigned long long g_next = 0;
    uint32_t           g_size = 16u;
    auto               ask    = [&](uint64_t from) {
        g_size = from < n_units - n_units / 4u ? 16u : (from < n_units - n_units / 16u ? 8u : 4u);
        if (lane == 0)
            g_next = atomicAdd(p.grab, (unsigned long long)g_size);
    };
    if (dyn)
        ask(unit);
    auto hash_of = [&](uint32_t& q0, uint32_t& q1) { // (the lane number through an empty asm: see gn_ibf_count_fast_kernel)
        uint32_t l = (uint32_t)lane;
        asm volatile("" : "+v"(l));
        q0 = l / HF;
        q1 = (l + GN_WAVE) / HF;
    };
    // (wpr and, at the stores, the lane number go through an empty asm: what the compiler makes of them ahead of the persistent loop --
    // the divisor's reciprocal, the lane's address in the match buffer -- would sit in registers for the whole kernel, and this one
    // has none to spare: 96 with nothing in scratch, tests/test_lean_screen_cpu.py reads the figures from the code object)
    auto load_meta = [&](uint64_t u, uint32_t& rd, uint32_t& nn, uint64_t& so) {
        uint32_t w = wpr;
        asm volatile("" : "+s"(w));
        rd = p.read_begin + (uint32_t)(u / w);
        const uint32_t nh = p.n_hashes[rd];
        nn = p.status[rd] == GN_READ_OK ? nh : 0u;
        so = p.slot_off[rd];
    };
    auto load_hashes = [&](uint32_t nn, uint64_t so, uint64_t& h0, uint64_t& h1) {
        h0 = h1 = 0;
        if (nn >= 1 && nn <= NMAX)
        {
            uint32_t q0, q1;
            hash_of(q0, q1);
            if (q0 < nn)
                h0 = p.hashes[so + q0];
            if (q1 < nn)
                h1 = p.hashes[so + q1];
        }
    };
    unsigned long long chunk_base = 0;
    uint32_t           chunk_left = 0, chunk_size = GN_MATCH_CHUNK;
    uint64_t           skipped_bytes = 0;
    uint32_t read, n;
    uint64_t slot, hA, hB;
    load_meta(unit, read, n, slot);
    load_hashes(n, slot, hA, hB);

    for (;;)
    {
    const uint32_t slice = (uint32_t)(unit - (uint64_t)(read - p.read_begin) * wpr);
    uint64_t unit_n = unit + 1;
    if (unit_n >= chunk_end)
    {
        if (dyn)
        {
            const uint32_t lo32 = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)g_next);
            const uint32_t hi32 = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(g_next >> 32));
            unit_n              = dyn_from + (((uint64_t)hi32 << 32) | lo32);
            chunk_end           = unit_n + g_size;
            if (unit_n < n_units)
                ask(unit_n);
        }
        else
        {
            unit_n    = unit + stride;
            chunk_end = unit_n + 1;
        }
    }
    const bool more = unit_n < n_units;
    uint32_t   read_n = 0, n_n = 0;
    uint64_t   slot_n = 0, hA_n = 0, hB_n = 0;

    // which flow: skipped (no minimisers, or more than the byte counters hold), no screen for this n (left to the list), screened
    const bool skip = n > NMAX || n == 0;
    uint32_t   T = 0, ds = 0;
    if (!skip)
    {
        T = (uint32_t)(uint64_t)ceil(__dmul_rn((double)n, p.rel_cutoff)); // GanonClassify.cpp:492-495,720-724
        if (T == 0)
            T = 1;
        if (p.early_exit && T >= 2)
        {
            ds = (p.screen[n >> 2] >> (8u * (n & 3u))) & 0xFFu;
            if (ds > n || ds + T <= n)
                ds = 0;
        }
    }
    if (skip || ds == 0)
    {
        if (lane == 0)
        {
            if (skip)
            {
                if (n > NMAX && slice == 0)
                    p.work_list_out[atomicAdd(p.work_count_out, 1ULL)] = read;
                uint32_t zero = 0; // (made here, not kept in a register pair across the loop)
                asm volatile("" : "+v"(zero));
                p.seg_begin[(size_t)read * wpr + slice] = zero;
                p.seg_count[(size_t)read * wpr + slice] = zero;
            }
            else
                p.unit_list_out[atomicAdd(p.unit_count_out, 1ULL)] = (uint32_t)unit;
        }
        if (!more)
            break;
        load_meta(unit_n, read_n, n_n, slot_n);
        load_hashes(n_n, slot_n, hA_n, hB_n);
        unit = unit_n; read = read_n; n = n_n; slot = slot_n; hA = hA_n; hB = hB_n;
        continue;
    }
    const uint32_t wi      = slice * 64 + (uint32_t)lane;
    const bool     col_act = wi < p.W;

    gn_wave_lds_sync(); // previous unit's row-table reads are done
    {
        uint32_t q0, q1;
        hash_of(q0, q1);
        if ((uint32_t)lane < n * HF)
            rowtab[(uint32_t)lane] = gn_ibf_row(hA, (uint32_t)lane - q0 * HF, p.shift, p.S);
        if ((uint32_t)lane + GN_WAVE < n * HF)
            rowtab[(uint32_t)lane + GN_WAVE] = gn_ibf_row(hB, (uint32_t)lane + GN_WAVE - q1 * HF, p.shift, p.S);
        for (uint32_t idx = (uint32_t)lane + 2 * GN_WAVE; idx < n * HF; idx += GN_WAVE) // reads with more than 32 minimisers
        {
            const uint32_t q = idx / HF, i = idx - q * HF;
            rowtab[idx] = gn_ibf_row(p.hashes[slot + q], i, p.shift, p.S);
        }
    }
    gn_wave_lds_sync();

    uint32_t nib[ND][4];
    uint32_t byt[ND][4][2];
#pragma unroll
    for (int d = 0; d < ND; ++d)
#pragma unroll
        for (int j = 0; j < 4; ++j)
        {
            nib[d][j]    = 0;
            byt[d][j][0] = 0;
            byt[d][j][1] = 0;
        }
    uint32_t acc_n = 0;
    auto spill_nibbles = [&]() {
#pragma unroll
        for (int d = 0; d < ND; ++d)
#pragma unroll
            for (int j = 0; j < 4; ++j)
            {
                byt[d][j][0] += nib[d][j] & 0x0F0F0F0Fu;
                byt[d][j][1] += (nib[d][j] >> 4) & 0x0F0F0F0Fu;
                nib[d][j] = 0;
            }
    };
    // an iteration = the hashes 2 it and 2 it + 1, rows 0 and 1 of each; every lane loads (a lane without a column reads word 0)
    const uint32_t wi_ld = col_act ? wi : 0u;
    auto issue = [&](uint32_t it, GnRowRegs<HF, 1>& R) {
        uint32_t row[HF];
#pragma unroll
        for (int i = 0; i < HF; ++i)
        {
            // (the second hash of an odd screen's last iteration is its first again: the same two lines, masked below)
            const uint32_t qs = 2 * it + (uint32_t)(i >> 1) < ds ? 2 * it + (uint32_t)(i >> 1) : 2 * it;
            row[i]            = rowtab[qs * HF + (uint32_t)(i & 1)];
        }
#pragma unroll
        for (int i = 0; i < HF; ++i)
        {
            const uint2 v = gn_row_load2<GN_ROWS_NT>(p.rows + ((uint64_t)row[i] * p.W + wi_ld));
            R.m[i][0] = v.x;
            R.m[i][1] = v.y;
        }
    };
    auto consume = [&](const GnRowRegs<HF, 1>& R, uint32_t it) {
        const uint32_t on = col_act ? 0xFFFFFFFFu : 0u, on2 = 2 * it + 1 < ds ? on : 0u;
#pragma unroll
        for (int d = 0; d < ND; ++d)
        {
            const uint32_t a = R.m[0][d] & R.m[1][d] & on, b = R.m[2][d] & R.m[3][d] & on2;
            if (2 * it < GN_PROBE_HASHES) // kept for the finish's probe (a hash an odd ds masks off keeps 0)
            {
                uint32_t l = (uint32_t)lane; // (through an empty asm: the lane's address is made here, not kept across the loop)
                asm volatile("" : "+v"(l));
                pmask[((2 * it) * ND + (uint32_t)d) * GN_WAVE + l]     = a;
                pmask[((2 * it + 1) * ND + (uint32_t)d) * GN_WAVE + l] = b;
            }
#pragma unroll
            for (int j = 0; j < 4; ++j)
                nib[d][j] += ((a >> j) & 0x11111111u) + ((b >> j) & 0x11111111u);
        }
        acc_n += 2;
        if (acc_n >= 14) // (two more would pass 15)
        {
            spill_nibbles();
            acc_n = 0;
        }
    };
    GnRowRegs<HF, 1> A, Bq;
    issue(0, A);
    if (more) // the next unit's metadata, under this unit's first rows
        load_meta(unit_n, read_n, n_n, slot_n);
    {
        const uint32_t its = (ds + 1) >> 1;
        uint32_t       it  = 0;
        for (; it + 2 < its; it += 2)
        {
            issue(it + 1, Bq);
            consume(A, it);
            issue(it + 2, A);
            consume(Bq, it + 1);
        }
        const bool two = it + 1 < its;
        if (two)
            issue(it + 1, Bq);
        consume(A, it);
        if (two)
            consume(Bq, it + 1);
    }
    // the one survey: bins with c2 >= T - (n - ds) -> sm[] (bit = bin inside the lane's word), `left` of them
    if (acc_n)
        spill_nibbles();
    uint32_t sm[ND];
    uint32_t left = 0;
    {
        const uint32_t Kt    = (0x80u - (T - (n - ds))) * 0x01010101u;
        uint32_t       any_t = 0;
#pragma unroll
        for (int d = 0; d < ND; ++d)
        {
            uint32_t m = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int pp = 0; pp < 2; ++pp)
                {
                    const uint32_t g = (byt[d][j][pp] + Kt) & 0x80808080u; // byte y <-> bit 8y + 4pp + j of dword d
                    any_t |= g;
                    m |= (g >> 7) << (4 * pp + j);
                }
            sm[d] = m;
        }
        if (__ballot(any_t != 0) != 0)
        {
            uint32_t c = 0;
#pragma unroll
            for (int d = 0; d < ND; ++d)
                c += (uint32_t)__popc(sm[d]);
            for (int off = 32; off > 0; off >>= 1)
                c += __shfl_xor(c, off);
            left = (uint32_t)__builtin_amdgcn_readfirstlane((int)c);
        }
    }
    const uint32_t wcol = slice * 64 < p.W ? (p.W - slice * 64 < 64u ? p.W - slice * 64 : 64u) : 0u; // words of this slice
    if (more) // next unit's hashes: the loads fly under the finish
        load_hashes(n_n, slot_n, hA_n, hB_n);
    if (left > GN_NARROW_MAX)
    {
        // dense rows: the screen did not thin the field.  The unit goes to the list; its screen's rows come on top of what the
        // unscreened flow will request.
        if (lane == 0)
            p.unit_list_out[atomicAdd(p.unit_count_out, 1ULL)] = (uint32_t)unit;
        skipped_bytes -= (uint64_t)(2 * ds) * wcol * 8ull;
        if (!more)
            break;
        unit = unit_n; read = read_n; n = n_n; slot = slot_n; hA = hA_n; hB = hB_n;
        continue;
    }
    // The finish (see gn_ibf_count_fast_kernel): the exact count of each bin of sm[] over all n hashes, word by word.
    uint32_t narrow_loads = 0;
    uint32_t total = 0;            // records so far (wave-uniform)
    uint32_t rec_t = 0, rec_c = 0; // lane k: target and count of record k
    if (left)
    {
        constexpr uint32_t QPC = GN_WAVE / HF; // hashes per pass
        uint64_t           grp = 0;            // bit q*HF for q < QPC
#pragma unroll
        for (uint32_t q = 0; q < QPC; ++q)
            grp |= 1ULL << (q * HF);
        const uint32_t l_q = (uint32_t)lane / HF, l_i = (uint32_t)lane - l_q * HF;
        // (the passes' bounds are set from these copies: n and ds themselves are captured by the lambdas above, and "q_to = n" in one
        // branch, "q_to = ds" in another comes out as one load through a selected address, which keeps both in scratch)
        const uint32_t n_f = n, ds_f = ds;
        gn_wave_lds_sync(); // the screen's hit masks are in LDS
        uint64_t       lm  = __ballot((sm[0] | sm[1]) != 0);
        while (lm)
        {
            const int L = __builtin_ctzll(lm);
            lm &= lm - 1;
#pragma unroll
            for (int d = 0; d < ND; ++d)
            {
                uint32_t mb = (uint32_t)__builtin_amdgcn_readlane((int)sm[d], L);
                while (mb)
                {
                    const uint32_t bit = (uint32_t)__builtin_ctz(mb);
                    mb &= mb - 1;
                    const uint32_t word = slice * 64 + (uint32_t)L;
                    const uint32_t sh   = 32u * d + bit;
                    uint32_t       c2   = 0;
#pragma unroll
                    for (int j = 0; j < 4; ++j)
#pragma unroll
                        for (int pp = 0; pp < 2; ++pp)
                            if ((bit & 3u) == (uint32_t)j && ((bit >> 2) & 1u) == (uint32_t)pp)
                                c2 = byt[d][j][pp];
                    c2 = ((uint32_t)__builtin_amdgcn_readlane((int)c2, L) >> (8u * (bit >> 3))) & 0xFFu;
                    uint32_t add     = 0;
                    uint32_t q_lo    = 0;
                    uint32_t q_known = ds_f;     // hashes below this one are taken to have the bit in rows 0 and 1
                    uint32_t q_to    = n_f;
                    bool     probe   = c2 != ds; // which hashes missed: known for the first Fp, else first the rows 2 and 3 of the screened hashes alone
                    bool     dropped = false;    // the probe's first stage settled it: no pass at all
                    uint32_t e1      = 0;        // what that stage counted
                    if (probe)
                    {
                        // stage 1 (gn_stray_probe.h): rows 2 and 3 of the hashes among the first Fp that hit, a lane a word
                        const uint32_t Fp   = gn_probe_first(p.probe_hashes, ds);
                        bool           hitq = false;
                        if (l_q < Fp)
                            hitq = ((pmask[(l_q * ND + (uint32_t)d) * GN_WAVE + (uint32_t)L] >> bit) & 1u) != 0;
                        const bool ld = hitq && l_i >= 2;
                        uint64_t   w1 = 0;
                        if (ld)
                            w1 = p.rows[(uint64_t)rowtab[l_q * HF + l_i] * p.W + word];
                        const uint64_t hb = __ballot(ld && ((w1 >> sh) & 1ULL));
                        const uint32_t m  = (uint32_t)__popcll(__ballot(hitq && l_i == 2));
                        e1                = (uint32_t)__popcll(hb & (hb >> 1) & (grp << 2));
                        narrow_loads += 2 * m;
                        dropped = gn_probe_drop1(n, T, ds, c2, m, e1);
                        q_lo    = Fp; // stage 2: the other screened hashes
                        q_to    = ds_f;
                    }
                    while (!dropped)
                    {
                        add = 0;
                        for (uint32_t q0 = q_lo; q0 < q_to; q0 += 2 * QPC)
                        {
                            const uint32_t qa = q0 + l_q, qb = qa + QPC;
                            const bool     ina = qa < q_to, inb = qb < q_to;
                            uint64_t       wa = ~0ULL, wb = ~0ULL;
                            if (ina && !(l_i < 2 && qa < q_known))
                                wa = p.rows[(uint64_t)rowtab[qa * HF + l_i] * p.W + word];
                            if (inb && !(l_i < 2 && qb < q_known))
                                wb = p.rows[(uint64_t)rowtab[qb * HF + l_i] * p.W + word];
                            const uint64_t bma = __ballot(ina && ((wa >> sh) & 1ULL)), bmb = __ballot(inb && ((wb >> sh) & 1ULL));
                            uint64_t       alla = bma, allb = bmb;
#pragma unroll
                            for (int i = 1; i < HF; ++i)
                            {
                                alla &= bma >> i;
                                allb &= bmb >> i;
                            }
                            add += (uint32_t)__popcll(alla & grp) + (uint32_t)__popcll(allb & grp);
                        }
                        narrow_loads += (q_to - q_lo) * HF - 2 * (q_known - (probe ? q_lo : 0u));
                        if (!probe)
                            break;
                        probe = false;
                        add += e1;
                        if (gn_probe_drop2(n, T, ds, add)) // below the survey's bound on rows 2 and 3 alone: the bin cannot reach T
                        {
                            add = 0;
                            break;
                        }
                        q_known = 0;
                        q_lo    = 0;
                        q_to    = n_f;
                    }
                    if (add >= T)
                    {
                        if ((uint32_t)lane == total)
                        {
                            rec_t = word * 64u + sh;
                            rec_c = add;
                        }
                        ++total;
                    }
                }
            }
        }
    }
    if (wcol)
        skipped_bytes += (uint64_t)(n * HF - 2 * ds) * wcol * 8ull - (uint64_t)narrow_loads * 128ull;

    unsigned long long base = 0;
    if (total)
    {
        // a wave-private chunk of the match buffer, doubling (see gn_ibf_count_fast_kernel)
        if (total > chunk_left)
        {
            const uint32_t need = total > chunk_size ? total : chunk_size;
            chunk_size = chunk_size * 2u <= GN_MATCH_CHUNK_MAX ? chunk_size * 2u : GN_MATCH_CHUNK_MAX;
            unsigned long long nb = 0;
            if (lane == 0)
                nb = atomicAdd(p.cursor, (unsigned long long)need);
            chunk_base = gn_readlane64(nb, 0);
            chunk_left = need;
        }
        base = chunk_base;
        chunk_base += total;
        chunk_left -= total;
        uint32_t l = (uint32_t)lane;
        asm volatile("" : "+v"(l));
        if (base + total <= p.match_cap && l < total)
        {
            gn_match mt;
            mt.read   = read;
            mt.target = rec_t;
            mt.count  = rec_c;
            p.matches[base + l] = mt;
        }
    }
    if (lane == 0)
    {
        p.seg_begin[(size_t)read * wpr + slice] = base;
        p.seg_count[(size_t)read * wpr + slice] = total;
    }
    if (!more)
        break;
    unit = unit_n; read = read_n; n = n_n; slot = slot_n; hA = hA_n; hB = hB_n;
    } // persistent loop
    if (lane == 0 && skipped_bytes) // wave-uniform amount, one atomic per wave
        atomicAdd(p.skip_ctr, (unsigned long long)skipped_bytes);
