    extern __shared__ __attribute__((aligned(16))) uint32_t gn_lds[];
    constexpr int      ND   = 2 * LW;
    constexpr int      HFP  = HF <= 4 ? 4 : 8;
    // counts live in 8-bit SWAR registers (4-bit first level, spilled every 15 iterations): exact up to 127, which
    // also keeps the byte-wise compare below carry-free.  Reads with more minimisers go to the generic kernel.
    constexpr uint32_t NMAX = 127;
    // with the two-row screen: four hash functions (its register sets are those of four loads an iteration); not the three-wave build of
    // 16-byte lanes, which would pay for it with 48 bytes of scratch a lane where it has 8
    constexpr bool     SCR  = SCRN && EE && HF == 4 && (LW == 1 || WIDE);
    static_assert(SCR == SCRN, "a screening instance: early exit, four hash functions, 8-byte lanes or the wide build");
    // the one instance that also runs over a list of units (p.unit_list: what the screen-only kernel below left to it); the list
    // changes which unit an index means -- in load_meta and where the slice is taken from it -- and nothing else
    constexpr bool     LST  = EE && !SCRN && !WIDE && HF == 4 && LW == 1;

    const int      lane  = threadIdx.x & (GN_WAVE - 1);
    const int      wave  = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)); // wave-uniform: unit, read, n, ... live in SGPRs
    const uint32_t wpr   = p.wpr;
    const uint32_t gpl   = SCR ? GN_FAST_EE_GP_LOG2 : p.gp_log2; // (a compile-time fact in the screening instances: it spares them registers)
    const uint32_t Gp    = 1u << gpl;
    const uint32_t H     = GN_WAVE >> gpl;
    const uint32_t gl    = lane & (Gp - 1);
    const uint32_t hsub  = lane >> gpl;
    uint32_t*      rowtab = gn_lds + (size_t)wave * 128 * HFP;
    uint32_t*      mlist  = gn_lds + (size_t)(blockDim.x >> 6) * 128 * HFP + (size_t)wave * GN_FAST_LIST; // the epilogue's match list (low cutoffs)
    // the screening instances: hit masks of the first GN_PROBE_HASHES screened hashes, dword (q * ND + d) * 64 + lane (behind the lists;
    // in LDS in both: <4,1,true,false,true> has no register for them, and the finish reads the owner lane's by address)
    uint32_t*      pmask  = gn_lds + (size_t)(blockDim.x >> 6) * (128 * HFP + GN_FAST_LIST) + (size_t)wave * (GN_PROBE_HASHES * ND * GN_WAVE);

    // Persistent waves: unit = (read, column slice), handed out in chunks (below).  The metadata of the NEXT unit
    // (status, n, hash slot) is loaded at the top of the current one (the screening instances: under its first rows) and its
    // hashes right after the current main loop, so the chain status -> n -> slot -> hashes -> rows of dependent HBM latencies that a fresh
    // wave would pay before its first row load is hidden behind the previous read's work.
    uint64_t       n_units = (uint64_t)(p.n_reads - p.read_begin) * wpr;
    if constexpr (LST)
        if (p.unit_list)
            n_units = *p.unit_count; // (at most the units of the launch that wrote the list)
    const uint64_t stride  = (uint64_t)gridDim.x * (blockDim.x >> 6);
    uint64_t       unit    = (uint64_t)blockIdx.x * (blockDim.x >> 6) + wave;
    if (unit >= n_units)
        return;
    // Which units a wave takes.  Wave i used to take units i, i + waves, ...: the same count for every wave.  But the waves of a launch do
    // not run at the same pace (the HIBF's packed kernel, which hands out its batches the same way: first wave through after 0.84 of the
    // launch, the XCDs with odd numbers 11 % behind the even ones -- gn_hibf.hip), and the launch ends with its slowest wave.  With 64 or
    // more units a wave, a wave starts with 16 units of its own and takes every later chunk from a cursor -- asked for one chunk ahead,
    // so that the answer is there when it is needed; 16 units a chunk, 8 in the last quarter of the launch, 4 in its last sixteenth
    // (a counter address takes ~90 atomics a microsecond).
    const bool     dyn      = p.grab != nullptr && n_units >= 64u * stride;
    const uint64_t dyn_from = stride * 16u; // the cursor counts from here
    uint64_t       chunk_end = unit + 1;
    if (dyn)
    {
        unit *= 16u;
        chunk_end = unit + 16u;
    }
    unsigned long long g_next = 0; // (lane 0: what the cursor answered)
    uint32_t           g_size = 16u;
    auto               ask    = [&](uint64_t from) {
        g_size = from < n_units - n_units / 4u ? 16u : (from < n_units - n_units / 16u ? 8u : 4u);
        if (lane == 0)
            g_next = atomicAdd(p.grab, (unsigned long long)g_size);
    };
    if (dyn)
        ask(unit);
    // hash q of a unit feeds row-table entries idx = lane and lane + 64 (idx = q*HF + i).  In the screening instances the lane number
    // goes through an empty asm where q is needed: hoisted out of the persistent loop, q0, q1 and the two hash addresses made of
    // them hold six registers for the whole unit, which those instances do not have to spare (<4,1,true,false,true> sits at
    // exactly 128 with nothing in scratch; tests/test_screen_table_cpu.py reads the figures from the code object, so a compiler
    // that sees through this shows up there and not as a slower kernel)
    // (the other instances keep the two as values of the whole kernel, as before the screen: written any other way the compiler's
    // register allocation of <4,1,true> and <4,2,true> comes out one and two spilled registers worse)
    const uint32_t q0_c = (uint32_t)lane / HF, q1_c = ((uint32_t)lane + GN_WAVE) / HF;
    auto hash_of = [&](uint32_t& q0, uint32_t& q1) {
        if constexpr (!SCR)
        {
            q0 = q0_c;
            q1 = q1_c;
            return;
        }
        uint32_t l = (uint32_t)lane;
        if constexpr (SCR)
            asm volatile("" : "+v"(l));
        q0 = l / HF;
        q1 = (l + GN_WAVE) / HF;
    };
    auto load_meta = [&](uint64_t u, uint32_t& rd, uint32_t& nn, uint64_t& so) {
        if constexpr (LST)
            if (p.unit_list)
                u = p.unit_list[u];
        rd = p.read_begin + (uint32_t)(u / wpr);
        const uint32_t nh = p.n_hashes[rd]; // (asked for beside the status, not after it: one round trip, not two)
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
    unsigned long long chunk_base = 0; // wave-private slice of the match buffer
    uint32_t           chunk_left = 0, chunk_size = GN_MATCH_CHUNK;
    uint64_t           skipped_bytes = 0; // row bytes this lane's column group did not fetch thanks to early exits
    uint32_t           n_pre = 0;         // matches of this lane left unwritten for the filter_matches pre-pass (pre_mode)
    uint32_t read, n;
    uint64_t slot, hA, hB;
    load_meta(unit, read, n, slot);
    load_hashes(n, slot, hA, hB);

    for (;;)
    {
    // (over a list the unit's number is read again here rather than carried beside `read` from load_meta: a scalar load that hits the
    // L2, paid by the few units on the list, against a register of every unit of every launch of this instance)
    uint64_t unit_id = unit;
    if constexpr (LST)
        if (p.unit_list)
            unit_id = p.unit_list[unit];
    const uint32_t slice = (uint32_t)(unit_id - (uint64_t)(read - p.read_begin) * wpr);
    // which unit is next; its metadata is asked for here, or under this unit's first rows (META_LATE below), and consumed after the main loop
    uint64_t unit_n = unit + 1;
    if (unit_n >= chunk_end)
    {
        if (dyn)
        {
            const uint32_t lo32 = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)g_next);
            const uint32_t hi32 = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(g_next >> 32));
            unit_n              = dyn_from + (((uint64_t)hi32 << 32) | lo32); // (asked for a chunk ago)
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
    uint32_t       read_n = 0, n_n = 0;
    uint64_t       slot_n = 0, hA_n = 0, hB_n = 0;
    // The metadata loads are scalar loads, and scalar loads come back in any order: whatever waits for the row table in LDS
    // waits for all of them too.  Asked for here, the wave stood waiting for them at the row table's barrier with nothing of its
    // own in flight (measured: 10.7 % of the wave time between the last store of a unit and its row table).  The screening
    // instances ask for them once the unit's first rows are in flight, so that wait is paid under those rows.  The other instances
    // keep the old place: the three-wave build of 16-byte lanes pays for the new one with 24 bytes of scratch a lane where it has 8.
    constexpr bool META_LATE = SCR;
    if (!META_LATE && more)
        load_meta(unit_n, read_n, n_n, slot_n);

    if (n > NMAX || n == 0)
    {
        if (lane == 0)
        {
            if (n > NMAX && slice == 0)
                p.work_list_out[atomicAdd(p.work_count_out, 1ULL)] = read;
            p.seg_begin[(size_t)read * wpr + slice] = 0;
            p.seg_count[(size_t)read * wpr + slice] = 0;
        }
        if (!more)
            break;
        if (META_LATE)
            load_meta(unit_n, read_n, n_n, slot_n);
        load_hashes(n_n, slot_n, hA_n, hB_n);
        unit = unit_n; read = read_n; n = n_n; slot = slot_n; hA = hA_n; hB = hB_n;
        continue;
    }
    const uint32_t  wi      = slice * 64 * LW + gl * LW;
    const bool      col_act = wi < p.W;

    gn_wave_lds_sync(); // previous unit's row-table reads are done
    uint32_t q0, q1;
    hash_of(q0, q1);
    if ((uint32_t)lane < n * HF)
        rowtab[q0 * HFP + ((uint32_t)lane - q0 * HF)] = gn_ibf_row(hA, (uint32_t)lane - q0 * HF, p.shift, p.S);
    if ((uint32_t)lane + GN_WAVE < n * HF)
        rowtab[q1 * HFP + ((uint32_t)lane + GN_WAVE - q1 * HF)] = gn_ibf_row(hB, (uint32_t)lane + GN_WAVE - q1 * HF, p.shift, p.S);
    for (uint32_t idx = (uint32_t)lane + 2 * GN_WAVE; idx < n * HF; idx += GN_WAVE) // reads with more than 128/HF minimisers
    {
        const uint32_t q = idx / HF, i = idx - q * HF;
        rowtab[q * HFP + i] = gn_ibf_row(p.hashes[slot + q], i, p.shift, p.S);
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
    uint32_t acc_n = 0; // iterations since the nibbles were last spilled into the byte counters (wave-uniform)
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

    const uint32_t iters = (n + H - 1) / H;
    uint32_t T = (uint32_t)(uint64_t)ceil(__dmul_rn((double)n, p.rel_cutoff)); // GanonClassify.cpp:492-495,720-724
    if (T == 0)
        T = 1;
    // Early exit (exact): after `done` iterations the hashes [0, done*H) are counted; a bin gains at most one per
    // remaining hash, so when no bin has reached T - (n - done*H) the read cannot match in this column slice and its
    // remaining rows need not be fetched.  First check where that bound exceeds half of the hashes seen so far
    // (random hits stay far below it, true matches far above), then every second iteration; the iteration already
    // in flight at a check is wasted, so checks that could not save a later one are not made.
    uint32_t chk1 = 0xFFFFFFFFu, chk2 = 0xFFFFFFFFu;
    if (EE && p.early_exit && T >= 2)
    {
        uint32_t c = (2 * (n - T + 1) + H - 1) / H;
        if (c < 1)
            c = 1;
        if (c + 2 <= iters)
        {
            chk1 = p.early_exit == 3 ? c : (c > 1 ? c - 1 : c); // first check (one hash before the half-way bound) ...
            chk2 = p.early_exit >= 2 && p.early_exit != 3 ? iters - 2 : c + 2; // ... then every iteration up to chk2
        }
    }
    // Two-row screen (SCR instances; see the screened flow below): the launch's table says on how many hashes a read of n
    // minimisers is screened, 0 = not at all.  The table only decides speed: whatever it holds, a screen runs only with
    // ds <= n and a bound T - (n - ds) of at least 1.
    uint32_t ds = 0;
    if constexpr (SCR)
    {
        if (p.early_exit && T >= 2)
        {
            ds = (p.screen[n >> 2] >> (8u * (n & 3u))) & 0xFFu;
            if (ds > n || ds + T <= n)
                ds = 0;
        }
    }
    // Row loads are issued by every lane, unconditionally (lanes without a column or past the last hash read a valid
    // word and are masked when the rows are consumed): with the loads inside an exec-masked region the compiler
    // cannot know how many are outstanding behind the set it waits for and falls back to s_waitcnt vmcnt(0) -- which
    // turned the double buffer into "issue two iterations, wait for both, consume both".
    const uint32_t wi_ld = col_act ? wi : 0u; // a word that exists in every row
    auto load_row = [&](uint32_t row, auto& R, int i) {
        const uint64_t* ptr = p.rows + ((uint64_t)row * p.W + wi_ld);
        if constexpr (LW == 2)
        {
            const gn_u32x4  v  = gn_row_load4<GN_ROWS_NT>(ptr);
            R.m[i][0] = v.x;
            R.m[i][1] = v.y;
            R.m[i][2] = v.z;
            R.m[i][3] = v.w;
        }
        else
        {
            const uint2 v = gn_row_load2<GN_ROWS_NT>(ptr);
            R.m[i][0] = v.x;
            R.m[i][1] = v.y;
        }
    };
    // scr (wave-uniform; SCR instances, where a wave is one hash group): the two-row screen is running and an iteration means
    // the hashes 2 it and 2 it + 1, rows 0 and 1 of each -- the same four loads into the same set, the same wait counts
    bool scr = SCR && ds != 0;
    auto issue = [&](uint32_t it, GnRowRegs<HF, LW>& R) {
        uint32_t q = it * H + hsub;
        q          = q < n ? q : n - 1;
        uint32_t row[HF];
#pragma unroll
        for (int i = 0; i < HF; ++i)
        {
            uint32_t idx = q * HFP + (uint32_t)i;
            if constexpr (SCR)
            {
                // (the second hash of an odd screen's last iteration is its first again: the same two lines, masked below)
                const uint32_t qs = 2 * it + (uint32_t)(i >> 1) < ds ? 2 * it + (uint32_t)(i >> 1) : 2 * it;
                idx               = scr ? qs * HFP + (uint32_t)(i & 1) : idx;
            }
            row[i] = rowtab[idx];
        }
#pragma unroll
        for (int i = 0; i < HF; ++i)
            load_row(row[i], R, i);
    };
    auto consume = [&](const GnRowRegs<HF, LW>& R, uint32_t it) {
        if (SCR && scr)
        {
            const uint32_t on = col_act ? 0xFFFFFFFFu : 0u, on2 = 2 * it + 1 < ds ? on : 0u;
#pragma unroll
            for (int d = 0; d < ND; ++d)
            {
                const uint32_t a = R.m[0][d] & R.m[1][d] & on, b = R.m[2 % HF][d] & R.m[3 % HF][d] & on2;
                if (2 * it < GN_PROBE_HASHES) // kept for the finish's probe (a hash an odd ds masks off keeps 0)
                {
                    pmask[((2 * it) * ND + (uint32_t)d) * GN_WAVE + (uint32_t)lane]     = a;
                    pmask[((2 * it + 1) * ND + (uint32_t)d) * GN_WAVE + (uint32_t)lane] = b;
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
            return;
        }
        const uint32_t on = (col_act && it * H + hsub < n) ? 0xFFFFFFFFu : 0u;
#pragma unroll
        for (int d = 0; d < ND; ++d)
        {
            uint32_t a = R.m[0][d] & on;
#pragma unroll
            for (int i = 1; i < HF; ++i)
                a &= R.m[i][d];
#pragma unroll
            for (int j = 0; j < 4; ++j)
                nib[d][j] += (a >> j) & 0x11111111u;
        }
        if (++acc_n == 15)
        {
            spill_nibbles();
            acc_n = 0;
        }
    };
    // Survey at a check point (EE instances run with one hash group per wave, so `done` iterations = `done` hashes):
    // which bins of this slice can still reach T?  A bin gains at most one per remaining hash, so only bins with
    // count >= t = T - (n - done) are left in the race; their bits go to sm[] (bit = bin inside the lane's words)
    // and their number is returned.  Same SWAR compare as the epilogue; spills the nibbles first.
    uint32_t sm[ND];
#pragma unroll
    for (int d = 0; d < ND; ++d)
        sm[d] = 0;
    // bins with count >= tval (1 <= tval <= 127; the byte counters must be complete) -> sm[], their number is returned
    auto survivors = [&](uint32_t tval) -> uint32_t {
        const uint32_t Kt = (0x80u - tval) * 0x01010101u;
        uint32_t any_t = 0;
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
        if (__ballot(any_t != 0) == 0)
            return 0u;
        uint32_t c = 0;
#pragma unroll
        for (int d = 0; d < ND; ++d)
            c += (uint32_t)__popc(sm[d]);
        for (int off = 32; off > 0; off >>= 1)
            c += __shfl_xor(c, off);
        return c;
    };
    auto survey = [&](uint32_t done) -> uint32_t {
        if (acc_n)
        {
            spill_nibbles();
            acc_n = 0;
        }
        return survivors(T - (n - done)); // >= 1 at every check point
    };
    bool     dead    = false; // no bin can reach T any more: nothing to report
    bool     narrow  = false; // a handful of bins can: the remaining hashes only look at those (below)
    uint32_t fetched = iters; // iterations whose full rows were requested
    // Screened flow (exact; reads the table gives a screen length ds).  The first ds hashes fetch rows 0 and 1 only -- the loop
    // below with two hashes an iteration (issue, consume) -- and count c2 = hashes whose rows 0 and 1 both have the bin's bit.
    // Nothing is checked on the way and no hash beyond ds is touched.
    // One survey at ds with the bound of the exit, T - (n - ds):
    //   no bin left        the read is dead after 2 ds row fetches;
    //   1 .. GN_NARROW_MAX the finish below fetches, word by word, the exact count of each over all n hashes;
    //   more               (dense rows: the screen did not thin the field) the counters are zeroed and the read runs the
    //                      unscreened flow from hash 0, its own exit and narrow mode included -- at most once a read.
    // Why the result is what every row would give:
    //   (a) c2 >= c4 (the count over all h rows) bin by bin, so a bin that can still reach T by c4 passes the survey;
    //   (b) a bin that did not pass keeps its c2 < T - (n - ds) <= T, which the epilogue's compare never reports;
    //   (c) a bin that passed gets c4 in place of c2 before the epilogue: c2 >= T > c4 vanishes, c4 >= T reports c4;
    //   (d) c2 <= ds <= n and c4 <= n <= 127: the byte counters and the carry-free compare hold in either flow.
    bool     finish   = false; // the bins in sm[] get their exact counts (below)
    bool     aborted  = false;
    uint32_t scr_rows = 0;     // rows a screen requested
    // Two row-register sets (A, Bq).  A pass of the loop below starts with iteration 0 in flight in A: issued here, and again
    // at the end of an aborted screen.  With these rows in flight the screening instances ask for the next unit's metadata.
    GnRowRegs<HF, LW> A, Bq;
    issue(0, A);
    if (META_LATE && more)
        load_meta(unit_n, read_n, n_n, slot_n);
    for (;;) // (a second pass only after an aborted screen)
    {
        // Two iterations per trip, straight-line: while set X is consumed the other
        // set's four loads stay in flight (s_waitcnt vmcnt(HF)).  Invariant at the top of a trip and after the loop:
        // A holds iteration `it`, in flight.  The survey sits after the second half (check points are even when a
        // wave is one hash group, and only those instances check).
        const uint32_t    its     = SCR && scr ? (ds + 1) >> 1 : iters;        // a screen: ds hashes, two an iteration, ...
        const uint32_t    c1      = SCR && scr ? 0xFFFFFFFFu : chk1, c2 = chk2; // ... no check on the way
        uint32_t          it      = 0;
        bool              drained = false; // a check on an odd iteration consumed everything that was in flight
        for (; it + 2 < its; it += 2)
        {
            if (EE && narrow)
                break;
            issue(it + 1, Bq);
            consume(A, it);
            if constexpr (EE)
            {
                const uint32_t done = it + 1; // odd check points: Bq (iteration `done`) is in flight
                if (done >= c1 && done <= c2)
                {
                    const uint32_t left = survey(done);
                    if (left == 0)
                    {
                        dead    = true;
                        fetched = done + 1;
                        break;
                    }
                    // At the very first check a stray bin that happens to be ahead is cheaper to wait out for one
                    // more iteration than to follow for the rest of the read: narrow there only when every survivor
                    // has been hit by (nearly) every hash so far, as a true match has.
                    if (left <= GN_NARROW_MAX && (done > c1 || (done > 2 && survivors(done - 1) == left)))
                    {
                        consume(Bq, it + 1);
                        narrow  = true;
                        fetched = it + 2;
                        drained = true;
                        break;
                    }
                }
            }
            issue(it + 2, A);
            consume(Bq, it + 1);
            if constexpr (EE)
            {
                const uint32_t done = it + 2;
                if (done >= c1 && done <= c2)
                {
                    const uint32_t left = survey(done);
                    if (left == 0)
                    {
                        dead    = true;
                        fetched = done + 1; // the iteration in flight
                        break;
                    }
                    if (left <= GN_NARROW_MAX)
                        narrow = true; // A (iteration `done`) is consumed below, then the narrow pass takes over
                }
            }
        }
        if (!dead && !drained)
        {
            const bool two = !(EE && narrow) && it + 1 < its; // the last one or two iterations
            if (two)
                issue(it + 1, Bq);
            consume(A, it);
            if (two)
                consume(Bq, it + 1);
            if (EE && narrow)
                fetched = it + 1;
        }
        if (!(SCR && scr))
            break;
        // the screen's one survey, with the bound of the exit
        scr                 = false;
        scr_rows            = 2 * ds;
        const uint32_t left = survey(ds);
        if (left == 0)
            dead = true;
        else if (left <= GN_NARROW_MAX)
            finish = true;
        if (dead || finish)
            break;
        aborted = true;
#pragma unroll
        for (int d = 0; d < ND; ++d)
#pragma unroll
            for (int j = 0; j < 4; ++j)
            {
                byt[d][j][0] = 0;
                byt[d][j][1] = 0;
            }
        issue(0, A); // (scr is off: iteration 0 of the unscreened flow)
    }
    // Narrow mode (exact): the bins that lost the race keep their stale counts (< t <= T, never reported); for each
    // of the few that are left, the remaining hashes fetch only the 8-byte word that holds the bin -- lane l looks at
    // (hash l / HF, row l % HF) and at the hash 64 / HF further on, one ballot each collects the bits, the HF rows of a hash are
    // AND-ed with shifts of the ballot -- and the hits are added to the owner lane's byte counter before the normal epilogue runs.
    // The screened flow's finish is the same pass from hash 0: the exact count replaces the bin's byte (it held c2).  A bin that
    // every screened hash hit (c2 = ds, an error-free read of its genome) needs no second look at rows 0 and 1 of those hashes.
    // Any other bin is first probed on the rows 2 .. of the screened hashes alone: a stray bin, ahead on rows 0 and 1 by chance,
    // falls below the bound there and gets 0; what is left is read in full.  The probe is staged (gn_stray_probe.h): first the
    // hashes among the first GN_PROBE_HASHES that are known to have hit (2 m words; the screen kept their hit masks in LDS), which
    // settles nearly every stray, then the other screened hashes (2 (ds - F') words).  Switch stray_masks: one stage of 2 ds words.
    uint32_t narrow_loads = 0;
    if (EE && (narrow || (SCR && finish)))
    {
        constexpr uint32_t QPC = GN_WAVE / HF; // hashes per pass
        uint64_t           grp = 0;            // bit q*HF for q < QPC
#pragma unroll
        for (uint32_t q = 0; q < QPC; ++q)
            grp |= 1ULL << (q * HF);
        const uint32_t l_q = (uint32_t)lane / HF, l_i = (uint32_t)lane - l_q * HF;
        const uint32_t q_from = SCR && finish ? 0u : fetched;
        uint32_t       any_sm = 0;
#pragma unroll
        for (int d = 0; d < ND; ++d)
            any_sm |= sm[d];
        if constexpr (SCR)
            gn_wave_lds_sync(); // the screen's hit masks are in LDS
        uint64_t lm = __ballot(any_sm != 0);
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
                    const uint32_t tp   = 32u * d + bit;
                    const uint32_t word = slice * 64 * LW + (uint32_t)L * LW + (tp >> 6);
                    const uint32_t sh   = tp & 63u;
                    uint32_t       add  = 0;
                    uint32_t       q_lo    = q_from;
                    uint32_t       q_known = 0;     // hashes below this one are taken to have the bit in rows 0 and 1
                    uint32_t       q_to    = n;
                    bool           probe   = false; // a first pass over the other rows of the screened hashes only
                    bool           dropped = false; // the probe's first stage settled it: no pass at all
                    uint32_t       e1      = 0;     // what that stage counted
                    if constexpr (SCR)
                        if (finish)
                        {
                            uint32_t c2 = 0;
#pragma unroll
                            for (int j = 0; j < 4; ++j)
#pragma unroll
                                for (int pp = 0; pp < 2; ++pp)
                                    if ((bit & 3u) == (uint32_t)j && ((bit >> 2) & 1u) == (uint32_t)pp)
                                        c2 = byt[d][j][pp];
                            c2      = ((uint32_t)__builtin_amdgcn_readlane((int)c2, L) >> (8u * (bit >> 3))) & 0xFFu;
                            q_known = ds;
                            if (c2 != ds)
                            {
                                // which hashes missed is known for the first Fp (gn_stray_probe.h).  Stage 1: rows 2 and 3 of those that hit, a
                                // lane a word; a stray bin, ahead on rows 0 and 1 by chance, nearly always falls below the bound here
                                const uint32_t Fp   = gn_probe_first(p.probe_hashes, ds);
                                bool           hitq = false;
                                if (l_q < Fp)
                                    hitq = ((pmask[(l_q * ND + (uint32_t)d) * GN_WAVE + (uint32_t)L] >> bit) & 1u) != 0;
                                const bool ld = hitq && l_i >= 2;
                                uint64_t   w1 = 0;
                                if (ld)
                                    w1 = p.rows[(uint64_t)rowtab[l_q * HFP + l_i] * p.W + word];
                                const uint64_t hb = __ballot(ld && ((w1 >> sh) & 1ULL));
                                const uint32_t m  = (uint32_t)__popcll(__ballot(hitq && l_i == 2));
                                e1                = (uint32_t)__popcll(hb & (hb >> 1) & (grp << 2));
                                narrow_loads += 2 * m;
                                dropped = gn_probe_drop1(n, T, ds, c2, m, e1);
                                // stage 2: the rows 2 .. of the other screened hashes say whether the bin is worth it
                                probe = true;
                                q_lo  = Fp;
                                q_to  = ds;
                            }
                        }
                    while (!dropped)
                    {
                        add = 0;
                        for (uint32_t q0 = q_lo; q0 < q_to; q0 += 2 * QPC)
                        {
                            // a lane takes two hash slots, l_q and l_q + QPC, and both of its word loads are requested before either
                            // ballot waits for one: a pass covers 2 QPC hashes in one round trip (every 150 bp read in one)
                            const uint32_t qa = q0 + l_q, qb = qa + QPC;
                            const bool     ina = l_q < QPC && qa < q_to, inb = l_q < QPC && qb < q_to;
                            uint64_t       wa = ~0ULL, wb = ~0ULL; // (rows 0 and 1 of a hash below q_known: taken to have the bit)
                            if (ina && !(SCR && l_i < 2 && qa < q_known))
                                wa = p.rows[(uint64_t)rowtab[qa * HFP + l_i] * p.W + word];
                            if (inb && !(SCR && l_i < 2 && qb < q_known))
                                wb = p.rows[(uint64_t)rowtab[qb * HFP + l_i] * p.W + word];
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
                        narrow_loads += (q_to - q_lo) * HF - 2 * (q_known - (SCR && probe ? q_lo : 0u));
                        if (!(SCR && probe))
                            break;
                        // add = screened hashes with the bit in rows 2 .. >= the bin's count over them: below the survey's bound the bin
                        // cannot reach T, whatever rows 0 and 1 say hash by hash, and vanishes; else every word of every hash is read
                        probe = false;
                        add += e1;
                        if (gn_probe_drop2(n, T, ds, add))
                        {
                            add = 0;
                            break;
                        }
                        q_known = 0;
                        q_lo    = 0;
                        q_to    = n;
                    }
                    // into byte (bit >> 3) of byt[d][bit & 3][(bit >> 2) & 1] of lane L
                    const uint32_t inc  = add << (8u * (bit >> 3));
                    const uint32_t keep = SCR && finish ? ~(0xFFu << (8u * (bit >> 3))) : 0xFFFFFFFFu;
#pragma unroll
                    for (int j = 0; j < 4; ++j)
#pragma unroll
                        for (int pp = 0; pp < 2; ++pp)
                            if ((bit & 3u) == (uint32_t)j && ((bit >> 2) & 1u) == (uint32_t)pp && lane == L)
                                byt[d][j][pp] = (byt[d][j][pp] & keep) + inc;
                }
            }
        }
    }
    // bytes this unit did not request: its algorithmic rows less the rows and the words it asked for.  A unit may have asked for
    // more than its algorithmic bytes -- a screen that was aborted (its rows come on top), a finish or a narrow pass over a slice
    // of few words (128 bytes a word load against 8 * wcol a row) -- so every term is added modulo 2^64, as the wave's atomic
    // and the host's difference are: the launch's sum is exact as long as the launch as a whole requested no more than its
    // algorithmic bytes.
    if (slice * 64 * LW < p.W)
    {
        const uint32_t wcol = p.W - slice * 64 * LW < 64u * LW ? p.W - slice * 64 * LW : 64u * LW; // words of this slice
        if constexpr (!SCR)
        {
            // the instances without the screen: the same sum in the shape it had before the screen (which keeps their register
            // allocation what it was), wrapping like the other
            if (dead || narrow)
            {
                const uint32_t got  = fetched < n ? fetched : n;
                const uint64_t full = (uint64_t)(n - got) * HF * wcol * 8ull;
                const uint64_t part = (uint64_t)narrow_loads * 128ull; // a narrow load fills a 128-byte L2 line (FETCH_SIZE agrees)
                skipped_bytes += full - part;
            }
        }
        else if (dead || narrow || finish)
        {
            const uint32_t got  = fetched < n ? fetched : n;
            const uint32_t rows = SCR && scr_rows && !aborted ? scr_rows : got * HF;
            const uint64_t full = (uint64_t)(n * HF - rows) * wcol * 8ull;
            const uint64_t part = (uint64_t)narrow_loads * 128ull; // a narrow load fills a 128-byte L2 line (FETCH_SIZE agrees)
            skipped_bytes += full - part;
        }
        if (SCR && aborted)
            skipped_bytes -= (uint64_t)scr_rows * wcol * 8ull;
    }

    if (more) // next unit's hashes: the loads fly while this unit's epilogue runs
        load_hashes(n_n, slot_n, hA_n, hB_n);

    // ---- epilogue: bytes, cross-group sum, SWAR threshold ----
    uint32_t Kc  = (0x80u - T) * 0x01010101u; // 1 <= T <= n <= 127 and counts <= 127: no carry between bytes
    uint32_t any = 0;
    if (!dead)
    {
        if (acc_n)
            spill_nibbles();
#pragma unroll
        for (int d = 0; d < ND; ++d)
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int pp = 0; pp < 2; ++pp)
                {
                    uint32_t x = byt[d][j][pp];
                    for (uint32_t off = Gp; off < GN_WAVE; off <<= 1) // partial counts of the H hash groups
                        x += __shfl_xor(x, (int)off);
                    byt[d][j][pp] = x;
                    any |= (x + Kc) & 0x80808080u;
                }
    }
    const bool owner = hsub == 0 && col_act; // one lane per column chunk reports
    uint64_t   hm    = dead ? 0ull : __ballot(owner && any != 0);
    if (p.pre_mode && __popcll(hm) > 6)
    {
        // A filter_matches pre-pass follows (gn_postfilter.hip) and many bins passed the cutoff (chance matches at a low
        // --rel-cutoff): with the largest count of THIS unit and a lower bound of the read's minimum, the --rel-filter threshold
        // of the read can only be higher than t2 below (gn_pf_threshold is non-decreasing in both), so bins under t2 are not
        // written at all.  What the pre-pass still needs of them is their number and their smallest count (the read's minimum
        // is taken over ALL bins that passed the cutoff).  Largest / smallest count by binary search with SWAR compares.
        auto any_ge = [&](uint32_t v) -> bool { // a bin with count >= v  (1 <= v <= 127)
            const uint32_t K = (0x80u - v) * 0x01010101u;
            uint32_t       a = 0;
#pragma unroll
            for (int d = 0; d < ND; ++d)
#pragma unroll
                for (int j = 0; j < 4; ++j)
#pragma unroll
                    for (int pp = 0; pp < 2; ++pp)
                        a |= byt[d][j][pp] + K;
            return __ballot(owner && (a & 0x80808080u) != 0) != 0;
        };
        uint32_t lo = T, hi = n;
        while (lo < hi)
        {
            const uint32_t mid = (lo + hi + 1) >> 1;
            if (any_ge(mid))
                lo = mid;
            else
                hi = mid - 1;
        }
        const uint32_t t2 = gn_pf_threshold(lo, p.pre_mode == 1 ? T : 0u, p.pre_rel);
        if (t2 > T && t2 <= lo)
        {
            const uint32_t K2 = (0x80u - t2) * 0x01010101u;
            auto in_range = [&](uint32_t v, bool count) -> uint32_t { // bins with T <= count <= v  (v < t2): any / how many (this lane)
                const uint32_t K1 = (0x80u - (v + 1u)) * 0x01010101u;
                uint32_t       a = 0;
#pragma unroll
                for (int d = 0; d < ND; ++d)
#pragma unroll
                    for (int j = 0; j < 4; ++j)
#pragma unroll
                        for (int pp = 0; pp < 2; ++pp)
                        {
                            const uint32_t e = ((byt[d][j][pp] + Kc) & ~(byt[d][j][pp] + K1)) & 0x80808080u;
                            a = count ? a + (uint32_t)__popc(e) : (a | e);
                        }
                return a;
            };
            const uint32_t below = owner ? in_range(t2 - 1u, true) : 0u;
            if (__ballot(below != 0))
            {
                uint32_t a = T, b = t2 - 1u; // the smallest count among them
                while (a < b)
                {
                    const uint32_t mid = (a + b) >> 1;
                    if (__ballot(owner && in_range(mid, false) != 0))
                        b = mid;
                    else
                        a = mid + 1u;
                }
                if (lane == 0)
                    p.seg_min[(size_t)read * wpr + slice] = a;
                n_pre += below;
                Kc  = K2;
                any = 0;
#pragma unroll
                for (int d = 0; d < ND; ++d)
#pragma unroll
                    for (int j = 0; j < 4; ++j)
#pragma unroll
                        for (int pp = 0; pp < 2; ++pp)
                            any |= (byt[d][j][pp] + Kc) & 0x80808080u;
                hm = __ballot(owner && any != 0);
            }
        }
    }
    uint32_t       total = 0;
    unsigned long long base = 0;
    if (hm)
    {
        // matches of this lane (counts are capped at n by construction: a bin is hit at most once per hash) as one bit
        // per bin: byte y of byt[d][j][pp] is bin 8y + 4pp + j of dword d, so its flag bits 7/15/23/31 shift into place
        uint32_t hit[ND];
        uint32_t mine = 0;
#pragma unroll
        for (int d = 0; d < ND; ++d)
        {
            hit[d] = 0;
            if (owner && any)
            {
#pragma unroll
                for (int j = 0; j < 4; ++j)
#pragma unroll
                    for (int pp = 0; pp < 2; ++pp)
                        hit[d] |= ((((byt[d][j][pp] + Kc) & 0x80808080u) >> 7) << (4 * pp + j));
            }
            mine += __popc(hit[d]);
        }
        // exclusive prefix over the lanes that have matches: a scalar loop over the ballot while they are few (high
        // cutoffs: one or two lanes), a shuffle scan otherwise (low cutoffs: chance matches in most lanes)
        uint32_t my_off = 0;
        if (__popcll(hm) <= 6)
        {
            uint64_t rem = hm;
            while (rem)
            {
                const uint32_t L = (uint32_t)__builtin_ctzll(rem);
                rem &= rem - 1;
                const uint32_t c = (uint32_t)__builtin_amdgcn_readlane((int)mine, (int)L);
                if ((uint32_t)lane == L)
                    my_off = total;
                total += c;
            }
        }
        else
        {
            uint32_t x = mine;
#pragma unroll
            for (int off = 1; off < GN_WAVE; off <<= 1)
            {
                const uint32_t y = (uint32_t)__shfl_up((int)x, off);
                if (lane >= off)
                    x += y;
            }
            my_off = x - mine;
            total  = (uint32_t)__builtin_amdgcn_readlane((int)x, GN_WAVE - 1);
        }
        // padding bins (>= B) of the last word never count: real filters keep them zero; be exact anyway
        // Output space comes from a wave-private chunk: one returning atomic on the global cursor per chunk instead of
        // one per read (a single address sustains only ~90 atomics/us, which would cap the kernel at a few M reads/ms).
        // A wave's chunks double from GN_MATCH_CHUNK to GN_MATCH_CHUNK_MAX: at low cutoffs (~100 chance matches per
        // read) fixed 256-match chunks meant 4 M atomics per 10 M reads -- 20 ms of the kernel.  Unused chunk tails are
        // holes; the gather pass compacts.
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
        const bool fits = base + total <= p.match_cap;
        if (__popcll(hm) > 6)
        {
            // Many lanes report (low cutoffs: ~100 chance matches a read at --rel-cutoff 0.2 on 4096 bins).  Up to round 5 every lane
            // stored its own matches straight to the segment: a store instruction then carried 64 twelve-byte records at 64 unrelated
            // offsets, and the address unit of the CU -- which the row loads of the other waves share -- took them one line at a time
            // (78.7 M such instructions per 10 M reads: the kernel ran 11 ms over its every-row time, profiles/r06_cutoff_counters).
            // Now the lanes put their matches, in segment order, into a list in LDS (bin in the unit << 8 | count; the lane's count bytes
            // go through the wave's row table, idle during the epilogue, 32 bins at a time as before) and the wave writes the list out
            // with lane i holding record i: whole lines per store.  Lists longer than GN_FAST_LIST (an eighth of the bins and more:
            // cutoffs near zero) keep the direct stores.
            const uint8_t* tabb   = reinterpret_cast<const uint8_t*>(rowtab);
            const bool     listed = total <= GN_FAST_LIST;
            if (p.emit_probe & 128u) // (emit_probe: what the epilogue costs without listing or storing anything)
                goto emitted;
            gn_match*      out    = p.matches + base + my_off;
            uint32_t       k      = 0;
#pragma unroll
            for (int d = 0; d < ND; ++d)
            {
                gn_wave_lds_sync();
                if (owner && any)
                {
#pragma unroll
                    for (int j = 0; j < 4; ++j)
#pragma unroll
                        for (int pp = 0; pp < 2; ++pp)
                            rowtab[(uint32_t)lane * 8u + (uint32_t)(j * 2 + pp)] = byt[d][j][pp];
                }
                gn_wave_lds_sync();
                uint32_t mbits = (fits && owner && any) ? hit[d] : 0u;
                while (mbits)
                {
                    const uint32_t b = (uint32_t)__builtin_ctz(mbits);
                    mbits &= mbits - 1;
                    // bit b = 8y + 4pp + j of dword d is byte y of byt[d][j][pp]
                    const uint32_t cnt = tabb[(uint32_t)lane * 32u + (((b & 3u) << 1) + ((b >> 2) & 1u)) * 4u + (b >> 3)];
                    const uint32_t bin = (uint32_t)(gl * LW) * 64u + 32u * (uint32_t)d + b; // bin inside the unit's column slice
                    if (listed)
                        mlist[my_off + k] = (bin << 8) | cnt;
                    else
                    {
                        gn_match mt;
                        mt.read   = read;
                        mt.target = slice * 64u * LW * 64u + bin;
                        mt.count  = cnt;
                        out[k]    = mt;
                    }
                    ++k;
                }
            }
            gn_wave_lds_sync(); // the list is complete; the next unit refills the row table
            if (listed && fits && !(p.emit_probe & 64u))
            {
                gn_match* seg = p.matches + base;
                for (uint32_t m = (uint32_t)lane; m < total; m += GN_WAVE)
                {
                    const uint32_t e = mlist[m];
                    gn_match       mt;
                    mt.read   = read;
                    mt.target = slice * 64u * LW * 64u + (e >> 8);
                    mt.count  = e & 0xFFu;
                    seg[m] = mt;
                }
                gn_wave_lds_sync(); // (the next unit's list must not overtake these reads)
            }
        }
        else if (fits && owner && any)
        {
            // every match goes to its rank among the lane's hit bits, so a read's segment leaves in ascending target
            // order (the gather pass then only copies)
            gn_match* out = p.matches + base + my_off;
            uint32_t  before = 0; // hits in the lane's lower dwords
#pragma unroll
            for (int d = 0; d < ND; ++d)
            {
#pragma unroll
                for (int j = 0; j < 4; ++j)
#pragma unroll
                    for (int pp = 0; pp < 2; ++pp)
                    {
                        uint32_t hbits = (byt[d][j][pp] + Kc) & 0x80808080u;
                        while (hbits)
                        {
                            const uint32_t y = (uint32_t)__builtin_ctz(hbits) >> 3;
                            hbits &= hbits - 1;
                            const uint32_t bitpos = 8 * y + 4 * pp + j; // bit t = 4*(2y+pp) + j of dword d
                            gn_match mt;
                            mt.read   = read;
                            mt.target = wi * 64 + 32 * d + bitpos;
                            mt.count  = (byt[d][j][pp] >> (8 * y)) & 0xFFu;
                            out[before + __popc(hit[d] & ((1u << bitpos) - 1u))] = mt;
                        }
                    }
                before += __popc(hit[d]);
            }
        }
    }
emitted:
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
    if (p.pre_mode)
    {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1)
            n_pre += (uint32_t)__shfl_xor((int)n_pre, off);
        if (lane == 0 && n_pre)
            atomicAdd(p.pre_ctr, (unsigned long long)n_pre);
    }
