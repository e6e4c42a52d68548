// sht_legendre.hip - K4: the Legendre contraction of the synthesis on FP64 MFMA, scalar (legendre_kernel) and
// spin-2 (legendre_pol_kernel) forms, and their launchers.  See sht_internal.h.
#include "sht_internal.h"

#ifndef LEG_STAMPS
#define LEG_STAMPS 0      // diagnostic build (make ab ... DEFS=-DLEG_STAMPS=1): s_memtime per phase of the item loop, summed over the workgroups' first waves
#endif
#if LEG_STAMPS
__device__ unsigned long long g_leg_stamps[16];
#define LEG_STAMP(acc)                                                                       \
    {                                                                                        \
        unsigned long long _t;                                                               \
        asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(_t)::"memory");           \
        acc += _t - leg_last;                                                                \
        leg_last = _t;                                                                       \
    }
#else
#define LEG_STAMP(acc)
#endif

// Lane roles of legendre_kernel (wave = 16 rings x 4 k-slots, the A operand of v_mfma_f64_16x16x4_f64):
// the K index of an MFMA is only a summation index, so slot kq need not hold row l0 + 2 kq of a window of 8
// consecutive l: it may hold ANY row, provided the B operand of that slot is the a_lm row of the same l.  Lane
// (ri = lane&15, kq = lane>>4) therefore walks its own CONTIGUOUS quarter of the item's l range (sht_internal.h:
// leg_seg): rows R(kq), R(kq) + 1, ... of ring ri, two per macro-step, and feeds BOTH - the even l-m row to the
// north+south accumulator, the odd one to the north-south accumulator.  Every lambda of a ring is computed once per
// column group (the staggered scheme of rounds 1-6, which legendre_pol_kernel below keeps, computed each four times:
// a lane ran all 8 rows of a window and fed 2 of them).  No cross-lane movement; the LDS-DMA puts global row
// R(kq) + par + 2 (7 st + ms) into LDS row 8 ms + 2 kq + par of stage st, with its coefficient pair beside it, so the
// consumer side (B reads, bank layout, accumulator tiles) is that of the staggered scheme.  The order in which an
// accumulator sums its rows depends on the item's l_begin, hence on the ring-tile height 128 RT.
// The recurrence runs in its SCALED two-instruction form (round 3): lambda_l = s_l mu_l with s_m = s_{m+1} = 1,
// s_l = B_l s_{l-2}, so that  mu_l = (alpha_l x) mu_{l-1} - mu_{l-2},  alpha_l = A_l s_{l-1} / s_l  - a multiply and an
// fma per step instead of two multiplies and an fma - and only the two values a lane feeds to the MFMAs are scaled back
// (lambda = s mu): 6 DP instructions per macro-step (2 steps + 2 scale-backs).  `coef` holds (alpha_l, s_l)
// (sht_plan.hip: d_coefmu); rows past lmax are zeros: s = 0 makes their A operand 0.
// A lane ENTERS AT A PAIR START.  `seed` is the plan's segment-seed table for this RT (sht_k4_segseed): per (m, ring)
// four states (mu_{R-2}, mu_{R-1}), one per lane group, in front of its entry row: the segment's first row when that
// is >= lstart - 1 (the lane is live from macro-step 0, no select), else the first pair start >= lstart - 1 inside the
// segment (one lane group per ring at the most; the head stages' macro-steps carry one compare + two selects per ring
// for it), zeros if the segment ends before (zero stays zero under the recurrence).
// NT = 16-column tiles per wave, RT = 16-ring row tiles per wave (RT x NT x 2 parities = 16 accumulator
// tiles = 128 VGPRs in both shipped shapes: <8,1> for >= 128 columns, <4,2> for 64-column shards, where a
// second, independent recurrence per lane keeps the recurrence : MFMA ratio of the wide shape).
template <int NT, int RT>
__global__ void __launch_bounds__(64 * LEG_WAVES, LEG_WAVES <= 4 ? 2 : 1)
legendre_kernel(int lmax, int npair, int nring, int ncols, const double *__restrict__ z,
                const double2 *__restrict__ coef, const int32_t *__restrict__ lstart,
                const double2 *__restrict__ seed, const int2 *__restrict__ items, int nitems,
                const double *__restrict__ alm, const double *__restrict__ zeros, double *__restrict__ inter,
                unsigned *__restrict__ queue) {
    using geom = leg_geom<NT, LEG_KT, LEG_NBUF, 0>;
    constexpr int TCOLS = geom::TCOLS, STRIDE = geom::STRIDE, CROWS = geom::CROWS, STAGE = geom::STAGE;
    constexpr int RPW = LEG_KT / LEG_WAVES;             // a_lm rows each wave moves per stage
    constexpr int PIECES = RPW + 1;                     // LDS-DMA pieces per wave per stage (+ coefficients)
    constexpr int TRINGS = LEG_RINGS * RT;              // ring pairs per workgroup
    constexpr int RPM = RPW / (LEG_KT / 8);             // a_lm pieces each wave issues per macro-step
    static_assert(RPM * (LEG_KT / 8) == RPW && RPM >= 1 && RPM == LEG_RPM, "whole a_lm pieces per macro-step");
    static_assert(LEG_WAVES == 8 && LEG_KT <= 64, "wave wv moves LDS rows wv + 8 ms: one segment (wv >> 1), one parity (wv & 1); one coefficient piece");
    extern __shared__ __attribute__((aligned(16))) double lds[];
    int *const s_next = reinterpret_cast<int *>(lds + LEG_NBUF * STAGE);  // next work item, two slots used in turn (carved after the ring)

    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int wv = __builtin_amdgcn_readfirstlane(wave);
    const int ri = lane & 15, kq = lane >> 4;
    const int d = 2 * kq;
    const int L = lmax + 1;
    const int G = ncols >> 3;
    const long last_row = nalm_of(lmax) - 1;
    const unsigned lds_base_bytes = (unsigned)(size_t)(__attribute__((address_space(3))) double *)lds;
    const bool odd_lane = lane & 1;

    // Rings of a tile -> waves: interleaved (ring = 8 j + wave), so every wave sees the tile's whole range of first
    // contributing l.  (Consecutive blocks of rings per wave were measured neutral, 56.6 vs 56.5 ms: HISTORY.md.)
    auto ring_in_tile = [&](int j) {     // j-th ring (0 .. 16 RT - 1) of this wave
        return j * LEG_WAVES + wave;
    };
    // Persistent workgroups.  Work item = (m, column group, ring tile); consecutive items are the ring
    // tiles of one a_lm slice, so the workgroups running at the same time share slices in L2 (they are
    // dealt over all 8 XCDs; packing a slice group onto ONE XCD was measured 24 % slower: every resident
    // workgroup of the XCD then hits the same 1-2 L2 channels in lock step; pairing the two ring tiles of a slice on
    // one XCD - LEG_XCD_PAIR of rounds 2-3 - was neutral and is gone).  Small m (long K) first.
    // `items` is the plan's list of the NON-EMPTY items in that order (sht_plan.hip: sht_k4_items; 27 % of the
    // (m, ring tile) pairs of cfg 3 have no contributing l at all), each with its first contributing l: decoding an
    // item is one 8-byte scalar load (rounds 1-3: two integer divisions and dependent loads from the first-l table).
    struct item_t {
        int m, cg, rtile, l_begin, T, nstage;
        long base_m;
        const double *src0;   // a_lm row (base_m + l_begin) of this column group (wave-uniform)
        int row_limit;        // rows behind src0 that exist: the last m's stage overhang is clamped to the last row
        int row0;             // first row (behind l_begin) of this WAVE's pieces: it serves segment wv >> 1, parity wv & 1
    };
    auto decode = [&](int it) {
        item_t w;
        const int2 e = items[it];                 // (m | rtile << 15 | cg << 23, first contributing l): wave-uniform
        w.m = e.x & 0x7fff;
        w.rtile = (e.x >> 15) & 0xff;
        w.cg = (e.x >> 23) & 0xff;
        const leg_seg sg = leg_seg::of(w.m, e.y, lmax);
        w.l_begin = sg.l_begin;
        w.T = sg.T;
        w.nstage = sg.nstage();
        w.base_m = alm_idx(0, w.m, lmax);
        w.src0 = alm + (size_t)w.cg * TCOLS + (size_t)(w.base_m + w.l_begin) * ncols;
        w.row_limit = (int)(last_row - (w.base_m + w.l_begin));
        w.row0 = (wv >> 1) * sg.Q() + (wv & 1);
        return w;
    };
    // LDS-DMA pieces: every wave issues exactly PIECES per stage (counted vmcnt): RPW a_lm rows (rows past
    // lmax are never used - their lambda is 0 - so any valid row is read, keeping the address scalar) and
    // the CROWS coefficient pairs (all waves write the same bytes).
    auto issue_row = [&](const item_t &w, int st, int rr) {
        const int row = wv + LEG_WAVES * rr;          // LDS row 8 ms + 2 kq + par of the stage: ms = rr
        int r = w.row0 + 2 * (st * LEG_MSPS + rr);
        r = r < w.row_limit ? r : w.row_limit;
        // wave-uniform: scalar address arithmetic only (the byte offset of a row fits 32 bits: < 2^12 rows of < 2^13 B... x 8)
        const char *src = reinterpret_cast<const char *>(w.src0) + (unsigned)(r * ncols) * 8u;
        const unsigned dst = lds_base_bytes + (unsigned)(((st % LEG_NBUF) * STAGE + row * STRIDE) * sizeof(double));
        if (lane < 8 * NT) glds16_s(src, 16u * lane, dst);
    };
    // The a_lm pieces of the steady-state stages ("fast" form: 3 instructions instead of 13).  Every instruction of
    // the macro-step loop costs issue time next to the MFMAs: the generic issue_row spends 8 scalar
    // instructions on the row address (clamp, multiply, 64-bit add, LDS offset) and 4 on saving / setting / restoring
    // M0.  Here the source is a per-STAGE scalar base + a per-lane byte offset that lives in a VGPR for the whole
    // kernel (one per piece of a stage: voff[p] = 16 lane + 16 p ncols - a wave's pieces are two rows apart), the LDS destination a per-stage
    // scalar + an immediate, written straight into M0 (nothing else in this kernel reads M0: the other LDS-DMA
    // helpers set it themselves and the compiler does not use it on gfx950; checked in the ISA).  Only taken when
    // every row of the refilled stage exists (no clamping): the stage loop's `refill_clean`.
    unsigned voff[RPW];
#pragma unroll
    for (int p = 0; p < RPW; p++) voff[p] = 16u * lane + (unsigned)(2 * p * ncols) * 8u;
    auto issue_row_fast = [&](const char *rsrc, unsigned rdst, auto pc) {
        constexpr int P = decltype(pc)::value;
        constexpr int IMM = P * LEG_WAVES * STRIDE * 8;
        const unsigned vo = voff[P];     // (asm operands inside a generic lambda do not capture: name a local)
        const bool on = NT == 8 || lane < 8 * NT;
        if (on)
            asm volatile("s_add_u32 m0, %2, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1"
                         :
                         : "v"(vo), "s"(rsrc), "s"(rdst), "n"(IMM)
                         : "memory", "scc");     // (s_add_u32 writes SCC: undeclared, it ate the stage loop's compare; M0 cannot be
                                                 //  declared: hipcc treats it as reserved - "may not be preserved" - so the
                                                 //  contract stays the comment above, checked in the ISA by tools/asm_of.sh)
    };
    auto issue_coef = [&](const item_t &w, int st) {
        // lane i < LEG_KT fetches the pair of LDS row i = 8 ms + 2 kq + par: global row R(kq) + par + 2 (7 st + ms)
        const int l = w.l_begin + ((lane >> 1) & 3) * 2 * w.T + (lane & 1) + 2 * (st * LEG_MSPS + (lane >> 3));
        const double *src = (l <= lmax) ? reinterpret_cast<const double *>(coef + w.base_m + l) : zeros;
        const unsigned dst = lds_base_bytes + (unsigned)(((st % LEG_NBUF) * STAGE + LEG_KT * STRIDE) * sizeof(double));
        if (lane < LEG_KT) glds16(src, dst);
    };
    auto issue_stage = [&](const item_t &w, int st) {
        issue_coef(w, st);
#pragma unroll
        for (int rr = 0; rr < RPW; rr++) issue_row(w, st, rr);
    };

    // dynamic work queue (one atomic per item, fetched one item ahead): items differ a lot in length
    // (polar ring tiles start late, large m is short), a static assignment left ~10 % on the table.
    // The first gridDim.x entries are pre-assigned; the queue starts behind them.
    const int nwg = (int)gridDim.x;
    auto clamp_item = [&](unsigned t) { return t < (unsigned)nitems ? (int)t : nitems; };
    // ring state of an item: cos(theta), first contributing l and the lane group's entry state (plan: sht_k4_segseed)
    auto load_rings = [&](const item_t &w, double (&x)[RT], int (&my_ls)[RT], double2 (&sd)[RT]) {
#pragma unroll
        for (int q = 0; q < RT; q++) {
            const int ring = w.rtile * TRINGS + ring_in_tile(ri + 16 * q);
            x[q] = 0.0;
            my_ls[q] = lmax + 1;
            sd[q] = make_double2(0.0, 0.0);
            if (ring < npair) {
                x[q] = z[ring];
                const long o = (long)w.m * npair + ring;
                my_ls[q] = lstart[o];
                sd[q] = seed[4 * o + kq];
            }
        }
    };
    int item = (int)blockIdx.x;
    if (item >= nitems) return;
    item_t w = decode(item);
    double x[RT];
    int my_ls[RT];
    double2 sd[RT];
    // order of the vector-memory operations at an item boundary (vmcnt retires in order): queue atomic, ring state,
    // first stage(s) of the next item, THEN the epilogue stores of the current one; the next item's prologue then has
    // nothing to load.  (Measured and dropped, round 4: a first-stage wait of vmcnt(<stores of a full tile>) that lets
    // the stores drain behind the next item's first macro-steps: +0.45 ms - the refill pieces of that stage queue behind
    // the stores; and an epilogue with a DPP exchange and scalar-base addressing, half the VALU instructions and no
    // LDS permutes: no change - the epilogue runs at the CU's store path, 32 B/clk for these 64-byte segments.)
    if (tid == 0) s_next[0] = clamp_item(nwg + atomicAdd(queue, 1u));
    load_rings(w, x, my_ls, sd);
#pragma unroll
    for (int st = 0; st < LEG_NBUF - 1; st++)
        if (st < w.nstage) issue_stage(w, st);
    int slot = 0;

#if LEG_STAMPS
    unsigned long long leg_last, t_pro = 0, t_head = 0, t_clean = 0, t_tail = 0, t_bnd = 0, t_epi = 0, t_bar2 = 0;
    unsigned long long n_head = 0, n_clean = 0, n_tail = 0, n_items = 0, t_tbar = 0, n_tail_ms = 0;
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(leg_last)::"memory");
#endif
    for (;;) {
        const int m = w.m;
        d4_t acce[RT][NT], acco[RT][NT];
#pragma unroll
        for (int q = 0; q < RT; q++)
#pragma unroll
            for (int t = 0; t < NT; t++) {
                acce[q][t] = (d4_t){0.0, 0.0, 0.0, 0.0};
                acco[q][t] = (d4_t){0.0, 0.0, 0.0, 0.0};
            }
        {
            // rings are dealt to the waves interleaved (ring = tile base + 8 (ri + 16 q) + wave) so that every
            // wave of the workgroup has the same mix of first-contributing l and reaches the barriers together
            double p0[RT], p1[RT];
            int ent[RT];
            int minent = LEG_NEVER, maxent = -1;
            const leg_seg sg = {w.l_begin, w.T};
#pragma unroll
            for (int q = 0; q < RT; q++) {
                // the lane's entry macro-step (item-wide index g = 7 st + ms): live from the start with the plan's state
                // (0), zero until it enters mid-way (> 0: the one lane group whose segment holds the ring's row
                // lstart - 1), or never (the plan's state is zero then)
                ent[q] = sg.entry(kq, my_ls[q], lmax);
                p0[q] = ent[q] == 0 ? sd[q].x : 0.0;
                p1[q] = ent[q] == 0 ? sd[q].y : 0.0;
                minent = min(minent, ent[q]);
                maxent = max(maxent, ent[q] == LEG_NEVER ? -1 : ent[q]);
            }
            // wave-uniform bounds of the entry steps: the skip tests of the macro-step loop become scalar compares
            // (every vector instruction there costs issue time next to the MFMAs).  Before ws_minent all 64 lanes of
            // the wave are zero; behind ws_maxent no lane enters any more.
            const int ws_minent = wave_min(minent), ws_maxent = wave_max(maxent);
            // The ring's loads (z, first row, seed pair) are CONSUMED here.  Left to the compiler, the wait for the seed pair
            // lands at its only use - the injection branch inside the macro-step loop - and where its registers are
            // reused in the epilogue, as an s_waitcnt vmcnt(0): vmcnt is in order, so that wait also drains every LDS-DMA
            // piece in flight (the stage being refilled; in the epilogue the next item's first stages, just requested).
#pragma unroll
            for (int q = 0; q < RT; q++) asm volatile("" ::"v"(x[q]), "v"(sd[q].x), "v"(sd[q].y), "v"(my_ls[q]));

            // Stage loop in three consecutive pieces (same body, `stage` below): the head stages in which lanes of
            // the wave still enter, the steady-state stages - no lane enters any more, all 7 macro-steps belong to the
            // item - whose macro-steps carry no tests at all and are fully unrolled (every scalar compare / branch / loop
            // increment costs issue time next to the MFMAs), and the last stage, which stops after T mod 7 macro-steps.
            // A stage is "clean" when (lo) some lane of the wave is live and none enters in it or later - true from some
            // stage on - and (hi) all its macro-steps are < T, it refills the ring and every row of the stage it refills
            // exists (the fast pieces do not clamp; segment 3 reaches furthest: row 6 T + 14 (st + 1) - 1 behind l_begin
            // is the last of stage st) - true up to some stage.  Both bounds are found once per item, so the steady-state
            // loop's own condition is one scalar compare.
            auto stage_lo = [&](int st) {
                const int g0 = st * LEG_MSPS;
                return (ws_minent <= g0) && (ws_maxent < g0);
            };
            int st_hi = min(min(w.T / LEG_MSPS, (w.row_limit + 1 - 6 * w.T) / (2 * LEG_MSPS) - LEG_NBUF + 1),
                            w.nstage - LEG_NBUF + 1);
            st_hi = __builtin_amdgcn_readfirstlane(st_hi);
            // One stage = LEG_MSPS macro-steps = LEG_KT rows of l, 2 LEG_MSPS from each segment.  CLEAN: 1 steady-state stages (no tests at all), 2 head stages whose rows all
            // exist and in which some lane of the wave is live from the first macro-step (unrolled like the steady-state
            // ones, fast refill pieces, one basic block: the entry select - a compare and two 64-bit selects per ring -
            // runs in every macro-step, no scalar tests), 0 the rolled generic form (the last stage, heads of items too
            // short for the fast pieces, and the rare stages in front of a wave's first entry: scalar skip tests).
            auto stage = [&](auto clean, const int st) __attribute__((always_inline)) {
                constexpr int CLEAN = decltype(clean)::value;
                // own pieces of stage st have landed when at most the pieces of the (up to LEG_NBUF-2) younger
                // stages are still in flight (anything younger than those only makes the wait stricter)
                if (LEG_NBUF >= 4 && st + 2 < w.nstage) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * PIECES) : "memory");
                else if (LEG_NBUF >= 3 && st + 1 < w.nstage) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(PIECES) : "memory");
                else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                __syncthreads();  // everyone's pieces of stage st landed; everyone is done reading stage st-1
#if LEG_STAMPS
                if constexpr (!CLEAN) LEG_STAMP(t_tbar);
#endif
                const bool refill = CLEAN ? true : (st + LEG_NBUF - 1 < w.nstage);   // (the clean loops only take refilling stages)
                if (refill) issue_coef(w, st + LEG_NBUF - 1);
                const int g0 = st * LEG_MSPS;
                const double *sb = lds + (st % LEG_NBUF) * STAGE;
                const double2 *sc = reinterpret_cast<const double2 *>(sb + LEG_KT * STRIDE) + d;
                // per-stage scalars of the fast refill pieces (CLEAN stages only)
                const char *const rsrc = reinterpret_cast<const char *>(w.src0) +
                                         (unsigned)((w.row0 + 2 * LEG_MSPS * (st + LEG_NBUF - 1)) * ncols) * 8u;
                const unsigned rdst = __builtin_amdgcn_readfirstlane(
                    lds_base_bytes + (unsigned)((((st + LEG_NBUF - 1) % LEG_NBUF) * STAGE + wv * STRIDE) * sizeof(double)));
                // One macro-step (2 rows of each segment, 16 MFMAs in the <8,1> shape).  `ms` is its index inside the stage: an
                // integral_constant in the CLEAN stages, so that every LDS offset and the LDS-DMA destination of the
                // refill piece are immediates, and the loop variable in the rolled stages.
                auto macro_step = [&](auto ms) __attribute__((always_inline)) {
                    // one a_lm piece of the stage being refilled per macro-step: spreads the LDS-DMA issue
                    // over the MFMA work instead of an 8-wave burst behind the barrier (measured 7 % of time)
                    if constexpr (CLEAN != 0) {
                        static_for<RPM>([&](auto r) {
                            constexpr int P = decltype(ms)::value * RPM + decltype(r)::value;
                            issue_row_fast(rsrc, rdst, std::integral_constant<int, P>{});
                        });
                    } else if (refill) {
#pragma unroll
                        for (int r = 0; r < RPM; r++) issue_row(w, st + LEG_NBUF - 1, ms * RPM + r);
                    }
                    const int g = g0 + ms;                 // macro-step of the item
                    if (!CLEAN && g >= w.T) return;
                    // no lane of this wave is live yet (all states and A operands are zero): skip the macro-step entirely
                    // (the stages in front of the wave's first entry run in the rolled form: see the stage loops)
                    if (CLEAN == 0 && g < ws_minent) return;
                    double ae[RT], ao[RT];
                    double2 c[2];
#pragma unroll
                    for (int j = 0; j < 2; j++) c[j] = sc[8 * ms + j];
                    // the entry select: in the unrolled head stages unconditionally - they stay one basic block, and a
                    // select no lane needs changes nothing; in the rolled form only while (scalar) some lane of the wave
                    // may still enter at or after this macro-step
                    if (CLEAN == 2 || (CLEAN == 0 && ws_maxent >= g)) {
#pragma unroll
                        for (int q = 0; q < RT; q++) {
                            const bool inj = (ent[q] == g);
                            p0[q] = inj ? sd[q].x : p0[q];
                            p1[q] = inj ? sd[q].y : p1[q];
                        }
                    }
#pragma unroll
                    for (int j = 0; j < 2; j++) {
#pragma unroll
                        for (int q = 0; q < RT; q++) {
                            const double vv = fma(c[j].x * x[q], p1[q], -p0[q]);
                            p0[q] = p1[q];
                            p1[q] = vv;
                            if (j == 0) ae[q] = vv * c[0].y;      // lambda = s mu
                            if (j == 1) ao[q] = vv * c[1].y;
                        }
                    }
#if LEG_STAMPS
                    if constexpr (!CLEAN) n_tail_ms++;
#endif
                    const double *be = sb + (8 * ms + d) * STRIDE + ri;
                    const double *bo = be + STRIDE;
#pragma unroll
                    for (int t = 0; t < NT; t++) {
                        const double bev = be[16 * t], bov = bo[16 * t];
#pragma unroll
                        for (int q = 0; q < RT; q++) {
                            acce[q][t] = __builtin_amdgcn_mfma_f64_16x16x4f64(ae[q], bev, acce[q][t], 0, 0, 0);
                            acco[q][t] = __builtin_amdgcn_mfma_f64_16x16x4f64(ao[q], bov, acco[q][t], 0, 0, 0);
                        }
                    }
                };
                // the macro-step loop of a CLEAN stage fully unrolled (loop counters and pointer increments become
                // immediates): 71.0 -> 69.5 ms; factors 2 and 3: no change
                if constexpr (CLEAN != 0) {
                    static_for<LEG_KT / 8>(macro_step);
                } else {
#pragma unroll 1
                    for (int ms = 0; ms < LEG_KT / 8; ms++) macro_step(ms);
                }
            };
            int st = 0;
            LEG_STAMP(t_pro);
#if LEG_STAMPS
            int st_mark = 0;
#endif
            // (rare: every lane of the wave is still zero at the start of the stage - the rolled form skips those macro-steps)
            for (; st < w.nstage && ws_minent > st * LEG_MSPS; st++) stage(std::integral_constant<int, 0>{}, st);
            for (; st < st_hi && !stage_lo(st); st++) stage(std::integral_constant<int, 2>{}, st);
            LEG_STAMP(t_head);
#if LEG_STAMPS
            n_head += st - st_mark, st_mark = st;
#endif
            for (; st < st_hi; st++) stage(std::integral_constant<int, 1>{}, st);
            LEG_STAMP(t_clean);
#if LEG_STAMPS
            n_clean += st - st_mark, st_mark = st;
#endif
            for (; st < w.nstage; st++) stage(std::integral_constant<int, 0>{}, st);
            LEG_STAMP(t_tail);
#if LEG_STAMPS
            n_tail += st - st_mark, n_items++;
#endif
        }

        // ---- next item: queue fetch for the one after it, its ring state and its first stages now, in front of this
        //      item's epilogue stores (see the note on the order above)
        const int cur_rtile = w.rtile, cur_cg = w.cg, cur_m = w.m;
        __syncthreads();  // all waves are done reading the stage ring; s_next[slot] (written during the previous boundary) is visible
        item = __builtin_amdgcn_readfirstlane(s_next[slot]);
        const bool have_next = item < nitems;
        unsigned fetched = 0;
        double xn[RT];
        int lsn[RT];
        double2 sdn[RT];
        if (have_next) {
            if (tid == 0) fetched = atomicAdd(queue, 1u);     // (its value is only needed behind the epilogue)
            w = decode(item);
            load_rings(w, xn, lsn, sdn);
#pragma unroll
            for (int st = 0; st < LEG_NBUF - 1; st++)
                if (st < w.nstage) issue_stage(w, st);
        }
        LEG_STAMP(t_bnd);

        // ---- epilogue: north = even + odd, south mirror = even - odd.  Adjacent lanes (columns n, n+1 of the
        //      same rows) swap one value each so that every lane stores 16 bytes: half the store instructions.
        //      (Tiles with no contributing l at all are not in the item list: K5 never reads cells with m >= mcut(ring).)
        {
#pragma unroll
            for (int q = 0; q < RT; q++)
#pragma unroll
                for (int t = 0; t < NT; t++) {
                    const int col = cur_cg * TCOLS + 16 * t + (ri & ~1);  // even column of the lane pair
                    const int g = col >> 3, cv = col & 7;
#pragma unroll
                    for (int rp = 0; rp < 2; rp++) {
                        const int r0 = 2 * rp, r1 = 2 * rp + 1;
                        const double n0 = acce[q][t][r0] + acco[q][t][r0], n1 = acce[q][t][r1] + acco[q][t][r1];
                        const double s0 = acce[q][t][r0] - acco[q][t][r0], s1 = acce[q][t][r1] - acco[q][t][r1];
                        // even lane keeps row r0 and sends its r1 value; odd lane keeps row r1 and sends its r0 value
                        const double nrecv = __shfl_xor(odd_lane ? n0 : n1, 1);
                        const double srecv = __shfl_xor(odd_lane ? s0 : s1, 1);
                        const int rr = odd_lane ? r1 : r0;
                        const int ro = cur_rtile * TRINGS + ring_in_tile(kq + 4 * rr + 16 * q);
                        if (ro < npair) {
                            const double2 nv = odd_lane ? make_double2(nrecv, n1) : make_double2(n0, nrecv);
                            *reinterpret_cast<double2 *>(inter + (((size_t)ro * G + g) * L + cur_m) * 8 + cv) = nv;
                            const int rs = nring - 1 - ro;
                            if (rs != ro) {
                                const double2 sv = odd_lane ? make_double2(srecv, s1) : make_double2(s0, srecv);
                                *reinterpret_cast<double2 *>(inter + (((size_t)rs * G + g) * L + cur_m) * 8 + cv) = sv;
                            }
                        }
                    }
                }
        }
        LEG_STAMP(t_epi);
        if (!have_next) break;
        // the other slot: its last readers passed the barrier above
        if (tid == 0) s_next[slot ^ 1] = clamp_item(nwg + fetched);
        slot ^= 1;
#pragma unroll
        for (int q = 0; q < RT; q++) x[q] = xn[q], my_ls[q] = lsn[q], sd[q] = sdn[q];
        LEG_STAMP(t_bar2);
    }
#if LEG_STAMPS
    if (tid == 0) {
        atomicAdd(&g_leg_stamps[0], t_pro), atomicAdd(&g_leg_stamps[1], t_head), atomicAdd(&g_leg_stamps[2], t_clean);
        atomicAdd(&g_leg_stamps[3], t_tail), atomicAdd(&g_leg_stamps[4], t_bnd), atomicAdd(&g_leg_stamps[5], t_epi);
        atomicAdd(&g_leg_stamps[6], t_bar2), atomicAdd(&g_leg_stamps[7], n_head), atomicAdd(&g_leg_stamps[8], n_clean);
        atomicAdd(&g_leg_stamps[9], n_tail), atomicAdd(&g_leg_stamps[10], n_items);
        atomicAdd(&g_leg_stamps[11], t_tbar), atomicAdd(&g_leg_stamps[12], n_tail_ms);
    }
#endif
}

// K4 for polarisation (spin 2): (E, B) -> (Q, U), what healpy.alm2map([T, E, B]) does for Q and U behind
// hputil.sphtrans_inv_real_pol (cora/util/hputil.py:394-432).  Same structure as legendre_kernel (persistent
// workgroups + queue, staggered-lane recurrence, LDS-DMA stage ring, even/odd parity accumulators), with the two
// A operands per parity derived from the scalar recurrence:
//     W_lm = (g1 r1 + g2) lambda_l + g3 r2 lambda_{l-1},     X_lm = g4 r2 lambda_l - m g3 r1 lambda_{l-1},
//     r1 = 1/sin^2, r2 = cos/sin^2 per ring (lane),  (g1..g4)(l, m) from the plan's table (staged through LDS):
//     g1 = -N2 (l - m^2), g2 = -N2 l(l-1)/2, g3 = N2 (2l+1)/A_l, g4 = N2 m (l-1), N2 = 2/sqrt((l+2)(l+1)l(l-1)).
// The kernel accumulates S_W = sum_l W a and S_X = sum_l X a for the natural columns; channels are interleaved
// (E_f, B_f) so that one a_lm cell [re x4 | im x4] holds (Re E, Re B, .., Im E, Im B, ..) and
//     Re Q = -(S_W[ReE] + S_X[ImB]),  Im Q = -(S_W[ImE] - S_X[ReB]),  Re U = -(S_W[ReB] - S_X[ImE]),  Im U = -(S_W[ImB] + S_X[ReE])
// is a lane-xor-5 exchange in the epilogue; Q_f, U_f leave in the cell positions of E_f, B_f.  W has the parity
// (-1)^{l+m} of lambda under theta -> pi - theta, X the opposite: north = (W_e + W_o, X_e + X_o), south = (W_e - W_o, X_o - X_e).
#define LEGP_KT 32     // l rows per stage (the 4 accumulator sets leave room for NT = 4 only)
#define LEGP_NBUF 3
template <int NT>
using leg_pol_geom = leg_geom<NT, LEGP_KT, LEGP_NBUF, 4>;   // a_lm rows + (A, B) pairs + (g1..g4) rows
template <int NT>
__global__ void __launch_bounds__(64 * LEG_WAVES)
legendre_pol_kernel(int lmax, int npair, int nring, int ncols, const double *__restrict__ z,
                    const double *__restrict__ sth, const double2 *__restrict__ coef,
                    const double *__restrict__ polc, const int32_t *__restrict__ lstart,
                    const double2 *__restrict__ seed, const int32_t *__restrict__ lmin_tab,
                    const double *__restrict__ alm, const double *__restrict__ zeros, double *__restrict__ inter,
                    unsigned *__restrict__ queue) {
    using geom = leg_pol_geom<NT>;
    constexpr int KT = LEGP_KT, NBUF = LEGP_NBUF;
    constexpr int TCOLS = geom::TCOLS, STRIDE = geom::STRIDE, CROWS = geom::CROWS, STAGE = geom::STAGE;
    constexpr int RPW = KT / LEG_WAVES;
    constexpr int PIECES = RPW + 3;         // a_lm rows + the (A, B) piece + two pieces of the g table (see issue_coef)
    constexpr int TRINGS = LEG_RINGS;
    extern __shared__ __attribute__((aligned(16))) double lds[];
    int &s_next = *reinterpret_cast<int *>(lds + NBUF * STAGE);

    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int wv = __builtin_amdgcn_readfirstlane(wave);
    const int ri = lane & 15, kq = lane >> 4;
    const int d = 2 * kq;
    const int L = lmax + 1;
    const int G = ncols >> 3;
    const int ntile128 = (npair + LMIN_RINGS - 1) / LMIN_RINGS;
    const int ntile = (npair + TRINGS - 1) / TRINGS;
    const int ncg = ncols / TCOLS;
    const int nitems = L * ncg * ntile;
    const long last_row = nalm_of(lmax) - 1;
    const unsigned lds_base_bytes = (unsigned)(size_t)(__attribute__((address_space(3))) double *)lds;

    struct item_t {
        int m, cg, rtile, l_begin, nstage;
        long base_m;
        const double *src0;   // a_lm row (base_m + l_begin) of this column group (wave-uniform)
        int row_limit;        // rows behind src0 that exist
    };
    auto decode = [&](int it) {
        item_t w;
        const int gidx = it / ntile;
        w.rtile = it - gidx * ntile;
        w.m = gidx / ncg;
        w.cg = gidx - w.m * ncg;
        int lmin = lmax + 1;
        const int t_first = (w.rtile * TRINGS) / LMIN_RINGS;
        const int t_last = min((w.rtile * TRINGS + TRINGS - 1) / LMIN_RINGS, ntile128 - 1);
        for (int t128 = t_first; t128 <= t_last; t128++) lmin = min(lmin, lmin_tab[w.m * ntile128 + t128]);
        w.l_begin = w.m + ((lmin - w.m) & ~7);
        w.nstage = lmin <= lmax ? (lmax - w.l_begin) / KT + 1 : 0;
        w.base_m = alm_idx(0, w.m, lmax);
        w.src0 = alm + (size_t)w.cg * TCOLS + (size_t)(w.base_m + w.l_begin) * ncols;
        w.row_limit = (int)(last_row - (w.base_m + w.l_begin));
        return w;
    };
    auto issue_row = [&](const item_t &w, int st, int rr) {
        const int row = wv + LEG_WAVES * rr;
        int r = st * KT + row;
        r = r < w.row_limit ? r : w.row_limit;
        const char *src = reinterpret_cast<const char *>(w.src0) + (unsigned)(r * ncols) * 8u;   // scalar arithmetic only
        const unsigned dst = lds_base_bytes + (unsigned)(((st % NBUF) * STAGE + row * STRIDE) * sizeof(double));
        if (lane < 8 * NT) glds16_s(src, 16u * lane, dst);
    };
    // coefficient pieces of a stage: CROWS (A, B) pairs (16 B each) and CROWS (g1..g4) rows (32 B each = 2 CROWS
    // 16-byte chunks, contiguous in the table): 1 + 2 wave-instructions (CROWS = 40: 40 + 80 lanes)
    auto issue_coef = [&](const item_t &w, int st) {
        const int l0 = w.l_begin + st * KT;
        const int l = l0 + lane;
        const double *src = (l <= lmax) ? reinterpret_cast<const double *>(coef + w.base_m + l) : zeros;
        const unsigned dst = lds_base_bytes + (unsigned)(((st % NBUF) * STAGE + KT * STRIDE) * sizeof(double));
        if (lane < CROWS) glds16(src, dst);
        const double *gsrc = polc + 4 * (size_t)(w.base_m + l0);     // the table is padded: rows past the end exist
        const unsigned gdst = dst + (unsigned)(2 * CROWS * sizeof(double));
        glds16(gsrc + 2 * lane, gdst);
        if (lane < 2 * CROWS - 64) glds16(gsrc + 2 * (64 + lane), gdst + 64 * 16);
    };
    auto issue_stage = [&](const item_t &w, int st) {
        issue_coef(w, st);
#pragma unroll
        for (int rr = 0; rr < RPW; rr++) issue_row(w, st, rr);
    };

    int item = blockIdx.x;
    if (item >= nitems) return;
    item_t w = decode(item);
#pragma unroll
    for (int st = 0; st < NBUF - 1; st++)
        if (st < w.nstage) issue_stage(w, st);

    for (;;) {
        const int m = w.m;
        const double mval = (double)m;
        if (tid == 0) s_next = (int)(gridDim.x + atomicAdd(queue, 1u));
        d4_t awe[NT], awo[NT], axe[NT], axo[NT];
#pragma unroll
        for (int t = 0; t < NT; t++) {
            awe[t] = (d4_t){0.0, 0.0, 0.0, 0.0};
            awo[t] = (d4_t){0.0, 0.0, 0.0, 0.0};
            axe[t] = (d4_t){0.0, 0.0, 0.0, 0.0};
            axo[t] = (d4_t){0.0, 0.0, 0.0, 0.0};
        }
        if (w.nstage > 0) {
            const int ring = w.rtile * TRINGS + ri * LEG_WAVES + wave;
            double x = 0.0, r1 = 0.0, r2 = 0.0, p0 = 0.0, p1 = 0.0;
            double2 sd = make_double2(0.0, 0.0);
            int my_ls = lmax + 1;
            if (ring < npair) {
                x = z[ring];
                const double s = sth[ring];
                r1 = 1.0 / (s * s);
                r2 = x * r1;
                const long o = (long)m * npair + ring;
                my_ls = lstart[o];
                sd = seed[o];
            }
            const int ls_min = wave_min(my_ls);  // wave-uniform: the skip tests become scalar compares
            int inj_l = my_ls;
            const double2 *cf = coef + w.base_m;
            {
                const int lf = w.l_begin + d;
                if (my_ls < lf) {
                    p0 = sd.x;
                    p1 = sd.y;
                    for (int l = my_ls + 1; l < lf; l++) {
                        const double2 c = (l <= lmax) ? cf[l] : make_double2(0.0, 0.0);
                        const double vv = fma(c.x * x, p1, -(c.y * p0));
                        p0 = p1;
                        p1 = vv;
                    }
                    inj_l = 0x7fffffff;
                }
            }
            const int ws_maxinj = wave_max(inj_l == 0x7fffffff ? -1 : inj_l);   // wave-uniform: last row at which a ring of the wave starts
            asm volatile("" ::"v"(x), "v"(sd.x), "v"(sd.y), "v"(my_ls), "v"(r1), "v"(r2));   // (the ring's loads are consumed here: see legendre_kernel)
            auto stage_clean = [&](int st) {
                const int ls = w.l_begin + st * KT;
                return (ls + KT - 1 <= lmax) && (ls_min <= ls) && (ws_maxinj < ls);
            };
            // One stage = KT rows of l, as in legendre_kernel: CLEAN = 1 for the steady-state stages (no tests, always
            // refilling, macro-steps unrolled), 0 otherwise (rolled).
            auto stage = [&](auto clean, const int st) __attribute__((always_inline)) {
                constexpr bool CLEAN = decltype(clean)::value != 0;
                if (st + 1 < w.nstage) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(PIECES) : "memory");
                else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                __syncthreads();
                const bool refill = CLEAN ? true : (st + NBUF - 1 < w.nstage);
                if (refill) issue_stage(w, st + NBUF - 1);
                const int ls = w.l_begin + st * KT;
                const double *sb = lds + (st % NBUF) * STAGE;
                const double2 *sc = reinterpret_cast<const double2 *>(sb + KT * STRIDE) + d;
                const double *sg = sb + KT * STRIDE + 2 * CROWS + 4 * d;
                auto macro_step = [&](const int ms) __attribute__((always_inline)) {
                    const int l0 = ls + 8 * ms;
                    if (!CLEAN && l0 > lmax) return;
                    if (!CLEAN && ls_min > l0 + 13) return;
                    double2 c[8];
#pragma unroll
                    for (int j = 0; j < 8; j++) c[j] = sc[8 * ms + j];
                    const int lf = l0 + d;
                    // lambda at lf-1, lf (even l-m slot of this lane), lf+1 (odd slot); then 6 more steps
                    double lm1 = p1, le = 0.0, lo = 0.0;
                    double lem1, lom1;
                    if (!CLEAN && ws_maxinj >= l0 && __any(inj_l >= lf && inj_l < lf + 8)) {
#pragma unroll
                        for (int j = 0; j < 8; j++) {
                            double vv = fma(c[j].x * x, p1, -(c[j].y * p0));
                            const bool inj = (lf + j == inj_l);
                            vv = inj ? sd.y : vv;
                            p0 = inj ? sd.x : p1;
                            p1 = vv;
                            if (j == 0) {
                                le = vv;
                                lm1 = p0;      // lambda_{lf-1} as the recurrence sees it (the seed if injected here)
                            }
                            if (j == 1) lo = vv;
                        }
                        lem1 = lm1, lom1 = le;
                        if (lf + 1 == inj_l) lom1 = sd.x;
                    } else {
                        // no ring of the wave starts inside this macro-step: plain recurrence (the compare and the
                        // three 64-bit selects per step were two thirds of the VALU instructions of the loop)
#pragma unroll
                        for (int j = 0; j < 8; j++) {
                            const double vv = fma(c[j].x * x, p1, -(c[j].y * p0));
                            p0 = p1;
                            p1 = vv;
                            if (j == 0) le = vv;
                            if (j == 1) lo = vv;
                        }
                        lem1 = lm1, lom1 = le;
                    }
                    if (!CLEAN && ls_min > l0 + 7) return;
                    // W, X at the two l of this lane
                    const double4 ge = *reinterpret_cast<const double4 *>(sg + 4 * (8 * ms));
                    const double4 go = *reinterpret_cast<const double4 *>(sg + 4 * (8 * ms + 1));
                    const double We = fma(fma(ge.x, r1, ge.y), le, (ge.z * r2) * lem1);
                    const double Xe = fma(ge.w * r2, le, -((mval * ge.z) * r1) * lem1);
                    const double Wo = fma(fma(go.x, r1, go.y), lo, (go.z * r2) * lom1);
                    const double Xo = fma(go.w * r2, lo, -((mval * go.z) * r1) * lom1);
                    const double *be = sb + (8 * ms + d) * STRIDE + ri;
                    const double *bo = be + STRIDE;
#pragma unroll
                    for (int t = 0; t < NT; t++) {
                        const double bev = be[16 * t], bov = bo[16 * t];
                        awe[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(We, bev, awe[t], 0, 0, 0);
                        awo[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(Wo, bov, awo[t], 0, 0, 0);
                        axe[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(Xe, bev, axe[t], 0, 0, 0);
                        axo[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(Xo, bov, axo[t], 0, 0, 0);
                    }
                };
                if constexpr (CLEAN) {
#pragma unroll
                    for (int ms = 0; ms < KT / 8; ms++) macro_step(ms);
                } else {
#pragma unroll 1
                    for (int ms = 0; ms < KT / 8; ms++) macro_step(ms);
                }
            };
            int st = 0;
            for (; st < w.nstage && !stage_clean(st); st++) stage(std::false_type{}, st);
            for (; st + NBUF - 1 < w.nstage && stage_clean(st); st++) stage(std::true_type{}, st);
            for (; st < w.nstage; st++) stage(std::false_type{}, st);
        }

        const int cur_rtile = w.rtile, cur_cg = w.cg, cur_m = w.m, cur_nstage = w.nstage;
        __syncthreads();
        item = __builtin_amdgcn_readfirstlane(s_next);
        const bool have_next = item < nitems;
        if (have_next) {
            w = decode(item);
#pragma unroll
            for (int st = 0; st < NBUF - 1; st++)
                if (st < w.nstage) issue_stage(w, st);
        }
        if (cur_nstage > 0) {
            // sigma of the column inside its 8-wide cell: +1 for (Re B, Im E) columns, -1 for (Re E, Im B)
            const int c8 = ri & 7;
            const double sigma = (((c8 & 1) ^ ((c8 >> 2) & 1)) != 0) ? 1.0 : -1.0;
#pragma unroll
            for (int t = 0; t < NT; t++) {
                const int col = cur_cg * TCOLS + 16 * t + ri;
                const int g = col >> 3, cv = col & 7;
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    const double swn = awe[t][r] + awo[t][r], sws = awe[t][r] - awo[t][r];
                    const double sxn = axe[t][r] + axo[t][r], sxs = axo[t][r] - axe[t][r];
                    const double pxn = __shfl_xor(sxn, 5), pxs = __shfl_xor(sxs, 5);
                    const int ro = cur_rtile * TRINGS + (kq + 4 * r) * LEG_WAVES + wave;
                    if (ro < npair) {
                        inter[(((size_t)ro * G + g) * L + cur_m) * 8 + cv] = -(swn - sigma * pxn);
                        const int rs = nring - 1 - ro;
                        if (rs != ro) inter[(((size_t)rs * G + g) * L + cur_m) * 8 + cv] = -(sws - sigma * pxs);
                    }
                }
            }
        }
        if (!have_next) break;
        __syncthreads();
    }
}
template <int NT, int RT>
static int launch_legendre(corahip_ctx *ctx, const corahip_sht_plan *p, int ncols, const double *alm, double *inter) {
    constexpr size_t shm = leg_geom<NT, LEG_KT, LEG_NBUF, 0>::LDS_BYTES;
    static_assert(LEG_KT != 56 || LEG_NBUF != 2 || shm == (NT == 8 ? 123920 : NT == 4 ? 66576 : NT == 2 ? 37904 : 23568),
                  "dynamic LDS of the shipped shapes");
    HIP_TRY(hipFuncSetAttribute((const void *)legendre_kernel<NT, RT>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)shm));
    const int2 *d_items = nullptr;
    int nitems = 0;
    int rc = sht_k4_items(ctx, p, RT, ncols / (16 * NT), &d_items, &nitems);
    if (rc) return rc;
    if (nitems == 0) return 0;
    const double2 *d_segseed = nullptr;
    if ((rc = sht_k4_segseed(ctx, p, RT, &d_segseed))) return rc;
    // persistent: as many workgroups as fit (LDS-limited: one per CU for NT = 8)
    const int per_cu = std::max<int>(1, std::min<int>(2, (int)((160 * 1024) / shm)));
    dim3 grid((unsigned)std::min<long>(nitems, (long)ctx->num_cu * per_cu));
    HIP_TRY(hipMemsetAsync(p->d_queue, 0, 1024, ctx->stream));
    legendre_kernel<NT, RT><<<grid, 64 * LEG_WAVES, shm, ctx->stream>>>(p->lmax, p->npair, p->nring, ncols, p->d_z,
                                                                       p->d_coefmu, p->d_lstart, d_segseed, d_items, nitems,
                                                                       alm, p->d_zeros, inter, p->d_queue);
    LAUNCH_CHECK();
#if LEG_STAMPS
    {
        unsigned long long hs[16], zero[16] = {0};
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        HIP_TRY(hipMemcpyFromSymbol(hs, HIP_SYMBOL(g_leg_stamps), sizeof(hs)));
        HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(g_leg_stamps), zero, sizeof(zero)));
        const double tot = (double)(hs[0] + hs[1] + hs[2] + hs[3] + hs[4] + hs[5] + hs[6] + hs[11]);
        fprintf(stderr, "K4 stamps: tail stages: wait + barrier %.0f ticks per stage, %.2f macro-steps with MFMAs per stage\n",
                hs[11] / std::max<double>(1.0, (double)hs[9]), hs[12] / std::max<double>(1.0, (double)hs[9]));
        fprintf(stderr, "K4 stamps <%d,%d> wg=%u items=%llu: prologue %.3f head %.3f (%llu st) clean %.3f (%llu st) tail %.3f (%llu st) "
                "boundary %.3f epilogue %.3f barrier2 %.3f | ticks/item %.0f ticks/clean-stage %.0f ticks/head-stage %.0f ticks/tail-stage %.0f\n",
                NT, RT, grid.x, hs[10], hs[0] / tot, hs[1] / tot, hs[7], hs[2] / tot, hs[8], hs[3] / tot, hs[9], hs[4] / tot, hs[5] / tot,
                hs[6] / tot, tot / std::max<double>(1.0, (double)hs[10]), hs[2] / std::max<double>(1.0, (double)hs[8]),
                hs[1] / std::max<double>(1.0, (double)hs[7]), hs[3] / std::max<double>(1.0, (double)hs[9]));
    }
#endif
    return 0;
}
int sht_legendre(corahip_ctx *ctx, const corahip_sht_plan *p, int ncols, const double *alm, double *inter) {
    StageTimer t(ctx, "legendre");
    const int ntile = ncols / 16;
    if (ntile % 8 == 0) return launch_legendre<8, 1>(ctx, p, ncols, alm, inter);
    if (ntile % 4 == 0) return launch_legendre<4, 2>(ctx, p, ncols, alm, inter);
    if (ntile % 2 == 0) return launch_legendre<2, 2>(ctx, p, ncols, alm, inter);
    return launch_legendre<1, 2>(ctx, p, ncols, alm, inter);
}

// (g1..g4)(l, m) of legendre_pol_kernel at alm_idx(l, m), long double on the host, once per plan
static int ensure_polc(corahip_ctx *ctx, corahip_sht_plan *p) {
    if (p->d_polc) return 0;
    const int lmax = p->lmax;
    std::vector<double> g((size_t)(p->nalm + 64) * 4, 0.0);
    for (int m = 0; m <= lmax; m++)
        for (int l = std::max(m, 2); l <= lmax; l++) {
            const long double ll = l, mm = m;
            const long double n2 = 2.0L / sqrtl((ll + 2.0L) * (ll + 1.0L) * ll * (ll - 1.0L));
            const long double al = l > m ? sqrtl((4.0L * ll * ll - 1.0L) / (ll * ll - mm * mm)) : 0.0L;
            double *o = &g[(size_t)alm_idx(l, m, lmax) * 4];
            o[0] = (double)(-n2 * (ll - mm * mm));
            o[1] = (double)(-n2 * ll * (ll - 1.0L) / 2.0L);
            o[2] = l > m ? (double)(n2 * (2.0L * ll + 1.0L) / al) : 0.0;
            o[3] = (double)(n2 * mm * (ll - 1.0L));
        }
    dev_buf<double> polc;
    HIP_TRY(polc.upload(g, ctx->stream));
    p->d_polc = std::move(polc);   // the guard above sees the table only once it is complete
    return 0;
}

template <int NT>
static int launch_legendre_pol(corahip_ctx *ctx, const corahip_sht_plan *p, int ncols, const double *alm, double *inter) {
    constexpr size_t shm = leg_pol_geom<NT>::LDS_BYTES;
    static_assert(shm == (NT == 4 ? 61072 : NT == 2 ? 36496 : 24208), "dynamic LDS of the shipped shapes");
    HIP_TRY(hipFuncSetAttribute((const void *)legendre_pol_kernel<NT>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)shm));
    const int ntile = (p->npair + LEG_RINGS - 1) / LEG_RINGS;
    const long nitems = (long)p->L * (ncols / (16 * NT)) * ntile;
    const int per_cu = std::max<int>(1, std::min<int>(2, (int)((160 * 1024) / shm)));
    dim3 grid((unsigned)std::min<long>(nitems, (long)ctx->num_cu * per_cu));
    HIP_TRY(hipMemsetAsync(p->d_queue, 0, 64, ctx->stream));
    legendre_pol_kernel<NT><<<grid, 64 * LEG_WAVES, shm, ctx->stream>>>(p->lmax, p->npair, p->nring, ncols, p->d_z, p->d_sth,
                                                                       p->d_coef, p->d_polc, p->d_lstart, p->d_seed,
                                                                       p->d_lmin, alm, p->d_zeros, inter, p->d_queue);
    LAUNCH_CHECK();
    return 0;
}
int sht_ensure_polc(corahip_ctx *ctx, corahip_sht_plan *p) { return ensure_polc(ctx, p); }
int sht_legendre_pol(corahip_ctx *ctx, corahip_sht_plan *p, int ncols, const double *alm, double *inter) {
    int rc = ensure_polc(ctx, p);
    if (rc) return rc;
    StageTimer t(ctx, "legendre_pol");
    const int ntile = ncols / 16;
    if (ntile % 4 == 0) return launch_legendre_pol<4>(ctx, p, ncols, alm, inter);
    if (ntile % 2 == 0) return launch_legendre_pol<2>(ctx, p, ncols, alm, inter);
    return launch_legendre_pol<1>(ctx, p, ncols, alm, inter);
}
