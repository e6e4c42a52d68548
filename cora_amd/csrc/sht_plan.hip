// sht_plan.hip - the (nside, lmax) plan of the HEALPix transforms: ring geometry, recurrence coefficients,
// polar seed table (first contributing l and the two recurrence values there), per-(m, ring block) first-l table,
// per-ring m cut-off, twiddles, Bluestein chirps / filters and the K5 launch classes.  See sht_internal.h.
#include "sht_internal.h"
#include "fft_shapes.h"

#include <array>
#include <memory>

// ------------------------------------------------------------------------------------
// plan-time kernels
// ------------------------------------------------------------------------------------
__device__ static inline void scaled_pow(double s, int n, double &mant, int &ex) {
    // s^n = mant * 2^ex with mant in [0.5, 1); exponentiation by squaring, renormalised
    int e;
    double f = frexp(s, &e);
    double rm = 1.0;
    int re = 0;
    double bm = f;
    int be = e;
    while (n) {
        if (n & 1) {
            rm *= bm;
            re += be;
            int t;
            rm = frexp(rm, &t);
            re += t;
        }
        bm *= bm;
        be *= 2;
        int t;
        bm = frexp(bm, &t);
        be += t;
        n >>= 1;
    }
    mant = rm;
    ex = re;
}

// Terms of the Legendre sums with |lambda_lm| < 2^SEED_MIN_EXP are dropped (K4 starts its recurrence at the first l
// that reaches it; K4 neither writes nor K5 reads the F_m cells beyond the per-ring cut-off it implies).  Rounds 2-3: 2^-80 =
// 8.3e-25: the sum of all 2e6 dropped terms of a channel stays below 2e-18 of an O(1) coefficient, two decades
// under fp64 rounding.  (SHT engines truncate in the same spirit - libsharp, as the builder recalls it, by an m limit per
// ring; its source is not in this image and no figure for it is claimed here.)  The exponent is a PLAN parameter
// (corahip_sht_plan_create_ex, default SEED_MIN_EXP): the error of a pixel is bounded by sum_lm |a_lm| 2^cut, so a
// caller with a_lm of extreme dynamic range lowers it (-900 = the oracle's "exactly zero").  The first version used 2^-900:
// with it the rings 513..1023 of nside 1024 kept lmax + 1 > h + 1 cells, so their ring FFT took the aliased
// (LDS-atomic) fold and read 20-45 % more cells; 2^-120 followed (K4 66.2 -> 58.3 ms), 2^-80 took another 1.1 ms off
// K4 (56.4 -> 55.3 ms at cfg 3) with no change in any printed digit of the full-size comparisons.  The oracle keeps 2^-900.
// Round 4: 2^-70 = 8.5e-22 - this library's own choice, justified by the bound below and by measurement.  tools/cut_probe.py
// (cfg 3, unit-variance a_lm, maps against the 2^-900 plan): 2^-120 1.6e-13, 2^-80 3.4e-13, 2^-70 3.6e-13, 2^-60 4.6e-13,
// 2^-40 4.7e-13 of the rms - all of it the rounding of recurrences started at different rows, none of it truncation (the
// bound with every dropped term of a pixel adding coherently, sum_lm |a_lm| 2^cut ~ sqrt(nalm) rms 2^-70, is 1e-18 rms at
// lmax = 2048); K4 52.4 ms at 2^-80, 52.1 at 2^-70, 51.6 at 2^-60, 50.9 at 2^-40: a looser cut would buy another
// 0.5-1.2 ms and is not taken.
#ifndef SEED_MIN_EXP
#define SEED_MIN_EXP (-70)
#endif

// lstart[m][r]: first l at which |lambda_lm(ring r)| >= 2^min_exp (the plan's cut, default SEED_MIN_EXP = -70), with
// the two recurrence values there; terms below (< 8.5e-22 at the default) are dropped.
__global__ void seed_kernel(int lmax, int npair, int min_exp, const double *__restrict__ z, const double *__restrict__ sth,
                            const double *__restrict__ pref, const double2 *__restrict__ coef,
                            const double2 *__restrict__ coefmu, int32_t *__restrict__ lstart, double2 *__restrict__ seed,
                            double2 *__restrict__ seedmu, double2 *__restrict__ seed4) {
    int r = blockIdx.x * blockDim.x + threadIdx.x;
    int m = blockIdx.y;
    if (r >= npair) return;
    // seed4[o][kq]: the state (mu_{R-2}, mu_{R-1}) of the scaled recurrence in front of row R = R_kq, the first row of the
    // form m + 2 kq + 8 k (k >= 0) that is >= lstart - 1 - the start of the first 8-row window of legendre_kernel's lane
    // group kq in which the ring contributes (its lanes feed rows R, R + 1 of every window).  Every lane then enters at
    // a window start: no per-step injection tests in the kernel.  Rows lstart - 3 .. lstart - 1 appear with their true
    // values (below the cut, i.e. < 2^min_exp: harmless); in front of row m the state is (-mu_m, 0), which makes
    // mu_m = alpha_m x 0 + mu_m and mu_{m+1} = alpha_{m+1} x mu_m come out of the recurrence itself.
    auto emit4 = [&](long o, int ls, const double *lam /* rows ls-3 .. ls+5 */) {
        const double2 *cm = coefmu + alm_idx(0, m, lmax);
        double mu[9];
        for (int i = 0; i < 9; i++) {
            const int row = ls - 3 + i;
            mu[i] = (row >= m && row <= lmax) ? lam[i] / cm[row].y : 0.0;
        }
        for (int i = 0; i < 9; i++)
            if (ls - 3 + i == m - 2) mu[i] = -(lam[m - (ls - 3)] / cm[m].y);   // (s_m = 1)
        for (int kq = 0; kq < 4; kq++) {
            const int t = ls - 1 - m - 2 * kq;
            const int R = m + 2 * kq + (t > 0 ? ((t + 7) >> 3) << 3 : 0);
            const int i0 = R - 2 - (ls - 3);
            seed4[4 * o + kq] = make_double2(mu[i0], mu[i0 + 1]);
        }
    };
    double x = z[r];
    double pm;
    int pe;
    scaled_pow(sth[r], m, pm, pe);
    int t;
    double mant = frexp(pm * pref[m], &t);
    int sc = pe + t;
    if (m & 1) mant = -mant;
    long o = (long)m * npair + r;
    const double2 *cf = coef + alm_idx(0, m, lmax);
    double lam[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};       // lambda at rows lstart - 3 .. lstart + 5
    auto forward5 = [&](int ls, double q0, double q1, int e) {           // rows ls + 1 .. ls + 5 behind (q0, q1) 2^e
        for (int l = ls + 1; l <= ls + 5; l++) {
            double v = 0.0;
            if (l <= lmax) {
                const double2 c = cf[l];
                v = fma(c.x * x, q1, -(c.y * q0));
            }
            q0 = q1;
            q1 = v;
            lam[3 + l - ls] = ldexp(v, e);
        }
    };
    if (sc >= min_exp) {
        lstart[o] = m;
        seed[o] = make_double2(0.0, ldexp(mant, sc));
        seedmu[o] = make_double2(0.0, ldexp(mant, sc));     // s_m = 1
        lam[3] = ldexp(mant, sc);
        forward5(m, 0.0, mant, sc);
        emit4(o, m, lam);
        return;
    }
    double p0 = 0.0, p1 = mant;  // scaled by 2^sc
    double pm1 = 0.0, pm2 = 0.0; // the two rows in front of p0
    int found = lmax + 1;
    double s0 = 0.0, s1 = 0.0;
    const double lam_m = ldexp(mant, sc);   // (may underflow to 0: row m - 2 is only asked for when lstart <= m + 1)
    for (int l = m + 1; l <= lmax; l++) {
        double2 c = cf[l];
        double v = fma(c.x * x, p1, -(c.y * p0));
        pm2 = pm1;
        pm1 = p0;
        p0 = p1;
        p1 = v;
        if (fabs(p1) > 0x1p100) {
            pm2 *= 0x1p-100;
            pm1 *= 0x1p-100;
            p0 *= 0x1p-100;
            p1 *= 0x1p-100;
            sc += 100;
        }
        if (p1 != 0.0 && sc + ilogb(p1) >= min_exp) {
            found = l;
            s0 = ldexp(p0, sc);
            s1 = ldexp(p1, sc);
            break;
        }
    }
    lstart[o] = found;
    seed[o] = make_double2(s0, s1);
    if (found <= lmax) {
        lam[0] = ldexp(pm2, sc), lam[1] = ldexp(pm1, sc), lam[2] = s0, lam[3] = s1;
        if (m >= found - 3) lam[m - (found - 3)] = lam_m;   // (row m itself, wherever it sits in the window)
        forward5(found, p0, p1, sc);
        emit4(o, found, lam);
    } else {
        for (int kq = 0; kq < 4; kq++) seed4[4 * o + kq] = make_double2(0.0, 0.0);
    }
    // the same pair in the scaled form of the synthesis kernel: mu_l = lambda_l / s_l
    const double2 *cm = coefmu + alm_idx(0, m, lmax);
    seedmu[o] = found <= lmax ? make_double2(s0 / cm[found - 1].y, s1 / cm[found].y) : make_double2(0.0, 0.0);
}

// test hook: lambda_lm for one (m, ring pair), l = m..lmax, as the synthesis kernel forms them: the scaled recurrence
// mu_l = (alpha_l x) mu_{l-1} - mu_{l-2} from the mu seeds, lambda_l = s_l mu_l
__global__ void lambda_kernel(int lmax, int npair, int m, int r, const double *__restrict__ z,
                              const double2 *__restrict__ coefmu, const int32_t *__restrict__ lstart,
                              const double2 *__restrict__ seedmu, double *__restrict__ out) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    double x = z[r];
    long o = (long)m * npair + r;
    int ls = lstart[o];
    double2 sd = seedmu[o];
    const double2 *cf = coefmu + alm_idx(0, m, lmax);
    double p0 = 0.0, p1 = 0.0;
    for (int l = m; l <= lmax; l++) {
        double2 c = cf[l];
        double v = fma(c.x * x, p1, -p0);
        bool inj = (l == ls);
        v = inj ? sd.y : v;
        p0 = inj ? sd.x : p1;
        p1 = v;
        out[l - m] = l >= ls ? v * c.y : 0.0;
    }
}

// test hook: the same values as legendre_kernel's lane group kq forms them - zero in front of its entry row
// R = m + 2 kq + 8 k >= lstart - 1, the plan's entry state (seed4) there, the scaled recurrence behind it
__global__ void lambda_entry_kernel(int lmax, int npair, int m, int r, int kq, const double *__restrict__ z,
                                    const double2 *__restrict__ coefmu, const int32_t *__restrict__ lstart,
                                    const double2 *__restrict__ seed4, double *__restrict__ out) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const double x = z[r];
    const long o = (long)m * npair + r;
    const int ls = lstart[o];
    const double2 sd = seed4[4 * o + kq];
    const double2 *cf = coefmu + alm_idx(0, m, lmax);
    const int t = ls - 1 - m - 2 * kq;
    const int R = ls <= lmax ? m + 2 * kq + (t > 0 ? ((t + 7) >> 3) << 3 : 0) : 0x7fffffff;
    double p0 = 0.0, p1 = 0.0;
    for (int l = m; l <= lmax; l++) {
        if (l == R) {
            p0 = sd.x;
            p1 = sd.y;
        }
        const double2 c = cf[l];
        const double v = fma(c.x * x, p1, -p0);
        p0 = p1;
        p1 = v;
        out[l - m] = v * c.y;
    }
}
// first l of the item (m, ring tile of 128 rt ring pairs) that holds ring pair r: the minimum of the tile's 128-ring blocks
__device__ static inline int tile_lmin(int lmax, int npair, int rt, int m, int r, const int32_t *__restrict__ lmin_tab) {
    const int trings = LEG_RINGS * rt;
    const int ntile128 = (npair + LMIN_RINGS - 1) / LMIN_RINGS;
    const int tile = r / trings;
    const int t_first = (tile * trings) / LMIN_RINGS;
    const int t_last = min((tile * trings + trings - 1) / LMIN_RINGS, ntile128 - 1);
    int lmin = lmax + 1;
    for (int t = t_first; t <= t_last; t++) lmin = min(lmin, lmin_tab[m * ntile128 + t]);
    return lmin;
}
// segseed[o][kq]: the state (mu_{R-2}, mu_{R-1}) in front of the entry row of legendre_kernel's lane group kq for
// ring tiles of 128 rt ring pairs (sht_internal.h: leg_seg) - row R(kq) + 2 entry(kq) - and zeros for a lane group that
// never enters.  One walk per (m, ring): from the staggered table's state in front of the first pair start
// P0 >= lstart - 1 (seed4 of the lane group that starts there) forward in the kernel's own two-instruction form and
// order, rows past lmax with the zero pair the kernel reads for them; every entry row is a pair start >= P0.
__global__ void segseed_kernel(int lmax, int npair, int rt, const double *__restrict__ z,
                               const double2 *__restrict__ coefmu, const int32_t *__restrict__ lstart,
                               const double2 *__restrict__ seed4, const int32_t *__restrict__ lmin_tab,
                               double2 *__restrict__ segseed) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    const int m = blockIdx.y;
    if (r >= npair) return;
    const long o = (long)m * npair + r;
    const int ls = lstart[o];
    double2 out[4];
    int erow[4], last = -1;
    const leg_seg sg = leg_seg::of(m, tile_lmin(lmax, npair, rt, m, r, lmin_tab), lmax);
    for (int kq = 0; kq < 4; kq++) {
        out[kq] = make_double2(0.0, 0.0);
        const int e = sg.entry(kq, ls, lmax);
        erow[kq] = e == LEG_NEVER ? -1 : sg.R(kq) + 2 * e;
        last = max(last, erow[kq]);
    }
    if (last >= 0) {
        const int t = ls - 1 - m;
        const int P0 = m + (t > 0 ? ((t + 1) >> 1) << 1 : 0);
        const double2 s0 = seed4[4 * o + (((P0 - m) >> 1) & 3)];
        const double2 *cm = coefmu + alm_idx(0, m, lmax);
        const double x = z[r];
        double p0 = s0.x, p1 = s0.y;
        for (int row = P0; row <= last; row += 2) {
            for (int kq = 0; kq < 4; kq++)
                if (erow[kq] == row) out[kq] = make_double2(p0, p1);
            for (int j = 0; j < 2; j++) {
                const double2 c = row + j <= lmax ? cm[row + j] : make_double2(0.0, 0.0);
                const double vv = fma(c.x * x, p1, -p0);
                p0 = p1;
                p1 = vv;
            }
        }
    }
    for (int kq = 0; kq < 4; kq++) segseed[4 * o + kq] = out[kq];
}
// test hook: lambda_lm as legendre_kernel's lane group kq forms them for ring tiles of 128 rt ring pairs - zero outside
// the rows it feeds, [entry row, R(kq) + Q) - and the geometry: info = (l_begin, T, R(kq), entry row or -1)
__global__ void lambda_segment_kernel(int lmax, int npair, int rt, int m, int r, int kq, const double *__restrict__ z,
                                      const double2 *__restrict__ coefmu, const int32_t *__restrict__ lstart,
                                      const double2 *__restrict__ segseed, const int32_t *__restrict__ lmin_tab,
                                      double *__restrict__ out, int32_t *__restrict__ info) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const double x = z[r];
    const long o = (long)m * npair + r;
    const leg_seg sg = leg_seg::of(m, tile_lmin(lmax, npair, rt, m, r, lmin_tab), lmax);
    const int e = sg.entry(kq, lstart[o], lmax);
    const int erow = e == LEG_NEVER ? -1 : sg.R(kq) + 2 * e;
    info[0] = sg.l_begin, info[1] = sg.T, info[2] = sg.R(kq), info[3] = erow;
    const double2 sd = segseed[4 * o + kq];
    const double2 *cf = coefmu + alm_idx(0, m, lmax);
    double p0 = 0.0, p1 = 0.0;
    for (int l = m; l <= lmax; l++) {
        double v = 0.0;
        if (l >= sg.R(kq) && l < sg.R(kq) + sg.Q()) {
            if (l == erow) {
                p0 = sd.x;
                p1 = sd.y;
            }
            const double2 c = cf[l];
            const double vv = fma(c.x * x, p1, -p0);
            p0 = p1;
            p1 = vv;
            v = vv * c.y;
        }
        out[l - m] = v;
    }
}
// per ring: mcut = number of m (from 0) whose lambda_lm reach the plan's cut for some l <= lmax; F_m of the ring
// is exactly zero beyond (lstart is monotone in m), so K4 need not write and K5 need not read those cells
__global__ void mcut_kernel(int lmax, int npair, int nring, const int32_t *__restrict__ lstart,
                            int32_t *__restrict__ mcut) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= npair) return;
    int c = 0;
    for (int m = 0; m <= lmax; m++)
        if (lstart[(long)m * npair + r] <= lmax) c = m + 1;
    mcut[r] = c;
    mcut[nring - 1 - r] = c;
}

// per (m, ring tile) minimum of lstart: the first l the tile's workgroup has to visit
__global__ void lmin_kernel(int lmax, int npair, int ntile, const int32_t *__restrict__ lstart,
                            int32_t *__restrict__ lmin_tab) {
    const int m = blockIdx.x, t = threadIdx.x;
    if (t >= ntile) return;
    int v = lmax + 1;
    for (int r = t * LMIN_RINGS; r < min((t + 1) * LMIN_RINGS, npair); r++) v = min(v, lstart[(long)m * npair + r]);
    lmin_tab[m * ntile + t] = v;
}
// FP64 MFMA instructions legendre_kernel<NT, RT> ISSUES for one column group, summed over (m, ring tile, wave): the
// kernel's own skip logic restated (sht_legendre.hip: legendre_kernel's macro_step) - an item starts at
// l_begin = m + ((lmin - m) & ~7) with lmin the tile's first contributing l and has T macro-steps (leg_seg); wave w of
// the workgroup owns the rings tile * 128 RT + 8 j + w (j < 16 RT) and executes the 2 NT RT MFMAs of macro-step g < T
// unless all its 64 lanes are still zero: g >= ws_minent, the first entry step of its (ring, lane group) lanes - 0 as
// soon as one ring contributes at the first row of some segment, so the count is close to T per wave.  Thread = (m, tile, wave);
// out accumulates the number of executed macro-steps.  The count is what SQ_INSTS_VALU_MFMA_F64 reads for the
// launch (tests/test_gpu_fullsize.py checks it against the committed PMC profile): the roofline fraction of K4 is
// priced on it, not on the algorithmic 8 nside nalm F of SURVEY 8(d), which counts terms nobody has to compute.
__global__ void k4_count_kernel(int lmax, int npair, int rt, const int32_t *__restrict__ lstart,
                                const int32_t *__restrict__ lmin_tab, unsigned long long *__restrict__ out,
                                unsigned long long *__restrict__ out_clean) {
    const int trings = LEG_RINGS * rt;
    const int ntile = (npair + trings - 1) / trings;
    const int ntile128 = (npair + LMIN_RINGS - 1) / LMIN_RINGS;
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long total = (long)(lmax + 1) * ntile * LEG_WAVES;
    unsigned long long n = 0;
    if (idx < total) {
        const int wave = (int)(idx % LEG_WAVES);
        const int tile = (int)((idx / LEG_WAVES) % ntile);
        const int m = (int)(idx / ((long)LEG_WAVES * ntile));
        int lmin = lmax + 1;
        const int t_first = (tile * trings) / LMIN_RINGS;
        const int t_last = min((tile * trings + trings - 1) / LMIN_RINGS, ntile128 - 1);
        for (int t = t_first; t <= t_last; t++) lmin = min(lmin, lmin_tab[m * ntile128 + t]);
        if (lmin <= lmax) {
            // the wave's entry bounds as the kernel forms them: over its 16 rt rings x 4 lane groups
            const leg_seg sg = leg_seg::of(m, lmin, lmax);
            int ws_minent = LEG_NEVER, ws_maxent = -1;
            for (int j = 0; j < 16 * rt; j++) {
                const int ring = tile * trings + j * LEG_WAVES + wave;
                if (ring >= npair) continue;
                const int ls = lstart[(long)m * npair + ring];
                for (int kq = 0; kq < 4; kq++) {
                    const int e = sg.entry(kq, ls, lmax);
                    ws_minent = min(ws_minent, e);
                    if (e != LEG_NEVER) ws_maxent = max(ws_maxent, e);
                }
            }
            if (ws_minent < sg.T) n = (unsigned long long)(sg.T - ws_minent);
            if (out_clean) {
                // macro-steps of this wave that run in the test-free steady-state stages (sht_legendre.hip: stage_lo && st < st_hi);
                // row_limit is not restated: it only matters for the last m's
                const int st_hi = min(sg.T / LEG_MSPS, sg.nstage() - LEG_NBUF + 1);
                unsigned long long nc = 0;
                for (int st = 0; st < st_hi; st++) {
                    const int g0 = st * LEG_MSPS;
                    if (ws_minent <= g0 && ws_maxent < g0) nc += LEG_MSPS;
                }
                if (nc) atomicAdd(out_clean, nc);     // (diagnostics only: one atomic per thread, divergent code - no wave reduction here)
            }
        }
    }
    // wave-level sum, one atomic per wave
    for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o);
    if ((threadIdx.x & 63) == 0 && n) atomicAdd(out, n);
}
// e^{i t phi0} of north-cap ring blockIdx.x, t < 512, and the steps e^{i 256 phi0}, e^{i 512 phi0}: the expression
// FrontEnd::fold (sht_ringfft_ct.hip) evaluated per item - phi0 / pi as the kernels form it, then sincospi
__global__ void fold_phase_kernel(const double *__restrict__ phi0, double2 *__restrict__ ph, double2 *__restrict__ step) {
    const int r = blockIdx.x, t = threadIdx.x;
    const double pop = phi0[r] / M_PI;
    double s, c;
    sincospi((double)t * pop, &s, &c);
    ph[(size_t)r * 512 + t] = make_double2(c, s);
    if (t < 2) {
        sincospi((double)(256 << t) * pop, &s, &c);
        step[r * 2 + t] = make_double2(c, s);
    }
}
// Bluestein tables for cap ring i (h = 2i not a power of two): chirp b_j = e^{i pi j^2/h}, j < h,
// and filt = FFT_P(conj chirp wrapped), stored in the digit-reversed order fft_dif produces.
__global__ void __launch_bounds__(256)
bluestein_table_kernel(const int32_t *__restrict__ blu_P, const int64_t *__restrict__ boff,
                       const int64_t *__restrict__ foff, double2 *__restrict__ chirp,
                       double2 *__restrict__ filt, const double2 *__restrict__ tw, int pmax, int tl_off) {
    extern __shared__ __attribute__((aligned(16))) double2 fbuf[];   // [fpad_len(maxlen) + 1]
    (void)tl_off;   // (size of fbuf; nothing lies behind it)
    const int i = blockIdx.x + 1;
    const int P = blu_P[i - 1];
    if (P == 0) return;
    const int h = 2 * i;
    double2 *b = chirp + boff[i - 1];
    for (int j = threadIdx.x; j < fpad_len(P); j += blockDim.x) fbuf[j] = make_double2(0.0, 0.0);
    __syncthreads();
    for (int j = threadIdx.x; j < h; j += blockDim.x) {
        const long q = ((long)j * j) % (2 * h);
        double s, c;
        sincospi((double)q / (double)h, &s, &c);
        b[j] = make_double2(c, s);
        fbuf[fpad(j)] = make_double2(c, -s);
        if (j > 0) fbuf[fpad(P - j)] = make_double2(c, -s);
    }
    __syncthreads();
    fft_dif<-1>(fbuf, 0, 1, P, tw, pmax);
    double2 *f = filt + foff[i - 1];
    for (int j = threadIdx.x; j < P; j += blockDim.x) f[j] = fbuf[fpad(j)];
}
// ------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------
int sht_k4_items(corahip_ctx *ctx, const corahip_sht_plan *cp, int rt, int ncg, const int2 **items, int *nitems) {
    corahip_sht_plan *p = const_cast<corahip_sht_plan *>(cp);      // (lazy caches of the plan)
    const auto key = std::make_pair(rt, ncg);
    auto it = p->k4_items.find(key);
    if (it == p->k4_items.end()) {
        const int ntile128 = (p->npair + LMIN_RINGS - 1) / LMIN_RINGS;
        if (p->h_lmin.empty()) {
            p->h_lmin.resize((size_t)p->L * ntile128);
            HIP_TRY(hipMemcpyAsync(p->h_lmin.data(), p->d_lmin, sizeof(int32_t) * p->h_lmin.size(), hipMemcpyDeviceToHost, ctx->stream));
            HIP_TRY(hipStreamSynchronize(ctx->stream));
        }
        const int trings = LEG_RINGS * rt;
        const int ntile = (p->npair + trings - 1) / trings;
        ARG_CHECK(p->lmax < (1 << 15) && ntile <= 256 && ncg <= 256);
        std::vector<int2> list;
        list.reserve((size_t)p->L * ncg * ntile);
        for (int m = 0; m <= p->lmax; m++)
            for (int cg = 0; cg < ncg; cg++)
                for (int t = 0; t < ntile; t++) {
                    int lmin = p->lmax + 1;
                    const int t_first = (t * trings) / LMIN_RINGS;
                    const int t_last = std::min((t * trings + trings - 1) / LMIN_RINGS, ntile128 - 1);
                    for (int t128 = t_first; t128 <= t_last; t128++) lmin = std::min(lmin, p->h_lmin[(size_t)m * ntile128 + t128]);
                    if (lmin <= p->lmax) list.push_back(make_int2(m | (t << 15) | (cg << 23), lmin));
                }
        dev_buf<int2> d;
        HIP_TRY(d.upload(list, ctx->stream));
        it = p->k4_items.emplace(key, std::make_pair(std::move(d), (int)list.size())).first;
    }
    *items = it->second.first;
    *nitems = it->second.second;
    return 0;
}

int sht_k4_segseed(corahip_ctx *ctx, const corahip_sht_plan *cp, int rt, const double2 **segseed) {
    corahip_sht_plan *p = const_cast<corahip_sht_plan *>(cp);      // (lazy caches of the plan)
    auto it = p->k4_segseed.find(rt);
    if (it == p->k4_segseed.end()) {
        dev_buf<double2> d;
        HIP_TRY(d.alloc(4 * (size_t)p->L * p->npair));
        dim3 grid((p->npair + 63) / 64, p->L);
        segseed_kernel<<<grid, 64, 0, ctx->stream>>>(p->lmax, p->npair, rt, p->d_z, p->d_coefmu, p->d_lstart, p->d_seed4,
                                                     p->d_lmin, d);
        LAUNCH_CHECK();
        it = p->k4_segseed.emplace(rt, std::move(d)).first;
    }
    *segseed = it->second;
    return 0;
}

// the Bluestein length of the run-time kernels for a cap ring of half length h: the power of two that holds 2 h - 1
static int blu_pow2_length(int h) {
    int P = 1;
    while (P < 2 * h - 1) P <<= 1;
    return P;
}

extern "C" {

int corahip_sht_plan_destroy(corahip_ctx *ctx, corahip_sht_plan *p) {
    delete p;   // every device table is a dev_buf member
    return 0;
}

int corahip_sht_plan_create(corahip_ctx *ctx, int nside, int lmax, corahip_sht_plan **out) {
    return corahip_sht_plan_create_ex(ctx, nside, lmax, 0, out);
}

int corahip_sht_plan_cut_exp(const corahip_sht_plan *p, int *cut_exp) {
    ARG_CHECK(p != nullptr && cut_exp != nullptr);
    *cut_exp = p->cut_exp;
    return 0;
}

int corahip_sht_plan_k4_mfma_count(corahip_ctx *ctx, const corahip_sht_plan *p, int nnu, uint64_t *mfma_instructions) {
    ARG_CHECK(ctx != nullptr && p != nullptr && mfma_instructions != nullptr && nnu >= 1);
    // the launch shape sht_legendre picks for this many channels (16-column tiles: 8 channels x re/im)
    const int ncols = 2 * nnu_pad_of(nnu);
    const int nt16 = ncols / 16;
    const int NT = nt16 % 8 == 0 ? 8 : (nt16 % 4 == 0 ? 4 : (nt16 % 2 == 0 ? 2 : 1));
    const int RT = NT == 8 ? 1 : 2;
    auto it = p->k4_macro_steps.find(RT);
    if (it == p->k4_macro_steps.end()) {
        HIP_TRY(hipSetDevice(ctx->device));
        unsigned long long h_n = 0;
        dev_buf<unsigned long long> d_n;
        HIP_TRY(d_n.alloc(1));
        HIP_TRY(hipMemsetAsync(d_n, 0, sizeof(h_n), ctx->stream));
        const int ntile = (p->npair + LEG_RINGS * RT - 1) / (LEG_RINGS * RT);
        const long total = (long)p->L * ntile * LEG_WAVES;
        k4_count_kernel<<<(unsigned)((total + 255) / 256), 256, 0, ctx->stream>>>(p->lmax, p->npair, RT, p->d_lstart, p->d_lmin, d_n, nullptr);
        LAUNCH_CHECK();
        HIP_TRY(hipMemcpyAsync(&h_n, d_n, sizeof(h_n), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        it = const_cast<corahip_sht_plan *>(p)->k4_macro_steps.emplace(RT, (uint64_t)h_n).first;
    }
    *mfma_instructions = it->second * (uint64_t)(2 * NT * RT) * (uint64_t)(ncols / (16 * NT));
    return 0;
}

int corahip_sht_plan_create_ex(corahip_ctx *ctx, int nside, int lmax, int cut_exp, corahip_sht_plan **out) {
    ARG_CHECK(ctx != nullptr && out != nullptr);
    ARG_CHECK(nside >= 1 && is_pow2(nside) && nside <= 8192);
    ARG_CHECK(lmax >= 0 && lmax <= 16384);
    ARG_CHECK(cut_exp <= 0 && cut_exp >= -1000);
    if (cut_exp == 0) cut_exp = SEED_MIN_EXP;
    HIP_TRY(hipSetDevice(ctx->device));
    // every early return below (HIP_TRY / rc checks) releases what was allocated so far
    std::unique_ptr<corahip_sht_plan> guard(new corahip_sht_plan());
    corahip_sht_plan *p = guard.get();
    p->nside = nside;
    p->lmax = lmax;
    p->cut_exp = cut_exp;
    p->L = lmax + 1;
    p->npair = 2 * nside;
    p->nring = 4 * nside - 1;
    p->npix = 12L * nside * nside;
    p->nalm = nalm_of(lmax);
    const int nring = p->nring;
    p->h_start.resize(nring);
    p->h_nphi.resize(nring);
    p->h_z.resize(nring);
    p->h_sth.resize(nring);
    p->h_phi0.resize(nring);
    // HEALPix RING geometry (pix2ang_ring conventions)
    const double fact2 = 4.0 / (double)p->npix;       // 1/(3 nside^2)
    const double fact1 = 2.0 * nside * fact2;         // 2/(3 nside)
    for (int r = 0; r < nring; r++) {
        const int i = r + 1;
        if (i < nside) {
            const double tmp = (double)i * i * fact2;
            p->h_z[r] = 1.0 - tmp;
            p->h_sth[r] = sqrt(tmp * (2.0 - tmp));
            p->h_nphi[r] = 4 * i;
            p->h_phi0[r] = M_PI / (4.0 * i);
            p->h_start[r] = 2L * i * (i - 1);
        } else if (i <= 3 * nside) {
            const double zz = (2 * nside - i) * fact1;
            p->h_z[r] = zz;
            p->h_sth[r] = sqrt((1.0 - zz) * (1.0 + zz));
            p->h_nphi[r] = 4 * nside;
            p->h_phi0[r] = (((i - nside) & 1) == 0) ? M_PI / (4.0 * nside) : 0.0;
            p->h_start[r] = 2L * nside * (nside - 1) + (long)(i - nside) * 4 * nside;
        } else {
            const int ip = 4 * nside - i;
            const double tmp = (double)ip * ip * fact2;
            p->h_z[r] = -(1.0 - tmp);
            p->h_sth[r] = sqrt(tmp * (2.0 - tmp));
            p->h_nphi[r] = 4 * ip;
            p->h_phi0[r] = M_PI / (4.0 * ip);
            p->h_start[r] = p->npix - 2L * ip * (ip + 1);
        }
    }
    hipStream_t s = ctx->stream;
    int rc;
    {
        std::vector<double> zz(p->h_z.begin(), p->h_z.begin() + p->npair);
        std::vector<double> ss(p->h_sth.begin(), p->h_sth.begin() + p->npair);
        HIP_TRY(p->d_z.upload(zz, s));
        HIP_TRY(p->d_sth.upload(ss, s));
    }
    HIP_TRY(p->d_nphi.upload(p->h_nphi, s));
    HIP_TRY(p->d_start.upload(p->h_start, s));
    HIP_TRY(p->d_phi0.upload(p->h_phi0, s));

    // recurrence coefficients: lambda_l = A_l x lambda_{l-1} - B_l lambda_{l-2},
    // A_l = alpha_lm, B_l = alpha_lm/alpha_{l-1,m}, alpha_lm = sqrt((4l^2-1)/(l^2-m^2))
    {
        std::vector<double2> coef(p->nalm + 32, make_double2(0.0, 0.0));  // +32: K4 prefetches past the end
        for (int m = 0; m <= lmax; m++) {
            long double aprev = 0.0L;
            for (int l = m; l <= lmax; l++) {
                const long o = alm_idx(l, m, lmax);
                if (l == m) {
                    coef[o] = make_double2(0.0, 0.0);
                    continue;
                }
                const long double ll = l, mm = m;
                const long double al = sqrtl((4.0L * ll * ll - 1.0L) / (ll * ll - mm * mm));
                coef[o] = make_double2((double)al, l == m + 1 ? 0.0 : (double)(al / aprev));
                aprev = al;
            }
        }
        HIP_TRY(p->d_coef.upload(coef, s));
        // scaled form: s_m = s_{m+1} = 1, s_l = B_l s_{l-2}; alpha_l = A_l s_{l-1} / s_l (alpha_m = 0: never used, the
        // recurrence starts from the seed at l >= m).  s_l stays within [~0.15, 1] (it tends to sqrt(A_inf / A_{m+1})).
        std::vector<double2> cmu(p->nalm + 32, make_double2(0.0, 0.0));
        for (int m = 0; m <= lmax; m++) {
            long double aprev = 0.0L, s1 = 1.0L, s2 = 1.0L;    // A_{l-1}, s_{l-1}, s_{l-2}
            for (int l = m; l <= lmax; l++) {
                const long o = alm_idx(l, m, lmax);
                if (l == m) {
                    cmu[o] = make_double2(0.0, 1.0);
                    continue;
                }
                const long double ll = l, mm = m;
                const long double al = sqrtl((4.0L * ll * ll - 1.0L) / (ll * ll - mm * mm));
                const long double sl = l == m + 1 ? 1.0L : (al / aprev) * s2;
                cmu[o] = make_double2((double)(al * s1 / sl), (double)sl);
                aprev = al;
                s2 = s1;
                s1 = sl;
            }
        }
        HIP_TRY(p->d_coefmu.upload(cmu, s));
    }
    // |lambda_mm| prefactor sqrt((2m+1)!!/(4 pi (2m)!!))
    dev_buf<double> d_pref;
    {
        std::vector<double> pref(p->L);
        long double pr = 1.0L / sqrtl(4.0L * acosl(-1.0L));
        pref[0] = (double)pr;
        for (int m = 1; m <= lmax; m++) {
            pr *= sqrtl((2.0L * m + 1.0L) / (2.0L * m));
            pref[m] = (double)pr;
        }
        HIP_TRY(d_pref.upload(pref, s));
    }
    HIP_TRY(p->d_lstart.alloc((size_t)p->L * p->npair));
    HIP_TRY(p->d_seed.alloc((size_t)p->L * p->npair));
    HIP_TRY(p->d_seedmu.alloc((size_t)p->L * p->npair));
    HIP_TRY(p->d_seed4.alloc(4 * (size_t)p->L * p->npair));
    {
        dim3 grid((p->npair + 63) / 64, p->L);
        seed_kernel<<<grid, 64, 0, s>>>(lmax, p->npair, cut_exp, p->d_z, p->d_sth, d_pref, p->d_coef, p->d_coefmu, p->d_lstart,
                                        p->d_seed, p->d_seedmu, p->d_seed4);
        LAUNCH_CHECK();
    }
    {
        const int ntile = (p->npair + LMIN_RINGS - 1) / LMIN_RINGS;
        HIP_TRY(p->d_queue.alloc(1024 / sizeof(unsigned)));   // 8 queue heads, 128 bytes apart
        HIP_TRY(p->d_mcut.alloc((size_t)p->nring));
        mcut_kernel<<<(p->npair + 63) / 64, 64, 0, s>>>(lmax, p->npair, p->nring, p->d_lstart, p->d_mcut);
        LAUNCH_CHECK();
        HIP_TRY(p->d_lmin.alloc((size_t)p->L * ntile));
        lmin_kernel<<<p->L, 64 * ((ntile + 63) / 64), 0, s>>>(lmax, p->npair, ntile, p->d_lstart, p->d_lmin);
        LAUNCH_CHECK();
    }
    HIP_TRY(hipStreamSynchronize(s));
    (void)d_pref.reset();

    HIP_TRY(p->d_zeros.alloc(4096 / sizeof(double)));
    HIP_TRY(hipMemsetAsync(p->d_zeros, 0, 4096, s));
    // FFT twiddles and Bluestein tables
    p->pmax = std::max(4 * nside, 4);
    p->log_pmax = ilog2(p->pmax);
    {
        std::vector<double2> tw(p->pmax / 2);
        for (int k = 0; k < p->pmax / 2; k++) {
            const long double a = 2.0L * acosl(-1.0L) * k / p->pmax;
            tw[k] = make_double2((double)cosl(a), (double)sinl(a));
        }
        HIP_TRY(p->d_tw.upload(tw, s));
    }
    {
        std::vector<int32_t> bp(nside, 0);
        std::vector<int64_t> bo(nside, 0), fo(nside, 0);
        int64_t nb = 0, nf = 0;
        int maxlen = 2 * nside + 1;  // belt: h + 1
        for (int i = 1; i < nside; i++) {
            const int h = 2 * i;
            if (is_pow2(h)) continue;
            const int P = blu_pow2_length(h);
            bp[i - 1] = P;
            bo[i - 1] = nb;
            fo[i - 1] = nf;
            nb += h;
            nf += P;
            maxlen = std::max(maxlen, P);
        }
        p->max_fft_len = maxlen;
        HIP_TRY(p->d_blu_P.upload(bp, s));
        HIP_TRY(p->d_blu_boff.upload(bo, s));
        HIP_TRY(p->d_blu_foff.upload(fo, s));
        HIP_TRY(p->d_bchirp.alloc(std::max<int64_t>(1, nb)));
        HIP_TRY(p->d_bfilt.alloc(std::max<int64_t>(1, nf)));
        if (nside > 1) {
            const int tl_off = fpad_len(maxlen) + 1;
            const size_t shm = sizeof(double2) * (size_t)tl_off;
            HIP_TRY(hipFuncSetAttribute((const void *)bluestein_table_kernel,
                                        hipFuncAttributeMaxDynamicSharedMemorySize, (int)shm));
            bluestein_table_kernel<<<nside - 1, 256, shm, s>>>(p->d_blu_P, p->d_blu_boff, p->d_blu_foff,
                                                                p->d_bchirp, p->d_bfilt, p->d_tw, p->pmax, tl_off);
            LAUNCH_CHECK();
        }
    }
    HIP_TRY(p->d_foldph.alloc(512 * (size_t)nside));
    HIP_TRY(p->d_foldstep.alloc(2 * (size_t)nside));
    if (nside > 1) {
        fold_phase_kernel<<<nside - 1, 512, 0, s>>>(p->d_phi0, p->d_foldph, p->d_foldstep);
        LAUNCH_CHECK();
    }
    // the second filter set: the rings whose compile-time kernel runs a length with filters of its own
    {
        p->h_ctfilt_len.assign(nside, 0);
        std::vector<int64_t> fo(nside, 0);
        int64_t nf = 0;
        for (int i = 1; i < nside; i++) {
            const int h = 2 * i;
            if (is_pow2(h)) continue;
            const int own = fft_shapes::ring_own_length(h, blu_pow2_length(h));
            if (own) {
                p->h_ctfilt_len[i - 1] = own;
                fo[i - 1] = nf;
                nf += own;
            }
        }
        HIP_TRY(p->d_ctfilt_off.upload(fo, s));
        HIP_TRY(p->d_ctfilt.alloc(std::max<int64_t>(1, nf)));
        if (nf && (rc = sht_ctfilt_tables(ctx, p))) return rc;
    }
    // K5 ring classes
    {
        // One class per (kind, run-time length, own compile-time length).  The classes are launched in the order of this
        // key, alternating two streams, and cost ties of the scheduler fall back on it, so it is part of the behaviour:
        // the belt (direct transform of the one length 2 nside: its own class so that the compile-time kernel can take
        // it), the few power-of-two cap rings (one run-time class), then the Bluestein lengths P ascending; within one P
        // the rings without a length of their own, then 3/4 P, P itself in the compile-time order, 5/8 P, 7/8 P.
        static const int eighths_rank[9] = {0, 0, 0, 0, 0, 3, 1, 4, 2};
        std::map<std::array<int, 3>, std::vector<int32_t>> by_key;     // (P or -1 belt / 0 mixed, rank, own length)
        for (int r = 0; r < nring; r++) {
            const int i = r + 1;
            int icap = 0;
            if (i < nside) icap = i;
            else if (i > 3 * nside) icap = 4 * nside - i;
            std::array<int, 3> key = {icap ? 0 : -1, 0, 0};
            if (icap && !is_pow2(2 * icap)) {
                const int P = blu_pow2_length(2 * icap), own = p->h_ctfilt_len[icap - 1];
                key = {P, eighths_rank[own / (P / 8)], own};
            }
            by_key[key].push_back(r);
        }
        const size_t lds_budget = 160 * 1024;
        for (auto &kv : by_key) {
            corahip_sht_plan::ring_class c;
            const int own = kv.first[2];
            c.blu = kv.first[0] > 0;
            c.len = c.blu ? kv.first[0] : (kv.first[0] < 0 ? 2 * nside : 0);
            const fft_shapes::ring_shape *ct = c.blu ? fft_shapes::find(fft_shapes::RING_BLU, own ? own : c.len)
                                                     : fft_shapes::find(fft_shapes::RING_DIRECT, c.len);
            c.ct_len = ct ? ct->len : 0;
            c.ct_own = own != 0;
            c.bstride = fpad_len(c.blu ? c.len : 2 * nside + 1) + K5_CH_SKEW;
            c.nch = 4;
            while (c.nch > 1 && (size_t)c.nch * c.bstride * sizeof(double2) > lds_budget) c.nch >>= 1;
            if ((size_t)c.nch * c.bstride * sizeof(double2) > lds_budget) {
                corahip_set_error("nside %d: ring FFT of length %d does not fit in LDS", nside, c.bstride);
                return CORAHIP_ENOMEM;
            }
            // the scheduler costs and aligns a class by c.nch, the compile-time kernel runs its own NCH: one number
            if (ct && ct->nch != c.nch) {
                corahip_set_error("ring FFT length %d: %d channels per item in the shape table, %d by the LDS budget", ct->len,
                                  ct->nch, c.nch);
                return CORAHIP_ESTATE;
            }
            // (measured and rejected for the P = 4096 class: one channel per 4-wave workgroup, two workgroups per CU,
            //  so that LDS and FP64 phases of different workgroups overlap: 12.8 -> 13.6 ms, the cells are read 4x)
            // The short Bluestein classes (P <= 512: 0.5 % of the pixels at nside 1024, but six launches in a row) run
            // workgroups of 64 / 128 threads instead of 512: a 512-point transform of four channels has 128 radix-16
            // butterflies per pass - most of a 512-thread workgroup only attended the barriers (P = 512 0.41 -> 0.19 ms,
            // P = 256 0.19 -> 0.05 ms, K5 -0.5 ms at cfg 3).
            if (c.blu && c.len <= 512) c.threads = c.len >= 512 ? 128 : 64;
            c.count = (int)kv.second.size();
            c.h_list = kv.second;
            HIP_TRY(c.d_list.upload(kv.second, s));
            p->classes.push_back(std::move(c));
        }
    }
    HIP_TRY(hipStreamSynchronize(s));
    *out = guard.release();
    return 0;
}

int corahip_sht_plan_rings(const corahip_sht_plan *p, int64_t *host_start, int32_t *host_nphi, double *host_z,
                           double *host_phi0) {
    ARG_CHECK(p != nullptr);
    for (int r = 0; r < p->nring; r++) {
        if (host_start) host_start[r] = p->h_start[r];
        if (host_nphi) host_nphi[r] = p->h_nphi[r];
        if (host_z) host_z[r] = p->h_z[r];
        if (host_phi0) host_phi0[r] = p->h_phi0[r];
    }
    return 0;
}

int corahip_sht_plan_ring_classes(const corahip_sht_plan *p, int32_t *host_len) {
    ARG_CHECK(p != nullptr && host_len != nullptr);
    for (const auto &c : p->classes)
        for (int32_t r : c.h_list) host_len[r] = c.blu ? c.length() : 0;
    return 0;
}

int corahip_sht_lambda(corahip_ctx *ctx, const corahip_sht_plan *p, int m, int ring_pair, double *out) {
    ARG_CHECK(ctx != nullptr && p != nullptr && out != nullptr);
    ARG_CHECK(m >= 0 && m <= p->lmax && ring_pair >= 0 && ring_pair < p->npair);
    lambda_kernel<<<1, 64, 0, ctx->stream>>>(p->lmax, p->npair, m, ring_pair, p->d_z, p->d_coefmu, p->d_lstart,
                                             p->d_seedmu, out);
    LAUNCH_CHECK();
    return 0;
}

int corahip_sht_lambda_entry(corahip_ctx *ctx, const corahip_sht_plan *p, int m, int ring_pair, int kq, double *out) {
    ARG_CHECK(ctx != nullptr && p != nullptr && out != nullptr);
    ARG_CHECK(m >= 0 && m <= p->lmax && ring_pair >= 0 && ring_pair < p->npair && kq >= 0 && kq < 4);
    lambda_entry_kernel<<<1, 64, 0, ctx->stream>>>(p->lmax, p->npair, m, ring_pair, kq, p->d_z, p->d_coefmu, p->d_lstart,
                                                   p->d_seed4, out);
    LAUNCH_CHECK();
    return 0;
}

int corahip_sht_lambda_segment_entry(corahip_ctx *ctx, const corahip_sht_plan *p, int rt, int m, int ring_pair, int kq,
                                     double *out, int32_t *info) {
    ARG_CHECK(ctx != nullptr && p != nullptr && out != nullptr && info != nullptr);
    ARG_CHECK((rt == 1 || rt == 2) && m >= 0 && m <= p->lmax && ring_pair >= 0 && ring_pair < p->npair && kq >= 0 && kq < 4);
    const double2 *d_segseed = nullptr;
    int rc = sht_k4_segseed(ctx, p, rt, &d_segseed);
    if (rc) return rc;
    lambda_segment_kernel<<<1, 64, 0, ctx->stream>>>(p->lmax, p->npair, rt, m, ring_pair, kq, p->d_z, p->d_coefmu, p->d_lstart,
                                                     d_segseed, p->d_lmin, out, info);
    LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
