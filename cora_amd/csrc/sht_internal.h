// sht_internal.h - shared by the translation units of the HEALPix transforms (sht_*.hip):
//   sht_plan.hip      geometry / recurrence / seed / Bluestein tables of a (nside, lmax) plan
//   sht_legendre.hip  K4: Legendre contraction on FP64 MFMA (scalar and spin-2 forms)
//   sht_ringfft.hip   K5 and K5^T: per-ring phase / fold / FFT (synthesis) and FFT / split (analysis)
//   sht_analysis.hip  K4^T: adjoint Legendre contraction + reduction over ring tiles
//   sht_polana_native.hip  K4^T for spin 2: (Q, U) ring spectra -> (E, B) in one Legendre pass + its tile reduction
//   sht_api.hip       C ABI entry points (alm2map, map2alm, alm2map_spin2, map2alm_spin2, workspace sizes)
//
// Replaces hputil.sphtrans_inv_sky -> healpy.alm2map (cora/util/hputil.py:369-391,500-531) and, for the
// "next" rows, healpy.map2alm and the polarised synthesis.  Definition implemented: SURVEY.md Appendix A
// (HEALPix software conventions).
//
// Synthesis = two kernels per pass over a chunk of channels:
//   K4 legendre_kernel : F_m(ring) = sum_l a_lm lambda_lm(cos theta_ring) for every ring pair,
//        as FP64 MFMA (v_mfma_f64_16x16x4_f64): A = lambda (rows = rings, generated in
//        registers by the three-term recurrence), B = a_lm (LDS-staged rows of the
//        [nalm][cols] device layout), even/odd (l-m) accumulated separately so the
//        north ring gets e+o and its southern mirror e-o.
//   K5 ringfft_kernel  : per ring and channel: phase e^{i m phi0}, alias fold onto nphi
//        bins, complex-to-real FFT of length nphi (radix-16/8/4/2 in LDS; Bluestein for the
//        cap rings whose length 4i is not a power of two), pixel store.
// Intermediate F_m layout: inter[ring][g][m][c*4+v] (g = channel/4, v = channel%4,
// c = re/im): 64-byte cells, contiguous in m for K5, 64-byte segments for K4's stores.
#pragma once
#include "common.h"

#include <algorithm>
#include <cmath>
#include <type_traits>
#include <cstdlib>
#include <map>

// ------------------------------------------------------------------------------------
struct corahip_sht_plan {
    int nside = 0, lmax = 0, L = 0, npair = 0, nring = 0;
    int cut_exp = 0;                                      // terms of the Legendre sums with |lambda_lm| < 2^cut_exp are dropped
    std::map<int, uint64_t> k4_macro_steps;               // by RT: macro-steps legendre_kernel executes per column group (lazy)
    std::map<std::pair<int, int>, std::pair<dev_buf<int2>, int>> k4_items;   // by (RT, column groups): legendre_kernel's list of non-empty items (lazy, sht_k4_items)
    std::vector<int32_t> h_lmin;                          // host copy of d_lmin (lazy)
    long npix = 0, nalm = 0;
    std::vector<int64_t> h_start;
    std::vector<int32_t> h_nphi;
    std::vector<double> h_z, h_sth, h_phi0;
    // device
    dev_buf<double> d_z, d_sth;                           // [npair] (north rings + equator)
    dev_buf<int32_t> d_nphi;                              // [nring]
    dev_buf<int64_t> d_start;                             // [nring]
    dev_buf<double> d_phi0;                               // [nring]
    dev_buf<double2> d_coef;                              // [nalm]: (A_l, B_l) at alm_idx(l,m)
    dev_buf<int32_t> d_lstart;                            // [L][npair]
    dev_buf<double2> d_seed;                              // [L][npair]: (lambda_{lstart-1}, lambda_{lstart})
    // the scalar synthesis kernel runs the recurrence in its two-instruction form mu_l = (alpha_l x) mu_{l-1} - mu_{l-2},
    // lambda_l = s_l mu_l (s_m = s_{m+1} = 1, s_l = B_l s_{l-2}, alpha_l = A_l s_{l-1} / s_l): its own coefficient and
    // seed tables (the spin-2 and the analysis kernels keep the (A, B) form)
    dev_buf<double2> d_coefmu;                            // [nalm]: (alpha_l, s_l) at alm_idx(l,m)
    dev_buf<double2> d_seedmu;                            // [L][npair]: (mu_{lstart-1}, mu_{lstart})
    dev_buf<double2> d_seed4;                             // [L][npair][4]: (mu_{R-2}, mu_{R-1}) in front of lane group kq's entry row R (seed_kernel)
    std::map<int, dev_buf<double2>> k4_segseed;           // by RT: [L][npair][4] (mu_{R-2}, mu_{R-1}) in front of the entry row of legendre_kernel's lane group kq (lazy, sht_k4_segseed)
    dev_buf<int32_t> d_lmin;                              // [L][ntile] first l per (m, ring tile)
    dev_buf<unsigned> d_queue;                            // K4 work-queue head
    dev_buf<int32_t> d_mcut;                              // [nring] number of m with any non-negligible lambda_lm
    dev_buf<double> d_polc;                               // [nalm + 64][4] spin-2 coefficients (g1..g4), built on first use
    dev_buf<double> d_zeros;                              // 4 KiB of zeros (source of padding rows for LDS-DMA)
    dev_buf<double2> d_tw;                                // e^{+2 pi i k/pmax}, k < pmax/2
    int pmax = 0, log_pmax = 0;
    // Bluestein tables, indexed by north-cap ring number i-1 (i = 1..nside-1)
    dev_buf<int32_t> d_blu_P;                             // [nside]: 0 = power-of-two ring
    dev_buf<int64_t> d_blu_boff, d_blu_foff;              // offsets into chirp / filter arrays
    dev_buf<double2> d_bchirp, d_bfilt;
    // second set of Bluestein filters, stored in the order of the compile-time passes: for the rings whose compile-time
    // kernel (synthesis or analysis) runs a length with filters of its own (fft_shapes.h, RING_BLU rows marked `own`: a
    // 3 / 5 / 7 * 2^k length that still holds 2 h - 1, or 8192, whose pass order differs from the generic one).  The
    // run-time kernels, and the compile-time kernels of the other lengths, keep blu_P and the first set.
    std::vector<int32_t> h_ctfilt_len;                    // [nside]: 0 = none
    dev_buf<int64_t> d_ctfilt_off;
    dev_buf<double2> d_ctfilt;
    // fold phases of the cap rings for the compile-time Bluestein kernels: e^{i t phi0(ring)}, t < 512, and the steps
    // e^{i 256 phi0}, e^{i 512 phi0}, by north-cap ring number i - 1
    dev_buf<double2> d_foldph, d_foldstep;
    int max_fft_len = 0;                                  // largest LDS FFT buffer (complex elems)
    // K5 launch classes: rings grouped by transform kind/length so each launch sizes its LDS
    struct ring_class {
        bool blu = false; // Bluestein (cap rings whose length is no power of two); false = direct power-of-two transform
        int len = 0;      // what the run-time kernel runs: Bluestein length P (a power of two, filters in d_bfilt) / direct:
                          // the half length h of the rings if they share one (the belt), 0 = mixed (power-of-two cap rings)
        int ct_len = 0;   // length of the compile-time kernel that takes the class (fft_shapes.h), 0 = none
        bool ct_own = false;   // that kernel reads the second filter set (d_ctfilt); then ct_len may differ from len
        int length() const { return ct_len ? ct_len : len; }   // of the transform the synthesis runs
        int nch = 4;      // channels transformed together per workgroup (the compile-time kernel's NCH where there is one)
        int threads = 0;  // workgroup size (0: K5_THREADS)
        int bstride = 0;  // complex elements per channel buffer in LDS
        int count = 0;
        dev_buf<int32_t> d_list;
        std::vector<int32_t> h_list;   // host copy of the ring list (corahip_sht_plan_ring_classes)
    };
    std::vector<ring_class> classes;
};

static inline int ilog2(int v) {
    int l = 0;
    while ((1 << l) < v) l++;
    return l;
}
static inline bool is_pow2(int v) { return v > 0 && (v & (v - 1)) == 0; }
// ------------------------------------------------------------------------------------
// K4: Legendre contraction on FP64 MFMA
// ------------------------------------------------------------------------------------
#ifndef LEG_KT
#define LEG_KT 56     // rows of l per LDS stage (re-tuned after the instruction-count pass: 48 x 3 68.5, 56 x 2 67.7, 48 x 2 68.9, 40 x 3 72.1, 32 x 4 69.8 ms)
#endif
#ifndef LEG_WAVES
#define LEG_WAVES 8
#endif
#define LEG_RINGS (16 * LEG_WAVES)  // ring pairs per workgroup (x RT)
#define LEG_RPM (8 / LEG_WAVES)     // a_lm pieces each wave issues per macro-step (= RPW / (LEG_KT / 8))
#define LMIN_RINGS 128              // granularity of the plan's per-(m, ring block) first-l table
#define ADJ_WAVES 8                 // waves per workgroup of the analysis kernel
#ifndef LEG_NBUF
#define LEG_NBUF 2     // LDS stage ring: one being read + one in flight
#endif

// Item geometry of legendre_kernel, for the kernel and the plan (segment seeds, item count): an item (m, ring tile)
// whose first contributing l is lmin walks T macro-steps from l_begin, as it always did, but lane group kq owns the
// CONTIGUOUS rows [R(kq), R(kq) + Q) - a quarter of the item's 8 T rows - and walks two of them per macro-step: at
// macro-step t it feeds row R(kq) + 2 t (l - m even) and the row behind it (odd).  Q is even, so the pairs are the
// pairs (m + 2 j, m + 2 j + 1) of the staggered scheme; rows past lmax (segment 3's overhang; for T < 4 the others'
// too) carry s = 0.  A ring whose first contributing l is ls is summed from the first pair whose even row is
// >= ls - 1 on: lane group kq enters at macro-step entry(kq, ls).
#define LEG_MSPS (LEG_KT / 8)       // macro-steps per LDS stage
#define LEG_NEVER 0x7fffffff
struct leg_seg {
    int l_begin, T;
    __host__ __device__ static inline leg_seg of(int m, int lmin, int lmax) {
        leg_seg g;
        g.l_begin = m + ((lmin - m) & ~7);
        g.T = (lmax - g.l_begin) / 8 + 1;
        return g;
    }
    __host__ __device__ inline int Q() const { return 2 * T; }
    __host__ __device__ inline int R(int kq) const { return l_begin + kq * 2 * T; }
    __host__ __device__ inline int nstage() const { return (T + LEG_MSPS - 1) / LEG_MSPS; }
    // macro-step at which lane group kq starts to feed a ring with first contributing l `ls` (0: from the segment's
    // first row, with the state the plan walked up to it), LEG_NEVER if the segment ends in front of row ls - 1
    __host__ __device__ inline int entry(int kq, int ls, int lmax) const {
        if (ls > lmax) return LEG_NEVER;
        const int need = ls - 1 - R(kq);
        if (need <= 0) return 0;
        const int e = (need + 1) >> 1;
        return e < T ? e : LEG_NEVER;
    }
};

// LDS stage ring of the two K4 kernels, for the kernel and its launcher: NT 16-column tiles, KT rows of l per stage,
// NBUF stages, XROWS doubles per coefficient row beyond the recurrence pair (0 scalar, 4 spin 2: its g table)
template <int NT, int KT, int NBUF, int XROWS>
struct leg_geom {
    static constexpr int TCOLS = 16 * NT;          // columns of a block
    static constexpr int STRIDE = TCOLS + 8;       // LDS row stride (doubles): 2 rows apart = 128 B mod 256
    static constexpr int CROWS = KT + 8;           // coefficient rows per stage (staggered lanes look 6 ahead)
    static constexpr int STAGE = KT * STRIDE + (2 + XROWS) * CROWS;   // doubles per stage: a_lm rows + coefficient rows
    static constexpr size_t LDS_BYTES = sizeof(double) * NBUF * STAGE + 16;   // dynamic LDS: the ring + the next-item slots behind it
};

// min / max over the wave, wave-uniform (an SGPR): tests on it are scalar compares
__device__ static inline int wave_min(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o));
    return __builtin_amdgcn_readfirstlane(v);
}
__device__ static inline int wave_max(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o));
    return __builtin_amdgcn_readfirstlane(v);
}

// LDS-DMA issued from inline asm: hipcc does not count it, so it does not drain the DMA with a
// vmcnt(0) in front of every later ds_read (which it does for the builtin: the DMA is a pending LDS
// write it cannot disambiguate).  The kernel waits itself: s_waitcnt vmcnt(0) before the stage barrier.
// lds_byte_addr must be wave-uniform; lane i's 16 bytes land at lds_byte_addr + 16 i.
__device__ static inline void glds16(const void *gsrc, unsigned lds_byte_addr) {
    unsigned keep;
    const unsigned dst = __builtin_amdgcn_readfirstlane(lds_byte_addr);
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep)
                 : "v"(gsrc), "s"(dst)
                 : "memory");
}
// same, with the source as a wave-uniform base (SGPR pair) + a 32-bit per-lane byte offset: the row address of an
// a_lm piece is then pure scalar arithmetic (every instruction of K4's macro-step costs issue time)
__device__ static inline void glds16_s(const void *sbase, unsigned lane_byte_off, unsigned lds_byte_addr) {
    unsigned keep;
    const unsigned dst = __builtin_amdgcn_readfirstlane(lds_byte_addr);
    // (dropping the save / restore of M0 was measured: no gain)
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep)
                 : "v"(lane_byte_off), "s"(sbase), "s"(dst)
                 : "memory");
}
// ------------------------------------------------------------------------------------
// K5: per-ring phase / fold / FFT
// ------------------------------------------------------------------------------------
__device__ static inline double2 cmul(double2 a, double2 b) {
    return make_double2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x);
}
__device__ static inline double2 cadd(double2 a, double2 b) { return make_double2(a.x + b.x, a.y + b.y); }
__device__ static inline double2 csub(double2 a, double2 b) { return make_double2(a.x - b.x, a.y - b.y); }
// multiply by SIGN * i
template <int SIGN>
__device__ static inline double2 cmuli(double2 a) {
    return SIGN > 0 ? make_double2(-a.y, a.x) : make_double2(a.y, -a.x);
}

// small DFTs in registers, kernel e^{SIGN 2 pi i r p / R}, natural order in and out
template <int SIGN>
__device__ static inline void dft2(double2 &a, double2 &b) {
    const double2 t = a;
    a = cadd(t, b);
    b = csub(t, b);
}
template <int SIGN>
__device__ static inline void dft4(double2 &x0, double2 &x1, double2 &x2, double2 &x3) {
    const double2 s02 = cadd(x0, x2), d02 = csub(x0, x2);
    const double2 s13 = cadd(x1, x3), d13 = cmuli<SIGN>(csub(x1, x3));
    x0 = cadd(s02, s13);
    x2 = csub(s02, s13);
    x1 = cadd(d02, d13);
    x3 = csub(d02, d13);
}
template <int R, int SIGN>
struct DftR;
template <int SIGN>
struct DftR<2, SIGN> {
    __device__ __forceinline__ static void run(double2 (&x)[2]) { dft2<SIGN>(x[0], x[1]); }
};
template <int SIGN>
struct DftR<4, SIGN> {
    __device__ __forceinline__ static void run(double2 (&x)[4]) { dft4<SIGN>(x[0], x[1], x[2], x[3]); }
};
template <int SIGN>
struct DftR<8, SIGN> {
    __device__ __forceinline__ static void run(double2 (&x)[8]) {
        // even / odd halves, then radix-2 combine with eighth roots
        dft4<SIGN>(x[0], x[2], x[4], x[6]);
        dft4<SIGN>(x[1], x[3], x[5], x[7]);
        const double h = 0.70710678118654752440;
        const double2 w1 = make_double2(h, SIGN * h), w3 = make_double2(-h, SIGN * h);
        const double2 o0 = x[1], o1 = cmul(x[3], w1), o2 = cmuli<SIGN>(x[5]), o3 = cmul(x[7], w3);
        const double2 e0 = x[0], e1 = x[2], e2 = x[4], e3 = x[6];
        x[0] = cadd(e0, o0);
        x[4] = csub(e0, o0);
        x[1] = cadd(e1, o1);
        x[5] = csub(e1, o1);
        x[2] = cadd(e2, o2);
        x[6] = csub(e2, o2);
        x[3] = cadd(e3, o3);
        x[7] = csub(e3, o3);
    }
};
template <int SIGN>
struct DftR<16, SIGN> {
    __device__ __forceinline__ static void run(double2 (&x)[16]) {
        // n = 4a + c, k = k1 + 4 k2: DFT4 over a, twiddle w16^{c k1}, DFT4 over c
        const double c1 = 0.92387953251128675613, s1 = 0.38268343236508977173;  // cos, sin(pi/8)
        const double h = 0.70710678118654752440;
#pragma unroll
        for (int c = 0; c < 4; c++) dft4<SIGN>(x[c], x[4 + c], x[8 + c], x[12 + c]);
        // after this x[4 k1 + c] holds t_c[k1]
        // twiddles w16^{c k1}, c,k1 in 1..3: exponents 1,2,3,2,4,6,3,6,9
        const double2 w1 = make_double2(c1, SIGN * s1), w2 = make_double2(h, SIGN * h), w3 = make_double2(s1, SIGN * c1);
        const double2 w6 = make_double2(-h, SIGN * h), w9 = make_double2(-c1, -SIGN * s1);
        x[4 + 1] = cmul(x[4 + 1], w1);
        x[4 + 2] = cmul(x[4 + 2], w2);
        x[4 + 3] = cmul(x[4 + 3], w3);
        x[8 + 1] = cmul(x[8 + 1], w2);
        x[8 + 2] = cmuli<SIGN>(x[8 + 2]);
        x[8 + 3] = cmul(x[8 + 3], w6);
        x[12 + 1] = cmul(x[12 + 1], w3);
        x[12 + 2] = cmul(x[12 + 2], w6);
        x[12 + 3] = cmul(x[12 + 3], w9);
#pragma unroll
        for (int k1 = 0; k1 < 4; k1++) dft4<SIGN>(x[4 * k1], x[4 * k1 + 1], x[4 * k1 + 2], x[4 * k1 + 3]);
        // now x[4 k1 + k2] = X[k1 + 4 k2]: transpose to natural order
#pragma unroll
        for (int k1 = 0; k1 < 4; k1++)
#pragma unroll
            for (int k2 = k1 + 1; k2 < 4; k2++) {
                const double2 t = x[4 * k1 + k2];
                x[4 * k1 + k2] = x[4 * k2 + k1];
                x[4 * k2 + k1] = t;
            }
    }
};

// LDS layout of an FFT buffer: logical element i lives at fpad(i); fpad_len(n) slots hold n elements.
// One spare slot per 8 elements plus 8 per 128.  A simulation of ds_read_b128 /
// ds_write_b128 with their real lane groups (MI355X_MICROARCH.md LDS table: reads are served in 4 groups of 16
// NON-contiguous lanes, writes in 8 x 8) gives this padding 1.5x the conflict-free LDS cycles on every
// radix-16/8/4/2 pass of N = 1024 ... 4096 - the 0.31 = SQ_LDS_BANK_CONFLICT / SQ_LDS_IDX_ACTIVE measured for all
// three instantiations (profiles/r01_k5_lds_pmc.csv): a padded unit-stride run is no longer aligned to the bank
// rows the lane groups assume.  (A conflict-free XOR swizzle was measured 0.7 ms SLOWER, 26.9 -> 27.6 ms: the ring FFT
// is bound by its FP64 VALU work, not by the LDS array - HISTORY.md; the flat-sky line FFT (flatsky.hip), whose
// radix-4 stages ARE LDS-bound, ships its own swizzle.)
__host__ __device__ static inline int fpad(int i) { return i + (i >> 3) + ((i >> 7) << 3); }
__host__ __device__ static inline int fpad_len(int n) { return fpad(n); }
#define K5_CH_SKEW 1                   // channel buffers start one slot apart

// e^{+2 pi i idx/pmax} from the half-circle table in HBM, tw[k] = e^{+2 pi i k/pmax}, k < pmax/2
__device__ static inline double2 tw_global(const double2 *__restrict__ tw, int pmax, int idx) {
    const int hp = pmax >> 1;
    double2 w = tw[idx >= hp ? idx - hp : idx];
    if (idx >= hp) w = make_double2(-w.x, -w.y);
    return w;
}
// (A two-level LDS table of the twiddles was measured slower, belt class 13.2 -> 15.8 ms: HISTORY.md.)
template <int SIGN>
__device__ static inline double2 tw_get(const double2 *tw, int pmax, int idx) {
    double2 w = tw_global(tw, pmax, idx);
    if (SIGN < 0) w.y = -w.y;
    return w;
}

// One radix-R pass over `nch` channel buffers (channel c at buf + c*bstride), transform
// length N, current sub-length Ls.  DIT = false: decimation in frequency (DFT then twiddle),
// true: its transpose (twiddle then DFT).  Ends with a workgroup barrier.
template <int R, int SIGN, bool DIT>
__device__ __forceinline__ static void fft_pass(double2 *buf, int bstride, int nch, int N, int Ls, const double2 *__restrict__ tw,
                                int pmax, const double2 *__restrict__ postmul = nullptr) {
    const int q = Ls / R;
    const int nb = N / R;
    const int total = nch * nb;
    const int twstep = pmax / Ls;
    for (int idx = threadIdx.x; idx < total; idx += blockDim.x) {
        const int ch = idx / nb, t = idx - ch * nb;
        const int b = t / q, j = t - b * q;
        double2 *cbuf = buf + (size_t)ch * bstride;
        const int i0 = b * Ls + j;
        double2 x[R];
#pragma unroll
        for (int r = 0; r < R; r++) x[r] = cbuf[fpad(i0 + r * q)];
        // twiddles w_Ls^{SIGN j r}: only the binary powers w, w^2, w^4, w^8 are kept in registers and
        // x[r] is multiplied by the ones its index selects (16 VGPRs instead of a 64-VGPR power table)
        constexpr int NB = R == 16 ? 4 : (R == 8 ? 3 : (R == 4 ? 2 : 1));
        double2 wp[NB];
        wp[0] = tw_get<SIGN>(tw, pmax, j * twstep);
#pragma unroll
        for (int b = 1; b < NB; b++) wp[b] = cmul(wp[b - 1], wp[b - 1]);
        auto twiddle_all = [&]() {
#pragma unroll
            for (int r = 1; r < R; r++) {
#pragma unroll
                for (int b = 0; b < NB; b++)
                    if (r & (1 << b)) x[r] = cmul(x[r], wp[b]);
            }
        };
        if (DIT) twiddle_all();
        DftR<R, SIGN>::run(x);
        if (!DIT) twiddle_all();
        if (postmul) {  // pointwise factor indexed by storage position (Bluestein filter, digit-reversed order)
#pragma unroll
            for (int r = 0; r < R; r++) x[r] = cmul(x[r], postmul[i0 + r * q]);
        }
#pragma unroll
        for (int r = 0; r < R; r++) cbuf[fpad(i0 + r * q)] = x[r];
    }
    __syncthreads();
}

#define K5_RADIX 16    // largest butterfly (radix 8 with 1024-thread workgroups: measured 30 % slower, spills)
#define K5_LOGR 4
#define K5_THREADS 512
// pass schedule for N = 2^k: radix K5_RADIX while it fits, then the remainder
// `postmul` (optional) is multiplied into the output of the LAST pass, indexed by storage position
template <int SIGN>
__device__ __forceinline__ static void fft_dif(double2 *buf, int bstride, int nch, int N, const double2 *__restrict__ tw, int pmax,
                                               const double2 *__restrict__ postmul = nullptr) {
    int Ls = N;
    while (Ls >= K5_RADIX) {
        fft_pass<K5_RADIX, SIGN, false>(buf, bstride, nch, N, Ls, tw, pmax, Ls == K5_RADIX ? postmul : nullptr);
        Ls >>= K5_LOGR;
    }
    if (Ls == 8) fft_pass<8, SIGN, false>(buf, bstride, nch, N, Ls, tw, pmax, postmul);
    else if (Ls == 4) fft_pass<4, SIGN, false>(buf, bstride, nch, N, Ls, tw, pmax, postmul);
    else if (Ls == 2) fft_pass<2, SIGN, false>(buf, bstride, nch, N, Ls, tw, pmax, postmul);
}
// transpose of fft_dif: digit-reversed order in -> natural order out
template <int SIGN>
__device__ __forceinline__ static void fft_dit(double2 *buf, int bstride, int nch, int N, const double2 *__restrict__ tw, int pmax) {
    int rem = N;
    while (rem >= K5_RADIX) rem >>= K5_LOGR;  // remainder radix handled first (it was last in DIF)
    int Ls = rem;
    if (rem == 8) fft_pass<8, SIGN, true>(buf, bstride, nch, N, Ls, tw, pmax);
    else if (rem == 4) fft_pass<4, SIGN, true>(buf, bstride, nch, N, Ls, tw, pmax);
    else if (rem == 2) fft_pass<2, SIGN, true>(buf, bstride, nch, N, Ls, tw, pmax);
    if (rem == 1) Ls = 1;
    while (Ls < N) {
        Ls <<= K5_LOGR;
        fft_pass<K5_RADIX, SIGN, true>(buf, bstride, nch, N, Ls, tw, pmax);
    }
}
// position of frequency index k in the digit-reversed output of fft_dif
__device__ static inline int fft_dif_pos(int k, int N) {
    int pos = 0, len = N, Ls = N;
    while (Ls >= K5_RADIX) {
        len >>= K5_LOGR;
        pos += (k & (K5_RADIX - 1)) * len;
        k >>= K5_LOGR;
        Ls >>= K5_LOGR;
    }
    if (Ls > 1) {
        len /= Ls;
        pos += (k & (Ls - 1)) * len;
    }
    return pos;
}

// ---- Bluestein convolution with the middle and the end kept in registers ----------------------
// forward DIF: every pass but the last
template <int SIGN>
__device__ __forceinline__ static int fft_dif_head(double2 *buf, int bstride, int nch, int N, const double2 *__restrict__ tw, int pmax) {
    int Ls = N;
    while (Ls > K5_RADIX) {   // stop with the final sub-length (<= K5_RADIX) left
        fft_pass<K5_RADIX, SIGN, false>(buf, bstride, nch, N, Ls, tw, pmax);
        Ls >>= K5_LOGR;
    }
    return Ls;  // radix of the last forward pass == radix of the first inverse pass (stride 1)
}
// last forward pass (DFT_R, sign -), pointwise filter, first inverse pass (DFT_R, sign +): both act on the
// same R consecutive storage positions and their twiddles are 1, so the data never leaves the registers
template <int R>
__device__ __forceinline__ static void fft_mid_fused(double2 *buf, int bstride, int nch, int N,
                                                     const double2 *__restrict__ filt) {
    const int nb = N / R;
    const int total = nch * nb;
    for (int idx = threadIdx.x; idx < total; idx += blockDim.x) {
        const int ch = idx / nb, b = idx - ch * nb;
        double2 *cbuf = buf + (size_t)ch * bstride;
        const int i0 = b * R;
        double2 x[R];
#pragma unroll
        for (int r = 0; r < R; r++) x[r] = cbuf[fpad(i0 + r)];
        DftR<R, -1>::run(x);
#pragma unroll
        for (int r = 0; r < R; r++) x[r] = cmul(x[r], filt[i0 + r]);
        DftR<R, 1>::run(x);
#pragma unroll
        for (int r = 0; r < R; r++) cbuf[fpad(i0 + r)] = x[r];
    }
    __syncthreads();
}
// inverse DIT passes after the first one, except the last (Ls == N), which is fft_dit_last_out
template <int SIGN>
__device__ __forceinline__ static void fft_dit_middle(double2 *buf, int bstride, int nch, int N, int Ls_first,
                                                      const double2 *__restrict__ tw, int pmax) {
    int Ls = Ls_first;
    while ((Ls << K5_LOGR) < N) {
        Ls <<= K5_LOGR;
        fft_pass<K5_RADIX, SIGN, true>(buf, bstride, nch, N, Ls, tw, pmax);
    }
}
// last inverse pass (radix K5_RADIX, Ls = N): results are natural-order j = j0 + r N/R; multiply by the
// chirp b_j / P and store the pixel pair (2j, 2j+1) of every channel straight to HBM (consecutive lanes ->
// consecutive j: coalesced 16-byte stores), j < h only.
template <int SIGN>
__device__ __forceinline__ static void fft_dit_last_out(const double2 *buf, int bstride, int nch, int N,
                                                        const double2 *__restrict__ tw, int pmax,
                                                        const double2 *__restrict__ chirpb, double invP, int h,
                                                        double *__restrict__ maps, long npix, long start, int ch0,
                                                        int nnu) {
    constexpr int R = K5_RADIX;
    const int q = N / R;
    const int total = nch * q;
    const int twstep = pmax / N;
    for (int idx = threadIdx.x; idx < total; idx += blockDim.x) {
        const int ch = idx / q, j = idx - ch * q;
        const double2 *cbuf = buf + (size_t)ch * bstride;
        double2 x[R];
#pragma unroll
        for (int r = 0; r < R; r++) x[r] = cbuf[fpad(j + r * q)];
        constexpr int NB = K5_LOGR;
        double2 wp[NB];
        wp[0] = tw_get<SIGN>(tw, pmax, j * twstep);
#pragma unroll
        for (int b = 1; b < NB; b++) wp[b] = cmul(wp[b - 1], wp[b - 1]);
#pragma unroll
        for (int r = 1; r < R; r++) {
#pragma unroll
            for (int b = 0; b < NB; b++)
                if (r & (1 << b)) x[r] = cmul(x[r], wp[b]);
        }
        DftR<R, SIGN>::run(x);
        if (ch0 + ch < nnu) {
            double *out = maps + (size_t)(ch0 + ch) * npix + start;
#pragma unroll
            for (int r = 0; r < R; r++) {
                const int jj = j + r * q;
                if (jj < h) {
                    double2 zv = cmul(x[r], chirpb[jj]);
                    zv.x *= invP;
                    zv.y *= invP;
                    *reinterpret_cast<double2 *>(out + 2 * jj) = zv;
                }
            }
        }
    }
}
#ifndef K5_MC_BLU4
#define K5_MC_BLU4 2   // prefetched cells of the four-channel Bluestein instantiation (2 spills 11 VGPRs)
#endif
#define K5_MC 4  // cells per thread held in registers for the next item (rest read in place)
#ifndef K5_STAMPS
#define K5_STAMPS 0  // diagnostic build: s_memtime phase breakdown
#endif
#if K5_STAMPS
__device__ unsigned long long g_k5_stamps[8];
#define K5STAMP(acc) { unsigned long long _t; asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(_t)::"memory"); acc += _t - k5_last; k5_last = _t; }
#else
#define K5STAMP(acc)
#endif
static inline int nnu_pad_of(int nnu) { return (nnu + 7) & ~7; }
// K5's register prefetch reads K5_MC * K5_THREADS cells from the start of a row without clamping: the last
// row of the F_m buffer needs that much readable memory behind it
// (the compile-time kernels of sht_ringfft_ct.hip prefetch up to 8 x 512 cells)
#define K5_TAIL_PAD ((size_t)8 * 512 * 64)

// ---- cross-translation-unit host functions -------------------------------------------------
// K4: alm [nalm][ncols] -> F_m cells; the launch shape is chosen from the number of 16-column tiles
int sht_legendre(corahip_ctx *ctx, const corahip_sht_plan *p, int ncols, const double *alm, double *inter);
// legendre_kernel's work list for (RT ring row tiles per wave, ncg column groups): the (m, column group, ring tile) items with at
// least one contributing l, m-major, as (m | rtile << 15 | cg << 23, first contributing l); cached in the plan
int sht_k4_items(corahip_ctx *ctx, const corahip_sht_plan *p, int rt, int ncg, const int2 **items, int *nitems);
// legendre_kernel's entry states for ring tiles of 128 rt ring pairs: per (m, ring pair) four states (mu_{R-2}, mu_{R-1}),
// one per lane group, in front of its entry row (leg_seg); zeros for a lane group that never enters; cached in the plan
int sht_k4_segseed(corahip_ctx *ctx, const corahip_sht_plan *p, int rt, const double2 **segseed);
// K4 spin-2: interleaved (E, B) channels -> (Q, U) cells (builds the plan's g table on first use)
int sht_legendre_pol(corahip_ctx *ctx, corahip_sht_plan *p, int ncols, const double *alm, double *inter);
// K5: F_m cells -> maps for nnu_valid channels (nnu_chunk_pad = channels in the cell layout)
int sht_ringfft(corahip_ctx *ctx, const corahip_sht_plan *p, const double *inter, int nnu_chunk_pad, int nnu_valid,
                double *maps);
// K5 with compile-time transform shapes (sht_ringfft_ct.hip): *took = it launched class c (false: the generic kernel
// has to take it); the return value is the error status only (0, CORAHIP_E* or a hipError_t)
// cu_limit: CUs the class may fill (its persistent grid is that many workgroups times those of it that fit one CU)
int sht_ringfft_ct(corahip_ctx *ctx, const corahip_sht_plan *p, const corahip_sht_plan::ring_class &c, const double *inter,
                   int G, int nnu, double *maps, int cu_limit, bool *took);
// does class c go to the ticketed belt kernel (ringfft_direct_ct)?  Such a class may be launched more than once per call:
// every launch draws its items from ctx->k5_tickets, which sht_ringfft zeroes once per call
bool sht_ringfft_ticketed(const corahip_sht_plan::ring_class &c);
// estimated cost of one (ring, channel group) item of class c in CU microseconds, with the CU not limited by HBM
double sht_ringfft_item_weight(const corahip_sht_plan::ring_class &c);
// zeroes the context's ticket counters on `stream` (allocating them on first use): once per sht_ringfft call, ahead of
// every launch of a ticketed class
#define K5_NTICKETS 8
int sht_k5_tickets(corahip_ctx *ctx, hipStream_t stream);
// plan time: the second filter set (fills p->d_ctfilt; h_ctfilt_len / d_ctfilt_off / d_bchirp must be set)
int sht_ctfilt_tables(corahip_ctx *ctx, corahip_sht_plan *p);
// creates ctx->stream2 and the fork / join events on first use
int sht_second_stream(corahip_ctx *ctx);
// Guard of the per-class launch loops of sht_ringfft / sht_ringana, which switch ctx->stream per launch: puts the
// caller's stream back on every exit path, and makes it wait for whatever was put on the second one (an error return in
// the middle of the loop must not leave class kernels running on stream2 unordered against the caller's next
// launches, or against its freeing of `inter` / `maps`).
struct StreamRestore {
    corahip_ctx *c;
    hipStream_t s;
    bool forked = false;
    // the second stream starts behind everything the caller's stream holds so far
    int fork() {
        const int rc = sht_second_stream(c);
        if (rc) return rc;
        HIP_TRY(hipEventRecord(c->ev_fork, s));
        HIP_TRY(hipStreamWaitEvent(c->stream2, c->ev_fork, 0));
        forked = true;
        return 0;
    }
    // the caller's stream is current again and waits for the second one (on an error here the destructor tries again)
    int join() {
        c->stream = s;
        HIP_TRY(hipEventRecord(c->ev_join, c->stream2));
        HIP_TRY(hipStreamWaitEvent(s, c->ev_join, 0));
        forked = false;
        return 0;
    }
    ~StreamRestore() {
        c->stream = s;
        if (forked && (hipEventRecord(c->ev_join, c->stream2) != hipSuccess || hipStreamWaitEvent(s, c->ev_join, 0) != hipSuccess))
            (void)hipStreamSynchronize(c->stream2);
    }
};
// K5^T: maps -> weighted G_m cells for nnu_pad8 channels (nnu present in `maps`)
int sht_ringana_ct(corahip_ctx *ctx, const corahip_sht_plan *p, const corahip_sht_plan::ring_class &c, const double *maps, int nvalid,
                   int nnu_pad, const double *ring_w, int G, double *inter, bool *took);
int sht_ringana(corahip_ctx *ctx, const corahip_sht_plan *p, const double *maps, int nnu, int nnu_pad8,
                const double *ring_w, double *inter);
// K4^T + reduction over ring tiles: G_m cells -> alm_dev (part: per-ring-tile scratch)
int sht_legendre_adj(corahip_ctx *ctx, const corahip_sht_plan *p, int ncols, const double *inter, double *part,
                     double *alm_dev);
// K4^T spin 2 + reduction over ring tiles (sht_polana_native.hip): G_m cells of nchan interleaved (Q, U) channels ->
// interleaved (E, B) alm_dev (part: two slabs, S_W and S_X, per ring tile; builds the plan's g table on first use)
int sht_legendre_adj_pol(corahip_ctx *ctx, corahip_sht_plan *p, int ncols, int nchan, const double *inter, double *part,
                         double *alm_dev);
