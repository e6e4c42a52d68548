// npnormal.hip - numpy's seeded normal stream, Generator(PCG64).standard_normal, generated on the device.
//
// The reference draws every normal of mkfullsky from the caller's numpy Generator (cora/util/nputil.py:121-125,
// called per l from cora/core/skysim.py:120; default_rng(seed) in cora/signal/lss.py:449-450): 1.07e9 values per
// cfg-3 realisation, 5-10 s of host time.  This file produces the SAME values on the GPU, bit for bit:
//
//   bit generator  PCG64 (pcg_setseq_128_xsl_rr_64): state <- state M + inc (mod 2^128), output rotr64(hi ^ lo, hi >> 58);
//                  a 128-bit LCG is position-addressable: f^n(s) = M^n s + inc (M^n - 1)/(M - 1)
//   sampler        numpy's 256-strip ziggurat (random_standard_normal of numpy/random/src/distributions/
//                  distributions.c, tables zig_tab.inc read out of numpy's own library by tools/gen_zig_tabs.py):
//                  one raw draw on the fast path (98.5 % of the positions), two for a wedge sample (accepted or
//                  not), 1 + 2 i for a tail sample.  Tail samples use glibc's log1p restated operation by operation
//                  (fdlibm's algorithm in glibc's evaluation order, no contraction), and the WEDGE test compares
//                  against glibc's exp restated the same way (glibc_exp_fma: the table-driven routine in the
//                  evaluation order of its FMA build, round 6; until then the device library's exp, within one ulp of
//                  it, could have flipped an accept at the threshold): bit-identical to numpy on glibc.
//
// "Which raw position starts a sample" is a prefix problem; oracle/npnormal_model.py states the decomposition in python
// (checked against numpy on the CPU), this is the same thing on the device:
//
//   row    64 consecutive positions, one per lane (lane p of row j of a block holds position 64 j + p; its LCG steps by
//          64: s <- M^64 s + inc G_64), classified AS IF each started a sample: nf (not fast), z (tail class), w (wedge
//          test of (p, p + 1) passes).  The compares that classify ARE the row's 64-bit masks (v_cmp writes a scalar
//          pair), so everything below is scalar code, once per wave.  With `pos` = the next position that starts a
//          sample, position p >= pos of the row starts one iff it is not the second draw of a wedge sample: inside a
//          maximal run of nf positions the starts alternate from the run's first position - found for all 64 at once
//          with an integer add (the carry runs through a run of ones; simdjson's odd-backslash scan).  A tail-class
//          start is walked where it is met (2 draws per iteration, wave-uniform), past the end of the block if need be,
//          like the wedge draw of a block's last position: the state at a block boundary is just k = positions of the
//          next block(s) already consumed.  The wedge tests (15 per block) are gathered in LDS and run 64 at a time.
//   block  16 rows = 1024 positions = one wave, rows in sequence (the scalar chain carries pos from row to row).
//   grid   zig_count_kernel: every block's (k_out, count) for block entry k in {0, 1} and the classes of its rows; a
//          block that hands k >= 2 to its successor (a tail sample across the boundary, 1.5e-4 of the blocks) evaluates
//          the successor for that k itself and appends the result to a patch list.  zig_tile / zig_top / zig_entry
//          compose the block functions (tiles of 512 blocks; inside a tile and across tiles by fixed-point iteration
//          from k = 0: almost every block maps 0 and 1 to the same k_out) and give every block its true
//          (k, first ordinal).  zig_emit_kernel re-runs the generator of every block with them and the stored classes:
//          the samples of a row leave as one store instruction at ordinal + mbcnt - consecutive addresses, no staging.
#include "common.h"

#include <algorithm>
#include <cstdlib>
#include <memory>

#include "stream_internal.h"

#define ZIG_TAB_Q __device__ static const
#include "zig_tab.inc"

typedef unsigned __int128 u128;

#define ZIG_ROWS 16         // rows of 64 consecutive positions per block: lane p of row j holds position 64 j + p
#define ZIG_BLK (64 * ZIG_ROWS)
#define ZIG_WG 256          // threads per workgroup of the count / emit kernels (independent waves, one block each)

namespace {

constexpr u128 mk128(uint64_t hi, uint64_t lo) { return ((u128)hi << 64) | lo; }
constexpr u128 PCG_MULT = mk128(2549297995355413924ULL, 4865540595714422341ULL);

struct jump_t {
    uint64_t mhi, mlo, ghi, glo;   // f^n(s) = m s + inc g (mod 2^128)
};
template <int N>
struct jump_tab {
    jump_t v[N];
};
// n = 2^i
constexpr jump_tab<64> make_pow2() {
    jump_tab<64> t{};
    u128 m = PCG_MULT, g = 1;
    for (int i = 0; i < 64; i++) {
        t.v[i] = jump_t{(uint64_t)(m >> 64), (uint64_t)m, (uint64_t)(g >> 64), (uint64_t)g};
        g = g * (m + 1);
        m = m * m;
    }
    return t;
}
// n = l + 1: from the state before a block's first position to the state that outputs position l
constexpr jump_tab<64> make_lane() {
    jump_tab<64> t{};
    u128 m = PCG_MULT, g = 1;
    for (int i = 0; i < 64; i++) {
        t.v[i] = jump_t{(uint64_t)(m >> 64), (uint64_t)m, (uint64_t)(g >> 64), (uint64_t)g};
        g = g * PCG_MULT + 1;
        m = m * PCG_MULT;
    }
    return t;
}
constexpr jump_tab<64> H_POW2 = make_pow2();
__device__ const jump_tab<64> ZIG_POW2 = make_pow2();
__device__ const jump_tab<64> ZIG_LANE = make_lane();

__host__ __device__ inline u128 jump_apply(const jump_t &j, u128 s, u128 inc) {
    return mk128(j.mhi, j.mlo) * s + inc * mk128(j.ghi, j.glo);
}
__host__ __device__ inline u128 pcg_step(u128 s, u128 inc) { return s * PCG_MULT + inc; }
__host__ __device__ inline uint64_t pcg_out(u128 s) {
    const uint64_t hi = (uint64_t)(s >> 64), lo = (uint64_t)s;
    const uint64_t x = hi ^ lo;
    const unsigned rot = (unsigned)(hi >> 58);
    return (x >> rot) | (x << ((64u - rot) & 63u));
}
inline u128 host_advance(u128 s, u128 inc, uint64_t n) {
    for (int i = 0; i < 64 && (n >> i); i++)
        if ((n >> i) & 1) s = jump_apply(H_POW2.v[i], s, inc);
    return s;
}

constexpr double ZIG_NOR_R = 3.6541528853610087963519472518;
constexpr double ZIG_NOR_INV_R = 0.27366123732975827203338247596;
constexpr uint64_t M52 = 0x000fffffffffffffull;

// glibc's log1p (sysdeps/ieee754/dbl-64/s_log1p.c: fdlibm's algorithm, polynomial in glibc's split evaluation order),
// for -1 < x <= 0, operation by operation in IEEE double without contraction: bit-identical to the libm numpy calls
// (oracle/npnormal.py holds the same restatement; tests/test_oracle.py compares it with math.log1p on the host).
__device__ __attribute__((noinline)) double glibc_log1p_neg(double x) {
#pragma clang fp contract(off)
    const double ln2_hi = 6.93147180369123816490e-01, ln2_lo = 1.90821492927058770002e-10;
    const double Lp1 = 6.666666666666735130e-01, Lp2 = 3.999999999940941908e-01, Lp3 = 2.857142874366239149e-01,
                 Lp4 = 2.222219843214978396e-01, Lp5 = 1.818357216161805012e-01, Lp6 = 1.531383769920937332e-01,
                 Lp7 = 1.479819860511658591e-01;
    const int hx = __double2hiint(x);
    const int ax = hx & 0x7fffffff;
    int k = 1, hu = 0;
    double f = 0.0, c = 0.0;
    if (hx < 0x3FDA827A) {
        if (ax < 0x3e200000) {                       // |x| < 2^-29
            if (ax < 0x3c900000) return x;           // |x| < 2^-54
            return x - x * x * 0.5;
        }
        if (hx > 0 || hx <= (int)0xbfd2bec3) {       // -0.2929 < x < 0.41422
            k = 0;
            f = x;
            hu = 1;
        }
    }
    if (k != 0) {
        double u = 1.0 + x;
        hu = __double2hiint(u);
        k = (hu >> 20) - 1023;
        c = (k > 0) ? 1.0 - (u - x) : x - (u - 1.0);
        c /= u;
        hu &= 0x000fffff;
        if (hu < 0x6a09e) {
            u = __hiloint2double(hu | 0x3ff00000, __double2loint(u));
        } else {
            k += 1;
            u = __hiloint2double(hu | 0x3fe00000, __double2loint(u));
            hu = (0x00100000 - hu) >> 2;
        }
        f = u - 1.0;
    }
    const double hfsq = 0.5 * f * f;
    if (hu == 0) {                                   // |f| < 2^-20
        if (f == 0.0) {
            if (k == 0) return 0.0;
            c += k * ln2_lo;
            return k * ln2_hi + c;
        }
        const double Rs = hfsq * (1.0 - 0.66666666666666666 * f);
        if (k == 0) return f - Rs;
        return k * ln2_hi - ((Rs - (k * ln2_lo + c)) - f);
    }
    const double s = f / (2.0 + f);
    const double z = s * s;
    const double R1 = z * Lp1, z2 = z * z;
    const double R2 = Lp2 + z * Lp3, z4 = z2 * z2;
    const double R3 = Lp4 + z * Lp5, z6 = z4 * z2;
    const double R4 = Lp6 + z * Lp7;
    const double Rr = R1 + z2 * R2 + z4 * R3 + z6 * R4;
    if (k == 0) return f - (hfsq - s * (hfsq + Rr));
    return k * ln2_hi - ((hfsq - (s * (hfsq + Rr) + (k * ln2_lo + c))) - f);
}

#include "glibc_exp.h"   // glibc_exp_fma: glibc's exp in the evaluation order of its FMA build
__global__ void glibc_exp_kernel(const double *__restrict__ x, long n, double *__restrict__ y) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) y[i] = glibc_exp_fma(x[i]);
}

__device__ inline double raw_to_double(uint64_t r) { return (double)(r >> 11) * (1.0 / 9007199254740992.0); }

// the value of a fast-path / wedge sample: rabs * wi[idx], negated by the sign bit
__device__ inline double zig_value(uint64_t r, const double *wi) {
    const double x = (double)((r >> 9) & M52) * wi[r & 0xff];
    return __longlong_as_double(__double_as_longlong(x) ^ (long long)(((r >> 8) & 1) << 63));
}

// wedge test of a sample started by r0 (idx != 0, not fast) with the uniform of the next draw r1
__device__ __attribute__((noinline)) bool zig_wedge_accept(uint64_t r0, uint64_t r1, const double *wi, const double *fi) {
#pragma clang fp contract(off)
    const unsigned idx = (unsigned)(r0 & 0xff);
    const double x = (double)((r0 >> 9) & M52) * wi[idx];
    const double u = raw_to_double(r1);
    const double lhs = (fi[idx - 1] - fi[idx]) * u + fi[idx];
    return lhs < glibc_exp_fma(-0.5 * x * x);
}

struct zig_status {
    unsigned long long total;      // ordinal after the last block of the round
    unsigned long long n_raw;      // raw draws consumed by the first n normals (absolute position count)
    unsigned k_last, npatch, error, pad;
};

#define ZIG_TAIL_CAP 4096   // iterations of one tail loop before the status word is flagged (rejection rate 8 %)

// ---- wave-level primitives ---------------------------------------------------------------------------------------
// (the builtins return int: without the casts the low word sign-extends over the high one)
__device__ inline unsigned uni32(unsigned v) { return (unsigned)__builtin_amdgcn_readfirstlane(v); }
__device__ inline uint64_t uni64(uint64_t v) { return ((uint64_t)uni32((unsigned)(v >> 32)) << 32) | uni32((unsigned)v); }
__device__ inline unsigned readlane32(unsigned v, int l) { return (unsigned)__builtin_amdgcn_readlane(v, l); }
// number of set bits of m below this lane
// lane i <- lane i + 1 (lane 63 keeps its own value): a DPP wave shift, two VALU moves - __shfl_down compiles to two
// ds_bpermute round trips through the LDS crossbar, which the classifying loop took in more than half of its rows
__device__ inline uint64_t wave_shl1(uint64_t v) {
    const int lo = (int)(unsigned)v, hi = (int)(unsigned)(v >> 32);
    const int slo = __builtin_amdgcn_update_dpp(lo, lo, 0x130, 0xF, 0xF, false);   // wave_shl:1
    const int shi = __builtin_amdgcn_update_dpp(hi, hi, 0x130, 0xF, 0xF, false);
    return ((uint64_t)(unsigned)shi << 32) | (unsigned)slo;
}
__device__ inline unsigned mbcnt64(uint64_t m) {
    return __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
}
__device__ inline uint64_t readlane64(uint64_t v, int l) {
    return ((uint64_t)readlane32((unsigned)(v >> 32), l) << 32) | readlane32((unsigned)v, l);
}
__device__ inline void wave_lds_fence() {      // LDS serves a wave's instructions in order; this stops the compiler
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    __builtin_amdgcn_wave_barrier();
}

// the 64-bit class masks of the 16 rows of a block, row j in lane j of each word ("columns"): wave-uniform values
// without spending 6 x 16 scalar registers
struct cols_t {
    unsigned nf_lo = 0, nf_hi = 0, z_lo = 0, z_hi = 0, w_lo = 0, w_hi = 0;
};
__device__ inline void col_set(unsigned &lo, unsigned &hi, int j, uint64_t m) {
    const bool mine = (int)(threadIdx.x & 63) == j;           // (m is wave-uniform: two selects against scalars)
    lo = mine ? (unsigned)m : lo;
    hi = mine ? (unsigned)(m >> 32) : hi;
}
__device__ inline uint64_t col_get(unsigned lo, unsigned hi, int j) {
    return ((uint64_t)readlane32(hi, j) << 32) | readlane32(lo, j);
}

// tail sample whose first draw came out of state `s` (wave-uniform; every lane computes the same): the value with its
// sign, and the draws consumed after that first one
__device__ __attribute__((noinline)) void zig_tail_from(u128 s, u128 inc, double &val, unsigned &consumed, unsigned *err) {
#pragma clang fp contract(off)
    const uint64_t r0 = pcg_out(s);
    unsigned c = 0;
    double xx = 0.0;
    for (int it = 0;; it++) {
        s = pcg_step(s, inc);
        const double u1 = raw_to_double(pcg_out(s));
        s = pcg_step(s, inc);
        const double u2 = raw_to_double(pcg_out(s));
        c += 2;
        xx = -ZIG_NOR_INV_R * glibc_log1p_neg(-u1);
        const double yy = -glibc_log1p_neg(-u2);
        if (yy + yy > xx * xx) break;
        if (it >= ZIG_TAIL_CAP) {
            atomicOr(err, 1u);
            break;
        }
    }
    const bool neg = (((r0 >> 9) & M52) >> 8) & 1;
    val = neg ? -(ZIG_NOR_R + xx) : ZIG_NOR_R + xx;
    consumed = c;
}
// the same for position q of a block, from the state before the block's first position (a jump of q + 1 steps)
__device__ inline void zig_tail_walk(u128 s_blk, u128 inc, unsigned q, double &val, unsigned &consumed, unsigned *err) {
    u128 s = s_blk;
    const unsigned n = q + 1;
    for (int i = 0; i < 32 && (n >> i); i++)
        if ((n >> i) & 1) s = jump_apply(ZIG_POW2.v[i], s, inc);
    zig_tail_from(s, inc, val, consumed, err);
}
__device__ inline u128 bcast128(u128 s, int l) {
    const uint64_t hi = (uint64_t)(s >> 64), lo = (uint64_t)s;
    return mk128(readlane64(hi, l), readlane64(lo, l));
}

// The tail-class positions of a block with what a sample started there consumes: up to four 16-bit entries
// q | (consumed / 2) << 10 (never 0: a tail sample consumes at least two draws); bit 63 = more than fits - the block
// then takes the sequential scalar chain.  Pass 1 makes the table where the row's generator state is live, pass 2
// reads it back.
#define ZIG_TT_OVER (1ull << 63)
__device__ inline uint64_t ttab_add(uint64_t tt, unsigned ntail, unsigned q, unsigned consumed) {
    if (ntail >= 4 || (consumed >> 1) >= 32) return tt | ZIG_TT_OVER;
    return tt | ((uint64_t)(q | ((consumed >> 1) << 10)) << (16 * ntail));
}
// draws consumed by the tail sample started at position q (0: not in the table)
__device__ inline unsigned ttab_lookup(uint64_t tt, unsigned q) {
    unsigned c = 0;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const unsigned en = (unsigned)(tt >> (16 * i)) & 0x7fffu;
        if (en != 0 && (en & 0x3ffu) == q) c = (en >> 10) << 1;
    }
    return c;
}

// ---- the run scan ------------------------------------------------------------------------------------------------
// One row = 64 consecutive positions, bit p of a mask = position p.  `pos` = the next position of the BLOCK that starts a
// sample (everything below it is consumed).  Returns for row j: e_fast / e_wedge = the fast-path / accepted-wedge
// samples of the row up to its first tail-class start, tl_bit = that start (64 = none), and moves pos on past the row
// or past what the row's samples up to there consume.  All values are wave-uniform: this is scalar code.
struct row_eval_t {
    uint64_t e_fast, e_wedge;
    int tl_bit;
};
__device__ inline row_eval_t row_eval(uint64_t nf_j, uint64_t z_j, uint64_t w_j, int j, unsigned &pos) {
    constexpr uint64_t EVEN = 0x5555555555555555ull;
    const unsigned lowk = pos - 64u * j;                                 // < 64 (the caller skips consumed rows)
    const uint64_t low = (1ull << lowk) - 1ull;
    const uint64_t nf = nf_j & ~low;
    const uint64_t starts = nf & ~(nf << 1);
    const uint64_t re = nf & ~(nf + (starts & EVEN));                    // runs whose first position is even
    const uint64_t ro = nf & ~(nf + (starts & ~EVEN));                   // ... odd
    const uint64_t sn = (re & EVEN) | (ro & ~EVEN);                      // sample starts that are not fast
    const uint64_t S = ~(sn << 1);                                       // sample starts
    const uint64_t valid = ~low;
    const uint64_t tl = S & z_j & valid;
    row_eval_t r;
    r.tl_bit = tl ? __builtin_ctzll(tl) : 64;
    const uint64_t upto = tl ? (valid & ((tl & (0ull - tl)) - 1ull)) : valid;
    r.e_fast = S & ~nf & upto;
    r.e_wedge = sn & ~z_j & w_j & upto;
    if (!tl) pos = 64u * (j + 1) + (unsigned)(sn >> 63);                 // a wedge sample at bit 63 takes the next row's first draw
    return r;
}

// (k_out, count) of a block entered with k positions consumed (pass 1: no values)
__device__ inline void block_chain(const cols_t &c, u128 s_blk, u128 inc, unsigned k, unsigned &kout, unsigned &cnt,
                                   unsigned &pos_row0, unsigned &cnt_row0, int rows, unsigned *err) {
    unsigned pos = k, n = 0;
    for (int j = 0; j < ZIG_ROWS; j++) {
        if (j == 1) {
            pos_row0 = pos;
            cnt_row0 = n;
            if (rows == 1) break;
        }
        if (pos >= 64u * (j + 1)) continue;
        const uint64_t nf_j = col_get(c.nf_lo, c.nf_hi, j), z_j = col_get(c.z_lo, c.z_hi, j), w_j = col_get(c.w_lo, c.w_hi, j);
        while (pos < 64u * (j + 1)) {
            const row_eval_t r = row_eval(nf_j, z_j, w_j, j, pos);
            n += __builtin_popcountll(r.e_fast | r.e_wedge);
            if (r.tl_bit == 64) break;
            double v;
            unsigned consumed;
            zig_tail_walk(s_blk, inc, 64u * j + r.tl_bit, v, consumed, err);
            n += 1;
            pos = 64u * j + r.tl_bit + 1 + consumed;
        }
    }
    kout = pos > ZIG_BLK ? pos - ZIG_BLK : 0u;
    cnt = n;
}

// ---- the run scan of all 16 rows at once (lanes 0..15 = rows, 64-bit VALU) -------------------------------------------
// Row j evaluated for both possible carries in (0: its first position starts a sample, 1: it is the wedge draw of the
// previous row's last position); the 16 carries follow from the rows' (carry out | carry in) pairs with one integer add
// (generate = out for carry 0, propagate = out only for carry 1).  A tail-class START anywhere on the chosen path
// (a quarter of the blocks) sends the block to the sequential scalar chain instead.
struct vrow_t {
    uint64_t e, ew, t;      // samples of the row: fast | accepted wedge, the accepted wedges among them, tail samples
    unsigned cout;          // positions of the next row the row's samples consume (0 / 1; more: `big`)
    bool big;
};
__device__ inline vrow_t row_eval_vec(uint64_t nf_j, uint64_t z_j, uint64_t w_j, unsigned cin, uint64_t tt, unsigned q0) {
    constexpr uint64_t EVEN = 0x5555555555555555ull;
    vrow_t r;
    r.e = r.ew = r.t = 0;
    r.cout = 0;
    r.big = false;
    uint64_t low = cin;                                   // positions of the row already consumed
    for (int it = 0; it < 6; it++) {
        const uint64_t nf = nf_j & ~low;
        const uint64_t starts = nf & ~(nf << 1);
        const uint64_t re = nf & ~(nf + (starts & EVEN));
        const uint64_t ro = nf & ~(nf + (starts & ~EVEN));
        const uint64_t sn = (re & EVEN) | (ro & ~EVEN);
        const uint64_t S = ~(sn << 1);
        const uint64_t valid = ~low;
        const uint64_t tl = S & z_j & valid;
        const uint64_t upto = tl ? (valid & ((tl & (0ull - tl)) - 1ull)) : valid;
        const uint64_t ew = sn & ~z_j & w_j & upto;
        r.e |= (S & ~nf & upto) | ew;
        r.ew |= ew;
        if (!tl) {
            r.cout = (unsigned)(sn >> 63);
            return r;
        }
        const unsigned p = (unsigned)__builtin_ctzll(tl);
        r.t |= 1ull << p;
        const unsigned nxt = p + 1 + ttab_lookup(tt, q0 + p);
        if (nxt >= 64) {
            r.cout = nxt - 64;
            r.big = r.cout > 1;
            return r;
        }
        low = (1ull << nxt) - 1ull;
    }
    r.big = true;                                          // (more tail samples in one row than the loop allows)
    return r;
}
// carries into rows 0..16 (bit j = row j's carry in; bit 16 = the block's carry out) for block entry k in {0, 1}
__device__ inline unsigned row_carries(unsigned G, unsigned C1, unsigned k) {
    if ((G & ~C1) == 0) {                       // no row inverts its carry: generate / propagate, one add
        const unsigned sum = C1 + G + k;
        return (sum ^ C1 ^ G) & 0x1ffffu;
    }
    unsigned c = k, cins = 0;
    for (int j = 0; j < ZIG_ROWS; j++) {
        cins |= c << j;
        c = c ? (C1 >> j) & 1u : (G >> j) & 1u;
    }
    return cins | (c << 16);
}
// sum over lanes 0..15 (DPP row shifts; lanes 16.. must hold 0 or are ignored): the total, wave-uniform
__device__ inline unsigned row16_sum(unsigned v) {
    v += (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xf, true);   // row_shr:8
    v += (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xf, true);   // row_shr:4
    v += (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, true);   // row_shr:2
    v += (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, true);   // row_shr:1
    return readlane32(v, 15);
}
// inclusive prefix over lanes 0..15
__device__ inline unsigned row16_scan(unsigned v) {
    unsigned t;
    t = (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, true); v += t;
    t = (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, true); v += t;
    t = (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xf, true); v += t;
    t = (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xf, true); v += t;
    return v;
}

struct zig_lds {
    uint64_t ki[256];
    double wi[256], fi[256];
};
__device__ inline void zig_lds_fill(zig_lds &L) {
    for (int i = threadIdx.x; i < 256; i += blockDim.x) {
        L.ki[i] = ZIG_KI[i];
        L.wi[i] = ZIG_WI[i];
        L.fi[i] = ZIG_FI[i];
    }
    __syncthreads();
}

// state before the first position of block b: f^(pos0 + b BLK)(s0)
__global__ void zig_seek_kernel(uint64_t s_hi, uint64_t s_lo, uint64_t i_hi, uint64_t i_lo, unsigned long long pos0,
                                long nblk, ulonglong2 *__restrict__ blk_state) {
    const long b = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= nblk) return;
    const u128 inc = mk128(i_hi, i_lo);
    u128 s = mk128(s_hi, s_lo);
    const unsigned long long n = pos0 + (unsigned long long)b * ZIG_BLK;
    for (int i = 0; i < 64 && (n >> i); i++)
        if ((n >> i) & 1) s = jump_apply(ZIG_POW2.v[i], s, inc);
    blk_state[b] = make_ulonglong2((uint64_t)(s >> 64), (uint64_t)s);
}

// wave-private LDS of the wedge tests: 1.45 % of the positions are wedge class (15 of a block's 1024); tested where
// they stand they cost a full instruction stream each, so the (draw, next draw) pairs of a block are gathered and
// tested 64 at a time, the verdicts coming back as bits of the rows' masks
#define ZIG_WCAP 128
struct zig_wlds {
    ulonglong2 cand[ZIG_WCAP];
    unsigned short where[ZIG_WCAP];     // position in the block
    unsigned wmask[2 * ZIG_ROWS];       // accepted-wedge masks, row j in words 2 j, 2 j + 1
};

__device__ inline void wedge_flush(zig_wlds *W, unsigned ncand, const double *wi, const double *fi) {
    const int lane = threadIdx.x & 63;
    wave_lds_fence();
    for (unsigned i = lane; i < ncand; i += 64) {
        const ulonglong2 pr = W->cand[i];
        const unsigned q = W->where[i];
        if (zig_wedge_accept(pr.x, pr.y, wi, fi)) atomicOr(&W->wmask[q >> 5], 1u << (q & 31));
    }
    wave_lds_fence();
}

// rows 0 .. 15 of block b: the class masks of every row (columns) - pass 1's vector work.
__device__ inline uint64_t block_classify(cols_t &c, u128 s_blk, u128 inc, u128 lane_m, u128 lane_c, u128 c64,
                                          const zig_lds &L, zig_wlds *W, unsigned *err) {
    const int lane = threadIdx.x & 63;
    constexpr u128 M64 = mk128(H_POW2.v[6].mhi, H_POW2.v[6].mlo);
    u128 s = lane_m * s_blk + lane_c;                            // state after position `lane` of row 0
    uint64_t raw_cur = pcg_out(s);
    if (lane < 2 * ZIG_ROWS) W->wmask[lane] = 0;
    unsigned ncand = 0, ntail = 0;
    uint64_t tt = 0;
#pragma unroll
    for (int j = 0; j < ZIG_ROWS; j++) {
        const u128 s_row = s;                                    // the states that put out row j
        s = s * M64 + c64;
        const uint64_t raw_next = pcg_out(s);                    // row j + 1 (row 16: the next block's first row)
        const unsigned idx = (unsigned)(raw_cur & 0xff);
        const bool slow = ((raw_cur >> 9) & M52) >= L.ki[idx];
        const uint64_t NF = __ballot(slow), Z = __ballot(slow && idx == 0);
        const uint64_t Wm = NF & ~Z;
        if (Wm) {
            // the wedge draw of position p is the draw of position p + 1: the next lane, or lane 0 of the next row
            uint64_t r1 = wave_shl1(raw_cur);
            const uint64_t first_next = readlane64(raw_next, 0);
            if (lane == 63) r1 = first_next;
            const unsigned add = __builtin_popcountll(Wm);
            if (ncand + add > ZIG_WCAP) {
                wedge_flush(W, ncand, L.wi, L.fi);
                ncand = 0;
            }
            if ((Wm >> lane) & 1) {
                const unsigned slot = ncand + mbcnt64(Wm);
                W->cand[slot] = make_ulonglong2(raw_cur, r1);
                W->where[slot] = (unsigned short)(64 * j + lane);
            }
            ncand += add;
        }
        if (Z) {                                                 // 1.6 % of the rows: what a sample started there would consume
            for (uint64_t zz = Z; zz; zz &= zz - 1) {
                const int pz = __builtin_ctzll(zz);
                double v;
                unsigned consumed;
                zig_tail_from(bcast128(s_row, pz), inc, v, consumed, err);
                tt = ttab_add(tt, ntail++, 64u * j + pz, consumed);
            }
        }
        col_set(c.nf_lo, c.nf_hi, j, NF);
        col_set(c.z_lo, c.z_hi, j, Z);
        raw_cur = raw_next;
    }
    wedge_flush(W, ncand, L.wi, L.fi);
    c.w_lo = lane < ZIG_ROWS ? W->wmask[2 * lane] : 0u;
    c.w_hi = lane < ZIG_ROWS ? W->wmask[2 * lane + 1] : 0u;
    wave_lds_fence();
    return tt;
}

// pass 1: fun[2 b + e] = k_out << 16 | count of block b entered with e in {0, 1} positions consumed; classes[b][j] =
// (A, B) of row j with A = wedge class, B = accepted wedge | tail class; successors that will be entered with k >= 2
// are evaluated here and appended to the patch list (key = b << 16 | k, value as fun).
// One wave per block; the waves of a workgroup share nothing but the tables.
__global__ void __launch_bounds__(ZIG_WG)
zig_count_kernel(const ulonglong2 *__restrict__ blk_state, uint64_t i_hi, uint64_t i_lo, long nblk,
                 unsigned *__restrict__ fun, ulonglong2 *__restrict__ classes, unsigned long long *__restrict__ tails,
                 ulonglong2 *__restrict__ patch, unsigned patch_cap, zig_status *st) {
    __shared__ zig_lds L;
    __shared__ zig_wlds Wall[ZIG_WG / 64];
    zig_wlds *W = &Wall[threadIdx.x >> 6];
    zig_lds_fill(L);
    const u128 inc = mk128(i_hi, i_lo);
    const u128 c64 = inc * mk128(H_POW2.v[6].ghi, H_POW2.v[6].glo);
    const int lane = threadIdx.x & 63;
    // from the state before a block's first position to the one that outputs position `lane`: s -> lane_m s + lane_c
    const jump_t lj = ZIG_LANE.v[lane];
    const u128 lane_m = mk128(lj.mhi, lj.mlo), lane_c = inc * mk128(lj.ghi, lj.glo);
    const long wave0 = (long)blockIdx.x * (ZIG_WG / 64) + (threadIdx.x >> 6), nwave = (long)gridDim.x * (ZIG_WG / 64);
    for (long b = wave0; b < nblk; b += nwave) {
        const ulonglong2 bs = blk_state[b];
        const u128 s_blk = mk128(uni64(bs.x), uni64(bs.y));
        cols_t c;
        const uint64_t tt = block_classify(c, s_blk, inc, lane_m, lane_c, c64, L, W, &st->error);
        if (lane < ZIG_ROWS) {
            const uint64_t nf = ((uint64_t)c.nf_hi << 32) | c.nf_lo, z = ((uint64_t)c.z_hi << 32) | c.z_lo,
                           w = ((uint64_t)c.w_hi << 32) | c.w_lo;
            classes[b * ZIG_ROWS + lane] = make_ulonglong2(nf & ~z, w | z);
        }
        if (lane == 0) tails[b] = tt;
        unsigned kb0, total0, kb1, total1;
        {
            const bool row = lane < ZIG_ROWS;
            const uint64_t nf = ((uint64_t)c.nf_hi << 32) | c.nf_lo, z = ((uint64_t)c.z_hi << 32) | c.z_lo,
                           w = ((uint64_t)c.w_hi << 32) | c.w_lo;
            const vrow_t v0 = row_eval_vec(nf, z, w, 0u, tt, 64u * lane), v1 = row_eval_vec(nf, z, w, 1u, tt, 64u * lane);
            const unsigned G = (unsigned)__ballot(row && v0.cout), C1 = (unsigned)__ballot(row && v1.cout);
            const unsigned p0 = row ? __builtin_popcountll(v0.e | v0.t) : 0u;
            const unsigned p1 = row ? __builtin_popcountll(v1.e | v1.t) : 0u;
            const unsigned sum0 = row16_sum(p0);
            const bool over = (tt & ZIG_TT_OVER) != 0;
            unsigned kk[2], tt_[2];
            for (unsigned e = 0; e < 2; e++) {
                const unsigned cins = row_carries(G, C1, e);
                const bool c1 = (cins >> lane) & 1u;
                const bool slow = over || __ballot(row && (c1 ? v1.big : v0.big)) != 0;
                if (!slow) {
                    kk[e] = cins >> 16;
                    tt_[e] = sum0 + row16_sum(c1 && row ? p1 - p0 : 0u);
                } else {
                    unsigned pp, cc;
                    block_chain(c, s_blk, inc, e, kk[e], tt_[e], pp, cc, ZIG_ROWS, &st->error);
                }
            }
            kb0 = kk[0];
            total0 = tt_[0];
            kb1 = kk[1];
            total1 = tt_[1];
        }
        if (lane == 0) *reinterpret_cast<uint2 *>(fun + 2 * b) = make_uint2((kb0 << 16) | total0, (kb1 << 16) | total1);
        // rare: a tail sample (or several) reaches across the end of the block
        for (int e = 0; e < 2; e++) {
            unsigned k = e ? kb1 : kb0;
            if (e == 1 && kb1 == kb0) break;
            for (long bb = b + 1; k >= 2 && bb < nblk; bb++) {
                const ulonglong2 bs2 = blk_state[bb];
                const u128 s2 = mk128(uni64(bs2.x), uni64(bs2.y));
                cols_t c2;
                block_classify(c2, s2, inc, lane_m, lane_c, c64, L, W, &st->error);
                unsigned kb, total, pp, cc;
                block_chain(c2, s2, inc, k, kb, total, pp, cc, ZIG_ROWS, &st->error);
                if (lane == 0) {
                    const unsigned slot = atomicAdd(&st->npatch, 1u);
                    if (slot < patch_cap) patch[slot] = make_ulonglong2(((unsigned long long)bb << 16) | k, (kb << 16) | total);
                    else atomicOr(&st->error, 2u);
                }
                k = kb;
            }
        }
    }
}

// ---- the scan over the block functions ---------------------------------------------------------------------------
// Three small kernels: (1) every tile of 64 x 8 consecutive blocks (one wave; lane = 8 blocks) reduced to its function
// on {0, 1}; (2) one workgroup composes the tile functions and gives every tile its (k, ordinal); (3) every tile
// writes the (k, ordinal) of its blocks.  Inside a tile the lane entries come from the same fixed-point iteration
// from k = 0: almost every block maps 0 and 1 to the same k_out, which ends the dependency.
__device__ inline unsigned patch_lookup(const ulonglong2 *patch, unsigned npatch, long b, unsigned k, unsigned *err) {
    const unsigned long long key = ((unsigned long long)b << 16) | k;
    for (unsigned i = 0; i < npatch; i++)
        if (patch[i].x == key) return (unsigned)patch[i].y;
    atomicOr(err, 4u);
    return 0u;
}
__device__ inline void fun_step(long b, uint2 w2, unsigned &k, unsigned &cnt, const ulonglong2 *patch, unsigned npatch,
                                unsigned *err) {
    const unsigned w = k < 2 ? (k ? w2.y : w2.x) : patch_lookup(patch, npatch, b, k, err);
    k = w >> 16;
    cnt += w & 0xffffu;
}
#define ZIG_SEG 8                       // blocks per lane
#define ZIG_TILE (64 * ZIG_SEG)         // blocks per tile
struct tile_t {
    uint2 w2[ZIG_SEG];
    long b0;                            // first block of the lane
    int nv;                             // blocks of the lane that exist
};
__device__ inline void tile_load(tile_t &t, const unsigned *fun, long tile, long nblk) {
    const int lane = threadIdx.x & 63;
    t.b0 = tile * ZIG_TILE + (long)lane * ZIG_SEG;
    t.nv = (int)std::max<long>(0, std::min<long>(ZIG_SEG, nblk - t.b0));
    const uint2 *f2 = reinterpret_cast<const uint2 *>(fun);
#pragma unroll
    for (int j = 0; j < ZIG_SEG; j++) t.w2[j] = j < t.nv ? f2[t.b0 + j] : make_uint2(0u, 0u);
}
// The function value of block b entered with k >= 2 (a tail sample reached across the boundary: 1.5e-4 of the blocks)
// is in the patch list, which pass 1 appends to in no order.  A lane that walked the list by itself held its whole wave
// for npatch dependent loads (~150 at cfg 3, ~2500 at cfg 5: the scan kernels took 0.2-0.26 ms each for trivial work);
// here the WAVE searches for it: every lane looks at npatch / 64 entries.  `need` lanes get their value in `w`.
__device__ inline void patch_lookup_wave(bool need, long b, unsigned k, unsigned &w, const ulonglong2 *patch, unsigned npatch,
                                         unsigned *err) {
    const int lane = threadIdx.x & 63;
    unsigned long long nm = __ballot(need);
    while (nm) {
        const int src = __builtin_ctzll(nm);
        const unsigned long long key = (readlane64((uint64_t)b, src) << 16) | readlane32(k, src);
        unsigned found = 0;
        bool hit = false;
        for (unsigned i = lane; i < npatch; i += 64)
            if (patch[i].x == key) {
                found = (unsigned)patch[i].y;
                hit = true;
            }
        const unsigned long long hm = __ballot(hit);
        unsigned val = 0;
        if (hm) val = readlane32(found, __builtin_ctzll(hm));
        else if (lane == src) atomicOr(err, 4u);
        if (lane == src) w = val;
        nm &= nm - 1;
    }
}
// one lane = ZIG_SEG consecutive blocks; all lanes of the wave call this together (uniform control flow)
__device__ inline void seg_eval(const tile_t &t, unsigned k, unsigned &kout, unsigned &cnt, const ulonglong2 *patch,
                                unsigned npatch, unsigned *err) {
    unsigned c = 0;
#pragma unroll
    for (int j = 0; j < ZIG_SEG; j++) {
        const bool act = j < t.nv;
        unsigned w = k ? t.w2[j].y : t.w2[j].x;
        patch_lookup_wave(act && k >= 2, t.b0 + j, k, w, patch, npatch, err);
        if (act) {
            k = w >> 16;
            c += w & 0xffffu;
        }
    }
    kout = k;
    cnt = c;
}
// lane entries of a tile entered with k_tile; returns the tile's k_out, every lane keeps its (kin, cnt)
__device__ inline unsigned tile_resolve(const tile_t &t, unsigned k_tile, unsigned &kin, unsigned &cnt,
                                        const ulonglong2 *patch, unsigned npatch, unsigned *err) {
    const int lane = threadIdx.x & 63;
    kin = lane == 0 ? k_tile : 0u;
    unsigned assumed = 0, kout = 0;
    for (int it = 0; it <= 64; it++) {
        seg_eval(t, kin, kout, cnt, patch, npatch, err);
        const bool changed = lane != 63 && kout != assumed;
        assumed = kout;
        if (!__any(changed)) break;
        const unsigned up = __shfl_up(kout, 1);
        kin = lane == 0 ? k_tile : up;
    }
    return __shfl(kout, 63);
}
__device__ inline unsigned wave_sum(unsigned v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

__global__ void __launch_bounds__(256)
zig_tile_kernel(long nblk, long ntile, const unsigned *__restrict__ fun, const ulonglong2 *__restrict__ patch,
                unsigned patch_cap, uint4 *__restrict__ tile_fun, zig_status *st) {
    const long tile = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (tile >= ntile) return;
    const unsigned npatch = min(st->npatch, patch_cap);
    tile_t t;
    tile_load(t, fun, tile, nblk);
    unsigned kin, cnt;
    const unsigned k0 = tile_resolve(t, 0u, kin, cnt, patch, npatch, &st->error);
    const unsigned c0 = wave_sum(cnt);
    const unsigned k1 = tile_resolve(t, 1u, kin, cnt, patch, npatch, &st->error);
    const unsigned c1 = wave_sum(cnt);
    if ((threadIdx.x & 63) == 0) tile_fun[tile] = make_uint4(k0, c0, k1, c1);
}

// one workgroup: tile_entry[t] = (k, ordinal) of every tile; a tile entered with k >= 2 (a tail sample across a tile
// boundary) is walked block by block here
#define ZIG_TOP_T 1024
__global__ void __launch_bounds__(ZIG_TOP_T)
zig_top_kernel(long nblk, long ntile, const unsigned *__restrict__ fun, const ulonglong2 *__restrict__ patch,
               unsigned patch_cap, const uint4 *__restrict__ tile_fun, unsigned long long ord0,
               ulonglong2 *__restrict__ tile_entry, zig_status *st, int force_serial) {
    constexpr int T = ZIG_TOP_T;
    __shared__ unsigned g_k[T][2];
    __shared__ unsigned long long g_c[T][2];
    __shared__ unsigned s_k[T];
    __shared__ unsigned long long s_o[T];
    const int t = threadIdx.x;
    const unsigned npatch = min(st->npatch, patch_cap);
    const long seg = (ntile + T - 1) / T;
    const long t0 = std::min<long>(ntile, t * seg), t1 = std::min<long>(ntile, t0 + seg);
    auto tile_step = [&](long tile, unsigned &k, unsigned long long &o) {
        if (k < 2) {
            const uint4 f = tile_fun[tile];
            o += k ? f.w : f.y;
            k = k ? f.z : f.x;
        } else {
            const uint2 *f2 = reinterpret_cast<const uint2 *>(fun);
            const long c0 = tile * ZIG_TILE, c1 = std::min<long>(nblk, c0 + ZIG_TILE);
            unsigned c = 0;
            for (long b = c0; b < c1; b++) fun_step(b, f2[b], k, c, patch, npatch, &st->error);
            o += c;
        }
    };
    for (int e = 0; e < 2; e++) {
        unsigned k = e;
        unsigned long long o = 0;
        for (long tile = t0; tile < t1; tile++) tile_step(tile, k, o);
        g_k[t][e] = k;
        g_c[t][e] = o;
    }
    __syncthreads();
    // The T thread functions are composed by ONE wave in three short steps (round 6; a single thread walking all T entries -
    // 1024 dependent LDS reads - was 0.25 ms of the 0.35 ms scan): lane L composes its T / 64 consecutive entries for both
    // entries k, the 64 lane functions are chained through readlane, every lane walks its entries again with its true
    // (k, ordinal).  An exit k >= 2 anywhere (a tail sample across a thread's boundary: ~15 % of the cfg-3 streams have
    // one) has no table entry: the serial walk below, which evaluates such tiles block by block, takes over.
    __shared__ int s_serial;
    if (t == 0) s_serial = 0;
    __syncthreads();
    if (t < 64) {
        constexpr int PER = T / 64;
        unsigned fk[2];
        unsigned long long fc[2];
        bool bad = false;
        for (int e = 0; e < 2; e++) {
            unsigned k = e;
            unsigned long long c = 0;
            for (int i = t * PER; i < (t + 1) * PER; i++) {
                if (k >= 2) {
                    bad = true;
                    break;
                }
                c += g_c[i][k];
                k = g_k[i][k];
            }
            fk[e] = k;
            fc[e] = c;
            bad = bad || k >= 2;
        }
        if (__any(bad) || force_serial) {
            if (t == 0) s_serial = 1;
        } else {
            unsigned k = 0, my_k = 0;
            unsigned long long o = ord0, my_o = 0;
            for (int L = 0; L < 64; L++) {
                if (t == L) {
                    my_k = k;
                    my_o = o;
                }
                const unsigned k0 = readlane32(fk[0], L), k1 = readlane32(fk[1], L);
                const unsigned long long c0 = readlane64(fc[0], L), c1 = readlane64(fc[1], L);
                o += k ? c1 : c0;
                k = k ? k1 : k0;
            }
            if (t == 0) {
                st->total = o;
                st->k_last = k;
            }
            for (int i = t * PER; i < (t + 1) * PER; i++) {
                s_k[i] = my_k;
                s_o[i] = my_o;
                my_o += g_c[i][my_k];
                my_k = g_k[i][my_k];
            }
        }
    }
    __syncthreads();
    if (s_serial && t == 0) {
        unsigned k = 0;
        unsigned long long o = ord0;
        for (int i = 0; i < T; i++) {
            s_k[i] = k;
            s_o[i] = o;
            if (k < 2) {
                o += g_c[i][k];
                k = g_k[i][k];
            } else {
                const long a0 = std::min<long>(ntile, i * seg), a1 = std::min<long>(ntile, a0 + seg);
                for (long tile = a0; tile < a1; tile++) tile_step(tile, k, o);
            }
        }
        st->total = o;
        st->k_last = k;
    }
    __syncthreads();
    unsigned k = s_k[t];
    unsigned long long o = s_o[t];
    for (long tile = t0; tile < t1; tile++) {
        tile_entry[tile] = make_ulonglong2(k, o);
        tile_step(tile, k, o);
    }
}

__global__ void __launch_bounds__(256)
zig_entry_kernel(long nblk, long ntile, const unsigned *__restrict__ fun, const ulonglong2 *__restrict__ patch,
                 unsigned patch_cap, const ulonglong2 *__restrict__ tile_entry, ulonglong2 *__restrict__ entry,
                 zig_status *st) {
    const long tile = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (tile >= ntile) return;
    const int lane = threadIdx.x & 63;
    const unsigned npatch = min(st->npatch, patch_cap);
    tile_t t;
    tile_load(t, fun, tile, nblk);
    const ulonglong2 te = tile_entry[tile];
    unsigned kin, cnt;
    tile_resolve(t, (unsigned)te.x, kin, cnt, patch, npatch, &st->error);
    unsigned incl = cnt;
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned v = __shfl_up(incl, o);
        if (lane >= o) incl += v;
    }
    unsigned k = kin;
    unsigned long long o = te.y + (incl - cnt);
#pragma unroll
    for (int j = 0; j < ZIG_SEG; j++) {
        const bool act = j < t.nv;
        if (act) entry[t.b0 + j] = make_ulonglong2(k, o);
        unsigned w = k ? t.w2[j].y : t.w2[j].x;
        patch_lookup_wave(act && k >= 2, t.b0 + j, k, w, patch, npatch, &st->error);
        if (act) {
            k = w >> 16;
            o += w & 0xffffu;
        }
    }
}

// Where pass 2 puts a normal: a functor called with (ordinal, value) at each of the emit kernel's store sites, after
// block(first ordinal of the block) - wave-uniform, once per block.
// The plain store: ordinal o goes to g[o - o_lo].
struct sink_store {
    double *__restrict__ g;
    unsigned long long o_lo;
    struct stage_t {};
    __device__ inline void attach(stage_t *) {}
    __device__ inline void block(unsigned long long) {}
    __device__ inline void operator()(unsigned long long o, double v) const { g[o - o_lo] = v; }
    __device__ inline void flush(unsigned long long) {}
};
// numpy's Generator.normal(0, scale[:, None], (nrow, ncol)) written or added in place: ordinal o is element (r, c) =
// divmod(o, ncol), its value 0.0 + scale[r] z (one rounded multiply, the rounded add of 0.0 that makes scale = 0 give
// +0.0 whatever the sign of z, and in accumulate mode one more rounded add), stored at out[row_off[r] + c] (row_off
// NULL: r ncol + c).  The ordinals of a block are consecutive and fewer than ZIG_BLK, so the one 64-bit division is
// that of the block's first ordinal: element d of the block is at column c0 + d of row r0 - past the end of the row at
// most once when ncol >= ZIG_BLK, and a 32-bit division (of a value < 2 ZIG_BLK) below that, where several field rows
// fall inside one block, or one 64-lane row.
// The store sites only park z in a wave-private LDS stage, at the ordinal's place in the block; flush(), once per block,
// walks the stage 64 consecutive ordinals at a time: consecutive addresses per instruction except across a field-row end,
// and in accumulate mode eight loads of the field in flight per lane before the first add.  (Read, add and store at the
// store sites themselves, one dependent memory round trip per wave row at four waves per SIMD, made this emit pass 2.5
// times as long as the plain one.)
struct sink_rows {
    struct stage_t {
        double z[ZIG_BLK];
    };
    const double *__restrict__ scale;
    const int64_t *__restrict__ row_off;
    double *out;
    unsigned long long ncol;
    int accumulate;
    unsigned long long ord_blk, r0, c0;
    stage_t *stage;
    __device__ inline void attach(stage_t *s) { stage = s; }
    __device__ inline void block(unsigned long long ob) {
        ord_blk = ob;
        r0 = ob / ncol;
        c0 = ob - r0 * ncol;
    }
    __device__ inline void operator()(unsigned long long o, double z) const {
        const unsigned long long d = o - ord_blk;
        if (d < ZIG_BLK) stage->z[d] = z;
    }
    // element d of the block: its address in out and its row's scale
    __device__ inline double *locate(unsigned d, double &sc) const {
        unsigned long long r = r0, c = c0 + d;
        if (c >= ncol) {
            if (ncol >= ZIG_BLK) {
                r += 1;
                c -= ncol;
            } else {
                const unsigned q = (unsigned)c / (unsigned)ncol;
                r += q;
                c -= (unsigned long long)q * ncol;
            }
        }
        sc = scale[r];
        return out + (row_off ? (unsigned long long)row_off[r] : r * ncol) + c;
    }
    // ord_end: the ordinal after the block's last sample that was handed over
    __device__ inline void flush(unsigned long long ord_end) const {
#pragma clang fp contract(off)
        constexpr int NB = 8;
        const unsigned cnt = (unsigned)std::min<unsigned long long>(ord_end - ord_blk, (unsigned long long)ZIG_BLK);
        const unsigned lane = threadIdx.x & 63;
        wave_lds_fence();
        for (unsigned h = 0; h < cnt; h += 64u * NB) {
            double *p[NB];
            double v[NB], old[NB];
#pragma unroll
            for (int i = 0; i < NB; i++) {
                const unsigned d = h + 64u * i + lane;
                p[i] = nullptr;
                v[i] = 0.0;
                if (d < cnt) {
                    double sc;
                    p[i] = locate(d, sc);
                    v[i] = __dadd_rn(0.0, __dmul_rn(sc, stage->z[d]));
                }
            }
            if (accumulate) {
#pragma unroll
                for (int i = 0; i < NB; i++) old[i] = p[i] ? *p[i] : 0.0;
#pragma unroll
                for (int i = 0; i < NB; i++)
                    if (p[i]) *p[i] = __dadd_rn(old[i], v[i]);
            } else {
#pragma unroll
                for (int i = 0; i < NB; i++)
                    if (p[i]) *p[i] = v[i];
            }
        }
        wave_lds_fence();                                   // (the next block parks its values in the same stage)
    }
};

// pass 2: every block with its true entry; the normals with ordinals in [o_lo, o_hi) go to the sink - sink_store: to
// g[ordinal - o_lo] (the whole stream: o_lo = 0, o_hi = n; one range of the l-range pipeline: its ordinals, g = the ring
// slot); sink_rows: scaled into the rows of a field.  blk_first: device
// word holding the first block to look at - the one that contains ordinal o_lo (zig_range_kernel) -, NULL = block 0.
// Lane p of row j holds position 64 j + p: the samples of a row leave as one store instruction to consecutive addresses.
template <class Sink>
__global__ void __launch_bounds__(ZIG_WG)
zig_emit_kernel(const ulonglong2 *__restrict__ blk_state, uint64_t i_hi, uint64_t i_lo, long nblk,
                const ulonglong2 *__restrict__ entry, const ulonglong2 *__restrict__ classes,
                const unsigned long long *__restrict__ tails, unsigned long long pos0, unsigned long long n,
                unsigned long long o_lo, unsigned long long o_hi, const long *__restrict__ blk_first,
                const Sink sink_arg, zig_status *st) {
    __shared__ zig_lds L;
    zig_lds_fill(L);
    __shared__ typename Sink::stage_t stages[ZIG_WG / 64];
    Sink sink = sink_arg;                                   // (block() keeps the block's row and column in it)
    sink.attach(&stages[threadIdx.x >> 6]);
    const u128 inc = mk128(i_hi, i_lo);
    const u128 c64 = inc * mk128(H_POW2.v[6].ghi, H_POW2.v[6].glo);
    constexpr u128 M64 = mk128(H_POW2.v[6].mhi, H_POW2.v[6].mlo);
    const int lane = threadIdx.x & 63;
    const jump_t lj = ZIG_LANE.v[lane];
    const u128 lane_m = mk128(lj.mhi, lj.mlo), lane_c = inc * mk128(lj.ghi, lj.glo);
    const long wave0 = (long)blockIdx.x * (ZIG_WG / 64) + (threadIdx.x >> 6), nwave = (long)gridDim.x * (ZIG_WG / 64);
    const long b_first = blk_first ? *blk_first : 0L;
    const unsigned long long o_n = o_hi - o_lo;            // ordinal o is written iff o - o_lo < o_n (unsigned: o < o_lo wraps)
    for (long b = b_first + wave0; b < nblk; b += nwave) {
        const ulonglong2 en = entry[b];
        const unsigned long long ord_blk = uni64(en.y);
        if (ord_blk >= o_hi) break;                         // (blocks are in ordinal order: nothing left to write)
        sink.block(ord_blk);
        const ulonglong2 bs = blk_state[b];
        const u128 s_blk = mk128(uni64(bs.x), uni64(bs.y));
        // classes of the 16 rows, row j in lane j
        ulonglong2 cl = make_ulonglong2(0ull, 0ull);
        if (lane < ZIG_ROWS) cl = classes[b * ZIG_ROWS + lane];
        const uint64_t z_col = cl.y & ~cl.x, w_col = cl.y & cl.x, nf_col = cl.x | z_col;
        u128 s = lane_m * s_blk + lane_c;                    // state after position `lane` of row 0
        unsigned pos = uni32((unsigned)en.x);
        const unsigned long long blk_pos = pos0 + (unsigned long long)b * ZIG_BLK;
        // fast path (entry 0 or 1): all rows evaluated at once in lanes 0..15
        const uint64_t tt = uni64(tails[b]);
        if (pos < 2 && !(tt & ZIG_TT_OVER)) {
            const bool row = lane < ZIG_ROWS;
            const vrow_t v0 = row_eval_vec(nf_col, z_col, w_col, 0u, tt, 64u * lane),
                         v1 = row_eval_vec(nf_col, z_col, w_col, 1u, tt, 64u * lane);
            const unsigned G = (unsigned)__ballot(row && v0.cout), C1 = (unsigned)__ballot(row && v1.cout);
            const unsigned cins = row_carries(G, C1, pos);
            const bool c1 = (cins >> lane) & 1u;
            if (__ballot(row && (c1 ? v1.big : v0.big)) == 0) {
                const uint64_t ew_col = row ? (c1 ? v1.ew : v0.ew) : 0ull;
                const uint64_t t_col = row ? (c1 ? v1.t : v0.t) : 0ull;
                const uint64_t e_col = row ? (c1 ? v1.e : v0.e) : 0ull;
                const unsigned pc = __builtin_popcountll(e_col | t_col);
                const unsigned base_col = row16_scan(pc) - pc;          // samples of the block before row `lane`
                const unsigned trows = (unsigned)__ballot(t_col != 0);  // rows with a tail sample
#pragma unroll
                for (int j = 0; j < ZIG_ROWS; j++) {
                    const uint64_t raw = pcg_out(s);
                    const uint64_t e = readlane64(e_col, j);
                    if ((trows >> j) & 1) {
                        const uint64_t tj = readlane64(t_col, j), all = e | tj;
                        for (uint64_t zz = tj; zz; zz &= zz - 1) {
                            const int pz = __builtin_ctzll(zz);
                            double v;
                            unsigned consumed;
                            zig_tail_from(bcast128(s, pz), inc, v, consumed, &st->error);
                            const unsigned long long o = ord_blk + readlane32(base_col, j) +
                                                         __builtin_popcountll(all & ((1ull << pz) - 1ull));
                            if (lane == 0 && o - o_lo < o_n) {
                                sink(o, v);
                                if (o + 1 == n) st->n_raw = blk_pos + 64u * j + pz + 1 + consumed;
                            }
                        }
                        if ((e >> lane) & 1) {
                            const unsigned long long o = ord_blk + readlane32(base_col, j) + mbcnt64(all);
                            if (o - o_lo < o_n) {
                                sink(o, zig_value(raw, L.wi));
                                if (o + 1 == n) st->n_raw = blk_pos + 64u * j + lane + 1 + ((readlane64(ew_col, j) >> lane) & 1);
                            }
                        }
                    } else if ((e >> lane) & 1) {
                        const unsigned long long o = ord_blk + readlane32(base_col, j) + mbcnt64(e);
                        if (o - o_lo < o_n) {
                            sink(o, zig_value(raw, L.wi));
                            if (o + 1 == n) st->n_raw = blk_pos + 64u * j + lane + 1 + ((readlane64(ew_col, j) >> lane) & 1);
                        }
                    }
                    s = s * M64 + c64;
                }
                sink.flush(std::min<unsigned long long>(ord_blk + readlane32(base_col + pc, ZIG_ROWS - 1), o_hi));
                continue;
            }
        }
        unsigned long long ord = ord_blk;                    // ordinal of the next sample
#pragma unroll
        for (int j = 0; j < ZIG_ROWS; j++) {
            const uint64_t raw = pcg_out(s);
            s = s * M64 + c64;
            if (pos >= 64u * (j + 1)) continue;
            const uint64_t nf_j = readlane64(nf_col, j), z_j = readlane64(z_col, j), w_j = readlane64(w_col, j);
            while (pos < 64u * (j + 1)) {
                const row_eval_t r = row_eval(nf_j, z_j, w_j, j, pos);
                const uint64_t e = r.e_fast | r.e_wedge;
                if ((e >> lane) & 1) {
                    const unsigned long long o = ord + mbcnt64(e);
                    if (o - o_lo < o_n) {
                        sink(o, zig_value(raw, L.wi));
                        if (o + 1 == n) st->n_raw = blk_pos + 64u * j + lane + 1 + ((r.e_wedge >> lane) & 1);
                    }
                }
                ord += __builtin_popcountll(e);
                if (r.tl_bit == 64) break;
                double v;
                unsigned consumed;
                zig_tail_walk(s_blk, inc, 64u * j + r.tl_bit, v, consumed, &st->error);
                if (lane == 0 && ord - o_lo < o_n) {
                    sink(ord, v);
                    if (ord + 1 == n) st->n_raw = blk_pos + 64u * j + r.tl_bit + 1 + consumed;
                }
                ord += 1;
                pos = 64u * j + r.tl_bit + 1 + consumed;
            }
        }
        sink.flush(std::min<unsigned long long>(ord, o_hi));
    }
}

// first block of every range of the l-range pipeline: blk_first[r] = the block that contains ordinal bounds[r] (the
// largest b with entry[b].ordinal <= bounds[r]; entry ordinals increase with b)
__global__ void zig_range_kernel(const ulonglong2 *__restrict__ entry, long nblk, const unsigned long long *__restrict__ bounds,
                                 int nr, long *__restrict__ blk_first) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= nr) return;
    const unsigned long long o = bounds[r];
    long lo = 0, hi = nblk - 1;                              // invariant: entry[lo].y <= o (or lo = 0), answer in [lo, hi]
    while (lo < hi) {
        const long mid = (lo + hi + 1) >> 1;
        if (entry[mid].y <= o) lo = mid;
        else hi = mid - 1;
    }
    blk_first[r] = lo;
}

}  // namespace

// ---- host side: one round = the tables of nblk blocks from raw position pos0 on ------------------------------------------
struct zig_round {
    long nblk = 0, ntile = 0;
    unsigned patch_cap = 0, grid = 0;
    ulonglong2 *blk_state = nullptr, *entry = nullptr, *patch = nullptr, *classes = nullptr, *tile_entry = nullptr;
    unsigned *fun = nullptr;
    unsigned long long *tails = nullptr;
    uint4 *tile_fun = nullptr;
    zig_status *st = nullptr;
    char *extra = nullptr;          // `extra_bytes` more, 16-byte aligned, behind the status word (range tables of the l-range pipeline)
};
// the block tables of a round that has to yield `want` normals, cut from scratch slot 6
static int zig_round_tables(corahip_ctx *ctx, unsigned long long want, size_t extra_bytes, zig_round &rd) {
    // 1.02145 raw draws per normal on average; the margin covers 200 sigma, and a short round is followed by another
    rd.nblk = (long)((want + want / 44 + 2 * ZIG_BLK) / ZIG_BLK) + 1;
    rd.patch_cap = (unsigned)(rd.nblk / 64 + 1024);
    rd.ntile = (rd.nblk + ZIG_TILE - 1) / ZIG_TILE;
    const size_t nblk = (size_t)rd.nblk, ntile = (size_t)rd.ntile;
    const size_t off_fun = sizeof(ulonglong2) * nblk;
    const size_t off_entry = off_fun + sizeof(unsigned) * 2 * nblk;
    const size_t off_patch = off_entry + sizeof(ulonglong2) * nblk;
    const size_t off_cls = off_patch + sizeof(ulonglong2) * rd.patch_cap;
    const size_t off_tt = off_cls + sizeof(ulonglong2) * ZIG_ROWS * nblk;
    const size_t off_tf = off_tt + sizeof(unsigned long long) * nblk;
    const size_t off_te = off_tf + sizeof(uint4) * ntile;
    const size_t off_st = off_te + sizeof(ulonglong2) * ntile;
    const size_t off_ex = (off_st + sizeof(zig_status) + 15) & ~(size_t)15;
    char *ws = nullptr;
    int rc = corahip_ctx_scratch(ctx, 6, off_ex + extra_bytes, (void **)&ws);
    if (rc) return rc;
    rd.blk_state = (ulonglong2 *)ws;
    rd.fun = (unsigned *)(ws + off_fun);
    rd.entry = (ulonglong2 *)(ws + off_entry);
    rd.patch = (ulonglong2 *)(ws + off_patch);
    rd.classes = (ulonglong2 *)(ws + off_cls);
    rd.tails = (unsigned long long *)(ws + off_tt);
    rd.tile_fun = (uint4 *)(ws + off_tf);
    rd.tile_entry = (ulonglong2 *)(ws + off_te);
    rd.st = (zig_status *)(ws + off_st);
    rd.extra = ws + off_ex;
    rd.grid = (unsigned)std::min<long>((rd.nblk + ZIG_WG / 64 - 1) / (ZIG_WG / 64), (long)ctx->num_cu * 32);
    return 0;
}
// seek + pass 1 + the scan over the block functions, on `stream`: afterwards every block has its (k, first ordinal)
static int zig_round_count_scan(corahip_ctx *ctx, hipStream_t stream, const uint64_t state[2], const uint64_t inc[2],
                                unsigned long long pos0, unsigned long long ord0, const zig_round &rd) {
    const bool other = stream != ctx->stream;
    HIP_TRY(hipMemsetAsync(rd.st, 0, sizeof(zig_status), stream));
    {
        StageTimer t0(ctx, "zig_seek", stream, other);
        zig_seek_kernel<<<(unsigned)((rd.nblk + 255) / 256), 256, 0, stream>>>(state[0], state[1], inc[0], inc[1], pos0, rd.nblk,
                                                                              rd.blk_state);
        LAUNCH_CHECK();
    }
    {
        StageTimer t1(ctx, "zig_count", stream, other);
        zig_count_kernel<<<rd.grid, ZIG_WG, 0, stream>>>(rd.blk_state, inc[0], inc[1], rd.nblk, rd.fun, rd.classes, rd.tails, rd.patch,
                                                        rd.patch_cap, rd.st);
        LAUNCH_CHECK();
    }
    {
        StageTimer t2(ctx, "zig_scan", stream, other);
        const unsigned tgrid = (unsigned)((rd.ntile + 3) / 4);
        zig_tile_kernel<<<tgrid, 256, 0, stream>>>(rd.nblk, rd.ntile, rd.fun, rd.patch, rd.patch_cap, rd.tile_fun, rd.st);
        LAUNCH_CHECK();
        const char *fs = getenv("CORAHIP_ZIG_TOP_SERIAL");       // (tests: the serial walk that takes over when a thread hands on k >= 2)
        zig_top_kernel<<<1, ZIG_TOP_T, 0, stream>>>(rd.nblk, rd.ntile, rd.fun, rd.patch, rd.patch_cap, rd.tile_fun, ord0, rd.tile_entry,
                                                   rd.st, fs && atoi(fs) ? 1 : 0);
        LAUNCH_CHECK();
        zig_entry_kernel<<<tgrid, 256, 0, stream>>>(rd.nblk, rd.ntile, rd.fun, rd.patch, rd.patch_cap, rd.tile_entry, rd.entry, rd.st);
        LAUNCH_CHECK();
    }
    return 0;
}
// the status word of a round read back into `hs` (synchronises `stream`); what the device flagged is an error of `what`
static int zig_status_read(hipStream_t stream, const zig_status *st, const char *what, zig_status &hs) {
    HIP_TRY(hipMemcpyAsync(&hs, st, sizeof(hs), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    if (hs.error) {
        corahip_set_error("%s: device status %u (1 tail loop cap, 2 patch list full, 4 patch missing)", what, hs.error);
        return CORAHIP_ESTATE;
    }
    return 0;
}

// ---- the stream in ranges (stream_internal.h), two-pass form ----------------------------------------------------------
struct zig_session {
    zig_round rd;
    uint64_t state[2], inc[2];
    unsigned long long n = 0;
    std::vector<unsigned long long> bounds;      // [nr + 1] ordinals; kept until finish (the upload is asynchronous)
    unsigned long long *d_bounds = nullptr;
    long *d_first = nullptr;
    int nr = 0;
};

int zig_stream_prepare(corahip_ctx *ctx, hipStream_t stream, const uint64_t state[2], const uint64_t inc[2], int64_t n,
                       const std::vector<unsigned long long> &bounds, zig_session **out) {
    ARG_CHECK(n > 0 && bounds.size() >= 2 && bounds.front() == 0 && bounds.back() == (unsigned long long)n);
    std::unique_ptr<zig_session> owner(new zig_session());   // freed on every failure below; handed out at the end
    zig_session *s = owner.get();
    s->n = (unsigned long long)n;
    s->bounds = bounds;
    s->nr = (int)bounds.size() - 1;
    for (int i = 0; i < 2; i++) {
        s->state[i] = state[i];
        s->inc[i] = inc[i];
    }
    const size_t nb = bounds.size();
    int rc = zig_round_tables(ctx, s->n, (sizeof(unsigned long long) + sizeof(long)) * nb, s->rd);
    if (!rc) {
        s->d_bounds = (unsigned long long *)s->rd.extra;
        s->d_first = (long *)(s->rd.extra + sizeof(unsigned long long) * nb);
        rc = zig_round_count_scan(ctx, stream, state, inc, 0ull, 0ull, s->rd);
    }
    if (!rc) {
        hipError_t e = hipMemcpyAsync(s->d_bounds, s->bounds.data(), sizeof(unsigned long long) * nb, hipMemcpyHostToDevice, stream);
        if (e != hipSuccess) rc = (int)e;
    }
    if (rc) return rc;
    zig_range_kernel<<<(s->nr + 63) / 64, 64, 0, stream>>>(s->rd.entry, s->rd.nblk, s->d_bounds, s->nr, s->d_first);
    if (hipGetLastError() != hipSuccess) {
        corahip_set_error("zig_range_kernel launch failed");
        return CORAHIP_ESTATE;
    }
    *out = owner.release();
    return 0;
}

int zig_stream_emit_range(corahip_ctx *ctx, hipStream_t stream, zig_session *s, int r, double *slot) {
    ARG_CHECK(s != nullptr && r >= 0 && r < s->nr && slot != nullptr);
    const unsigned long long o_lo = s->bounds[r], o_hi = s->bounds[r + 1];
    // one wave per block of ~1000 normals; the grid covers the range's blocks (+ slack: the loop strides, nothing is missed)
    const long est = (long)((o_hi - o_lo) / 960) + 8;
    const unsigned grid = (unsigned)std::max<long>(1, std::min<long>((est + ZIG_WG / 64 - 1) / (ZIG_WG / 64), (long)ctx->num_cu * 32));
    StageTimer t3(ctx, "zig_emit", stream, stream != ctx->stream);
    zig_emit_kernel<<<grid, ZIG_WG, 0, stream>>>(s->rd.blk_state, s->inc[0], s->inc[1], s->rd.nblk, s->rd.entry, s->rd.classes,
                                                s->rd.tails, 0ull, s->n, o_lo, o_hi, s->d_first + r, sink_store{slot, o_lo},
                                                s->rd.st);
    LAUNCH_CHECK();
    return 0;
}

int zig_stream_finish(corahip_ctx *ctx, hipStream_t stream, zig_session *s, uint64_t *n_raw) {
    ARG_CHECK(s != nullptr && n_raw != nullptr);
    zig_status hs;
    const int rc = zig_status_read(stream, s->rd.st, "normals_pcg64 (ranges)", hs);
    if (rc) return rc;
    if (hs.total < s->n) {      // (the margin of the block count is 200 sigma: never met)
        corahip_set_error("normals_pcg64 (ranges): the raw range held %llu normals, %llu needed", hs.total, s->n);
        return CORAHIP_ESTATE;
    }
    *n_raw = hs.n_raw;
    return 0;
}

void zig_stream_free(zig_session *s) { delete s; }

// the next n normals from (state, inc) through `sink`, ordinals 0 .. n: rounds of block tables until n are out
// (almost always one; a short round is followed by another from where it ended)
template <class Sink>
static int zig_rounds(corahip_ctx *ctx, const uint64_t state[2], const uint64_t inc[2], unsigned long long n, const Sink &sink,
                      const char *what, uint64_t *n_raw) {
    unsigned long long pos0 = 0, ord0 = 0;
    for (int round = 0; round < 64; round++) {
        zig_round rd;
        int rc = zig_round_tables(ctx, n - ord0, 0, rd);
        if (rc) return rc;
        if ((rc = zig_round_count_scan(ctx, ctx->stream, state, inc, pos0, ord0, rd))) return rc;
        {
            StageTimer t3(ctx, "zig_emit");
            zig_emit_kernel<<<rd.grid, ZIG_WG, 0, ctx->stream>>>(rd.blk_state, inc[0], inc[1], rd.nblk, rd.entry, rd.classes, rd.tails,
                                                                pos0, n, 0ull, n, nullptr, sink, rd.st);
            LAUNCH_CHECK();
        }
        zig_status hs;
        if ((rc = zig_status_read(ctx->stream, rd.st, what, hs))) return rc;
        if (hs.total >= n) {
            *n_raw = hs.n_raw;
            return 0;
        }
        pos0 += (unsigned long long)rd.nblk * ZIG_BLK + hs.k_last;
        ord0 = hs.total;
    }
    corahip_set_error("%s: no convergence", what);
    return CORAHIP_ESTATE;
}

// values per session of corahip_normal_rows_pcg64
#define ZIG_ROWS_SESSION (1ull << 28)

extern "C" {

int corahip_glibc_exp(corahip_ctx *ctx, const double *x, int64_t n, double *y) {
    ARG_CHECK(ctx != nullptr && n >= 0 && (n == 0 || (x != nullptr && y != nullptr)));
    if (n == 0) return 0;
    glibc_exp_kernel<<<(unsigned)((n + 255) / 256), 256, 0, ctx->stream>>>(x, (long)n, y);
    LAUNCH_CHECK();
    return 0;
}

int corahip_pcg64_advance(const uint64_t state[2], const uint64_t inc[2], uint64_t delta, uint64_t out_state[2]) {
    ARG_CHECK(state != nullptr && inc != nullptr && out_state != nullptr);
    const u128 s = host_advance(mk128(state[0], state[1]), mk128(inc[0], inc[1]), delta);
    out_state[0] = (uint64_t)(s >> 64);
    out_state[1] = (uint64_t)s;
    return 0;
}

int corahip_normals_pcg64(corahip_ctx *ctx, const uint64_t state[2], const uint64_t inc[2], int64_t n, double *g,
                          uint64_t *n_raw) {
    ARG_CHECK(ctx != nullptr && state != nullptr && inc != nullptr && n >= 0 && n_raw != nullptr);
    ARG_CHECK(n == 0 || g != nullptr);
    *n_raw = 0;
    if (n == 0) return 0;
    if (ctx->draw_pending) {
        corahip_set_error("normals_pcg64: a corahip_draw_alm_numpy_begin session is pending (its tables share this call's scratch)");
        return CORAHIP_ESTATE;
    }
    StageTimer timer(ctx, "normals_pcg64");
    return zig_rounds(ctx, state, inc, (unsigned long long)n, sink_store{g, 0ull}, "normals_pcg64", n_raw);
}

int corahip_normal_rows_pcg64(corahip_ctx *ctx, const uint64_t state[2], const uint64_t inc[2], long nrow, long ncol,
                              const double *scale, const int64_t *row_off, double *out, int accumulate, uint64_t *n_raw) {
    ARG_CHECK(ctx != nullptr && state != nullptr && inc != nullptr && nrow >= 0 && ncol >= 0 && n_raw != nullptr);
    ARG_CHECK(accumulate == 0 || accumulate == 1);
    ARG_CHECK(nrow == 0 || ncol == 0 || ncol <= (long)(0x7fffffffffffffffll / nrow));
    *n_raw = 0;
    if (nrow == 0 || ncol == 0) return 0;
    ARG_CHECK(scale != nullptr && out != nullptr);
    if (ctx->draw_pending) {
        corahip_set_error("normal_rows_pcg64: a corahip_draw_alm_numpy_begin session is pending (its tables share this call's scratch)");
        return CORAHIP_ESTATE;
    }
    StageTimer timer(ctx, "normal_rows_pcg64");
    // whole rows per session, so that the block tables (0.3 bytes per value) stay below ~80 MB; a session ends on a
    // sample boundary and the next continues from the state numpy would be in there: the bits do not depend on the cut
    const long per = std::max<long>(1, (long)(ZIG_ROWS_SESSION / (unsigned long long)ncol));
    uint64_t st[2] = {state[0], state[1]};
    for (long r0 = 0; r0 < nrow; r0 += per) {
        const long nr = std::min<long>(per, nrow - r0);
        sink_rows sink{scale + r0, row_off ? row_off + r0 : nullptr, row_off ? out : out + (size_t)r0 * (size_t)ncol,
                       (unsigned long long)ncol, accumulate, 0ull, 0ull, 0ull, nullptr};
        uint64_t used = 0;
        const int rc = zig_rounds(ctx, st, inc, (unsigned long long)nr * (unsigned long long)ncol, sink, "normal_rows_pcg64", &used);
        if (rc) return rc;
        const u128 s = host_advance(mk128(st[0], st[1]), mk128(inc[0], inc[1]), used);
        st[0] = (uint64_t)(s >> 64);
        st[1] = (uint64_t)s;
        *n_raw += used;
    }
    return 0;
}

}  // extern "C"
