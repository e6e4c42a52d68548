// lsschain.hip - the steps of cora/signal/lss.py around the Zel'dovich step, on fields [n, ncol] (row = slice, float64,
// row-major): Lagrangian bias (GenerateBiasedFieldBase.process, lss.py:556-603), linear dynamics
// (LinearDynamics.process, :862-918), Fingers of God (FingersOfGod.process, :1162-1220) and the map
// (BiasedLSSToMap.process, :944-993), with lssutil's diff2 and lognormal_transform.
//
//   slice_mix_kernel       out = K f, K [n, n]: gemm_nn_128 of mfma_tile.h with M = output slice, N = columns,
//                          K-dimension = input slice, the k ranges below and the 16-byte path for the f tile.  A
//                          workgroup owns 128 output rows x 128 columns; for n <= 128 every element of f leaves HBM
//                          once and every element of out is written once; for larger n the row blocks of a column tile
//                          are neighbours in the grid, so the re-reads of f are served by the L2.  K comes through LDS
//                          from the L2.
//                          Skipping: per block of 16 output rows the host gives the range [klo, khi) of input slices
//                          (multiples of the MFMA depth 4) whose K entries are not all exactly zero; MFMAs outside it
//                          are not issued and chunks of 16 input slices outside the union of the workgroup's ranges
//                          are not loaded.  Skipped terms are exact zeros: for finite f the result is the same with
//                          and without skipping, bit for bit (the remaining products are accumulated in the same
//                          order; adding +0 changes nothing).  A non-finite f in a skipped slice does NOT propagate
//                          (0 * inf would be NaN in a dense product).  No atomics: the sum order is fixed.
//   slice_diff2_kernel     lssutil.diff2 along axis 0 from a host table of coefficients [n][4], rows kept in registers
//                          (every element of f read once), optional fused epilogue (h + s g) + d2 t.
//   slice_moments_*        per-row sum (f - c), sum (f - c)^2 in a fixed order (block partials, ordered final pass)
//   bias_field_kernel      c1 f + c2 (f^2 - m2)
//   lognormal_kernel       (exp(f - hv) - 1) pre rs, into a strided destination
// Rows may be only 8-byte aligned (odd ncol): the streaming kernels use 16-byte accesses when every row start is
// 16-byte aligned and 8-byte ones otherwise.  All element offsets are 64-bit.
#include <type_traits>

#include "common.h"
#include "glibc_exp.h"
#include "mfma_tile.h"

namespace {

// vec: ncol even and f 16-byte aligned, so that the f tile can be read 16 bytes per lane
__global__ void __launch_bounds__(GT_NT, 2)
slice_mix_kernel(const double *__restrict__ K, const double *__restrict__ f, const int *__restrict__ rng, int n, long ncol,
                 int nrb, int vec, double *__restrict__ out) {
    const int rb = (int)(blockIdx.x % (unsigned)nrb);
    const long cb = (long)(blockIdx.x / (unsigned)nrb);
    const int row0 = rb * GT_T;
    const int wr = wave_roles<4, 4>().wr;
    const int n4 = (n + 3) & ~3;

    // ranges of the wave's 16-row tiles (wave-uniform) and their union over the workgroup's eight
    int klo[4], khi[4], blo = n4, bhi = 0;
#pragma unroll
    for (int t = 0; t < GT_T / 16; t++) {
        const int r16 = row0 + 16 * t;
        int lo = 0, hi = 0;
        if (r16 < n) {
            lo = rng ? rng[2 * (r16 >> 4)] : 0;
            hi = rng ? rng[2 * (r16 >> 4) + 1] : n4;
            lo = max(0, lo) & ~3;
            hi = min(n4, (hi + 3) & ~3);
            if (hi > lo) blo = min(blo, lo), bhi = max(bhi, hi);
        }
#pragma unroll
        for (int u = 0; u < 4; u++)
            if (t == (wr >> 4) + u) klo[u] = lo, khi[u] = hi;
    }
#pragma unroll
    for (int u = 0; u < 4; u++) {
        klo[u] = __builtin_amdgcn_readfirstlane(klo[u]);
        khi[u] = __builtin_amdgcn_readfirstlane(khi[u]);
    }
    // chunks of 16 input slices outside the union are not loaded
    const int kbeg = blo / GT_K * GT_K;
    const int nchunk = bhi > blo ? (bhi - kbeg + GT_K - 1) / GT_K : 0;
    gemm_nn_128<true, true, long>(K, n, f, ncol, out, ncol, row0, cb * GT_T, n, ncol, n, kbeg, nchunk, klo, khi, vec);
}

template <int V> struct vec_of { typedef double type; };
template <> struct vec_of<2> { typedef double2 type; };

// every product and sum rounded on its own (the reference's numpy statements), no contraction into FMAs
__device__ inline double d2_row(double c0, double c1, double c2, double c3, double w0, double w1, double w2, double w3) {
#pragma clang fp contract(off)
    return ((c0 * w0 + c1 * w1) + c2 * w2) + c3 * w3;
}
__device__ inline double lin_row(double h, double s, double g, double d2, double t, bool vel) {
#pragma clang fp contract(off)
    const double a = h + s * g;
    return vel ? a + d2 * t : a;
}
__device__ inline double bias_value(double a, double b, double m, double x, bool second) {
#pragma clang fp contract(off)
    return second ? a * x + b * (x * x - m) : a * x;
}

// lssutil.diff2 along axis 0 (+ optional epilogue).  Output row i uses input rows st .. st + 3, st = clamp(i - 2, 0, n - 4)
// (rows 0, 1: 0 .. 3; interior rows 2 .. n - 2: i - 2 .. i + 1; row n - 1: n - 4 .. n - 1), with coef[i] = (c0, c1, c2, c3):
//   d2 = ((c0 w0 + c1 w1) + c2 w2) + c3 w3, every product and sum rounded on its own.
// The interior rows of the reference are ((alpha f[i-2] + beta f[i-1]) - (alpha + beta + gamma) f[i]) + gamma f[i+1]: the
// host stores c2 = -(alpha + beta + gamma), and x + (-s) y == x - s y exactly.  A thread walks the rows of its column(s)
// with the four rows of the window and the next one in registers.
// f == NULL (needs g, h): no stencil term, out = h + s g.  g, h != NULL: out = (h + s[i] g) + d2 t[i].
template <int V>
__global__ void __launch_bounds__(256)
slice_diff2_kernel(const double *__restrict__ f, const double *__restrict__ coef, const double *g, const double *h,
                   const double *__restrict__ s, const double *__restrict__ t, int n, long ncol, double *out) {
    typedef typename vec_of<V>::type vec;
    const long nv = ncol / V;
    for (long p = (long)blockIdx.x * blockDim.x + threadIdx.x; p < nv; p += (long)gridDim.x * blockDim.x) {
        const vec *src = reinterpret_cast<const vec *>(f) + p;
        const vec *gs = reinterpret_cast<const vec *>(g) + p, *hs = reinterpret_cast<const vec *>(h) + p;
        vec *dst = reinterpret_cast<vec *>(out) + p;
        vec w0 = {}, w1 = {}, w2 = {}, w3 = {}, nxt = {};
        int cur = 0;
        if (f) {
            w0 = src[0], w1 = src[(size_t)nv], w2 = src[(size_t)2 * nv], w3 = src[(size_t)3 * nv];
            if (n > 4) nxt = src[(size_t)4 * nv];
        }
        for (int i = 0; i < n; i++) {
            vec r = {};
            if (f) {
                const int st = min(max(i - 2, 0), n - 4);
                if (st > cur) {
                    w0 = w1, w1 = w2, w2 = w3, w3 = nxt;
                    cur++;
                    if (cur + 4 < n) nxt = src[(size_t)(cur + 4) * nv];      // in flight while row i is formed
                }
                const double c0 = coef[4 * i], c1 = coef[4 * i + 1], c2 = coef[4 * i + 2], c3 = coef[4 * i + 3];
                if constexpr (V == 2)
                    r = make_double2(d2_row(c0, c1, c2, c3, w0.x, w1.x, w2.x, w3.x), d2_row(c0, c1, c2, c3, w0.y, w1.y, w2.y, w3.y));
                else
                    r = d2_row(c0, c1, c2, c3, w0, w1, w2, w3);
            }
            if (g) {
                const vec gv = gs[(size_t)i * nv], hv = hs[(size_t)i * nv];
                const double si = s[i], ti = f ? t[i] : 0.0;
                if constexpr (V == 2)
                    r = make_double2(lin_row(hv.x, si, gv.x, r.x, ti, f != nullptr), lin_row(hv.y, si, gv.y, r.y, ti, f != nullptr));
                else
                    r = lin_row(hv, si, gv, r, ti, f != nullptr);
            }
            dst[(size_t)i * nv] = r;
        }
    }
}

// partial sums of row i over the columns [b per, (b + 1) per): work[(i nb + b) 2 + (0, 1)] = sum (f - c), sum (f - c)^2.
// Fixed order: a thread adds its strided elements in sequence, then block_sum2.
template <int V>
__global__ void __launch_bounds__(256)
slice_moments_partial_kernel(const double *__restrict__ f, long ld, const double *__restrict__ c, int n, long ncol, int nb,
                             long per, double *__restrict__ work) {
    typedef typename vec_of<V>::type vec;
    const int i = (int)(blockIdx.x / (unsigned)nb), b = (int)(blockIdx.x % (unsigned)nb);
    const long lo = (long)b * per, hi = min(ncol, lo + per);
    const double ci = c ? c[i] : 0.0;
    const double *row = f + (size_t)i * (size_t)ld;
    double s1 = 0.0, s2 = 0.0;
    {
#pragma clang fp contract(off)
        for (long p = lo + (long)threadIdx.x * V; p < hi; p += 256 * V) {
            if constexpr (V == 2) {
                const vec x = *reinterpret_cast<const vec *>(row + p);
                const double dx = x.x - ci, dy = x.y - ci;
                s1 = s1 + (dx + dy);
                s2 = s2 + (dx * dx + dy * dy);
            } else {
                const double dx = row[p] - ci;
                s1 = s1 + dx;
                s2 = s2 + dx * dx;
            }
        }
    }
    __shared__ double red[8];
    block_sum2(s1, s2, red);
    if (threadIdx.x == 0) work[(size_t)blockIdx.x * 2] = s1, work[(size_t)blockIdx.x * 2 + 1] = s2;
}

__global__ void __launch_bounds__(256)
slice_moments_final_kernel(const double *__restrict__ work, int n, int nb, double *__restrict__ sum1,
                           double *__restrict__ sum2) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double s1 = 0.0, s2 = 0.0;
    for (int b = 0; b < nb; b++) {
        s1 += work[((size_t)i * nb + b) * 2];
        s2 += work[((size_t)i * nb + b) * 2 + 1];
    }
    sum1[i] = s1;
    sum2[i] = s2;
}

// out = c1[i] f + c2[i] (f f - m2[i]) (c2 == NULL: exactly c1[i] f); the reference's statement order
// (lss.py:582-592), products and sums rounded one by one
template <int V>
__global__ void __launch_bounds__(256)
bias_field_kernel(const double *f, const double *__restrict__ c1, const double *__restrict__ c2,
                  const double *__restrict__ m2, int n, long ncol, double *out) {
    typedef typename vec_of<V>::type vec;
    const long nv = ncol / V;
    for (long p = (long)blockIdx.x * blockDim.x + threadIdx.x; p < nv; p += (long)gridDim.x * blockDim.x) {
        const vec *src = reinterpret_cast<const vec *>(f) + p;
        vec *dst = reinterpret_cast<vec *>(out) + p;
#pragma unroll 4
        for (int i = 0; i < n; i++) {
            const vec x = src[(size_t)i * nv];
            const double a = c1[i];
            const double b = c2 ? c2[i] : 0.0, m = c2 ? m2[i] : 0.0;
            vec r;
            if constexpr (V == 2)
                r = make_double2(bias_value(a, b, m, x.x, c2 != nullptr), bias_value(a, b, m, x.y, c2 != nullptr));
            else
                r = bias_value(a, b, m, x, c2 != nullptr);
            dst[(size_t)i * nv] = r;
        }
    }
}

__device__ inline double ln_value(double x, double hv, bool tr, double pre, double rs) {
#pragma clang fp contract(off)
    double v = x;
    if (tr) {
        const double a = x - hv;
        // glibc_exp_fma holds for |a| < 512; beyond it (and for NaN) the device's own exp gives the limits
        v = (fabs(a) < 512.0 ? glibc_exp_fma(a) : exp(a)) - 1.0;
    }
    return (v * pre) * rs;
}

// out[i ld_out + p] = ((exp(f[i ncol + p] - hv[i]) - 1) pre) rs[i]; hv == NULL: no transform (copy), rs == NULL: 1
template <int V>
__global__ void __launch_bounds__(256)
lognormal_kernel(const double *f, const double *__restrict__ hv, const double *__restrict__ rs, double pre, int n,
                 long ncol, long ld_out, double *out) {
    typedef typename vec_of<V>::type vec;
    const long nv = ncol / V, ldv = ld_out / V;
    for (long p = (long)blockIdx.x * blockDim.x + threadIdx.x; p < nv; p += (long)gridDim.x * blockDim.x) {
        const vec *src = reinterpret_cast<const vec *>(f) + p;
        vec *dst = reinterpret_cast<vec *>(out) + p;
#pragma unroll 2
        for (int i = 0; i < n; i++) {
            const vec x = src[(size_t)i * nv];
            const double hvi = hv ? hv[i] : 0.0, rsi = rs ? rs[i] : 1.0;
            vec r;
            if constexpr (V == 2)
                r = make_double2(ln_value(x.x, hvi, hv != nullptr, pre, rsi), ln_value(x.y, hvi, hv != nullptr, pre, rsi));
            else
                r = ln_value(x, hvi, hv != nullptr, pre, rsi);
            dst[(size_t)i * ldv] = r;
        }
    }
}

}  // namespace

extern "C" {

int corahip_slice_mix(corahip_ctx *ctx, const double *K, const double *f, const int32_t *ranges, int n, long ncol,
                      double *out) {
    ARG_CHECK(ctx && K && f && out && n >= 1 && n <= 4096 && ncol >= 1);
    ARG_CHECK(is_aligned(K, 8) && is_aligned(f, 8) && is_aligned(out, 8));
    ARG_CHECK(ranges == nullptr || is_aligned(ranges, 4));
    const size_t nbytes = (size_t)n * (size_t)ncol * 8;
    ARG_CHECK(!overlaps(out, nbytes, f, nbytes) && !overlaps(out, nbytes, K, (size_t)n * n * 8));
    const long nrb = (n + GT_T - 1) / GT_T, ncb = (ncol + GT_T - 1) / GT_T;
    ARG_CHECK(nrb * ncb <= 0x7fffffffL);
    StageTimer t(ctx, "slice_mix");
    const int vec = (ncol & 1) == 0 && is_aligned(f, 16);
    hipLaunchKernelGGL(slice_mix_kernel, dim3((unsigned)(nrb * ncb)), dim3(GT_NT), 0, ctx->stream, K, f, ranges, n, ncol,
                       (int)nrb, vec, out);
    LAUNCH_CHECK();
    return 0;
}

int corahip_slice_diff2(corahip_ctx *ctx, const double *f, const double *coef, const double *g, const double *h,
                        const double *s, const double *t, int n, long ncol, double *out) {
    ARG_CHECK(ctx && out && n >= 1 && ncol >= 1);
    ARG_CHECK((g == nullptr) == (h == nullptr));
    ARG_CHECK(f != nullptr || g != nullptr);
    ARG_CHECK(f == nullptr || (coef != nullptr && n >= 4));
    ARG_CHECK(g == nullptr || (s != nullptr && (f == nullptr || t != nullptr)));
    ARG_CHECK(is_aligned(f, 8) && is_aligned(g, 8) && is_aligned(h, 8) && is_aligned(out, 8));
    const size_t nbytes = (size_t)n * (size_t)ncol * 8;
    ARG_CHECK(f == nullptr || !overlaps(out, nbytes, f, nbytes));
    StageTimer tm(ctx, "slice_diff2");
    const bool v2 = (ncol & 1) == 0 && is_aligned(f, 16) && is_aligned(g, 16) && is_aligned(h, 16) && is_aligned(out, 16);
    const long nv = v2 ? ncol / 2 : ncol;
    const unsigned blocks = grid_blocks(ctx, nv, 32);
    if (v2)
        hipLaunchKernelGGL(slice_diff2_kernel<2>, dim3(blocks), dim3(256), 0, ctx->stream, f, coef, g, h, s, t, n,
                           ncol, out);
    else
        hipLaunchKernelGGL(slice_diff2_kernel<1>, dim3(blocks), dim3(256), 0, ctx->stream, f, coef, g, h, s, t, n,
                           ncol, out);
    LAUNCH_CHECK();
    return 0;
}

int corahip_slice_moments_workspace_bytes(int n, long ncol, size_t *bytes) {
    ARG_CHECK(bytes && n >= 1 && ncol >= 1);
    int nb;
    long per;
    partials_split(ncol, 2, &nb, &per);     // per even: the 16-byte path reads pairs
    *bytes = (size_t)n * nb * 2 * sizeof(double);
    return 0;
}

int corahip_slice_moments(corahip_ctx *ctx, const double *f, long ld, const double *c, int n, long ncol, void *work,
                          size_t work_bytes, double *sum1, double *sum2) {
    ARG_CHECK(ctx && f && work && sum1 && sum2 && n >= 1 && ncol >= 1 && ld >= ncol);
    ARG_CHECK(is_aligned(f, 8) && is_aligned(work, 8));
    int nb;
    long per;
    partials_split(ncol, 2, &nb, &per);     // per even: the 16-byte path reads pairs
    ARG_CHECK(work_bytes >= (size_t)n * nb * 2 * sizeof(double));
    ARG_CHECK((long)n * nb <= 0x7fffffffL);
    StageTimer t(ctx, "slice_moments");
    const bool v2 = (ncol & 1) == 0 && (ld & 1) == 0 && is_aligned(f, 16);
    if (v2)
        hipLaunchKernelGGL(slice_moments_partial_kernel<2>, dim3((unsigned)((long)n * nb)), dim3(256), 0, ctx->stream, f, ld,
                           c, n, ncol, nb, per, (double *)work);
    else
        hipLaunchKernelGGL(slice_moments_partial_kernel<1>, dim3((unsigned)((long)n * nb)), dim3(256), 0, ctx->stream, f, ld,
                           c, n, ncol, nb, per, (double *)work);
    LAUNCH_CHECK();
    hipLaunchKernelGGL(slice_moments_final_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream,
                       (const double *)work, n, nb, sum1, sum2);
    LAUNCH_CHECK();
    return 0;
}

int corahip_bias_field(corahip_ctx *ctx, const double *f, const double *c1, const double *c2, const double *m2, int n,
                       long ncol, double *out) {
    ARG_CHECK(ctx && f && c1 && out && n >= 1 && ncol >= 1);
    ARG_CHECK((c2 == nullptr) == (m2 == nullptr));
    ARG_CHECK(is_aligned(f, 8) && is_aligned(out, 8));
    const size_t nbytes = (size_t)n * (size_t)ncol * 8;
    ARG_CHECK(out == f || !overlaps(out, nbytes, f, nbytes));
    StageTimer t(ctx, "bias_field");
    const bool v2 = (ncol & 1) == 0 && is_aligned(f, 16) && is_aligned(out, 16);
    const long nv = v2 ? ncol / 2 : ncol;
    const unsigned blocks = grid_blocks(ctx, nv, 32);
    if (v2)
        hipLaunchKernelGGL(bias_field_kernel<2>, dim3(blocks), dim3(256), 0, ctx->stream, f, c1, c2, m2, n, ncol, out);
    else
        hipLaunchKernelGGL(bias_field_kernel<1>, dim3(blocks), dim3(256), 0, ctx->stream, f, c1, c2, m2, n, ncol, out);
    LAUNCH_CHECK();
    return 0;
}

int corahip_lognormal(corahip_ctx *ctx, const double *f, const double *hv, const double *rs, double pre, int n, long ncol,
                      long ld_out, double *out) {
    ARG_CHECK(ctx && f && out && n >= 1 && ncol >= 1 && ld_out >= ncol);
    ARG_CHECK(is_aligned(f, 8) && is_aligned(out, 8));
    // in place (same pointer, same stride) or disjoint
    ARG_CHECK((out == f && ld_out == ncol) ||
              !overlaps(out, ((size_t)(n - 1) * (size_t)ld_out + (size_t)ncol) * 8, f, (size_t)n * (size_t)ncol * 8));
    StageTimer t(ctx, "lognormal");
    const bool v2 = (ncol & 1) == 0 && (ld_out & 1) == 0 && is_aligned(f, 16) && is_aligned(out, 16);
    const long nv = v2 ? ncol / 2 : ncol;
    const unsigned blocks = grid_blocks(ctx, nv, 32);
    if (v2)
        hipLaunchKernelGGL(lognormal_kernel<2>, dim3(blocks), dim3(256), 0, ctx->stream, f, hv, rs, pre, n, ncol,
                           ld_out, out);
    else
        hipLaunchKernelGGL(lognormal_kernel<1>, dim3(blocks), dim3(256), 0, ctx->stream, f, hv, rs, pre, n, ncol,
                           ld_out, out);
    LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
