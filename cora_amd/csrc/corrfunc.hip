// corrfunc.hip - xi(r) -> C_l(chi, chi'): replaces corrfunc.corr_to_clarray
// (cora/signal/corrfunc.py:290-400) for correlation functions given as cubic-spline tables
// (cora/util/cubicspline.pyx Interpolater / LogInterpolater / SinhInterpolater), and its Legendre
// projection  C_l = sum_m (w_m 4 pi / wsum) P_l(mu_m) xi_m  (corrfunc.py:387-397) for any input.
//
//   xi_table_kernel      [mu][i][j >= i]: radial-bin average of the spline at r(mu, x_i + a, x_j + b)
//   xi_multi_kernel      the same for up to 4 tables on shared knots at once, [mu][table][packed i <= j], tables read from
//                        interval records in global memory (no knot limit from LDS); cl_blocks_kernel unpacks / assembles
//   legendre_matrix      lm[l][m] = weight_m P_l(mu_m) by the three-term recurrence (one thread per node)
//   dgemm_nn_kernel      C[L x N] = A[L x M] B[M x N] on FP64 MFMA: gemm_nn_128 of mfma_tile.h as it is
#include "common.h"
#include "mfma_tile.h"
#include "spline_dev.h"

#include "rng_dev.h"   // fast_log01, fast_sqrt_pos (both hold their accuracy over every positive normal argument met here)

// natural cubic spline with end-slope extrapolation, as cubicspline.pyx:126-175.  Knot tables in LDS:
// xs, ys, y2 and per interval 1/h and h^2/6 (no divisions per evaluation); the interval comes from a uniform
// look-up grid over [xs[0], xs[n-1]] (lut[g] = last knot at or before the left edge of cell g) walked forward to
// the reference's bisection result - the last knot with xs[k] <= x - instead of ~log2(n) dependent LDS reads.
struct spline_lds {
    const double *xs, *ys, *y2, *invh, *h2o6;
    const int *lut;
    int n, nlut;
    double x0, inv_dx;
};
// the three expressions of one evaluation and the bisection of a look-up cell: spline_dev.h
// interval of xs[0] <= x < xs[n-1]: the last knot with xs[k] <= x, from the look-up cell walked both ways;
// knot(k) = xs[k], next(k) = xs[k + 1]
template <class Knot, class Next>
__device__ static inline int spline_interval(Knot knot, Next next, const int *lut, int n, int nlut, double x0,
                                             double inv_dx, double x) {
    int g = (int)((x - x0) * inv_dx);
    g = g < 0 ? 0 : (g >= nlut ? nlut - 1 : g);
    int kl = lut[g];
    while (kl > 0 && knot(kl) > x) kl--;            // (rounding of the cell index at a cell edge)
    while (kl + 2 < n && next(kl) <= x) kl++;
    return kl;
}
__device__ static inline double spline_eval(const spline_lds &S, double x) {
    const int n = S.n;
    if (x < S.xs[0]) return spline_below(S.xs[0], S.xs[1], S.ys[0], S.ys[1], S.y2[1], x);
    if (x >= S.xs[n - 1]) return spline_above(S.xs[n - 2], S.xs[n - 1], S.ys[n - 2], S.ys[n - 1], S.y2[n - 2], x);
    const int kl = spline_interval([&](int k) { return S.xs[k]; }, [&](int k) { return S.xs[k + 1]; }, S.lut, n, S.nlut,
                                   S.x0, S.inv_dx, x);
    return spline_interp(S.xs[kl], S.xs[kl + 1], S.invh[kl], S.h2o6[kl], S.ys[kl], S.ys[kl + 1], S.y2[kl], S.y2[kl + 1], x);
}

// asinh(u), u >= 0: log(u + sqrt(u^2 + 1)) with the short log / sqrt of rng_dev.h (the argument is >= 1, where
// fast_log01 keeps full relative accuracy); below 2^-6 the odd series (the log would cancel)
__device__ static inline double fast_asinh_pos(double u) {
    const double u2 = u * u;
    const double big = fast_log01(u + fast_sqrt_pos(u2 + 1.0));
    const double small = u * (1.0 + u2 * (-1.0 / 6.0 + u2 * (3.0 / 40.0 + u2 * (-15.0 / 336.0 + u2 * (105.0 / 3456.0)))));
    return u < 0.015625 ? small : big;
}
// sinh(y) for |y| < ~700, branch-free: E = expm1(|y|) = 2^k p + (2^k - 1) with p = expm1(r), r = |y| - k ln2
// (|r| <= ln2 / 2, degree-13 Taylor polynomial: remainder 4e-18), sinh = (E + E / (E + 1)) / 2
__device__ static inline double fast_expm1_pos(double ay) {   // ay >= 0
    const double kf = __builtin_rint(ay * 1.44269504088896340736);
    const double r = fma(-kf, 1.90821492927058770002e-10, fma(-kf, 6.93147180369123816490e-01, ay));   // ln2 hi / lo
    double p = 1.0 / 6227020800.0;
    p = fma(p, r, 1.0 / 479001600.0);
    p = fma(p, r, 1.0 / 39916800.0);
    p = fma(p, r, 1.0 / 3628800.0);
    p = fma(p, r, 1.0 / 362880.0);
    p = fma(p, r, 1.0 / 40320.0);
    p = fma(p, r, 1.0 / 5040.0);
    p = fma(p, r, 1.0 / 720.0);
    p = fma(p, r, 1.0 / 120.0);
    p = fma(p, r, 1.0 / 24.0);
    p = fma(p, r, 1.0 / 6.0);
    p = fma(p, r, 0.5);
    p = fma(p * r, r, r);                       // expm1(r)
    const int k = (int)kf;
    const double two_k = __builtin_amdgcn_ldexp(1.0, k);
    return fma(two_k, p, two_k - 1.0);
}
__device__ static inline double fast_sinh(double y) {
    const double E = fast_expm1_pos(fabs(y));
    const double s = 0.5 * (E + E / (E + 1.0));
    return y < 0.0 ? -s : s;
}
// e^y: the short kernel for |y| < 700; beyond it (2^k or its reciprocal would leave the normal range on the way: the
// subnormal results down to y ~ -745, the last normal ones up to y ~ 709.78, e^{-inf} = 0, NaN) the library's exp
__device__ static inline double fast_exp(double y) {
    const double ay = fabs(y);
    if (!(ay < 700.0)) return exp(y);
    const double E1 = fast_expm1_pos(ay) + 1.0;
    return y < 0.0 ? 1.0 / E1 : E1;
}

// (i, j >= i) from the row-major index p of the packed upper triangle of an F x F matrix
__device__ static inline void pair_decode(long p, int F, int &i, int &j) {
    i = (int)(((2.0 * F + 1.0) - sqrt((2.0 * F + 1.0) * (2.0 * F + 1.0) - 8.0 * (double)p)) * 0.5);
    i = max(0, min(i, F - 1));
    while (i > 0 && (long)i * F - (long)i * (i - 1) / 2 > p) i--;
    while ((long)(i + 1) * F - (long)(i + 1) * i / 2 <= p) i++;
    j = i + (int)(p - ((long)i * F - (long)i * (i - 1) / 2));
}

// kind: 0 plain, 1 log-log (exp(spline(log r))), 2 sinh (f_t sinh(spline(asinh(r / x_t))))
__global__ void __launch_bounds__(256)
xi_table_kernel(const double *__restrict__ kx, const double *__restrict__ ky, const double *__restrict__ ky2, int nk,
                int nlut, int kind, double x_t, double f_t, const double *__restrict__ mu, int nm,
                const double *__restrict__ xa, const double *__restrict__ xw, int F, int xint,
                double *__restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) double sm[];
    double *sx = sm, *sy = sm + nk, *s2 = sm + 2 * nk, *sih = sm + 3 * nk, *sh2 = sm + 4 * nk;
    int *slut = reinterpret_cast<int *>(sm + 5 * nk);
    for (int t = threadIdx.x; t < nk; t += blockDim.x) {
        sx[t] = kx[t];
        sy[t] = ky[t];
        s2[t] = ky2[t];
        if (t + 1 < nk) {
            const double h = kx[t + 1] - kx[t];
            sih[t] = 1.0 / h;
            sh2[t] = (h * h) / 6.0;
        }
    }
    __syncthreads();
    spline_lds S;
    S.xs = sx, S.ys = sy, S.y2 = s2, S.invh = sih, S.h2o6 = sh2, S.lut = slut, S.n = nk, S.nlut = nlut;
    S.x0 = sx[0];
    const double dx = (sx[nk - 1] - sx[0]) / (double)nlut;
    S.inv_dx = 1.0 / dx;
    for (int g = threadIdx.x; g < nlut; g += blockDim.x) {
        slut[g] = spline_lut_cell(sx, nk, S.x0 + g * dx);        // left edge of the cell
    }
    __syncthreads();
    const double inv_xt = 1.0 / x_t;
    const long npair = (long)F * (F + 1) / 2;
    const long total = (long)nm * npair;
    for (long q = (long)blockIdx.x * blockDim.x + threadIdx.x; q < total; q += (long)gridDim.x * blockDim.x) {
        const int m = (int)(q / npair);
        const long p = q - (long)m * npair;
        int i, j;
        pair_decode(p, F, i, j);
        const double om = 1.0 - mu[m];
        double acc = 0.0;
        for (int a = 0; a < xint; a++) {
            const double x1 = xa[i * xint + a];
            double row = 0.0;
            for (int b = 0; b < xint; b++) {
                const double x2 = xa[j * xint + b];
                const double dx12 = x1 - x2;
                // one fma on the rounded product ((2 x1) x2) om - what the compiler contracts the plain expression to,
                // written out so that the host oracle of the tests can restate r bit for bit
                const double r = sqrt(fma(dx12, dx12, 2.0 * x1 * x2 * om));
                double v;
                if (kind == 1) v = fast_exp(spline_eval(S, r > 0.0 ? fast_log01(r) : -INFINITY));
                else if (kind == 2) v = f_t * fast_sinh(spline_eval(S, fast_asinh_pos(r * inv_xt)));
                else v = spline_eval(S, r);
                row += xw[b] * v;
            }
            acc += xw[a] * row;
        }
        out[((size_t)m * F + i) * F + j] = acc;
        out[((size_t)m * F + j) * F + i] = acc;
    }
}

// ---- several tables on shared knots, read through the caches (no knot limit from LDS) ----------------------------
// One record per interval k = 0 .. nk - 2, XI_REC(nfun) doubles: xs_k, xs_{k+1}, 1/h, h^2/6, then per function
// y_k, y_{k+1}, y''_k, y''_{k+1} (three functions: 16 doubles, one 128-byte line), so that an evaluation reads one look-up
// cell and one record.  The end-slope branches read records 0 and nk - 2, which hold every knot value they need.
#define XI_MULTI_MAX 4
#define XI_REC(nfun) (4 + 4 * (nfun))
struct xi_multi_ft {
    double v[XI_MULTI_MAX];
};

__global__ void xi_multi_records_kernel(const double *__restrict__ kx, const double *__restrict__ ky,
                                        const double *__restrict__ ky2, int nk, int nfun, int nlut,
                                        double *__restrict__ rec, int *__restrict__ lut) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < nk - 1) {
        double *R = rec + (size_t)t * XI_REC(nfun);
        const double h = kx[t + 1] - kx[t];
        R[0] = kx[t];
        R[1] = kx[t + 1];
        R[2] = 1.0 / h;
        R[3] = (h * h) / 6.0;
        for (int f = 0; f < nfun; f++) {
            const size_t o = (size_t)f * nk + t;
            R[4 + 4 * f] = ky[o];
            R[5 + 4 * f] = ky[o + 1];
            R[6 + 4 * f] = ky2[o];
            R[7 + 4 * f] = ky2[o + 1];
        }
    }
    if (t < nlut) {
        const double x0 = kx[0];
        const double dx = (kx[nk - 1] - x0) / (double)nlut;
        lut[t] = min(spline_lut_cell(kx, nk, x0 + t * dx), nk - 2);     // (an interval index: the walk ends there anyway)
    }
}

// out [nm_rows, NF, F (F + 1) / 2]: per (node, i, j >= i, a, b) the separation, the abscissa and the interval once, then
// NF evaluations and output transforms; rows nm .. nm_rows - 1 are written as zeros
template <int NF>
__global__ void __launch_bounds__(256)
xi_multi_kernel(const double *__restrict__ rec, const int *__restrict__ lut, int nk, int nlut, int kind, double x_t,
                xi_multi_ft ft, const double *__restrict__ mu, int nm, int nm_rows, const double *__restrict__ xa,
                const double *__restrict__ xw, int F, int xint, double *__restrict__ out) {
    constexpr int RS = XI_REC(NF);
    const double *last = rec + (size_t)(nk - 2) * RS;
    const double xfirst = rec[0], xlast = last[1];
    const double dx = (xlast - xfirst) / (double)nlut;
    const double inv_dx = 1.0 / dx;
    const double inv_xt = 1.0 / x_t;
    const long npair = (long)F * (F + 1) / 2;
    const long total = (long)nm_rows * npair;
    for (long q = (long)blockIdx.x * blockDim.x + threadIdx.x; q < total; q += (long)gridDim.x * blockDim.x) {
        const int m = (int)(q / npair);
        const long p = q - (long)m * npair;
        double *o = out + (size_t)m * NF * npair + p;
        if (m >= nm) {
#pragma unroll
            for (int f = 0; f < NF; f++) o[(size_t)f * npair] = 0.0;
            continue;
        }
        int i, j;
        pair_decode(p, F, i, j);
        const double om = 1.0 - mu[m];
        double acc[NF];
#pragma unroll
        for (int f = 0; f < NF; f++) acc[f] = 0.0;
        for (int a = 0; a < xint; a++) {
            const double x1 = xa[i * xint + a];
            double row[NF];
#pragma unroll
            for (int f = 0; f < NF; f++) row[f] = 0.0;
            for (int b = 0; b < xint; b++) {
                const double x2 = xa[j * xint + b];
                const double dx12 = x1 - x2;
                const double r = sqrt(fma(dx12, dx12, 2.0 * x1 * x2 * om));      // as xi_table_kernel
                double x;
                if (kind == 1) x = r > 0.0 ? fast_log01(r) : -INFINITY;
                else if (kind == 2) x = fast_asinh_pos(r * inv_xt);
                else x = r;
                double s[NF];
                if (x < xfirst) {
#pragma unroll
                    for (int f = 0; f < NF; f++) s[f] = spline_below(rec[0], rec[1], rec[4 + 4 * f], rec[5 + 4 * f], rec[7 + 4 * f], x);
                } else if (x >= xlast) {
#pragma unroll
                    for (int f = 0; f < NF; f++) s[f] = spline_above(last[0], last[1], last[4 + 4 * f], last[5 + 4 * f], last[6 + 4 * f], x);
                } else {
                    const int kl = spline_interval([&](int k) { return rec[(size_t)k * RS]; },
                                                   [&](int k) { return rec[(size_t)k * RS + 1]; }, lut, nk, nlut, xfirst,
                                                   inv_dx, x);
                    const double *R = rec + (size_t)kl * RS;
                    const double xk = R[0], xk1 = R[1], ih = R[2], h2o6 = R[3];
#pragma unroll
                    for (int f = 0; f < NF; f++)
                        s[f] = spline_interp(xk, xk1, ih, h2o6, R[4 + 4 * f], R[5 + 4 * f], R[6 + 4 * f], R[7 + 4 * f], x);
                }
#pragma unroll
                for (int f = 0; f < NF; f++) {
                    double v;
                    if (kind == 1) v = fast_exp(s[f]);
                    else if (kind == 2) v = ft.v[f] * fast_sinh(s[f]);
                    else v = s[f];
                    row[f] += xw[b] * v;
                }
            }
#pragma unroll
            for (int f = 0; f < NF; f++) acc[f] += xw[a] * row[f];
        }
#pragma unroll
        for (int f = 0; f < NF; f++) o[(size_t)f * npair] = acc[f];
    }
}

// packed projection output -> full blocks.  NF = 1: in [L, npair] -> out [L, F, F].  NF = 3: in [L, 3, npair] with the
// slots (delta delta, phi delta, phi phi) -> out [L, 2F, 2F] = [[phi phi, phi delta], [phi delta, delta delta]]
// (lss.py:441-445).  Every value goes to its mirror positions from one register.
template <int NF>
__global__ void cl_blocks_kernel(const double *__restrict__ in, long L, int F, double *__restrict__ out) {
    const long npair = (long)F * (F + 1) / 2;
    const long total = L * npair;
    for (long q = (long)blockIdx.x * blockDim.x + threadIdx.x; q < total; q += (long)gridDim.x * blockDim.x) {
        const long l = q / npair;
        const long p = q - l * npair;
        int ii, jj;
        pair_decode(p, F, ii, jj);
        const size_t i = (size_t)ii, j = (size_t)jj, Fs = (size_t)F;
        const double *src = in + ((size_t)l * NF) * (size_t)npair + (size_t)p;
        if (NF == 1) {
            double *o = out + (size_t)l * Fs * Fs;
            const double v = src[0];
            o[i * Fs + j] = v;
            o[j * Fs + i] = v;
        } else {
            const size_t N = 2 * Fs;
            double *o = out + (size_t)l * N * N;
            const double dd = src[0], pd = src[(size_t)npair], pp = src[2 * (size_t)npair];
            o[i * N + j] = pp;
            o[j * N + i] = pp;
            o[(Fs + i) * N + Fs + j] = dd;
            o[(Fs + j) * N + Fs + i] = dd;
            o[i * N + Fs + j] = pd;
            o[(Fs + j) * N + i] = pd;
            o[j * N + Fs + i] = pd;
            o[(Fs + i) * N + j] = pd;
        }
    }
}

// lm[l][m] = wt[m] * P_l(mu[m]), l = 0..lmax (row stride ldm >= nm, padding columns zero)
__global__ void legendre_matrix_kernel(const double *__restrict__ mu, const double *__restrict__ wt, int nm, int lmax,
                                       int ldm, double *__restrict__ lm) {
    const int m = blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= ldm) return;
    const bool ok = m < nm;
    const double x = ok ? mu[m] : 0.0, w = ok ? wt[m] : 0.0;
    double p0 = 1.0, p1 = x;
    lm[m] = w;
    if (lmax >= 1) lm[(size_t)ldm + m] = w * x;
    for (int l = 2; l <= lmax; l++) {
        const double p2 = ((2.0 * l - 1.0) * x * p1 - (l - 1.0) * p0) / (double)l;
        p0 = p1;
        p1 = p2;
        lm[(size_t)l * ldm + m] = w * p2;
    }
}

// C[Mr x N] = A[Mr x K] B[K x N], row-major (lda, ldb, ldc), K a multiple of 16 (callers pad with zeros): the plain case
// of gemm_nn_128 (mfma_tile.h), one workgroup per 128 x 128 tile of C.
__global__ void __launch_bounds__(256)
dgemm_nn_kernel(const double *__restrict__ A, int lda, const double *__restrict__ B, int ldb, double *__restrict__ C,
                int ldc, int Mr, int N, int K) {
    gemm_nn_128<false, false, int>(A, lda, B, ldb, C, ldc, blockIdx.y * GT_T, blockIdx.x * GT_T, Mr, N, K, 0, K / GT_K,
                              nullptr, nullptr, 0);
}

// LDS of xi_table_kernel per knot: xs, ys, y2, 1/h, h^2/6 (5 doubles) and the 4 look-up cells (4 ints)
#define XI_LDS_PER_KNOT (5 * sizeof(double) + 4 * sizeof(int))

static int xi_lds_bytes(corahip_ctx *ctx, int *bytes) {
    HIP_TRY(hipDeviceGetAttribute(bytes, hipDeviceAttributeMaxSharedMemoryPerBlock, ctx->device));
    return 0;
}

// the largest table xi_multi_average takes: its look-up grid of 4 nk cells is indexed by int
#define XI_MULTI_MAX_KNOTS (1 << 24)

template <int NF>
static void xi_multi_launch(corahip_ctx *ctx, int blocks, const double *rec, const int *lut, int nk, int nlut, int kind,
                            double x_t, const xi_multi_ft &ft, const double *mu, int nm, int nm_rows, const double *xa,
                            const double *xw, int F, int xint, double *out) {
    xi_multi_kernel<NF><<<blocks, 256, 0, ctx->stream>>>(rec, lut, nk, nlut, kind, x_t, ft, mu, nm, nm_rows, xa, xw, F, xint, out);
}

extern "C" {

int corahip_xi_table_max_knots(corahip_ctx *ctx, int *max_knots) {
    ARG_CHECK(ctx != nullptr && max_knots != nullptr);
    int lds = 0;
    if (int rc = xi_lds_bytes(ctx, &lds)) return rc;
    *max_knots = (int)((size_t)lds / XI_LDS_PER_KNOT);
    return 0;
}

int corahip_xi_table_average(corahip_ctx *ctx, const double *knots_x, const double *knots_y, const double *knots_y2,
                             int nk, int kind, double x_t, double f_t, const double *mu, int nm, const double *xa,
                             const double *xw, int F, int xint, double *out) {
    ARG_CHECK(ctx != nullptr && knots_x && knots_y && knots_y2 && mu && xa && xw && out);
    ARG_CHECK(nk >= 4 && kind >= 0 && kind <= 2 && nm >= 1 && F >= 1 && xint >= 1);
    int lds = 0;
    if (int rc = xi_lds_bytes(ctx, &lds)) return rc;
    const int nk_max = (int)((size_t)lds / XI_LDS_PER_KNOT);
    if (nk > nk_max) {   // the whole table lives in the LDS of every workgroup: nothing is launched for one that cannot
        corahip_set_error("invalid argument: nk = %d knots exceed the limit of %d (%d bytes of LDS per workgroup, %d per knot) (%s:%d)",
                          nk, nk_max, lds, (int)XI_LDS_PER_KNOT, __FILE__, __LINE__);
        return CORAHIP_EINVAL;
    }
    StageTimer t(ctx, "xi_average");
    const int nlut = 4 * nk;
    const size_t shm = XI_LDS_PER_KNOT * (size_t)nk;
    HIP_TRY(hipFuncSetAttribute((const void *)xi_table_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shm));
    const long total = (long)nm * F * (F + 1) / 2;
    const int blocks = (int)std::min<long>((total + 255) / 256, (long)ctx->num_cu * 8);
    xi_table_kernel<<<blocks, 256, shm, ctx->stream>>>(knots_x, knots_y, knots_y2, nk, nlut, kind, x_t, f_t, mu, nm, xa, xw,
                                                      F, xint, out);
    LAUNCH_CHECK();
    return 0;
}

int corahip_xi_multi_average(corahip_ctx *ctx, const double *knots_x, const double *knots_y, const double *knots_y2,
                             int nk, int nfun, int kind, double x_t, const double *f_t, const double *mu, int nm,
                             const double *xa, const double *xw, int F, int xint, int nm_rows, double *out) {
    ARG_CHECK(ctx != nullptr && knots_x && knots_y && knots_y2 && f_t && mu && xa && xw && out);
    ARG_CHECK(kind >= 0 && kind <= 2 && nm >= 1 && F >= 1 && xint >= 1);
    if (nfun < 1 || nfun > XI_MULTI_MAX) {
        corahip_set_error("invalid argument: nfun = %d tables, xi_multi_average takes 1 to %d (%s:%d)", nfun, XI_MULTI_MAX,
                          __FILE__, __LINE__);
        return CORAHIP_EINVAL;
    }
    if (nk < 4 || nk > XI_MULTI_MAX_KNOTS) {
        corahip_set_error("invalid argument: nk = %d knots, xi_multi_average takes 4 to %d (%s:%d)", nk, XI_MULTI_MAX_KNOTS,
                          __FILE__, __LINE__);
        return CORAHIP_EINVAL;
    }
    if (nm_rows < nm) {
        corahip_set_error("invalid argument: nm_rows = %d output rows for nm = %d nodes (%s:%d)", nm_rows, nm, __FILE__, __LINE__);
        return CORAHIP_EINVAL;
    }
    ARG_CHECK((long)F * xint <= 0x7fffffffL);
    StageTimer t(ctx, "xi_multi_average");
    const int nlut = 4 * nk;
    const size_t rec_bytes = sizeof(double) * XI_REC(nfun) * (size_t)(nk - 1);
    char *ws = nullptr;
    int rc = corahip_ctx_scratch(ctx, 12, rec_bytes + sizeof(int) * (size_t)nlut, (void **)&ws);
    if (rc) return rc;
    double *rec = reinterpret_cast<double *>(ws);
    int *lut = reinterpret_cast<int *>(ws + rec_bytes);
    xi_multi_records_kernel<<<(nlut + 255) / 256, 256, 0, ctx->stream>>>(knots_x, knots_y, knots_y2, nk, nfun, nlut, rec, lut);
    LAUNCH_CHECK();
    xi_multi_ft ft;
    for (int f = 0; f < XI_MULTI_MAX; f++) ft.v[f] = f < nfun ? f_t[f] : 0.0;
    const long total = (long)nm_rows * ((long)F * (F + 1) / 2);
    const int blocks = (int)std::min<long>((total + 255) / 256, (long)ctx->num_cu * 8);
    if (nfun == 1) xi_multi_launch<1>(ctx, blocks, rec, lut, nk, nlut, kind, x_t, ft, mu, nm, nm_rows, xa, xw, F, xint, out);
    else if (nfun == 2) xi_multi_launch<2>(ctx, blocks, rec, lut, nk, nlut, kind, x_t, ft, mu, nm, nm_rows, xa, xw, F, xint, out);
    else if (nfun == 3) xi_multi_launch<3>(ctx, blocks, rec, lut, nk, nlut, kind, x_t, ft, mu, nm, nm_rows, xa, xw, F, xint, out);
    else xi_multi_launch<4>(ctx, blocks, rec, lut, nk, nlut, kind, x_t, ft, mu, nm, nm_rows, xa, xw, F, xint, out);
    LAUNCH_CHECK();
    return 0;
}

int corahip_cl_blocks(corahip_ctx *ctx, const double *packed, long L, int nfun, int F, double *out) {
    ARG_CHECK(ctx != nullptr && packed && out && L >= 1 && F >= 1);
    if (nfun != 1 && nfun != 3) {
        corahip_set_error("invalid argument: nfun = %d, cl_blocks unpacks 1 function or assembles 3 (%s:%d)", nfun, __FILE__, __LINE__);
        return CORAHIP_EINVAL;
    }
    StageTimer t(ctx, "cl_blocks");
    const long total = L * ((long)F * (F + 1) / 2);
    const unsigned blocks = grid_blocks(ctx, total);
    if (nfun == 1) cl_blocks_kernel<1><<<blocks, 256, 0, ctx->stream>>>(packed, L, F, out);
    else cl_blocks_kernel<3><<<blocks, 256, 0, ctx->stream>>>(packed, L, F, out);
    LAUNCH_CHECK();
    return 0;
}

int corahip_legendre_project(corahip_ctx *ctx, const double *mu, const double *wt, int nm, int lmax, const double *xi,
                             long ncol, double *out) {
    ARG_CHECK(ctx != nullptr && mu && wt && xi && out && nm >= 1 && lmax >= 0 && ncol >= 1);
    StageTimer t(ctx, "legendre_project");
    const int L = lmax + 1;
    const int Kp = (nm + GT_K - 1) / GT_K * GT_K;       // the GEMM runs K in chunks of 16: lm gets zero columns up to Kp
    double *lm = nullptr;
    int rc = corahip_ctx_scratch(ctx, 4, sizeof(double) * (size_t)L * Kp, (void **)&lm);
    if (rc) return rc;
    legendre_matrix_kernel<<<(Kp + 255) / 256, 256, 0, ctx->stream>>>(mu, wt, nm, lmax, Kp, lm);
    LAUNCH_CHECK();
    ARG_CHECK(ncol <= 0x7fffffffL);
    dim3 grid((unsigned)((ncol + GT_T - 1) / GT_T), (L + GT_T - 1) / GT_T);
    const double *Bop = xi;
    if (Kp != nm) {
        // rows nm..Kp-1 of the B operand must exist (and be zero): zero-padded copy of xi
        double *pad = nullptr;
        if ((rc = corahip_ctx_scratch(ctx, 5, sizeof(double) * (size_t)Kp * ncol, (void **)&pad))) return rc;
        HIP_TRY(hipMemcpyAsync(pad, xi, sizeof(double) * (size_t)nm * ncol, hipMemcpyDeviceToDevice, ctx->stream));
        HIP_TRY(hipMemsetAsync(pad + (size_t)nm * ncol, 0, sizeof(double) * (size_t)(Kp - nm) * ncol, ctx->stream));
        Bop = pad;
    }
    dgemm_nn_kernel<<<grid, 256, 0, ctx->stream>>>(lm, Kp, Bop, (int)ncol, out, (int)ncol, L, (int)ncol, Kp);
    LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
