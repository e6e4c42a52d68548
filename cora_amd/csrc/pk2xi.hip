// pk2xi.hip - P(k) -> xi(r): the kernels behind corrfunc.ps_to_corr
//
// Replaces the two numerical halves of the reference's ps_to_corr (cora/signal/corrfunc.py:189-264):
//   - _corr_direct (corrfunc.py:72-84): scipy.integrate.romb over 2^k + 1 log-spaced wavenumbers of
//     P(k) k^3 / 2 pi^2 sinc(k r) for every small separation r.  The reference builds the [nr, 2^k + 1] integrand
//     (1 GB at the defaults); Romberg is linear in the samples, so here one workgroup per separation keeps k + 1 sums.
//   - _corr_hankl_richardson (corrfunc.py:150-186): hankl.P2xi(k, P, 0, lowring=False), i.e. FFTLog with mu = 1/2,
//     q = 0: g = irfft(rfft(P k^1.5) U) with the unit-modulus Mellin kernel U_m.  The Richardson levels are up to
//     3 584 000 points long; the line FFTs of flatsky.hip stop at 4096, so a long signal is split N = N1 N2 and
//     transformed by the four-step scheme on the [N1, N2] view, which needs no transpose.
#include <cmath>

#include "common.h"

#define PX_THREADS 256
#define PX_MAXK 24          // Romberg order: 2^24 + 1 samples at the most
#define PX_MAXLINE 4096     // longest line corahip_fft_c2c takes (FS_MAXN of flatsky.hip)
#define PX_SHIFT 16         // recurrence shift of lnGamma before the Stirling series

__device__ static inline double sinc_of(double x) { return x == 0.0 ? 1.0 : sin(x) / x; }

// out[j] = dlk * romb_i(g[i] sinc(ka[i] r[j])), i = 0 .. K = 2^k, unit sample spacing (scipy.integrate.romb).
// S[t]: sum of the interior samples whose index has exactly t trailing zero bits; e = (f_0 + f_K) / 2.  The trapezoid
// estimate at stride 2^t is 2^t (e + sum_{s >= t} S[s]); the 4^j table over the k + 1 estimates, coarsest first, is
// scipy's.  Thread tid owns the samples i = tid (mod 256): every sample of a thread other than thread 0 is of class
// ctz(tid) < 8, thread 0 holds the classes >= 8.  Order of every sum: a thread's samples ascending, the threads of a
// class t < 8 (tid = 2^t (2 j + 1), j ascending) two per lane of wave 0 and then halving __shfl_down - a function of
// k alone, so a call repeats its bits.
__global__ void __launch_bounds__(PX_THREADS)
sinc_romb_kernel(const double *__restrict__ g, const double *__restrict__ ka, int k, double dlk,
                 const double *__restrict__ r, double *__restrict__ out) {
    __shared__ double part[PX_THREADS];
    __shared__ double S[PX_MAXK + 1];
    __shared__ double tab[2][PX_MAXK + 1];
    const int tid = threadIdx.x;
    const long K = 1L << k;
    const double rj = r[blockIdx.x];
    if (tid <= PX_MAXK) S[tid] = 0.0;
    __syncthreads();
    double acc = 0.0;
    if (tid) {
        for (long i = tid; i < K; i += PX_THREADS) acc += g[i] * sinc_of(ka[i] * rj);
    } else {
        for (long i = PX_THREADS; i < K; i += PX_THREADS) S[__ffsll((long long)i) - 1] += g[i] * sinc_of(ka[i] * rj);
    }
    part[tid] = acc;
    __syncthreads();
    if (tid < 64) {
        for (int t = 0; t < 8; t++) {
            const int cnt = 128 >> t;
            double v = 0.0;
            for (int j = tid; j < cnt; j += 64) v += part[(2 * j + 1) << t];
#pragma unroll
            for (int o = 32; o >= 1; o >>= 1) v += __shfl_down(v, o, 64);
            if (tid == 0) S[t] = v;
        }
    }
    if (tid == 0) {
        double c = 0.5 * (g[0] * sinc_of(ka[0] * rj) + g[K] * sinc_of(ka[K] * rj));
        int cur = 0;
        for (int i = 0; i <= k; i++, cur ^= 1) {
            if (i) c += S[k - i];
            double *row = tab[cur];
            const double *prv = tab[cur ^ 1];
            row[0] = ldexp(c, k - i);
            double p4 = 1.0;
            for (int j = 1; j <= i; j++) {
                p4 *= 4.0;
                row[j] = row[j - 1] + (row[j - 1] - prv[j - 1]) / (p4 - 1.0);
            }
        }
        out[blockIdx.x] = dlk * tab[cur ^ 1][k];
    }
}

// ---- j_0, j_2, j_4 in one pass ------------------------------------------------------------------------------------
// One sine and one cosine of x serve the three orders.  j_0 = sinc_of(x), the bits of sinc_romb.  j_2 and j_4: above
// the switch argument the closed forms in y = 1 / x,
//   j_2 = ((3 y^2 - 1) sin x - 3 y cos x) y,   j_4 = ((105 y^4 - 45 y^2 + 1) sin x - (105 y^3 - 10 y) cos x) y,
// whose terms are of size 3 / x^2 (105 / x^4) where the result is x^2 / 15 (x^4 / 945): each rounding of a term shows
// in the result, so the absolute error is 6 eps (3 y^3 + 3 y^2 + y) and 7 eps (105 y^5 + 105 y^4 + 45 y^3 + 10 y^2 + y),
// 9.75 eps at x = 2 and 14.7 eps at x = 4 and falling from there.  Below the switch the ascending series
//   j_l = x^l / (2l + 1)!! sum_m prod_{i <= m} (-x^2 / (2 i (2 i + 2 l + 1))),
// Horner in x^2 from the last term in: no cancellation (every ratio is below 1 for x^2 < 2 (2 l + 3)), the first term
// left out is 1.2e-18 (l = 2, 11 terms, x = 2) and 1.6e-18 (l = 4, 13 terms, x = 4) absolutely.  tests/_rsdcorr_oracle.py
// derives the constants and restates the arithmetic.  x = 0: j_0 = 1 and j_2 = j_4 = +0.0.
#define JL_SWITCH2 2.0
#define JL_SWITCH4 4.0
#define JL_TERMS2 11
#define JL_TERMS4 13
#define JL_MAXSPEC 3

template <int L, int NT>
__device__ static inline double jl_series(double x2) {
    double acc = 1.0;
#pragma unroll
    for (int m = NT; m >= 1; m--) acc = fma(-(x2 * (1.0 / (2.0 * m * (2.0 * m + 2 * L + 1)))), acc, 1.0);
    return acc;
}

__device__ static inline void jl_024(double x, double &j0, double &j2, double &j4) {
    j0 = sinc_of(x);                               // sinc_romb's own function: the l = 0 slot has its bits by construction
    const double s = sin(x), c = cos(x);           // (the sine is the one sinc_of has just computed: same call, same argument)
    const double ax = fabs(x), x2 = x * x;
    const double y = 1.0 / x, y2 = y * y;          // (inf at x = 0: only the series branches are taken there)
    if (ax < JL_SWITCH2) j2 = x2 * (1.0 / 15.0) * jl_series<2, JL_TERMS2>(x2);
    else j2 = (fma(3.0, y2, -1.0) * s - 3.0 * y * c) * y;
    if (ax < JL_SWITCH4) j4 = (x2 * x2) * (1.0 / 945.0) * jl_series<4, JL_TERMS4>(x2);
    else j4 = (fma(fma(105.0, y2, -45.0), y2, 1.0) * s - fma(105.0, y2, -10.0) * y * c) * y;
}

// out[s][i][j] = dlk * romb_n(g[s][n] j_{2i}(ka[n] r[j])): sinc_romb_kernel with 3 NS accumulators per thread - the same
// ownership of the samples, the same class sums, the same table, per slot q = 3 s + i; thread q runs the table of slot q.
// A slot whose bit in lmask[s] is clear is written as +0.0, and so are the l = 2, 4 slots at r = 0.
struct jl_masks {
    int m[JL_MAXSPEC];
};

template <int NS>
__global__ void __launch_bounds__(PX_THREADS)
jl_romb_kernel(const double *__restrict__ g, jl_masks lmask, const double *__restrict__ ka, int k, double dlk,
               const double *__restrict__ r, int nr, double *__restrict__ out) {
    constexpr int NQ = 3 * NS;
    __shared__ double part[NQ][PX_THREADS];
    __shared__ double S[NQ][PX_MAXK + 1];
    __shared__ double tab[NQ][2][PX_MAXK + 1];
    const int tid = threadIdx.x;
    const long K = 1L << k;
    const double rj = r[blockIdx.x];
    for (int e = tid; e < NQ * (PX_MAXK + 1); e += PX_THREADS) S[e / (PX_MAXK + 1)][e % (PX_MAXK + 1)] = 0.0;
    __syncthreads();
    double acc[NQ];
#pragma unroll
    for (int q = 0; q < NQ; q++) acc[q] = 0.0;
    if (tid) {
        for (long i = tid; i < K; i += PX_THREADS) {
            double j[3];
            jl_024(ka[i] * rj, j[0], j[1], j[2]);
#pragma unroll
            for (int q = 0; q < NQ; q++) acc[q] += g[(q / 3) * (K + 1) + i] * j[q % 3];
        }
    } else {
        for (long i = PX_THREADS; i < K; i += PX_THREADS) {
            double j[3];
            jl_024(ka[i] * rj, j[0], j[1], j[2]);
            const int t = __ffsll((long long)i) - 1;
#pragma unroll
            for (int q = 0; q < NQ; q++) S[q][t] += g[(q / 3) * (K + 1) + i] * j[q % 3];
        }
    }
#pragma unroll
    for (int q = 0; q < NQ; q++) part[q][tid] = acc[q];
    __syncthreads();
    if (tid < 64) {
#pragma unroll
        for (int q = 0; q < NQ; q++) {
            for (int t = 0; t < 8; t++) {
                const int cnt = 128 >> t;
                double v = 0.0;
                for (int j = tid; j < cnt; j += 64) v += part[q][(2 * j + 1) << t];
#pragma unroll
                for (int o = 32; o >= 1; o >>= 1) v += __shfl_down(v, o, 64);
                if (tid == 0) S[q][t] = v;
            }
        }
    }
    __syncthreads();
    if (tid < NQ) {
        const int s = tid / 3, l = tid % 3;
        const double *gs = g + (size_t)s * (K + 1);
        double j0[3], jK[3];
        jl_024(ka[0] * rj, j0[0], j0[1], j0[2]);
        jl_024(ka[K] * rj, jK[0], jK[1], jK[2]);
        double c = 0.5 * (gs[0] * j0[l] + gs[K] * jK[l]);
        int cur = 0;
        for (int i = 0; i <= k; i++, cur ^= 1) {
            if (i) c += S[tid][k - i];
            double *row = tab[tid][cur];
            const double *prv = tab[tid][cur ^ 1];
            row[0] = ldexp(c, k - i);
            double p4 = 1.0;
            for (int j = 1; j <= i; j++) {
                p4 *= 4.0;
                row[j] = row[j - 1] + (row[j - 1] - prv[j - 1]) / (p4 - 1.0);
            }
        }
        const bool on = ((lmask.m[s] >> l) & 1) && !(l > 0 && rj == 0.0);
        out[(size_t)tid * nr + blockIdx.x] = on ? dlk * tab[tid][cur ^ 1][k] : 0.0;
    }
}

__device__ static inline double2 px_cmul(double2 a, double2 b) {
    return make_double2(fma(a.x, b.x, -a.y * b.y), fma(a.x, b.y, a.y * b.x));
}

// u[m] = exp(i theta_m), theta_m = eta ln 2 + 2 Im lnGamma((mu + 1 + i eta) / 2), eta = 2 pi m / L: the Mellin kernel
// 2^{i eta} Gamma((mu + 1 + i eta) / 2) / Gamma((mu + 1 - i eta) / 2) of FFTLog at q = 0, which has modulus one.
// Im lnGamma(z) = Im lnGamma(z + n) - sum_{j < n} arg(z + j) with n = PX_SHIFT, then Stirling at w = z + n, |w| >= 16:
//   Im[(w - 1/2) ln w - w] + Im sum_{k = 1..7} B_2k / (2k (2k - 1) w^(2k - 1));  the first term left out is
//   B_16 / (240 w^15), below 2.6e-20.  eta = 0 gives theta = 0 and u = 1 exactly.
__global__ void fftlog_phase_kernel(double mu, double L, long nh, double2 *__restrict__ u) {
    const double TWO_PI = 6.283185307179586476925286766559, LN2 = 0.693147180559945309417232121458;
    for (long m = (long)blockIdx.x * blockDim.x + threadIdx.x; m < nh; m += (long)gridDim.x * blockDim.x) {
        const double eta = TWO_PI * (double)m / L;
        const double x = 0.5 * (mu + 1.0), y = 0.5 * eta;
        double sa = 0.0;
        for (int j = 0; j < PX_SHIFT; j++) sa += atan2(y, x + (double)j);
        const double xw = x + (double)PX_SHIFT;
        const double r2 = fma(xw, xw, y * y);
        const double lnabs = 0.5 * log(r2), arg = atan2(y, xw);
        const double2 iw = make_double2(xw / r2, -y / r2), iw2 = px_cmul(iw, iw);
        double2 s = make_double2(1.0 / 156.0, 0.0);
        s = px_cmul(s, iw2), s.x += -691.0 / 360360.0;
        s = px_cmul(s, iw2), s.x += 1.0 / 1188.0;
        s = px_cmul(s, iw2), s.x += -1.0 / 1680.0;
        s = px_cmul(s, iw2), s.x += 1.0 / 1260.0;
        s = px_cmul(s, iw2), s.x += -1.0 / 360.0;
        s = px_cmul(s, iw2), s.x += 1.0 / 12.0;
        s = px_cmul(s, iw);
        const double im = (xw - 0.5) * arg + y * (lnabs - 1.0) + s.y;
        const double theta = eta * LN2 + 2.0 * (im - sa);
        double sn, cs;
        sincos(theta, &sn, &cs);
        u[m] = make_double2(cs, sn);
    }
}

// element [k1, n2] of the [N1, N2] view times omega_N^{k1 n2} (conj = 0: e^{-2 pi i k1 n2 / N}; 1: its conjugate).
// The angle is 2 pi p / N with p = k1 n2 < N an exact integer, folded to |p| <= N / 2 before the one rounding.
__global__ void logconv_twiddle_kernel(double2 *__restrict__ d, long N, int N2, int conj) {
    for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < N; e += (long)gridDim.x * blockDim.x) {
        const long k1 = e / N2, n2 = e - k1 * N2;
        long p = k1 * n2;
        if (p == 0) continue;
        if (2 * p > N) p -= N;
        double sn, cs;
        sincospi(2.0 * (double)p / (double)N, &sn, &cs);
        d[e] = px_cmul(d[e], make_double2(cs, conj ? sn : -sn));
    }
}

// element [k1, k2] holds mode m = k1 + N1 k2 of a real signal: times U_m, conj U_{N - m} above N / 2; the imaginary
// parts of the DC and (even N) Nyquist products are dropped as numpy.fft.irfft drops them
__global__ void logconv_mul_kernel(double2 *__restrict__ d, const double2 *__restrict__ u, long N, int N1, int N2) {
    for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < N; e += (long)gridDim.x * blockDim.x) {
        const long k1 = e / N2, k2 = e - k1 * N2;
        const long m = k1 + (long)N1 * k2;
        double2 w;
        if (2 * m <= N) {
            w = u[m];
        } else {
            w = u[N - m];
            w.y = -w.y;
        }
        double2 p = px_cmul(d[e], w);
        if (m == 0 || 2 * m == N) p.y = 0.0;
        d[e] = p;
    }
}

// cost of one line-FFT pass in butterfly stages: log2 n for a power of two, three transforms of the Bluestein length else
static int px_pass_cost(long n) {
    int lg = 0;
    if ((n & (n - 1)) == 0) {
        while ((1L << lg) < n) lg++;
        return lg;
    }
    while ((1L << lg) < 2 * n - 1) lg++;
    return 3 * lg;
}

extern "C" {

int corahip_sinc_romb(corahip_ctx *ctx, const double *g, const double *ka, int k, double dlk, const double *r, int nr,
                      double *out) {
    ARG_CHECK(ctx != nullptr && g && ka && r && out && k >= 1 && k <= PX_MAXK && nr >= 0);
    if (nr == 0) return 0;
    StageTimer t(ctx, "sinc_romb");
    sinc_romb_kernel<<<nr, PX_THREADS, 0, ctx->stream>>>(g, ka, k, dlk, r, out);
    LAUNCH_CHECK();
    return 0;
}

int corahip_jl_romb(corahip_ctx *ctx, const double *g, int nspec, const int *lmask, const double *ka, int k, double dlk,
                    const double *r, int nr, double *out) {
    ARG_CHECK(ctx != nullptr && g && lmask && ka && r && out && nr >= 0);
    ARG_CHECK(nspec >= 1 && nspec <= JL_MAXSPEC && k >= 1 && k <= PX_MAXK);
    jl_masks m;
    for (int s = 0; s < JL_MAXSPEC; s++) m.m[s] = s < nspec ? lmask[s] : 0;
    for (int s = 0; s < nspec; s++) ARG_CHECK(m.m[s] >= 0 && m.m[s] <= 7);
    if (nr == 0) return 0;
    StageTimer t(ctx, "jl_romb");
    if (nspec == 1) jl_romb_kernel<1><<<nr, PX_THREADS, 0, ctx->stream>>>(g, m, ka, k, dlk, r, nr, out);
    else if (nspec == 2) jl_romb_kernel<2><<<nr, PX_THREADS, 0, ctx->stream>>>(g, m, ka, k, dlk, r, nr, out);
    else jl_romb_kernel<3><<<nr, PX_THREADS, 0, ctx->stream>>>(g, m, ka, k, dlk, r, nr, out);
    LAUNCH_CHECK();
    return 0;
}

int corahip_fftlog_phase(corahip_ctx *ctx, double mu, double L, int64_t N, double *u) {
    ARG_CHECK(ctx != nullptr && u && N >= 1 && mu > -1.0 && L > 0.0);
    StageTimer t(ctx, "fftlog_phase");
    const long nh = N / 2 + 1;
    fftlog_phase_kernel<<<grid_blocks(ctx, nh), 256, 0, ctx->stream>>>(mu, L, nh, reinterpret_cast<double2 *>(u));
    LAUNCH_CHECK();
    return 0;
}

int corahip_logconv_split(int64_t N, int *N1, int *N2) {
    ARG_CHECK(N1 && N2 && N >= 1);
    if (N <= PX_MAXLINE) {
        *N1 = (int)N, *N2 = 1;
        return 0;
    }
    int best = -1;
    for (long a = 2; a <= PX_MAXLINE; a++) {
        if (N % a || N / a > PX_MAXLINE) continue;
        const long b = N / a;
        // at equal cost the power of two goes to the contiguous axis: the strided passes have the tuned Bluestein route
        const int c = 2 * (px_pass_cost(a) + px_pass_cost(b)) + ((b & (b - 1)) ? 1 : 0);
        if (best < 0 || c < best) best = c, *N1 = (int)a, *N2 = (int)b;
    }
    if (best < 0) {
        corahip_set_error("invalid argument: N = %ld has no split N1 N2 with both factors <= %d (%s:%d)", (long)N,
                          PX_MAXLINE, __FILE__, __LINE__);
        return CORAHIP_EINVAL;
    }
    return 0;
}

int corahip_logconv(corahip_ctx *ctx, double *data, const double *u, int64_t N, int N1, int N2) {
    ARG_CHECK(ctx != nullptr && data && u && N >= 1 && N1 >= 1 && N2 >= 1 && N1 <= PX_MAXLINE && N2 <= PX_MAXLINE);
    ARG_CHECK((int64_t)N1 * N2 == N);
    StageTimer t(ctx, "logconv");
    double2 *d = reinterpret_cast<double2 *>(data);
    const double2 *u2 = reinterpret_cast<const double2 *>(u);
    const unsigned blocks = grid_blocks(ctx, N);
    int rc;
    if (N1 == 1 || N2 == 1) {         // one pass each way
        const int64_t dims[1] = {N};
        if ((rc = corahip_fft_c2c(ctx, data, 1, dims, 0, 0))) return rc;
        logconv_mul_kernel<<<blocks, 256, 0, ctx->stream>>>(d, u2, N, (int)N, 1);
        LAUNCH_CHECK();
        return corahip_fft_c2c(ctx, data, 1, dims, 0, 1);
    }
    const int64_t dims[2] = {N1, N2};
    if ((rc = corahip_fft_c2c(ctx, data, 2, dims, 0, 0))) return rc;
    logconv_twiddle_kernel<<<blocks, 256, 0, ctx->stream>>>(d, N, N2, 0);
    LAUNCH_CHECK();
    if ((rc = corahip_fft_c2c(ctx, data, 2, dims, 1, 0))) return rc;
    logconv_mul_kernel<<<blocks, 256, 0, ctx->stream>>>(d, u2, N, N1, N2);
    LAUNCH_CHECK();
    if ((rc = corahip_fft_c2c(ctx, data, 2, dims, 1, 1))) return rc;
    logconv_twiddle_kernel<<<blocks, 256, 0, ctx->stream>>>(d, N, N2, 1);
    LAUNCH_CHECK();
    return corahip_fft_c2c(ctx, data, 2, dims, 0, 1);
}

}  // extern "C"
