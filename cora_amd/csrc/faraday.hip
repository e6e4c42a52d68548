// faraday.hip - the body of ConstrainedGalaxy.getpolsky (cora/foreground/galaxy.py:209-344) behind its random maps:
// the variance of the depth cube, the fused Faraday-depth -> frequency product, and the packing of synthesised
// maps into the depth cube.  Complex arrays are interleaved (re, im) float64.
//
//   faraday_mix_kernel     P[f, p] = sat(scale / W[p] * sum_phi A[f, phi] e[p, phi] y[p, phi]),
//                          e = exp(-0.25 (phi / sigma[p])^2), W[p] = sum_phi e[p, phi], sat(z) = z tanh|z| / |z|.
//                          FP64 MFMA (v_mfma_f64_16x16x4_f64): M = channel, N = column, K = depth; the complex product
//                          is four real MFMAs per step on (re, im) operand planes, -Im A formed in a register.
//                          A workgroup owns 128 channels x 64 columns (4 waves of 64 x 32: 64 accumulator doubles per
//                          lane; acc_tile, complex_mma and staged_k_loop of mfma_tile.h); depth goes through LDS in
//                          chunks of 8 (chunks of 16 with their staging registers spill).  The weight is formed in the
//                          kernel: the thread that stages y[p, phi] multiplies it by e[p, phi] on the way to LDS
//                          (operand prologue) and keeps the running sum of its e; the normaliser W[p] does not depend
//                          on the summation index, so it is applied with `scale` in the epilogue, where the saturation
//                          and the product with the intensity are done on the accumulators.  Nothing of the size of y
//                          is written.  The channel blocks of a column tile are neighbours in the grid, so for
//                          nfreq > 128 the re-reads of y are served by the L2.  A [nfreq, nphi] comes from the L2.
//                          No atomics; the order of every sum is fixed by the shape alone.
//   cvar_*                 mean and variance of a complex array: block partials, one ordered final pass (twice: the
//                          mean first, then sum |y - m|^2), as slice_moments does.
//   faraday_pack_kernel    [R, npix] -> y[p, off + r]: LDS tile transpose, coalesced on both sides.
// All element offsets are 64-bit.
#include "common.h"
#include "mfma_tile.h"

namespace {

constexpr int FM_BM = 128, FM_BN = 64, FM_KC = 8;     // channels, columns per workgroup; depths per LDS chunk
constexpr int FM_NT = 256;                            // 4 waves: (wave >> 1) picks 64 channels, (wave & 1) 32 columns
constexpr int FM_LS = FM_KC + 1;                      // LDS row stride (doubles): the padding slice_mix uses for K
constexpr int FM_NA = FM_BM * FM_KC / FM_NT;          // complex elements of A a thread stages per chunk (4)
constexpr int FM_NB = FM_BN * FM_KC / FM_NT;          // complex elements of y a thread stages per chunk (2)

__device__ inline double sat_factor(double zr, double zi) {
    const double m = hypot(zr, zi);
    return m > 0.0 ? tanh(m) / m : 0.0;     // z = 0 gives P = 0; a NaN z stays NaN (0 * NaN)
}

// MODE 0: out complex [nfreq, ncol] = P.  MODE 1: out [nfreq, 4, ncol] = (T, Re P T, Im P T, 0).
template <int MODE>
__global__ void __launch_bounds__(FM_NT, 2)
faraday_mix_kernel(const double2 *__restrict__ y, long ncol, int nphi, const double *__restrict__ phi,
                   const double *__restrict__ sigma, const double2 *__restrict__ A, int nfreq, double scale,
                   const double *__restrict__ T, int nfb, double *__restrict__ out) {
    __shared__ double Ars[2][FM_BM * FM_LS], Ais[2][FM_BM * FM_LS];
    __shared__ double Brs[2][FM_BN * FM_LS], Bis[2][FM_BN * FM_LS];
    __shared__ double Wn[FM_BN];
    const wave_roles<4, 2> w;                                       // a wave owns 64 channels x 32 columns
    const int tid = w.tid, ri = w.ri, kq = w.kq, wr = w.wr, wc = w.wc;
    const int fb = (int)(blockIdx.x % (unsigned)nfb);
    const long cb = (long)(blockIdx.x / (unsigned)nfb);
    const int f0 = fb * FM_BM;
    const long col0 = cb * FM_BN;

    // staging: element e = tid + 256 u is (row e / 8, depth e % 8): 8 lanes read one 128-byte run
    constexpr int SR = FM_NT / FM_KC;     // rows per staging step
    const int sk = tid & (FM_KC - 1), sr = tid / FM_KC;
    double isg[FM_NB], esum[FM_NB];
#pragma unroll
    for (int u = 0; u < FM_NB; u++) {
        const long gc = col0 + sr + SR * u;
        isg[u] = gc < ncol ? 1.0 / sigma[gc] : 0.0;
        esum[u] = 0.0;
    }
    double2 ra[FM_NA], rb[FM_NB];
    double rphi = 0.0;
    auto gload = [&](int c) {
        const int k = c * FM_KC + sk;
        const bool kin = k < nphi;
        rphi = kin ? phi[k] : 0.0;
#pragma unroll
        for (int u = 0; u < FM_NA; u++) {
            const int gf = f0 + sr + SR * u;
            ra[u] = (kin && gf < nfreq) ? A[(size_t)gf * (size_t)nphi + (size_t)k] : make_double2(0.0, 0.0);
        }
#pragma unroll
        for (int u = 0; u < FM_NB; u++) {
            const long gc = col0 + sr + SR * u;
            rb[u] = (kin && gc < ncol) ? y[(size_t)gc * (size_t)nphi + (size_t)k] : make_double2(0.0, 0.0);
        }
    };
    // operand prologue: y e on its way to LDS; the staging thread keeps the sum of its e (depths sk, sk + 8, ...)
    auto lstore = [&](int buf, int c) {
        double *Ar = Ars[buf], *Ai = Ais[buf], *Br = Brs[buf], *Bi = Bis[buf];
        const bool kin = c * FM_KC + sk < nphi;
#pragma unroll
        for (int u = 0; u < FM_NA; u++) {
            Ar[(sr + SR * u) * FM_LS + sk] = ra[u].x;
            Ai[(sr + SR * u) * FM_LS + sk] = ra[u].y;
        }
#pragma unroll
        for (int u = 0; u < FM_NB; u++) {
            const double q = rphi * isg[u];
            const double e = (kin && col0 + sr + SR * u < ncol) ? exp(-0.25 * (q * q)) : 0.0;
            esum[u] += e;
            Br[(sr + SR * u) * FM_LS + sk] = e * rb[u].x;
            Bi[(sr + SR * u) * FM_LS + sk] = e * rb[u].y;
        }
    };

    acc_tile<4, 2> accr, acci;
    accr.zero();
    acci.zero();
    auto compute = [&](int, int buf) {
        const double *Ar = Ars[buf], *Ai = Ais[buf], *Br = Brs[buf], *Bi = Bis[buf];
#pragma unroll
        for (int ks = 0; ks < FM_KC / 4; ks++) {
            double ar[4], ai[4], br[2], bi[2];
#pragma unroll
            for (int v = 0; v < 2; v++) {
                br[v] = Br[(wc + 16 * v + ri) * FM_LS + 4 * ks + kq];
                bi[v] = Bi[(wc + 16 * v + ri) * FM_LS + 4 * ks + kq];
            }
#pragma unroll
            for (int u = 0; u < 4; u++) {
                ar[u] = Ar[(wr + 16 * u + ri) * FM_LS + 4 * ks + kq];
                ai[u] = Ai[(wr + 16 * u + ri) * FM_LS + 4 * ks + kq];
            }
            complex_mma(accr, acci, ar, ai, br, bi);
        }
    };
    staged_k_loop((nphi + FM_KC - 1) / FM_KC, gload, lstore, compute);

    // normaliser: the 8 staging lanes of a column hold its partial sums; folded in a fixed order
#pragma unroll
    for (int u = 0; u < FM_NB; u++) {
        double s = esum[u];
#pragma unroll
        for (int o = FM_KC / 2; o >= 1; o >>= 1) s += __shfl_xor(s, o, 64);
        if (sk == 0) Wn[sr + SR * u] = s;
    }
    __syncthreads();

    // epilogue: normaliser and scale, saturation, product with the intensity; column blocks outermost, so that a block
    // beyond ncol is left before its scale / W is formed
#pragma unroll
    for (int v = 0; v < 2; v++) {
        const int lc = wc + w.col(v);
        const long gc = col0 + lc;
        if (gc >= ncol) continue;
        const double fac = scale / Wn[lc];
#pragma unroll
        for (int u = 0; u < 4; u++)
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int gf = f0 + wr + w.row(u, r);
                if (gf >= nfreq) continue;
                const double zr = accr.acc[u][v][r] * fac, zi = acci.acc[u][v][r] * fac;
                const double s = sat_factor(zr, zi);
                const double pr = zr * s, pi = zi * s;
                if (MODE == 0) {
                    reinterpret_cast<double2 *>(out)[(size_t)gf * (size_t)ncol + (size_t)gc] = make_double2(pr, pi);
                } else {
                    const double t = T[(size_t)gf * (size_t)ncol + (size_t)gc];
                    double *o = out + (size_t)gf * 4 * (size_t)ncol + (size_t)gc;
                    o[0] = t;
                    o[(size_t)ncol] = pr * t;
                    o[2 * (size_t)ncol] = pi * t;
                    o[3 * (size_t)ncol] = 0.0;
                }
            }
    }
}

// ---- complex mean / variance ---------------------------------------------------------------------------------------

constexpr int CV_MAXB = 4096;     // partials_split gives at most this many

// PASS 0: partial sums of (re, im).  PASS 1: partial sums of |y - m|^2 (second slot 0), m = out2[1..2].
template <int PASS>
__global__ void __launch_bounds__(256)
cvar_partial_kernel(const double2 *__restrict__ y, long count, long per, const double *__restrict__ out2,
                    double *__restrict__ work) {
    __shared__ double red[8];
    const long lo = (long)blockIdx.x * per;
    const long hi = lo + per < count ? lo + per : count;
    const double mr = PASS ? out2[1] : 0.0, mi = PASS ? out2[2] : 0.0;
    double a = 0.0, b = 0.0;
    for (long i = lo + threadIdx.x; i < hi; i += 256) {
        const double2 v = y[i];
        if (PASS == 0) {
            a += v.x;
            b += v.y;
        } else {
            const double dr = v.x - mr, di = v.y - mi;
            a += dr * dr + di * di;
        }
    }
    block_sum2(a, b, red);
    if (threadIdx.x == 0) work[2 * (size_t)blockIdx.x] = a, work[2 * (size_t)blockIdx.x + 1] = b;
}

template <int PASS>
__global__ void __launch_bounds__(256)
cvar_final_kernel(const double *__restrict__ work, int nb, long count, double *__restrict__ out2) {
    __shared__ double red[8];
    double a = 0.0, b = 0.0;
    for (int i = threadIdx.x; i < nb; i += 256) a += work[2 * (size_t)i], b += work[2 * (size_t)i + 1];
    block_sum2(a, b, red);
    if (threadIdx.x == 0) {
        if (PASS == 0)
            out2[1] = a / (double)count, out2[2] = b / (double)count;
        else
            out2[0] = a / (double)count;
    }
}

// ---- pack ----------------------------------------------------------------------------------------------------------

// y[p ld + off + r] = maps[r npix + p], r < R: 32 x 32 tiles through LDS
__global__ void __launch_bounds__(256)
faraday_pack_kernel(const double *__restrict__ maps, int R, long npix, long ld, long off, double *__restrict__ y) {
    __shared__ double tile[32][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int nrb = (R + 31) / 32;
    const int r0 = (int)(blockIdx.x % (unsigned)nrb) * 32;
    const long p0 = (long)(blockIdx.x / (unsigned)nrb) * 32;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int r = r0 + ty + 8 * j;
        const long p = p0 + tx;
        tile[ty + 8 * j][tx] = (r < R && p < npix) ? maps[(size_t)r * (size_t)npix + (size_t)p] : 0.0;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const long p = p0 + ty + 8 * j;
        const int r = r0 + tx;
        if (r < R && p < npix) y[(size_t)p * (size_t)ld + (size_t)(off + r)] = tile[tx][ty + 8 * j];
    }
}

}  // namespace

extern "C" {

int corahip_complex_variance(corahip_ctx *ctx, const double *y, long count, double *out2) {
    ARG_CHECK(ctx && y && out2 && count >= 1);
    ARG_CHECK(is_aligned(y, 16) && is_aligned(out2, 8));
    ARG_CHECK(!overlaps(out2, 3 * sizeof(double), y, (size_t)count * 16));
    int nb;
    long per;
    partials_split(count, 1, &nb, &per);
    void *work = nullptr;
    int rc = corahip_ctx_scratch(ctx, 10, (size_t)CV_MAXB * 2 * sizeof(double), &work);
    if (rc != 0) return rc;
    StageTimer t(ctx, "complex_variance");
    const double2 *yc = reinterpret_cast<const double2 *>(y);
    hipLaunchKernelGGL(cvar_partial_kernel<0>, dim3((unsigned)nb), dim3(256), 0, ctx->stream, yc, count, per, out2, (double *)work);
    LAUNCH_CHECK();
    hipLaunchKernelGGL(cvar_final_kernel<0>, dim3(1), dim3(256), 0, ctx->stream, (const double *)work, nb, count, out2);
    LAUNCH_CHECK();
    hipLaunchKernelGGL(cvar_partial_kernel<1>, dim3((unsigned)nb), dim3(256), 0, ctx->stream, yc, count, per, out2, (double *)work);
    LAUNCH_CHECK();
    hipLaunchKernelGGL(cvar_final_kernel<1>, dim3(1), dim3(256), 0, ctx->stream, (const double *)work, nb, count, out2);
    LAUNCH_CHECK();
    return 0;
}

int corahip_faraday_mix(corahip_ctx *ctx, const double *y, long ncol, int nphi, const double *phi, const double *sigma,
                        const double *A, int nfreq, double scale, const double *intensity, double *out) {
    ARG_CHECK(ctx && y && phi && sigma && A && out);
    ARG_CHECK(ncol >= 1 && nfreq >= 1 && nphi >= 2 && (nphi & 1) == 0);
    ARG_CHECK(is_aligned(y, 16) && is_aligned(A, 16));
    ARG_CHECK(is_aligned(phi, 8) && is_aligned(sigma, 8) && is_aligned(intensity, 8));
    ARG_CHECK(is_aligned(out, intensity ? 8 : 16));
    const size_t ybytes = (size_t)ncol * (size_t)nphi * 16, abytes = (size_t)nfreq * (size_t)nphi * 16;
    const size_t tbytes = (size_t)nfreq * (size_t)ncol * 8;
    const size_t obytes = intensity ? 4 * tbytes : 2 * tbytes;
    ARG_CHECK(!overlaps(out, obytes, y, ybytes) && !overlaps(out, obytes, A, abytes));
    ARG_CHECK(!overlaps(out, obytes, phi, (size_t)nphi * 8) && !overlaps(out, obytes, sigma, (size_t)ncol * 8));
    ARG_CHECK(intensity == nullptr || !overlaps(out, obytes, intensity, tbytes));
    const long nfb = (nfreq + FM_BM - 1) / FM_BM, ncb = (ncol + FM_BN - 1) / FM_BN;
    ARG_CHECK(nfb * ncb <= 0x7fffffffL);
    StageTimer t(ctx, "faraday_mix");
    const double2 *yc = reinterpret_cast<const double2 *>(y), *Ac = reinterpret_cast<const double2 *>(A);
    if (intensity)
        hipLaunchKernelGGL(faraday_mix_kernel<1>, dim3((unsigned)(nfb * ncb)), dim3(FM_NT), 0, ctx->stream, yc, ncol, nphi,
                           phi, sigma, Ac, nfreq, scale, intensity, (int)nfb, out);
    else
        hipLaunchKernelGGL(faraday_mix_kernel<0>, dim3((unsigned)(nfb * ncb)), dim3(FM_NT), 0, ctx->stream, yc, ncol, nphi,
                           phi, sigma, Ac, nfreq, scale, intensity, (int)nfb, out);
    LAUNCH_CHECK();
    return 0;
}

int corahip_faraday_pack(corahip_ctx *ctx, const double *maps, int nchunk, long npix, int k0, int nphi, double *y) {
    ARG_CHECK(ctx && maps && y && nchunk >= 1 && npix >= 1 && k0 >= 0 && nphi >= 1 && (long)k0 + nchunk <= nphi);
    ARG_CHECK(is_aligned(maps, 8) && is_aligned(y, 8));
    ARG_CHECK(!overlaps(y, (size_t)npix * (size_t)nphi * 16, maps, (size_t)nchunk * 2 * (size_t)npix * 8));
    const int R = 2 * nchunk;
    const long nrb = (R + 31) / 32, npb = (npix + 31) / 32;
    ARG_CHECK(nrb * npb <= 0x7fffffffL);
    StageTimer t(ctx, "faraday_pack");
    hipLaunchKernelGGL(faraday_pack_kernel, dim3((unsigned)(nrb * npb)), dim3(256), 0, ctx->stream, maps, R, npix,
                       2 * (long)nphi, 2 * (long)k0, y);
    LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
