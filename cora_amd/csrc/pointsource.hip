// pointsource.hip - extra-galactic point sources (cora/foreground/pointsource.py) on the device: the synthetic
// population of PointSourceModel.generate_population / getsky (:131-173, :213-251), the painting of a population or a
// catalogue into a HEALPix cube (:238-250, :478-516), the polarisation and Faraday rotation at the end of getpolsky
// (:21-51, :253-278) and healpy.ud_grade for the rotation-measure map.
//
//   ps_population_kernel   source i of the population, from Philox counters that depend on (seed, i) alone:
//                            block A = philox(counter (i lo, i hi, 0, PS_DOMAIN), key seed),  block B = (.., 1, PS_DOMAIN)
//                            u1 = (A0 2^21 + (A1 >> 11)) 2^-53,  u2 = (A2 2^21 + (A3 >> 11)) 2^-53     (exact, [0, 1))
//                            z  = the first Box-Muller normal of block B (rng_dev.h)
//                            S = flux_min exp(spline(u1)),  ind = mean + width z,  pix = min((long)(u2 npix), npix - 1)
//                          The a_lm and flat-sky streams use counters (.., .., 0, 0) only, so no block is shared with
//                          them under any seed.  The spline is cubicspline.Interpolater's: bisection for the last knot
//                          <= u1, then the cubic in that interval; its 10000-knot tables are read through the L2.
//   ps_csr_kernel          start[p] = number of sources with pix < p, p = 0 .. npix, by bisection of the sorted pix[].
//   ps_paint_kernel        one lane per pixel, PS_CH channels per thread: the sources of the pixel are summed in
//                          ascending order, out[f, 0, p] (+)= ((sum_i S_i exp(beta_i x_f + gamma_i x_f^2)) 1e-26 c2) / den_f,
//                          planes 1, 2 the same sums weighted by polw[i, 0 / 1].  Consecutive lanes own consecutive
//                          pixels: the stores of a channel coalesce, every element has one writer, no atomics, and a
//                          sum depends on its pixel's sources and its channel alone - a subset of channels, or a second
//                          call, gives the same bits.  A pixel with more than PS_LONG sources is summed by its whole
//                          wave (lane l takes sources l, l + 64, ... in order, then a fixed butterfly), so one crowded
//                          pixel does not hold 63 lanes idle.
//   ps_rotate_kernel       (Q + iU) = I (q + iu) exp(-2i wv_f rm_p) into [F, 4, npix], or the same factor applied in
//                          place to planes 1, 2 of a cube.  The angle is -2 wv rm with wv the WAVELENGTH 1e-6 c / freq,
//                          not its square: the reference's own form (pointsource.py:43-45), kept.
//   ps_udgrade_kernel      RING -> RING between two powers of two through the NESTED hierarchy (Gorski et al. 2005,
//                          section 4.1): a pixel's (face, x, y) at the finer resolution is its parent's times 2^k plus
//                          the child offset.  Degrading: arithmetic mean of the 4^k children, summed pairwise in NESTED
//                          order (equal children sum exactly: upgrading then degrading is the identity); upgrading:
//                          replication (healpy's power = None, no UNSEEN handling).
// All element offsets are 64-bit.
#include "healpix_geom.h"
#include "rng_dev.h"

namespace {

constexpr uint32_t PS_DOMAIN = 0x50535243u;     // "PSRC": counter word 3 of every block of this stream
constexpr int PS_UD_MAXK = 6;                   // ud_grade degrades by at most 2^6 in nside: one thread walks the 4^k children
constexpr int PS_LONG = 16;                     // pixels with more sources than this are summed by the wave

__device__ inline double uniform53(uint32_t hi, uint32_t lo) {
    return (double)(((uint64_t)hi << 21) | (uint64_t)(lo >> 11)) * 0x1p-53;     // < 2^53: the conversion is exact
}

__global__ __launch_bounds__(256) void ps_population_kernel(uint64_t seed, long n, const double *__restrict__ xs,
                                                            const double *__restrict__ ys, const double *__restrict__ y2,
                                                            int nk, double flux_min, double mean, double width, long npix,
                                                            long *__restrict__ pix, double *__restrict__ S,
                                                            double *__restrict__ ind, int *__restrict__ interval,
                                                            double *__restrict__ spline_value) {
#pragma clang fp contract(off)
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        uint32_t a[4], b[4];
        philox4x32_10((uint32_t)i, (uint32_t)((uint64_t)i >> 32), 0u, PS_DOMAIN, seed, a);
        philox4x32_10((uint32_t)i, (uint32_t)((uint64_t)i >> 32), 1u, PS_DOMAIN, seed, b);
        const double u1 = uniform53(a[0], a[1]), u2 = uniform53(a[2], a[3]);
        const double z = rng_boxmuller_bits(b).x;
        // xs[lo] <= u1 < xs[hi]: xs[0] = 0 and xs[nk - 1] = 1 bracket every u1 in [0, 1)
        int lo = 0, hi = nk - 1;
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (xs[mid] <= u1) lo = mid;
            else hi = mid;
        }
        const double h = xs[hi] - xs[lo];
        const double wa = (xs[hi] - u1) / h, wb = (u1 - xs[lo]) / h;
        const double h26 = h * h / 6.0;
        const double t = ((wa * ys[lo] + wb * ys[hi]) + (wa * wa * wa - wa) * h26 * y2[lo]) + (wb * wb * wb - wb) * h26 * y2[hi];
        S[i] = flux_min * exp(t);
        ind[i] = mean + width * z;
        const long p = (long)(u2 * (double)npix);
        pix[i] = p < npix - 1 ? p : npix - 1;
        if (interval) interval[i] = lo;
        if (spline_value) spline_value[i] = t;
    }
}

// start[p] = the number of i with pix[i] < p.  Reads pix[0 .. n) only, whatever pix holds.
__global__ __launch_bounds__(256) void ps_csr_kernel(const long *__restrict__ pix, long n, long npix, int *__restrict__ start) {
    for (long p = (long)blockIdx.x * blockDim.x + threadIdx.x; p <= npix; p += (long)gridDim.x * blockDim.x) {
        long lo = 0, hi = n;
        while (lo < hi) {
            const long mid = (lo + hi) >> 1;
            if (pix[mid] < p) lo = mid + 1;
            else hi = mid;
        }
        start[p] = (int)lo;
    }
}

// NPL: planes summed (1: I; 3: I, Q, U).  CH: channels per thread.
template <int NPL, int CH>
struct PaintAcc {
    double v[CH][NPL];
    __device__ inline void clear() {
#pragma unroll
        for (int c = 0; c < CH; c++)
#pragma unroll
            for (int k = 0; k < NPL; k++) v[c][k] = 0.0;
    }
};

template <int NPL, int CH>
__device__ inline void paint_add(PaintAcc<NPL, CH> &acc, long i, const double *__restrict__ S, const double *__restrict__ beta,
                                 const double *__restrict__ gamma, const double *__restrict__ polw, const double (&xf)[CH]) {
#pragma clang fp contract(off)
    const double s = S[i], b = beta[i], g = gamma ? gamma[i] : 0.0;
    double w0 = 0.0, w1 = 0.0;
    if (NPL == 3) w0 = polw[2 * i], w1 = polw[2 * i + 1];
#pragma unroll
    for (int c = 0; c < CH; c++) {
        const double x = xf[c];
        const double y = gamma ? b * x + g * (x * x) : b * x;
        const double t = s * exp(y);
        acc.v[c][0] = acc.v[c][0] + t;
        if (NPL == 3) {
            acc.v[c][1] = acc.v[c][1] + t * w0;
            acc.v[c][2] = acc.v[c][2] + t * w1;
        }
    }
}

template <int NPL, int CH>
__global__ __launch_bounds__(256) void ps_paint_kernel(const int *__restrict__ start, const double *__restrict__ S,
                                                       const double *__restrict__ beta, const double *__restrict__ gamma,
                                                       const double *__restrict__ polw, const double *__restrict__ x,
                                                       const double *__restrict__ den, double c2, int F, long npix, int npol,
                                                       int accumulate, double *__restrict__ out) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63;
    const long p = (long)blockIdx.x * 256 + threadIdx.x;
    const int f0 = blockIdx.y * CH;
    const bool inside = p < npix;
    const int s0 = inside ? start[p] : 0, s1 = inside ? start[p + 1] : 0;
    const int len = s1 > s0 ? s1 - s0 : 0;
    double xf[CH];
#pragma unroll
    for (int c = 0; c < CH; c++) xf[c] = f0 + c < F ? x[f0 + c] : 0.0;

    PaintAcc<NPL, CH> acc;
    acc.clear();
    if (len <= PS_LONG)
        for (int i = s0; i < s0 + len; i++) paint_add<NPL, CH>(acc, i, S, beta, gamma, polw, xf);

    // crowded pixels, one after the other, by the whole wave (every lane of the wave reaches this loop)
    unsigned long long crowded = __ballot(len > PS_LONG);
    while (crowded) {
        const int l = __ffsll(crowded) - 1;
        crowded &= crowded - 1;
        const int ls0 = __shfl(s0, l, 64), llen = __shfl(len, l, 64);
        PaintAcc<NPL, CH> part;
        part.clear();
        for (int i = lane; i < llen; i += 64) paint_add<NPL, CH>(part, ls0 + i, S, beta, gamma, polw, xf);
#pragma unroll
        for (int c = 0; c < CH; c++)
#pragma unroll
            for (int k = 0; k < NPL; k++) {
                double v = part.v[c][k];
#pragma unroll
                for (int o = 32; o >= 1; o >>= 1) v = v + __shfl_xor(v, o, 64);
                if (lane == l) acc.v[c][k] = v;
            }
    }

    if (!inside || (accumulate && len == 0)) return;
#pragma unroll
    for (int c = 0; c < CH; c++) {
        const int f = f0 + c;
        if (f >= F) break;
        const double d = den[f];
        double *o = out + ((size_t)f * (size_t)npol) * (size_t)npix + (size_t)p;
#pragma unroll
        for (int k = 0; k < 3; k++) {
            if (k >= npol) break;
            const double v = k < NPL ? ((acc.v[c][k < NPL ? k : 0] * 1e-26) * c2) / d : 0.0;
            if (accumulate) {
                if (k < NPL) o[(size_t)k * (size_t)npix] = o[(size_t)k * (size_t)npix] + v;
            } else {
                o[(size_t)k * (size_t)npix] = v;
            }
        }
        if (npol == 4 && !accumulate) o[3 * (size_t)npix] = 0.0;
    }
}

// out (Q, U) = (Q c - U s, Q s + U c), (c, s) = (cos, sin)(-2 wv rm)
__device__ inline void rotate_qu(double q, double u, double wv, double rm, double &qo, double &uo) {
#pragma clang fp contract(off)
    double s, c;
    sincos((-2.0 * wv) * rm, &s, &c);
    qo = q * c - u * s;
    uo = q * s + u * c;
}

// INPLACE 0: I [F, npix], q, u [npix] -> out [F, 4, npix].  INPLACE 1: planes 1, 2 of out [F, npol, npix] rotated.
template <int INPLACE>
__global__ __launch_bounds__(256) void ps_rotate_kernel(const double *__restrict__ I, const double *__restrict__ qf,
                                                        const double *__restrict__ uf, const double *__restrict__ rm,
                                                        const double *__restrict__ wv, int F, int npol, long npix,
                                                        double *out) {
#pragma clang fp contract(off)
    const int f = blockIdx.y;                  // one channel per grid row: wv[f] is uniform, no division per element
    const double wvf = wv ? wv[f] : 0.0;
    for (long p = (long)blockIdx.x * blockDim.x + threadIdx.x; p < npix; p += (long)gridDim.x * blockDim.x) {
        const long e = (long)f * npix + p;
        double *o = out + ((size_t)f * (size_t)npol) * (size_t)npix + (size_t)p;
        double q, u;
        if (INPLACE) {
            q = o[(size_t)npix];
            u = o[2 * (size_t)npix];
        } else {
            const double t = I[e];
            o[0] = t;
            o[3 * (size_t)npix] = 0.0;
            q = t * qf[p];
            u = t * uf[p];
        }
        if (rm) rotate_qu(q, u, wvf, rm[p], q, u);
        if (!INPLACE || rm) {
            o[(size_t)npix] = q;
            o[2 * (size_t)npix] = u;
        }
    }
}

// k = log2(nside_out / nside_in): > 0 replicates, < 0 averages 4^-k children, 0 copies
__global__ __launch_bounds__(256) void ps_udgrade_kernel(Geom gin, Geom gout, int k, const double *__restrict__ in, long nmap,
                                                         double *__restrict__ out) {
#pragma clang fp contract(off)
    for (long p = (long)blockIdx.x * blockDim.x + threadIdx.x; p < gout.npix; p += (long)gridDim.x * blockDim.x) {
        if (k == 0) {
            for (long m = 0; m < nmap; m++) out[m * gout.npix + p] = in[m * gin.npix + p];
            continue;
        }
        long ix, iy;
        int face;
        ring2xyf(gout, p, ix, iy, face);
        if (k > 0) {
            const long q = xyf2ring(gin, ix >> k, iy >> k, face);
            for (long m = 0; m < nmap; m++) out[m * gout.npix + p] = in[m * gin.npix + q];
        } else {
            const int kk = -k;
            const long nchild = 1L << (2 * kk);
            // pairwise over the NESTED order (tree_push of healpix_geom.h): equal children sum exactly
            for (long m = 0; m < nmap; m++) {
                double part[2 * PS_UD_MAXK + 1];
                for (long j = 0; j < nchild; j++) tree_push(part, j, in[m * gin.npix + child_pixel(gin, ix, iy, face, kk, j)]);
                out[m * gout.npix + p] = part[2 * kk] / (double)nchild;
            }
        }
    }
}

}  // namespace

extern "C" {

int corahip_pointsource_population(corahip_ctx *ctx, uint64_t seed, long n, const double *knots, const double *values,
                                   const double *second, int nknots, double flux_min, double spectral_mean,
                                   double spectral_width, long npix, int64_t *pix, double *flux, double *index,
                                   int32_t *interval, double *spline_value) {
    ARG_CHECK(ctx && knots && values && second && n >= 0 && nknots >= 2 && npix >= 1);
    if (n == 0) return 0;
    ARG_CHECK(pix && flux && index);
    StageTimer t(ctx, "pointsource_population");
    hipLaunchKernelGGL(ps_population_kernel, dim3(grid_blocks(ctx, n)), dim3(256), 0, ctx->stream, seed, n, knots, values, second,
                       nknots, flux_min, spectral_mean, spectral_width, npix, (long *)pix, flux, index, (int *)interval,
                       spline_value);
    LAUNCH_CHECK();
    return 0;
}

int corahip_pointsource_paint(corahip_ctx *ctx, long n, const int64_t *pix, const double *flux, const double *beta,
                              const double *gamma, const double *polw, const double *x, const double *den, double c2,
                              int nfreq, int npol, long npix, int accumulate, double *out) {
    ARG_CHECK(ctx && x && den && out && n >= 0 && n < 0x7fffffffL && nfreq >= 1 && npix >= 1 && (npol == 1 || npol == 4));
    ARG_CHECK(n == 0 || (pix && flux && beta));
    ARG_CHECK(polw == nullptr || npol == 4);
    ARG_CHECK((npix + 255) / 256 <= 0x7fffffffL);
    const size_t obytes = (size_t)nfreq * (size_t)npol * (size_t)npix * 8;
    ARG_CHECK(!overlaps(out, obytes, pix, (size_t)n * 8) && !overlaps(out, obytes, flux, (size_t)n * 8));
    ARG_CHECK(!overlaps(out, obytes, beta, (size_t)n * 8) && !overlaps(out, obytes, gamma, (size_t)n * 8));
    ARG_CHECK(!overlaps(out, obytes, polw, (size_t)n * 16) && !overlaps(out, obytes, x, (size_t)nfreq * 8));
    ARG_CHECK(!overlaps(out, obytes, den, (size_t)nfreq * 8));
    if (n == 0 && accumulate) return 0;
    void *start = nullptr;
    int rc = corahip_ctx_scratch(ctx, 11, ((size_t)npix + 1) * sizeof(int), &start);
    if (rc != 0) return rc;
    StageTimer t(ctx, "pointsource_paint");
    hipLaunchKernelGGL(ps_csr_kernel, dim3(grid_blocks(ctx, npix + 1)), dim3(256), 0, ctx->stream, (const long *)pix, n, npix,
                       (int *)start);
    LAUNCH_CHECK();
    const unsigned pb = (unsigned)((npix + 255) / 256);
    if (polw) {
        constexpr int CH = 8;
        hipLaunchKernelGGL((ps_paint_kernel<3, CH>), dim3(pb, (unsigned)((nfreq + CH - 1) / CH)), dim3(256), 0, ctx->stream,
                           (const int *)start, flux, beta, gamma, polw, x, den, c2, nfreq, npix, npol, accumulate, out);
    } else {
        constexpr int CH = 16;
        hipLaunchKernelGGL((ps_paint_kernel<1, CH>), dim3(pb, (unsigned)((nfreq + CH - 1) / CH)), dim3(256), 0, ctx->stream,
                           (const int *)start, flux, beta, gamma, polw, x, den, c2, nfreq, npix, npol, accumulate, out);
    }
    LAUNCH_CHECK();
    return 0;
}

int corahip_polarise_rotate(corahip_ctx *ctx, const double *intensity, const double *qfrac, const double *ufrac,
                            const double *rm, const double *wv, int nfreq, long npix, double *out) {
    ARG_CHECK(ctx && intensity && qfrac && ufrac && out && nfreq >= 1 && nfreq <= 65535 && npix >= 1);
    ARG_CHECK(rm == nullptr || wv != nullptr);
    const size_t ibytes = (size_t)nfreq * (size_t)npix * 8;
    ARG_CHECK(!overlaps(out, 4 * ibytes, intensity, ibytes) && !overlaps(out, 4 * ibytes, qfrac, (size_t)npix * 8));
    ARG_CHECK(!overlaps(out, 4 * ibytes, ufrac, (size_t)npix * 8) && !overlaps(out, 4 * ibytes, rm, (size_t)npix * 8));
    ARG_CHECK(!overlaps(out, 4 * ibytes, wv, (size_t)nfreq * 8));
    StageTimer t(ctx, "polarise_rotate");
    hipLaunchKernelGGL(ps_rotate_kernel<0>, dim3(grid_blocks(ctx, npix), (unsigned)nfreq), dim3(256), 0, ctx->stream, intensity, qfrac,
                       ufrac, rm, wv, nfreq, 4, npix, out);
    LAUNCH_CHECK();
    return 0;
}

int corahip_faraday_rotate(corahip_ctx *ctx, double *polmap, const double *rm, const double *wv, int nfreq, int npol,
                           long npix) {
    ARG_CHECK(ctx && polmap && rm && wv && nfreq >= 1 && nfreq <= 65535 && npol >= 3 && npix >= 1);
    const size_t obytes = (size_t)nfreq * (size_t)npol * (size_t)npix * 8;
    ARG_CHECK(!overlaps(polmap, obytes, rm, (size_t)npix * 8) && !overlaps(polmap, obytes, wv, (size_t)nfreq * 8));
    StageTimer t(ctx, "faraday_rotate");
    hipLaunchKernelGGL(ps_rotate_kernel<1>, dim3(grid_blocks(ctx, npix), (unsigned)nfreq), dim3(256), 0, ctx->stream,
                       (const double *)nullptr, (const double *)nullptr, (const double *)nullptr, rm, wv, nfreq, npol, npix,
                       polmap);
    LAUNCH_CHECK();
    return 0;
}

int corahip_healpix_ud_grade(corahip_ctx *ctx, const double *maps, long nmap, int nside_in, int nside_out, double *out) {
    ARG_CHECK(ctx && maps && out && nmap >= 1 && nside_in >= 1 && nside_in <= 8192 && nside_out >= 1 && nside_out <= 8192);
    const int ki = log2_exact(nside_in), ko = log2_exact(nside_out);
    ARG_CHECK(ki >= 0 && ko >= 0);
    ARG_CHECK(ki - ko <= PS_UD_MAXK);
    const Geom gin = make_geom(nside_in), gout = make_geom(nside_out);
    ARG_CHECK(!overlaps(out, (size_t)nmap * (size_t)gout.npix * 8, maps, (size_t)nmap * (size_t)gin.npix * 8));
    StageTimer t(ctx, "healpix_ud_grade");
    hipLaunchKernelGGL(ps_udgrade_kernel, dim3(grid_blocks(ctx, gout.npix)), dim3(256), 0, ctx->stream, gin, gout, ko - ki, maps,
                       nmap, out);
    LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
