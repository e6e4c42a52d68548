// galaxy.hip - the pieces of ConstrainedGalaxy.getsky (cora/foreground/galaxy.py:43-55, :109-111, :147-207) that the
// library did not have: healpy.reorder, map_variance, the per-l scaling of a_lm behind healpy.smoothing and the last
// third of getsky (:181-198) as one streaming launch.
//
//   gx_reorder_kernel      RING <-> NESTED gather, out[i, q] = in[i, p(q)], one lane per output pixel and the pixel map
//                          computed in the lane (nest2ring_dev / ring2nest_dev of healpix_geom.h): no index array in
//                          memory.
//   gx_blockvar_kernel     out[i, P] = numpy var (ddof 0) of the 4^k children of RING pixel P at nside_out, two passes:
//                          the mean, then the mean of the squared deviations (never E[x^2] - E[x]^2).  Both sums run
//                          over the balanced binary tree of the NESTED child order (tree_push of healpix_geom.h, as in
//                          ps_udgrade_kernel), in which equal children sum exactly: a constant block has variance 0.
//                          WAVE = 0 (up to 16 children): a lane owns an output pixel and walks its children with a
//                          binary counter of partial sums.
//                          WAVE = 1 (64 children and more): a wave owns an output pixel, lane l takes children
//                          64 i + l, a xor butterfly (offsets 1 .. 32) sums 64 neighbours - the six lowest levels of
//                          the same tree - and the binary counter runs over i.  The two forms give the same bits.
//   gx_alm_scale_kernel    alm_dev [nalm][G][re, im][4] times fl[channel, l]: one multiply per component; the padding
//                          channels of the last group are copied.
//   gx_combine_kernel      S = haslam exp(sc lnr_c), x = ((am inv_mv) (fg - fgs)) / S, out = S (1 + (x < 0 ? tanh x : x)).
//                          A thread owns two neighbouring pixels (16-byte loads and stores) and GX_CH channels: haslam, sc
//                          and am inv_mv are loaded once per chunk, lnr[c] is the same address in every lane (a scalar
//                          load).  exp is glibc's (glibc_exp.h, < 1 ulp), tanh the device library's.
// No atomics, one writer per element: identical bits from call to call.  All element offsets are 64-bit.
#include "glibc_exp.h"
#include "healpix_geom.h"

namespace {

constexpr int GX_MAXK = 6;      // block variance: at most 4^6 children per output pixel (as ud_grade)
constexpr int GX_CH = 16;       // combine: channels per thread

// r2n 1: out in NESTED order from in in RING order; 0: the other way
__global__ __launch_bounds__(256) void gx_reorder_kernel(Geom g, int k, int r2n, const double *__restrict__ in, long nmap,
                                                         double *__restrict__ out) {
    for (long q = (long)blockIdx.x * blockDim.x + threadIdx.x; q < g.npix; q += (long)gridDim.x * blockDim.x) {
        const long p = r2n ? nest2ring_dev(g, k, q) : ring2nest_dev(g, k, q);
        for (long m = 0; m < nmap; m++) out[m * g.npix + q] = in[m * g.npix + p];
    }
}

template <int WAVE>
__global__ __launch_bounds__(256) void gx_blockvar_kernel(Geom gin, Geom gout, int k, const double *__restrict__ in, long nmap,
                                                          double *__restrict__ out) {
#pragma clang fp contract(off)
    const long nitem = nmap * gout.npix, nchild = 1L << (2 * k);
    const double dn = (double)nchild;
    if (WAVE) {
        const int lane = threadIdx.x & 63;
        const long wave0 = ((long)blockIdx.x * blockDim.x + threadIdx.x) >> 6, nwave = ((long)gridDim.x * blockDim.x) >> 6;
        const long nstep = nchild >> 6;
        for (long item = wave0; item < nitem; item += nwave) {      // the same item in every lane of the wave
            const long m = item / gout.npix, P = item - m * gout.npix;
            const double *src = in + m * gin.npix;
            long ix, iy;
            int face;
            ring2xyf(gout, P, ix, iy, face);
            double mean = 0.0, part[2 * GX_MAXK - 5];
            for (int pass = 0; pass < 2; pass++) {
                for (long i = 0; i < nstep; i++) {
                    double v = src[child_pixel(gin, ix, iy, face, k, 64 * i + lane)];
                    if (pass) {
                        v = v - mean;
                        v = v * v;
                    }
#pragma unroll
                    for (int o = 1; o <= 32; o <<= 1) v = v + __shfl_xor(v, o, 64);
                    tree_push(part, i, v);
                }
                mean = part[2 * k - 6] / dn;
            }
            if (lane == 0) out[item] = mean;
        }
    } else {
        for (long item = (long)blockIdx.x * blockDim.x + threadIdx.x; item < nitem; item += (long)gridDim.x * blockDim.x) {
            const long m = item / gout.npix, P = item - m * gout.npix;
            const double *src = in + m * gin.npix;
            long ix, iy;
            int face;
            ring2xyf(gout, P, ix, iy, face);
            double mean = 0.0, part[5];
            for (int pass = 0; pass < 2; pass++) {
                for (long j = 0; j < nchild; j++) {
                    double v = src[child_pixel(gin, ix, iy, face, k, j)];
                    if (pass) {
                        v = v - mean;
                        v = v * v;
                    }
                    tree_push(part, j, v);
                }
                mean = part[2 * k] / dn;
            }
            out[item] = mean;
        }
    }
}

// one thread per (packed index, group of 4 channels): 8 doubles
__global__ __launch_bounds__(256) void gx_alm_scale_kernel(const double *alm, int lmax, int nnu, int G, const double *__restrict__ fl,
                                                           double *out) {
    const long n = nalm_of(lmax) * G, L = lmax + 1;
    for (long q = (long)blockIdx.x * blockDim.x + threadIdx.x; q < n; q += (long)gridDim.x * blockDim.x) {
        const long idx = q / G;
        const int g = (int)(q - idx * G);
        const long l = alm_l_of_idx(idx, lmax);
        const d4_t re = *reinterpret_cast<const d4_t *>(alm + q * 8), im = *reinterpret_cast<const d4_t *>(alm + q * 8 + 4);
        d4_t ore, oim;
#pragma unroll
        for (int v = 0; v < 4; v++) {
            const int nu = 4 * g + v;
            const double f = nu < nnu ? fl[(long)nu * L + l] : 1.0;
            ore[v] = nu < nnu ? re[v] * f : re[v];
            oim[v] = nu < nnu ? im[v] * f : im[v];
        }
        *reinterpret_cast<d4_t *>(out + q * 8) = ore;
        *reinterpret_cast<d4_t *>(out + q * 8 + 4) = oim;
    }
}

__device__ inline double combine_one(double S, double a, double fg, double fgs) {
#pragma clang fp contract(off)
    const double t = a * (fg - fgs);
    const double x = t / S;
    return S * (1.0 + (x < 0.0 ? tanh(x) : x));
}

// grid: x pixel pairs, y chunks of GX_CH output channels.  npair = npix / 2 (npix = 12 nside^2 is even)
__global__ __launch_bounds__(256) void gx_combine_kernel(const double *__restrict__ fg, const double *__restrict__ fgs,
                                                         const double *__restrict__ haslam, const double *__restrict__ sc,
                                                         const double *__restrict__ am, double inv_mv,
                                                         const double *__restrict__ lnr, int nchan, int skip, long npix,
                                                         double *__restrict__ out) {
#pragma clang fp contract(off)
    const long pair = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (pair >= (npix >> 1)) return;
    const long p = 2 * pair;
    const double2 h = *reinterpret_cast<const double2 *>(haslam + p);
    const double2 s = *reinterpret_cast<const double2 *>(sc + p);
    double2 a = *reinterpret_cast<const double2 *>(am + p);
    a.x = a.x * inv_mv;
    a.y = a.y * inv_mv;
    const int c0 = skip + blockIdx.y * GX_CH;
    const int c1 = c0 + GX_CH < nchan ? c0 + GX_CH : nchan;
    for (int c = c0; c < c1; c++) {
        const double r = lnr[c];                                  // one address for the whole grid row: a scalar load
        const size_t e = (size_t)c * (size_t)npix + (size_t)p;
        const double2 f = *reinterpret_cast<const double2 *>(fg + e);
        const double2 fs = *reinterpret_cast<const double2 *>(fgs + e);
        const double Sx = h.x * glibc_exp_fma(s.x * r), Sy = h.y * glibc_exp_fma(s.y * r);
        double2 o;
        o.x = combine_one(Sx, a.x, f.x, fs.x);
        o.y = combine_one(Sy, a.y, f.y, fs.y);
        *reinterpret_cast<double2 *>(out + (size_t)(c - skip) * (size_t)npix + (size_t)p) = o;
    }
}

}  // namespace

extern "C" {

int corahip_healpix_reorder(corahip_ctx *ctx, const double *maps, long nmap, int nside, int r2n, double *out) {
    ARG_CHECK(ctx && maps && out && nmap >= 1 && nside >= 1 && nside <= 8192);
    const int k = log2_exact(nside);
    ARG_CHECK(k >= 0);
    const Geom g = make_geom(nside);
    const size_t bytes = (size_t)nmap * (size_t)g.npix * 8;
    ARG_CHECK(!overlaps(out, bytes, maps, bytes));
    StageTimer t(ctx, "healpix_reorder");
    hipLaunchKernelGGL(gx_reorder_kernel, dim3(grid_blocks(ctx, g.npix)), dim3(256), 0, ctx->stream, g, k, r2n ? 1 : 0, maps, nmap, out);
    LAUNCH_CHECK();
    return 0;
}

int corahip_healpix_block_variance(corahip_ctx *ctx, const double *maps, long nmap, int nside_in, int nside_out, double *out) {
    ARG_CHECK(ctx && maps && out && nmap >= 1 && nside_in >= 1 && nside_in <= 8192 && nside_out >= 1 && nside_out <= nside_in);
    const int ki = log2_exact(nside_in), ko = log2_exact(nside_out);
    ARG_CHECK(ki >= 0 && ko >= 0);
    const int k = ki - ko;
    ARG_CHECK(k <= GX_MAXK);
    const Geom gin = make_geom(nside_in), gout = make_geom(nside_out);
    ARG_CHECK(!overlaps(out, (size_t)nmap * (size_t)gout.npix * 8, maps, (size_t)nmap * (size_t)gin.npix * 8));
    const long nitem = nmap * gout.npix;
    StageTimer t(ctx, "healpix_block_variance");
    if (k >= 3)
        hipLaunchKernelGGL(gx_blockvar_kernel<1>, dim3(grid_blocks(ctx, nitem * 64)), dim3(256), 0, ctx->stream, gin, gout, k, maps, nmap,
                           out);
    else
        hipLaunchKernelGGL(gx_blockvar_kernel<0>, dim3(grid_blocks(ctx, nitem)), dim3(256), 0, ctx->stream, gin, gout, k, maps, nmap, out);
    LAUNCH_CHECK();
    return 0;
}

int corahip_alm_scale_l(corahip_ctx *ctx, const double *alm, int lmax, int nnu, const double *fl, double *out) {
    ARG_CHECK(ctx && alm && fl && out && lmax >= 0 && nnu >= 1);
    const int G = (nnu + 3) / 4;
    const size_t abytes = (size_t)nalm_of(lmax) * (size_t)G * 64;
    ARG_CHECK(out == alm || !overlaps(out, abytes, alm, abytes));          // in place, or apart
    ARG_CHECK(!overlaps(out, abytes, fl, (size_t)nnu * (size_t)(lmax + 1) * 8));
    ARG_CHECK(is_aligned(alm, 32) && is_aligned(out, 32));
    StageTimer t(ctx, "alm_scale_l");
    hipLaunchKernelGGL(gx_alm_scale_kernel, dim3(grid_blocks(ctx, nalm_of(lmax) * G)), dim3(256), 0, ctx->stream, alm, lmax, nnu, G, fl,
                       out);
    LAUNCH_CHECK();
    return 0;
}

int corahip_galaxy_combine(corahip_ctx *ctx, const double *fg, const double *fgs, const double *haslam, const double *sc,
                           const double *am, double inv_mv, const double *lnr, int nchan, int skip, long npix, double *out) {
    ARG_CHECK(ctx && fg && fgs && haslam && sc && am && lnr && out);
    ARG_CHECK(skip >= 0 && nchan > skip && npix >= 2 && (npix & 1) == 0 && inv_mv > 0.0 && inv_mv <= 1.7976931348623157e308);
    const int nout = nchan - skip;
    ARG_CHECK((nout + GX_CH - 1) / GX_CH <= 65535 && (npix / 2 + 255) / 256 <= 0x7fffffffL);
    ARG_CHECK(is_aligned(fg, 16) && is_aligned(fgs, 16) && is_aligned(haslam, 16) && is_aligned(sc, 16) && is_aligned(am, 16) &&
              is_aligned(out, 16));
    const size_t obytes = (size_t)nout * (size_t)npix * 8, ibytes = (size_t)nchan * (size_t)npix * 8, pbytes = (size_t)npix * 8;
    ARG_CHECK(!overlaps(out, obytes, fg, ibytes) && !overlaps(out, obytes, fgs, ibytes));
    ARG_CHECK(!overlaps(out, obytes, haslam, pbytes) && !overlaps(out, obytes, sc, pbytes));
    ARG_CHECK(!overlaps(out, obytes, am, pbytes) && !overlaps(out, obytes, lnr, (size_t)nchan * 8));
    StageTimer t(ctx, "galaxy_combine");
    hipLaunchKernelGGL(gx_combine_kernel, dim3((unsigned)((npix / 2 + 255) / 256), (unsigned)((nout + GX_CH - 1) / GX_CH)), dim3(256), 0,
                       ctx->stream, fg, fgs, haslam, sc, am, inv_mv, lnr, nchan, skip, npix, out);
    LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
