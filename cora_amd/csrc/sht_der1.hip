// sht_der1.hip - first derivatives of a scalar field on the HEALPix sphere (healpy.alm2map_der1, as
// cora/signal/lssutil.py:225-261 `gradient` calls it) composed around the scalar synthesis, and numpy.gradient along
// the slice axis (cora/signal/lss.py:806-810): together the Zel'dovich displacement field of lss.py:806-828.
//
// With lambda_lm the normalised Legendre functions of SURVEY Appendix A, x = cos theta:
//   sin(theta) d lambda_lm / d theta = l x lambda_lm - c_lm lambda_{l-1,m},  c_lm = sqrt((2l+1)/(2l-1) (l^2 - m^2))
// so for one field with coefficients a_lm and S[.] the scalar synthesis (corahip_alm2map)
//   dT/dtheta       = (x S[a1] - S[a2]) / sin theta,   a1_lm = l a_lm,   a2_{l-1,m} = c_lm a_lm  (a2_{lmax,m} = 0)
//   (1/sin) dT/dphi =  S[a3] / sin theta,              a3_lm = i m a_lm
// - the closed form the HEALPix library uses for alm2map_der1, 1/sin theta included.  Three scalar syntheses per field
// and no change to the Legendre or ring-FFT kernels (a two-operand spin-1 Legendre kernel would need two).
//
// Conditioning: near the poles x S[a1] and S[a2] are sums of size l |T| whose difference is divided by sin theta, so
// the rounding of the two syntheses is amplified by 1/sin theta on the first rings.
// Truncation: the synthesis drops Legendre terms below 2^cut_exp per unit coefficient (corahip_sht_plan_create_ex);
// here the coefficients carry a factor l and the result a factor 1/sin theta: the bound is
// 2 sum |l a_lm| 2^cut_exp / sin theta.
//
// Three bandwidth-bound kernels:
//   der1_alm_prep_kernel    alm_dev groups -> [a1 | a2 | a3] channel-group blocks   (16 B read, 48 B written per a_lm)
//   der1_combine_kernel     three synthesised maps of a field -> (d/dtheta, d/dphi / sin), per-field factors fused
//   radial_gradient_kernel  numpy.gradient(f, x, axis=0) with a per-row factor, every element of f read once
#include "sht_internal.h"

// (l, m) of a packed index: m-major, idx = m (2 lmax + 1 - m) / 2 + l
__device__ static inline void lm_of_idx(long idx, int lmax, int &l, int &m) {
    int mm = (int)(((2.0 * lmax + 3.0) - sqrt((2.0 * lmax + 3.0) * (2.0 * lmax + 3.0) - 8.0 * (double)idx)) * 0.5);
    mm = max(0, min(mm, lmax));
    while (mm > 0 && alm_idx(mm, mm, lmax) > idx) mm--;
    while (mm < lmax && alm_idx(mm + 1, mm + 1, lmax) <= idx) mm++;
    m = mm;
    l = mm + (int)(idx - alm_idx(mm, mm, lmax));
}

// One item = 16 bytes of the real parts and 16 bytes of the imaginary parts of one cell: (idx, group g, channel pair j).
// Items are numbered w = 2 g + j inside a row of W = 2 Gin; a thread walks items item0 + k * stride and carries
// (row, w) along by additions: `srow` and `sw` are stride / W and stride % W, computed once on the host.
__global__ void __launch_bounds__(256)
der1_alm_prep_kernel(const double *__restrict__ src, int Gsrc, int g0, int Gin, int lmax, long nalm, long srow, int sw,
                     double *__restrict__ dst) {
    const int W = 2 * Gin;
    const long item0 = (long)blockIdx.x * blockDim.x + threadIdx.x;
    long row = item0 / W;                    // (once per thread)
    int w = (int)(item0 - row * W);
    const size_t drow = (size_t)3 * Gin * 8;
    while (row < nalm) {
        int l, m;
        lm_of_idx(row, lmax, l, m);
        const int g = w >> 1, j = w & 1;
        const double *p = src + ((size_t)row * Gsrc + g0 + g) * 8 + 2 * j;
        const double2 re = *reinterpret_cast<const double2 *>(p), im = *reinterpret_cast<const double2 *>(p + 4);
        double2 re2 = make_double2(0.0, 0.0), im2 = re2;
        if (l < lmax) {                      // a2_lm = c_{l+1,m} a_{l+1,m}: the next packed index, same m column
            const double l1 = (double)(l + 1), md = (double)m;
            const double c = sqrt((2.0 * l1 + 1.0) / (2.0 * l1 - 1.0) * (l1 * l1 - md * md));
            const double2 nre = *reinterpret_cast<const double2 *>(p + (size_t)Gsrc * 8);
            const double2 nim = *reinterpret_cast<const double2 *>(p + (size_t)Gsrc * 8 + 4);
            re2 = make_double2(c * nre.x, c * nre.y);
            im2 = make_double2(c * nim.x, c * nim.y);
        }
        const double ld = (double)l, md = (double)m;
        double *q = dst + (size_t)row * drow + (size_t)g * 8 + 2 * j;
        *reinterpret_cast<double2 *>(q) = make_double2(ld * re.x, ld * re.y);
        *reinterpret_cast<double2 *>(q + 4) = make_double2(ld * im.x, ld * im.y);
        q += (size_t)Gin * 8;
        *reinterpret_cast<double2 *>(q) = re2;
        *reinterpret_cast<double2 *>(q + 4) = im2;
        q += (size_t)Gin * 8;
        // i m a: (re, im) -> (-m im, m re); the m = 0 column is zero whatever its imaginary parts hold
        double2 re3 = make_double2(0.0, 0.0), im3 = re3;
        if (m > 0) re3 = make_double2(-md * im.x, -md * im.y), im3 = make_double2(md * re.x, md * re.y);
        *reinterpret_cast<double2 *>(q) = re3;
        *reinterpret_cast<double2 *>(q + 4) = im3;
        // next item of this thread
        w += sw;
        row += srow;
        if (w >= W) w -= W, row++;
    }
}

// block = (ring, field): out_theta = s_theta[f] (z A - B) / sth, out_phi = s_phi[f] C / sth^(1 + phi_extra) on the
// pixels of the ring; A, B, C = rows f, 4 Gin + f, 8 Gin + f of maps3.  Ring starts and lengths are even: double2.
__global__ void __launch_bounds__(256)
der1_combine_kernel(const double *__restrict__ maps3, int Gin, long npix, int nring, const int64_t *__restrict__ start,
                    const int32_t *__restrict__ nphi, const double *__restrict__ z, const double *__restrict__ sin_th,
                    const double *__restrict__ s_theta,
                    const double *__restrict__ s_phi, int phi_extra, double *__restrict__ out_theta,
                    double *__restrict__ out_phi) {
    const int ring = blockIdx.x, f = blockIdx.y;
    const int rn = min(ring, nring - 1 - ring);
    const double zz = ring == rn ? z[rn] : -z[rn];
    // the plan's own sin theta (sqrt(t (2 - t)), t = 1 - z, in the caps): sqrt((1 - z)(1 + z)) from the rounded z loses
    // eps / (1 - z) of relative accuracy, 3.5e-10 on the first ring of nside 1024
    const double sth = sin_th[rn];
    const double ft = (s_theta ? s_theta[f] : 1.0) / sth;
    const double fp = (s_phi ? s_phi[f] : 1.0) / (phi_extra ? sth * sth : sth);
    const size_t o = (size_t)f * npix + start[ring];
    const double2 *A = reinterpret_cast<const double2 *>(maps3 + o);
    const double2 *B = reinterpret_cast<const double2 *>(maps3 + (size_t)4 * Gin * npix + o);
    const double2 *C = reinterpret_cast<const double2 *>(maps3 + (size_t)8 * Gin * npix + o);
    double2 *ot = reinterpret_cast<double2 *>(out_theta + o), *op = reinterpret_cast<double2 *>(out_phi + o);
    const int n2 = nphi[ring] >> 1;
    for (int j = threadIdx.x; j < n2; j += blockDim.x) {
        const double2 a = A[j], b = B[j], c = C[j];
        ot[j] = make_double2(ft * (zz * a.x - b.x), ft * (zz * a.y - b.y));
        op[j] = make_double2(fp * c.x, fp * c.y);
    }
}

// numpy.gradient(f, x, axis=0) * s_r[:, None]: a block walks the n slices of a pixel tile with (f[i-1], f[i], f[i+1])
// in registers, so every element of f comes from HBM once; coef [n][3] = (a, b, c) of row i (end rows: the one-sided
// pair, with the coefficient of the missing neighbour 0).  V = doubles per thread and access (2 needs npix even).
template <int V>
__global__ void __launch_bounds__(256)
radial_gradient_kernel(const double *__restrict__ f, const double *__restrict__ coef, const double *__restrict__ s_r, int n,
                       long npix, double *__restrict__ out) {
    typedef typename std::conditional<V == 2, double2, double>::type vec;
    const long nv = npix / V;
    for (long p = (long)blockIdx.x * blockDim.x + threadIdx.x; p < nv; p += (long)gridDim.x * blockDim.x) {
        const vec *src = reinterpret_cast<const vec *>(f) + p;
        vec *dst = reinterpret_cast<vec *>(out) + p;
        vec fm, f0 = src[0], fp = src[nv];
        fm = f0;
        for (int i = 0; i < n; i++) {
            vec fn = fp;
            if (i + 2 < n) fn = src[(size_t)(i + 2) * nv];      // in flight while row i is formed
            const double a = coef[3 * i], b = coef[3 * i + 1], c = coef[3 * i + 2];
            const double s = s_r ? s_r[i] : 1.0;
            vec r;
            {
                // numpy's own order, products and sums rounded one by one: interior rows equal numpy.gradient bit for bit
#pragma clang fp contract(off)
                if constexpr (V == 2)
                    r = make_double2(((a * fm.x + b * f0.x) + c * fp.x) * s, ((a * fm.y + b * f0.y) + c * fp.y) * s);
                else
                    r = ((a * fm + b * f0) + c * fp) * s;
            }
            dst[(size_t)i * nv] = r;
            fm = f0, f0 = fp, fp = fn;
        }
    }
}

extern "C" {

int corahip_der1_alm_prep(corahip_ctx *ctx, corahip_sht_plan *plan, const double *alm_dev, int g_src, int g0, int g_in,
                          double *alm3_dev) {
    ARG_CHECK(ctx && plan && alm_dev && alm3_dev);
    ARG_CHECK(g_in >= 1 && g0 >= 0 && g_src >= 1 && g0 + g_in <= g_src && g_in <= 16384);
    ARG_CHECK(is_aligned(alm_dev, 16) && is_aligned(alm3_dev, 16));
    StageTimer t(ctx, "der1_prep");
    const long W = 2L * g_in, total = plan->nalm * W;
    const unsigned blocks = grid_blocks(ctx, total);
    const long stride = (long)blocks * 256;
    hipLaunchKernelGGL(der1_alm_prep_kernel, dim3(blocks), dim3(256), 0, ctx->stream, alm_dev, g_src, g0, g_in,
                       plan->lmax, plan->nalm, stride / W, (int)(stride % W), alm3_dev);
    LAUNCH_CHECK();
    return 0;
}

int corahip_der1_combine(corahip_ctx *ctx, corahip_sht_plan *plan, const double *maps3, int g_in, int nfields,
                         const double *s_theta, const double *s_phi, int phi_extra, double *out_theta, double *out_phi) {
    ARG_CHECK(ctx && plan && maps3 && out_theta && out_phi);
    ARG_CHECK(g_in >= 1 && nfields >= 1 && nfields <= 4 * g_in && nfields <= 65535);
    ARG_CHECK(phi_extra == 0 || phi_extra == 1);
    ARG_CHECK(is_aligned(maps3, 16) && is_aligned(out_theta, 16) && is_aligned(out_phi, 16));
    StageTimer t(ctx, "der1_combine");
    dim3 grid((unsigned)plan->nring, (unsigned)nfields);
    hipLaunchKernelGGL(der1_combine_kernel, grid, dim3(256), 0, ctx->stream, maps3, g_in, plan->npix, plan->nring,
                       plan->d_start, plan->d_nphi, plan->d_z, plan->d_sth, s_theta, s_phi, phi_extra, out_theta, out_phi);
    LAUNCH_CHECK();
    return 0;
}

int corahip_radial_gradient(corahip_ctx *ctx, const double *f, const double *x_coef, const double *s_r, int n, long npix,
                            double *out) {
    ARG_CHECK(ctx && f && x_coef && out && n >= 2 && npix >= 1);
    ARG_CHECK(is_aligned(f, 8) && is_aligned(out, 8));
    StageTimer t(ctx, "radial_gradient");
    const bool v2 = (npix & 1) == 0 && is_aligned(f, 16) && is_aligned(out, 16);
    const long nv = v2 ? npix / 2 : npix;
    const unsigned blocks = grid_blocks(ctx, nv, 32);
    if (v2)
        hipLaunchKernelGGL(radial_gradient_kernel<2>, dim3(blocks), dim3(256), 0, ctx->stream, f, x_coef, s_r, n,
                           npix, out);
    else
        hipLaunchKernelGGL(radial_gradient_kernel<1>, dim3(blocks), dim3(256), 0, ctx->stream, f, x_coef, s_r, n,
                           npix, out);
    LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
