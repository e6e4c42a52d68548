// rsdcorr.hip - xi(pi, sigma; z1, z2), the flat-sky redshift-space correlation function
// (cora/signal/corr.py:274-348), for many points in one pass.
//
// The reference evaluates six Cython splines of r = sqrt(pi^2 + sigma^2) (three when only the velocity spectrum is
// known), scales them with the per-redshift factors and combines them with P_2(mu), P_4(mu), mu = pi / (r + 1e-100),
// through about twenty numpy temporaries.  Here a point reads its 16 bytes, finds its interval once for all tables,
// reads one interval record through the caches and writes its 8 bytes.
//
//   xi_rsd_records_kernel  one record per interval: xs_k, xs_{k+1}, 1/h, h^2/6 and per table y_k, y_{k+1}, y''_k, y''_{k+1}
//                          (3 tables: 16 doubles = 128 B; 6 tables: 28 doubles, padded to 32 = 256 B), and the look-up grid
//                          (cells uniform in the bit pattern of r: see RSD_KEY_BITS)
//   xi_rsd_kernel          the points, grid-stride, one writer per element
#include "common.h"
#include "spline_dev.h"

#define RSD_REC(nfun) ((nfun) == 3 ? 16 : 32)
#define RSD_MAX_KNOTS (1 << 24)
#define RSD_SCRATCH 12              // the records live in the slot of xi_multi_average's: both rebuild them every call

// The look-up grid.  The tables this kernel is for are tabulated on a logarithmic grid of r (gen_cache), where the uniform
// grid of xi_multi_average puts half of the knots into its first cell and the walk from there costs hundreds of dependent
// loads (measured: 24 ms for 2^26 points).  The cells here are uniform in the bit pattern of r: for x >= 0 the pattern is
// monotone in x, and its top 11 + RSD_KEY_BITS bits split every octave into 2^RSD_KEY_BITS cells.  lut[g] is the last knot
// at or before the left edge of cell g, so the interval of x lies between lut[g] and lut[g + 1] and is found by bisection
// between the two: no step for a log grid with fewer than 64 knots per octave, at most log2(nk) for any table.
#define RSD_KEY_BITS 6
#define RSD_MAX_CELLS ((2047 << RSD_KEY_BITS) + 1)

__device__ static inline long rsd_key(double x) {       // x >= 0 (negative knots all share the cell of 0)
    return x > 0.0 ? (__double_as_longlong(x) >> (52 - RSD_KEY_BITS)) : 0;
}

__global__ void xi_rsd_records_kernel(const double *__restrict__ kx, const double *__restrict__ ky,
                                      const double *__restrict__ ky2, int nk, int nfun, int nlut,
                                      double *__restrict__ rec, int *__restrict__ lut) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    const int RS = RSD_REC(nfun);
    if (t < nk - 1) {
        double *R = rec + (size_t)t * RS;
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
        for (int e = 4 + 4 * nfun; e < RS; e++) R[e] = 0.0;
    }
    const long key0 = rsd_key(kx[0]);
    if (t < nlut && t <= rsd_key(kx[nk - 1]) - key0) {
        const double edge = t ? __longlong_as_double((key0 + t) << (52 - RSD_KEY_BITS)) : fmax(kx[0], 0.0);
        lut[t] = min(spline_lut_cell(kx, nk, edge), nk - 2);
    }
}

// tables in the order vv0 vv2 vv4 (dd0 dv0 dv2); coef rows (b1 b2, (b1 f2 + b2 f1) / 2, f1 f2, D1 D2 pf1 pf2), point i
// reads row i % ncoef.  The combination is the reference's expression in its order, without contraction.
template <int NF>
__global__ void __launch_bounds__(256)
xi_rsd_kernel(const double *__restrict__ rec, const int *__restrict__ lut, int nk, int nlut,
              const double *__restrict__ pi, const double *__restrict__ sigma, long n, const double *__restrict__ coef,
              long ncoef, double *__restrict__ out) {
    constexpr int RS = RSD_REC(NF);
    const double *last = rec + (size_t)(nk - 2) * RS;
    const double xfirst = rec[0], xlast = last[1];
    const long key0 = rsd_key(xfirst);
    const int ncell = (int)min((long)nlut, rsd_key(xlast) - key0 + 1);
    for (long q = (long)blockIdx.x * blockDim.x + threadIdx.x; q < n; q += (long)gridDim.x * blockDim.x) {
        const double p = pi[q], sg = sigma[q];
        double r, mu;
        {
#pragma clang fp contract(off)
            r = sqrt(p * p + sg * sg);
            mu = p / (r + 1e-100);
        }
        double s[NF];
        if (r < xfirst) {
#pragma unroll
            for (int f = 0; f < NF; f++) s[f] = spline_below(rec[0], rec[1], rec[4 + 4 * f], rec[5 + 4 * f], rec[7 + 4 * f], r);
        } else if (r >= xlast) {
#pragma unroll
            for (int f = 0; f < NF; f++) s[f] = spline_above(last[0], last[1], last[4 + 4 * f], last[5 + 4 * f], last[6 + 4 * f], r);
        } else {
            // xfirst <= r < xlast (or r is NaN: every comparison fails and the bisection ends at the top of its cell)
            long g = rsd_key(r) - key0;
            g = g < 0 ? 0 : (g >= ncell ? ncell - 1 : g);
            int kl = lut[g], kh = (g + 1 < ncell ? lut[g + 1] : nk - 2) + 1;
            while (kh - kl > 1) {
                const int km = (kh + kl) >> 1;
                if (rec[(size_t)km * RS] > r) kh = km;
                else kl = km;
            }
            const double *R = rec + (size_t)kl * RS;
            const double xk = R[0], xk1 = R[1], ih = R[2], h2o6 = R[3];
#pragma unroll
            for (int f = 0; f < NF; f++)
                s[f] = spline_interp(xk, xk1, ih, h2o6, R[4 + 4 * f], R[5 + 4 * f], R[6 + 4 * f], R[7 + 4 * f], r);
        }
        // (a 64-bit remainder costs more than the rest of the point: none for one row, 32-bit where the counts allow it)
        const long row = ncoef == 1 ? 0 : (n <= 0xffffffffL && ncoef <= 0xffffffffL ? (long)((unsigned)q % (unsigned)ncoef) : q % ncoef);
        const double *c = coef + 4 * row;
        const double c0 = c[0], c1 = c[1], c2 = c[2], c3 = c[3];
        {
#pragma clang fp contract(off)
            const double vv0 = s[0] * c2, vv2 = s[1] * c2, vv4 = s[2] * c2;
            const double dd0 = (NF == 6 ? s[3] : s[0]) * c0;
            const double dv0 = (NF == 6 ? s[4] : s[0]) * c1, dv2 = (NF == 6 ? s[5] : s[1]) * c1;
            const double mu2 = mu * mu;
            const double pl2 = (3.0 * mu2 - 1.0) / 2.0;
            const double pl4 = (35.0 * (mu2 * mu2) - 30.0 * mu2 + 3.0) / 8.0;
            out[q] = ((dd0 + 2.0 / 3.0 * dv0 + 1.0 / 5.0 * vv0) - (4.0 / 3.0 * dv2 + 4.0 / 7.0 * vv2) * pl2
                      + 8.0 / 35.0 * vv4 * pl4) * c3;
        }
    }
}

extern "C" {

int corahip_xi_rsd(corahip_ctx *ctx, const double *knots_x, const double *knots_y, const double *knots_y2, int nk,
                   int nfun, const double *pi, const double *sigma, long n, const double *coef, long ncoef,
                   double *out) {
    if (nfun != 3 && nfun != 6) {
        corahip_set_error("invalid argument: nfun = %d tables, xi_rsd takes 3 (vv0 vv2 vv4) or 6 (+ dd0 dv0 dv2) (%s:%d)",
                          nfun, __FILE__, __LINE__);
        return CORAHIP_EINVAL;
    }
    if (nk < 4 || nk > RSD_MAX_KNOTS) {
        corahip_set_error("invalid argument: nk = %d knots, xi_rsd takes 4 to %d (%s:%d)", nk, RSD_MAX_KNOTS, __FILE__, __LINE__);
        return CORAHIP_EINVAL;
    }
    ARG_CHECK(ncoef >= 1 && n >= 0);
    ARG_CHECK(ctx != nullptr && knots_x && knots_y && knots_y2 && pi && sigma && coef && out);
    if (n == 0) return 0;
    StageTimer t(ctx, "xi_rsd");
    const int nlut = RSD_MAX_CELLS;     // (the cells in use depend on the knots, which are on the device: room for all)
    const size_t rec_bytes = sizeof(double) * RSD_REC(nfun) * (size_t)(nk - 1);
    char *ws = nullptr;
    int rc = corahip_ctx_scratch(ctx, RSD_SCRATCH, rec_bytes + sizeof(int) * (size_t)nlut, (void **)&ws);
    if (rc) return rc;
    double *rec = reinterpret_cast<double *>(ws);
    int *lut = reinterpret_cast<int *>(ws + rec_bytes);
    xi_rsd_records_kernel<<<(std::max(nlut, nk) + 255) / 256, 256, 0, ctx->stream>>>(knots_x, knots_y, knots_y2, nk, nfun, nlut, rec, lut);
    LAUNCH_CHECK();
    const unsigned blocks = grid_blocks(ctx, n, 8);
    if (nfun == 3) xi_rsd_kernel<3><<<blocks, 256, 0, ctx->stream>>>(rec, lut, nk, nlut, pi, sigma, n, coef, ncoef, out);
    else xi_rsd_kernel<6><<<blocks, 256, 0, ctx->stream>>>(rec, lut, nk, nlut, pi, sigma, n, coef, ncoef, out);
    LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
