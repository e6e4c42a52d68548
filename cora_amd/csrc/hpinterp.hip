// hpinterp.hip - HEALPix RING bilinear interpolation (healpy.get_interp_weights / get_interp_val) as a gather and as a
// scatter: interpolation weights and values at given directions, the fused rotation of a stack of maps
// (cora/util/hputil.py:534-604 coord_x2y) and the grid form of the Zel'dovich density step
// (cora/signal/lss.py:996-1096 za_density_grid).
//
// The scheme is the published HEALPix one (get_interpol, Gorski et al. 2005), restated: the two rings around theta,
// on each the two nearest pixel centres with weights linear in phi (wrapping round), between the rings weights linear in
// theta; past the first / last ring the pole is a virtual sample, the mean of the 4 pixels of that ring.  interp_geom
// repeats tests/_interp_oracle.py (interp_weights) operation for operation, without contraction into FMAs, so that
// both pick the same cell away from exact ties.  Ring colatitudes are acos of the ring's z as pix2zphi forms it: a query
// at a pixel centre sits exactly on its ring.
//
// Every pixel index is sp + (i mod nr) of a ring 1 .. 4 nside - 1, whatever theta and phi hold (NaN included), so no
// gather or scatter leaves the map.  The gathers have no atomics: identical bits from call to call.  The density step
// adds with global f64 atomics, 8 per particle: sums depend on arrival order, repeated calls agree to rounding only.
#include "healpix_geom.h"

namespace {

struct Rot {
    double m[9];
};

// colatitude of ring ir (1 .. 4 nside - 1); 0 for ir <= 0 and pi for ir >= 4 nside
__device__ inline double ring_theta(const Geom &g, long ir) {
#pragma clang fp contract(off)
    const long ns = g.nside;
    if (ir <= 0) return 0.0;
    if (ir >= 4 * ns) return M_PI;
    const double dn = (double)ns;
    if (ir < ns || ir > 3 * ns) {
        const bool south = ir > 3 * ns;
        const double di = (double)(south ? 4 * ns - ir : ir);
        const double zc = 1.0 - di * di / (3.0 * dn * dn);
        return acos(south ? -zc : zc);
    }
    return acos(4.0 / 3.0 - 2.0 * (double)ir / (3.0 * dn));
}

// the two pixels of ring ir (1 .. 4 nside - 1) around phi and the weight w of the second one
__device__ inline void along_ring(const Geom &g, long ir, double phi, long &p0, long &p1, double &w) {
#pragma clang fp contract(off)
    const long ns = g.nside;
    long sp, nr;
    double sh = 1.0;
    if (ir < ns) {
        nr = 4 * ir;
        sp = 2 * ir * (ir - 1);
    } else if (ir > 3 * ns) {
        const long j = 4 * ns - ir;
        nr = 4 * j;
        sp = g.npix - 2 * j * (j + 1);
    } else {
        nr = 4 * ns;
        sp = g.ncap + (ir - ns) * 4 * ns;
        sh = ((ir - ns) & 1) == 0 ? 1.0 : 0.0;
    }
    const double dphi = 2.0 * M_PI / (double)nr;
    double f1 = floor(phi / dphi - 0.5 * sh);
    if (!(f1 >= -1.0 && f1 <= (double)nr)) f1 = 0.0;             // a phi that is not finite: any pixel of the ring
    w = (phi - (f1 + 0.5 * sh) * dphi) / dphi;
    long i1 = (long)f1 % nr;                                     // f1 in [-1, nr] for phi in [0, 2 pi]
    if (i1 < 0) i1 += nr;
    p0 = sp + i1;
    p1 = sp + (i1 + 1 == nr ? 0 : i1 + 1);
}

// (nside, theta, phi) -> pix[4], w[4]: the upper ring's pair, then the lower ring's
__device__ inline void interp_geom(const Geom &g, double theta, double phi_in, long pix[4], double w[4]) {
#pragma clang fp contract(off)
    const long ns = g.nside, nl4 = 4 * ns;
    const double dn = (double)ns;
    const double phi = np_mod(phi_in, 2.0 * M_PI);
    // ring_above: a first guess from z, then the rings are compared in theta, where the weights are formed
    const double z = cos(theta);
    const double za = fabs(z);
    double gs;
    if (za <= 2.0 / 3.0) {
        gs = floor(dn * (2.0 - 1.5 * z));
    } else {
        gs = floor(dn * sqrt(3.0 * (1.0 - za)));
        if (!(z > 0)) gs = (double)nl4 - gs - 1.0;
    }
    long ir1 = (long)fmin(fmax(gs, 0.0), (double)(nl4 - 1));
    ir1 = min(max(ir1, 0L), nl4 - 1);
    while (ir1 > 0 && theta < ring_theta(g, ir1)) --ir1;
    while (ir1 < nl4 - 1 && theta >= ring_theta(g, ir1 + 1)) ++ir1;
    const long ir2 = ir1 + 1;
    const bool npole = ir1 == 0, spole = ir2 == nl4;
    const double th1 = ring_theta(g, ir1), th2 = ring_theta(g, ir2);
    long a0, a1, b0, b1;
    double wa, wb;
    along_ring(g, npole ? 1 : ir1, phi, a0, a1, wa);
    along_ring(g, spole ? nl4 - 1 : ir2, phi, b0, b1, wb);
    const double wt = (theta - th1) / (th2 - th1);
    pix[0] = a0;
    pix[1] = a1;
    pix[2] = b0;
    pix[3] = b1;
    w[0] = (1.0 - wa) * (1.0 - wt);
    w[1] = wa * (1.0 - wt);
    w[2] = (1.0 - wb) * wt;
    w[3] = wb * wt;
    if (npole) {
        const double fn = (1.0 - wt) * 0.25;
        pix[0] = (b0 + 2) & 3;
        pix[1] = (b1 + 2) & 3;
        w[0] = fn;
        w[1] = fn;
        w[2] = w[2] + fn;
        w[3] = w[3] + fn;
    }
    if (spole) {
        const double fs = wt * 0.25;
        pix[2] = ((a0 + 2) & 3) + g.npix - 4;
        pix[3] = ((a1 + 2) & 3) + g.npix - 4;
        w[2] = fs;
        w[3] = fs;
        w[0] = w[0] + fs;
        w[1] = w[1] + fs;
    }
}

// out[m][q] = sum_k w[k] maps[m][pix[k]] for every map; weights stay in registers
__device__ inline void gather_maps(const double *__restrict__ maps, long nmap, long npix, const long pix[4],
                                   const double w[4], double *__restrict__ out, long ld_out, long q) {
#pragma clang fp contract(off)
    const double *row = maps;
    double *o = out + q;
#pragma unroll 4
    for (long m = 0; m < nmap; ++m, row += npix, o += ld_out)
        *o = ((w[0] * row[pix[0]] + w[1] * row[pix[1]]) + w[2] * row[pix[2]]) + w[3] * row[pix[3]];
}

__global__ __launch_bounds__(256) void interp_weights_kernel(Geom g, const double *__restrict__ theta,
                                                             const double *__restrict__ phi, long n,
                                                             long *__restrict__ pix_out, double *__restrict__ w_out) {
    for (long q = (long)blockIdx.x * blockDim.x + threadIdx.x; q < n; q += (long)gridDim.x * blockDim.x) {
        long pix[4];
        double w[4];
        interp_geom(g, theta[q], phi[q], pix, w);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            pix_out[k * n + q] = pix[k];
            w_out[k * n + q] = w[k];
        }
    }
}

__global__ __launch_bounds__(256) void interp_val_kernel(Geom g, const double *__restrict__ maps, long nmap,
                                                         const double *__restrict__ theta, const double *__restrict__ phi,
                                                         long n, double *__restrict__ out) {
    for (long q = (long)blockIdx.x * blockDim.x + threadIdx.x; q < n; q += (long)gridDim.x * blockDim.x) {
        long pix[4];
        double w[4];
        interp_geom(g, theta[q], phi[q], pix, w);
        gather_maps(maps, nmap, g.npix, pix, w, out, n, q);
    }
}

// out[m][p] = interp(maps[m], R n_p): one thread per output pixel, no theta / phi arrays in memory
__global__ __launch_bounds__(256) void rotate_maps_kernel(Geom g, const double *__restrict__ maps, long nmap, Rot R,
                                                          double *__restrict__ out) {
#pragma clang fp contract(off)
    for (long p = (long)blockIdx.x * blockDim.x + threadIdx.x; p < g.npix; p += (long)gridDim.x * blockDim.x) {
        double v[3];
        pix2vec(g, p, v);
        const double r0 = (R.m[0] * v[0] + R.m[1] * v[1]) + R.m[2] * v[2];
        const double r1 = (R.m[3] * v[0] + R.m[4] * v[1]) + R.m[5] * v[2];
        const double r2 = (R.m[6] * v[0] + R.m[7] * v[1]) + R.m[8] * v[2];
        const double theta = atan2(sqrt(r0 * r0 + r1 * r1), r2);
        double phi = atan2(r1, r0);
        if (phi < 0.0) phi = phi + 2.0 * M_PI;
        long pix[4];
        double w[4];
        interp_geom(g, theta, phi, pix, w);
        gather_maps(maps, nmap, g.npix, pix, w, out, g.npix, p);
    }
}

// one thread per particle e = ii npix + p (64-bit): 4 pixels x 2 radial bins receive rho pw rw
__global__ __launch_bounds__(256) void za_grid_kernel(Geom g, const double *__restrict__ psi,
                                                      const double *__restrict__ delta_b, const double *__restrict__ chi,
                                                      int nchi, double *__restrict__ out) {
#pragma clang fp contract(off)
    const long npix = g.npix;
    const long plane = (long)nchi * npix;
    // chi extended by one extrapolated cell at each end (lss.py:1041-1046): ext[0], ext[k + 1] = chi[k], ext[nchi + 1]
    const double ext_lo = chi[0] - (chi[1] - chi[0]);
    const double ext_hi = chi[nchi - 1] + (chi[nchi - 1] - chi[nchi - 2]);
    const int next = nchi + 2;
    auto ext = [&](int k) { return k == 0 ? ext_lo : (k == next - 1 ? ext_hi : chi[k - 1]); };
    for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < plane; e += (long)gridDim.x * blockDim.x) {
        const int ii = (int)(e / npix);
        const long p = e - (long)ii * npix;
        double zp, php;
        pix2zphi(g, p, zp, php);
        const double thp = acos(zp);
        const double rho = 1.0 + delta_b[e];
        double th, ph;
        displaced_position(thp, php, psi[plane + e], psi[2 * plane + e], th, ph);
        const double x = chi[ii] + psi[e];

        long pix[4];
        double pw[4];
        interp_geom(g, th, ph, pix, pw);

        // np.digitize(x, ext): the number of ext[k] <= x (0 .. nchi + 2; a NaN counts none and drops both bins)
        int lo = 0, hi = next;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (ext(mid) <= x) lo = mid + 1;
            else hi = mid;
        }
        const double chi0 = ext((lo - 1 + next) % next), chi1 = ext(lo % next);
        const double dchi = chi1 - chi0;
        const double rw[2] = {fabs((chi1 - x) / dchi), fabs((x - chi0) / dchi)};
        const int rb[2] = {lo - 2, lo - 1};
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            if (rb[j] < 0 || rb[j] >= nchi) continue;             // outside chi: that share is dropped, as in the reference
            double *row = out + (long)rb[j] * npix;
#pragma unroll
            for (int k = 0; k < 4; ++k) atomicAdd(&row[pix[k]], (rho * pw[k]) * rw[j]);
        }
    }
}

}  // namespace

int corahip_healpix_interp_weights(corahip_ctx *ctx, int nside, const double *theta, const double *phi, long n,
                                   int64_t *pix_out, double *w_out) {
    ARG_CHECK(ctx && theta && phi && pix_out && w_out && nside >= 1 && nside <= 8192 && n >= 0);
    if (n == 0) return 0;
    StageTimer st(ctx, "healpix_interp_weights");
    hipLaunchKernelGGL(interp_weights_kernel, dim3(grid_blocks(ctx, n)), dim3(256), 0, ctx->stream, make_geom(nside), theta,
                       phi, n, (long *)pix_out, w_out);
    LAUNCH_CHECK();
    return 0;
}

int corahip_healpix_interp_val(corahip_ctx *ctx, const double *maps, long nmap, int nside, const double *theta,
                               const double *phi, long n, double *out) {
    ARG_CHECK(ctx && maps && theta && phi && out && nside >= 1 && nside <= 8192 && nmap >= 1 && n >= 0);
    if (n == 0) return 0;
    StageTimer st(ctx, "healpix_interp_val");
    hipLaunchKernelGGL(interp_val_kernel, dim3(grid_blocks(ctx, n)), dim3(256), 0, ctx->stream, make_geom(nside), maps, nmap,
                       theta, phi, n, out);
    LAUNCH_CHECK();
    return 0;
}

int corahip_healpix_rotate_maps(corahip_ctx *ctx, const double *maps, long nmap, int nside, const double *R, double *out) {
    ARG_CHECK(ctx && maps && R && out && nside >= 1 && nside <= 8192 && nmap >= 1);
    const Geom g = make_geom(nside);
    const size_t bytes = (size_t)nmap * (size_t)g.npix * sizeof(double);
    ARG_CHECK(!overlaps(out, bytes, maps, bytes));
    Rot rot;
    for (int i = 0; i < 9; ++i) rot.m[i] = R[i];
    StageTimer st(ctx, "healpix_rotate_maps");
    hipLaunchKernelGGL(rotate_maps_kernel, dim3(grid_blocks(ctx, g.npix)), dim3(256), 0, ctx->stream, g, maps, nmap, rot, out);
    LAUNCH_CHECK();
    return 0;
}

int corahip_za_density_grid(corahip_ctx *ctx, const double *psi, const double *delta_bias, const double *chi, int nchi,
                            int nside, double *out) {
    ARG_CHECK(ctx && psi && delta_bias && chi && out);
    ARG_CHECK(nchi >= 2 && nside >= 1 && nside <= 8192);
    StageTimer st(ctx, "za_density_grid");
    const Geom g = make_geom(nside);
    const long n = (long)nchi * g.npix;
    hipLaunchKernelGGL(za_grid_kernel, dim3(grid_blocks(ctx, n)), dim3(256), 0, ctx->stream, g, psi, delta_bias, chi, nchi, out);
    LAUNCH_CHECK();
    hipLaunchKernelGGL(minus_one_kernel, dim3(grid_blocks(ctx, n)), dim3(256), 0, ctx->stream, out, n);
    LAUNCH_CHECK();
    return 0;
}
