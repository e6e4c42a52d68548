// pmesh.hip - Zel'dovich SPH density assignment (cora/signal/lss.py:1305-1419 za_density_sph with
// cora/util/pmesh.pyx:29-279 + pmesh_util.c:4-42) and the HEALPix RING neighbour table it needs.
//
// Geometry: get_all_neighbours restated from the published HEALPix algorithm (Gorski et al. 2005): ring -> (x, y, face),
// step within or across base faces (the tables below), back to ring.  The two conversions, ang2pix and the pixel
// centres are healpix_geom.h's, as for every other map-domain kernel; this file keeps (x, y) in int (nside <= 8192).
//
// Deposit: one workgroup owns a 16 x 16 block of one base face (RING pixels of those (x, y)) and 8 slices.  Its
// particles add into an LDS f64 tile of that block with a 4-pixel halo and 3 radial bins of halo on each side
// (ds_add_f64); a target outside the tile (another face, farther away) goes straight to a global f64 atomic add.  The
// tile is flushed once with global atomic adds of its non-zero cells.  Sums therefore depend on arrival order: repeated
// calls agree to rounding, not bit for bit.
#include "healpix_geom.h"

namespace {

constexpr int TB = 16;                 // face block edge (pixels) owned by a workgroup
constexpr int TH = 4;                  // angular halo of the tile (pixels)
constexpr int TE = TB + 2 * TH;        // tile edge
constexpr int TS = 8;                  // slices per workgroup
constexpr int TRH = 3;                 // radial halo (bins) on each side
constexpr int TNB = TS + 2 * TRH;      // radial bins of the tile
constexpr int TCELLS = TNB * TE * TE;  // 8064 doubles = 63 KiB of LDS

// base-face neighbour of face f across the side / corner nbnum (0..8, 4 = same face) and the (x, y) flips that go with
// it (bit 1: x -> n-1-x, 2: y -> n-1-y, 4: swap), by face row (face >> 2)
__constant__ int8_t c_nb_face[9][12] = {
    {8, 9, 10, 11, -1, -1, -1, -1, 10, 11, 8, 9},  // S
    {5, 6, 7, 4, 8, 9, 10, 11, 9, 10, 11, 8},      // SE
    {-1, -1, -1, -1, 5, 6, 7, 4, -1, -1, -1, -1},  // E
    {4, 5, 6, 7, 11, 8, 9, 10, 11, 8, 9, 10},      // SW
    {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11},        // centre
    {1, 2, 3, 0, 0, 1, 2, 3, 5, 6, 7, 4},          // NE
    {-1, -1, -1, -1, 7, 4, 5, 6, -1, -1, -1, -1},  // W
    {3, 0, 1, 2, 3, 0, 1, 2, 4, 5, 6, 7},          // NW
    {2, 3, 0, 1, -1, -1, -1, -1, 0, 1, 2, 3}};     // N
__constant__ int8_t c_nb_swap[9][3] = {{0, 0, 3}, {0, 0, 6}, {0, 0, 0}, {0, 0, 5}, {0, 0, 0},
                                       {5, 0, 0}, {0, 0, 0}, {6, 0, 0}, {3, 0, 0}};
// healpy's order of get_all_neighbours: SW, W, NW, N, NE, E, SE, S
__constant__ int8_t c_nb_dx[8] = {-1, -1, 0, 1, 1, 1, 0, -1};
__constant__ int8_t c_nb_dy[8] = {0, 1, 1, 1, 0, -1, -1, -1};

// the 8 neighbours of (ix, iy, face) in healpy's order: (x, y, face) each, face -1 where there is none
__device__ void neighbours_xyf(const Geom &g, int ix, int iy, int face, int nx[8], int ny[8], int nf[8]) {
    const int ns = (int)g.nside;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        int x = ix + c_nb_dx[i], y = iy + c_nb_dy[i];
        int nbnum = 4;
        if (x < 0) {
            x += ns;
            nbnum -= 1;
        } else if (x >= ns) {
            x -= ns;
            nbnum += 1;
        }
        if (y < 0) {
            y += ns;
            nbnum -= 3;
        } else if (y >= ns) {
            y -= ns;
            nbnum += 3;
        }
        int f = c_nb_face[nbnum][face];
        if (f >= 0) {
            int bits = c_nb_swap[nbnum][face >> 2];
            if (bits & 1) x = ns - x - 1;
            if (bits & 2) y = ns - y - 1;
            if (bits & 4) {
                int t = x;
                x = y;
                y = t;
            }
        }
        nx[i] = x;
        ny[i] = y;
        nf[i] = f;
    }
}

__global__ __launch_bounds__(256) void neighbours_kernel(Geom g, int32_t *__restrict__ out) {
    for (long p = (long)blockIdx.x * blockDim.x + threadIdx.x; p < g.npix; p += (long)gridDim.x * blockDim.x) {
        int ix, iy, f;
        ring2xyf(g, p, ix, iy, f);
        int nx[8], ny[8], nf[8];
        neighbours_xyf(g, ix, iy, f, nx, ny, nf);
        int32_t *o = out + p * 9;
        o[0] = (int32_t)p;
#pragma unroll
        for (int k = 0; k < 8; ++k) o[1 + k] = nf[k] >= 0 ? (int32_t)xyf2ring(g, nx[k], ny[k], nf[k]) : -1;
    }
}

// grid: x = face block (nbf^2 per face), y = base face, z = group of TS slices
__global__ __launch_bounds__(256) void za_sph_kernel(Geom g, const double *__restrict__ psi,
                                                     const double *__restrict__ delta_b,
                                                     const double *__restrict__ delta_m,
                                                     const double *__restrict__ chi, int nchi, double sigma_ang,
                                                     double sigma_chi, double *__restrict__ out) {
#pragma clang fp contract(off)
    __shared__ double acc[TCELLS];
    const int nbf = (int)((g.nside + TB - 1) / TB);
    const int face = blockIdx.y;
    const int x0 = (int)(blockIdx.x % nbf) * TB, y0 = (int)(blockIdx.x / nbf) * TB;
    const int s0 = blockIdx.z * TS;
    const int b0 = s0 - TRH;
    const int tx0 = x0 - TH, ty0 = y0 - TH;
    const long npix = g.npix;
    const long plane = (long)nchi * npix;

    for (int c = threadIdx.x; c < TCELLS; c += blockDim.x) acc[c] = 0.0;
    __syncthreads();

    const int x = x0 + (int)(threadIdx.x % TB), y = y0 + (int)(threadIdx.x / TB);
    if (x < g.nside && y < g.nside) {
        const long p = xyf2ring(g, x, y, face);
        double zp, php;
        pix2zphi(g, p, zp, php);
        const double thp = acos(zp);
        const int s1 = min(s0 + TS, nchi);
        for (int ii = s0; ii < s1; ++ii) {
            const long e = (long)ii * npix + p;                    // 64-bit particle index
            const double rho = 1.0 + delta_b[e];
            const double dr = psi[e], dth = psi[plane + e], dph = psi[2 * plane + e];
            double sc = fmin(fmax(1.0 + delta_m[e], 0.1), 3.0);
            sc = pow(sc, -1.0 / 3.0);

            // pmesh.calculate_positions
            double th, ph;
            displaced_position(thp, php, dth, dph, th, ph);
            const double nchi_pos = chi[ii] + dr;

            // angular weights over the pixel of the new position and its 8 neighbours (pmesh._pixel_weights).
            // sin^2 of the angle as |v x w|^2, not 1 - (v.w)^2: equal for unit vectors, without the cancellation
            const long q = ang2pix(g, th, ph);
            double st, ct, sp, cp;
            sincos(th, &st, &ct);
            sincos(ph, &sp, &cp);
            const double w0 = st * cp, w1 = st * sp, w2 = ct;
            int cx[9], cy[9], cf[9];
            ring2xyf(g, q, cx[0], cy[0], cf[0]);
            neighbours_xyf(g, cx[0], cy[0], cf[0], cx + 1, cy + 1, cf + 1);
            const double sa = sc * sigma_ang;
            const double inv_sa2 = 1.0 / (sa * sa);
            long cpix[9];
            double pw[9], wsum = 0.0;
#pragma unroll
            for (int k = 0; k < 9; ++k) {
                if (cf[k] >= 0) {
                    cpix[k] = k == 0 ? q : xyf2ring(g, cx[k], cy[k], cf[k]);
                    double v[3];
                    pix2vec(g, cpix[k], v);
                    const double c0 = v[1] * w2 - v[2] * w1, c1 = v[2] * w0 - v[0] * w2, c2 = v[0] * w1 - v[1] * w0;
                    const double d2 = c0 * c0 + c1 * c1 + c2 * c2;
                    pw[k] = exp(-0.5 * d2 * inv_sa2);
                } else {
                    cpix[k] = 0;
                    pw[k] = 0.0;
                }
                wsum += pw[k];
            }

            // radial weights over 3 bins (pmesh._radial_weights, nnh = 1); ind = searchsorted(chi, new_chi, 'left')
            int lo = 0, hi = nchi;
            while (lo < hi) {
                int mid = (lo + hi) >> 1;
                if (chi[mid] < nchi_pos) lo = mid + 1;
                else hi = mid;
            }
            const int low = min(max(0, lo - 1), nchi - 3);
            const double sr = sc * sigma_chi;
            const double inv_sr2 = 1.0 / (sr * sr);
            double rw[3], rsum = 0.0;
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const double dc = chi[low + j] - nchi_pos;
                rw[j] = exp(-0.5 * (dc * dc) * inv_sr2);
                rsum += rw[j];
            }

            // deposit rho w_pix w_bin: into the tile when the voxel is in it, else straight to out
#pragma unroll
            for (int k = 0; k < 9; ++k) {
                if (cf[k] < 0) continue;
                const double v = rho * (pw[k] / wsum);
                const int lx = cx[k] - tx0, ly = cy[k] - ty0;
                const bool in_xy = cf[k] == face && (unsigned)lx < (unsigned)TE && (unsigned)ly < (unsigned)TE;
#pragma unroll
                for (int j = 0; j < 3; ++j) {
                    const double d = v * (rw[j] / rsum);
                    const int b = low + j;
                    const int lb = b - b0;
                    if (in_xy && (unsigned)lb < (unsigned)TNB)
                        atomicAdd(&acc[(lb * TE + ly) * TE + lx], d);
                    else
                        atomicAdd(&out[(long)b * npix + cpix[k]], d);
                }
            }
        }
    }
    __syncthreads();

    // flush the tile: one global add per non-zero cell (cells off the face or outside [0, nchi) never receive one)
    for (int c = threadIdx.x; c < TCELLS; c += blockDim.x) {
        const double v = acc[c];
        if (v == 0.0) continue;
        const int lb = c / (TE * TE), r = c % (TE * TE);
        const int gx = tx0 + r % TE, gy = ty0 + r / TE, b = b0 + lb;
        if (b < 0 || b >= nchi || gx < 0 || gy < 0 || gx >= g.nside || gy >= g.nside) continue;
        atomicAdd(&out[(long)b * npix + xyf2ring(g, gx, gy, face)], v);
    }
}

}  // namespace

int corahip_healpix_neighbours(corahip_ctx *ctx, int nside, int32_t *out) {
    ARG_CHECK(ctx && out && nside >= 1 && nside <= 8192);
    StageTimer st(ctx, "healpix_neighbours");
    const Geom g = make_geom(nside);
    hipLaunchKernelGGL(neighbours_kernel, dim3(grid_blocks(ctx, g.npix)), dim3(256), 0, ctx->stream, g, out);
    LAUNCH_CHECK();
    return 0;
}

int corahip_za_density_sph(corahip_ctx *ctx, const double *psi, const double *delta_bias, const double *delta_m,
                           const double *chi, int nchi, int nside, double sigma_ang, double sigma_chi, double *out) {
    ARG_CHECK(ctx && psi && delta_bias && delta_m && chi && out);
    ARG_CHECK(nchi >= 3 && nside >= 1 && nside <= 8192 && (nchi + TS - 1) / TS <= 65535);
    ARG_CHECK(sigma_ang > 0.0 && sigma_chi > 0.0);
    StageTimer st(ctx, "za_density_sph");
    const Geom g = make_geom(nside);
    const long nbf = (nside + TB - 1) / TB;
    hipLaunchKernelGGL(za_sph_kernel, dim3((unsigned)(nbf * nbf), 12u, (unsigned)((nchi + TS - 1) / TS)), dim3(256), 0,
                       ctx->stream, g, psi, delta_bias, delta_m, chi, nchi, sigma_ang, sigma_chi, out);
    LAUNCH_CHECK();
    const long n = (long)nchi * g.npix;
    hipLaunchKernelGGL(minus_one_kernel, dim3(grid_blocks(ctx, n)), dim3(256), 0, ctx->stream, out, n);
    LAUNCH_CHECK();
    return 0;
}
