// lofar.hip - the body of LofarGDSE.getfield (cora/foreground/lofar.py:63-71) behind its two random fields: the
// standard deviations the fields are rescaled by, and the line-of-sight sum of a power law per voxel.
//
//   powerlaw_los_kernel    out[i, p] = sum_z (a0 + sa A[p, z]) exp(x[i] (b0 + sb beta[p, z])),  x[i] = ln(nu_i / nu_0).
//                          A workgroup owns 64 pixels (columns of the [ncol, nz] fields) and walks the channels in blocks
//                          of 32: wave w takes channels 8 w .. 8 w + 7 of the block, lane l pixel l, eight accumulators in
//                          registers.  Depth is the contiguous axis, so a lane-per-pixel walk of global memory would read
//                          with stride 8 nz: the fields go through LDS in chunks of 32 depths instead - 32 neighbouring
//                          lanes read one 256-byte run of a column, and apply the affine maps (one fma each, so a and b
//                          are rounded once) on the way in; rows are padded to 33 doubles, which makes the lane-per-pixel
//                          reads conflict-free.  Per (pixel, channel): t = x b, e = exp(t), acc = fma(a, e, acc), z
//                          ascending from 0 to nz - 1.  That order does not know the launch shape, the channel block or the
//                          number of live channels of a wave: a channel computed alone has the bits of the same channel
//                          computed among many.  x[i] is the same address in every lane (a scalar load).
//                          exp is glibc's (glibc_exp.h): below 1 ulp for |t| < 512, which the caller ensures (E = 1 in
//                          the bound of tests/_lofar_oracle.py).
//                          One writer per element of out, no atomics.  The fields are re-read once per block of 32
//                          channels (the channel blocks of a pixel tile run in one workgroup, or in neighbouring ones
//                          when the pixel tiles alone do not fill the device): 16 bytes per 32 exponentials, served by
//                          the caches where the tile stays in them - the kernel is bound by the FP64 exp rate either way.
//   fm_*                   field_moments: the column sums s[p] = sum_z f[p, z] (a wave per column: lane l sums depths
//                          l, l + 64, ..., then a halving __shfl_down tree), then mean and population variance of s and
//                          of all elements by block partials and one ordered final pass, twice each (the mean first, then
//                          sum (v - mean)^2: two passes, nothing cancels), as complex_variance does; max |f| rides on the
//                          first pass over the elements.  corahip_slice_moments is not used: it would give the column
//                          sums at one workgroup per 8 nz bytes, it has no maximum, and its sum of squares of a flat field
//                          needs the mean on the host in between.  No atomics, every order a function of the shape alone.
// All element offsets are 64-bit.
#include "common.h"
#include "glibc_exp.h"

namespace {

constexpr int PL_NT = 256;                          // 4 waves
constexpr int PL_PT = 64;                           // pixels per workgroup, one per lane
constexpr int PL_ZC = 32;                           // depths per LDS chunk
constexpr int PL_LS = PL_ZC + 1;                    // LDS row stride (doubles)
constexpr int PL_FC = 8;                            // channels per wave
constexpr int PL_FB = PL_FC * (PL_NT / 64);         // channels per workgroup pass
constexpr int PL_SR = PL_NT / PL_ZC;                // rows per staging step

// nzc depths of one pixel (as, bs: its LDS rows) into the accumulators of the wave's channels
template <bool FULL>
__device__ __forceinline__ void pl_chunk(const double *as, const double *bs, int nzc, const double (&xs)[PL_FC], int nlive,
                                         double (&acc)[PL_FC]) {
#pragma clang fp contract(off)
    for (int z = 0; z < nzc; z++) {
        const double a = as[z], b = bs[z];
#pragma unroll
        for (int j = 0; j < PL_FC; j++)
            if (FULL || j < nlive) acc[j] = fma(a, glibc_exp_fma(xs[j] * b), acc[j]);
    }
}

// grid: x pixel tiles, y workgroups that share the channel blocks of a tile (block fb goes to y = fb mod gridDim.y)
__global__ void __launch_bounds__(PL_NT)
powerlaw_los_kernel(const double *__restrict__ A, const double *__restrict__ B, const double *__restrict__ x, double a0,
                    double sa, double b0, double sb, int nfreq, long ncol, int nz, int nfb, double *__restrict__ out) {
    __shared__ double As[PL_PT * PL_LS], Bs[PL_PT * PL_LS];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const long p0 = (long)blockIdx.x * PL_PT;
    const int sz = tid & (PL_ZC - 1), sr = tid / PL_ZC;
    for (int fb = blockIdx.y; fb < nfb; fb += gridDim.y) {
        const int f0 = fb * PL_FB + wave * PL_FC;
        const int nlive = nfreq - f0 < 0 ? 0 : (nfreq - f0 > PL_FC ? PL_FC : nfreq - f0);
        double xs[PL_FC], acc[PL_FC];
#pragma unroll
        for (int j = 0; j < PL_FC; j++) {
            xs[j] = j < nlive ? x[f0 + j] : 0.0;
            acc[j] = 0.0;
        }
        for (int z0 = 0; z0 < nz; z0 += PL_ZC) {
            __syncthreads();                                  // the chunk before has been consumed
#pragma unroll
            for (int u = 0; u < PL_PT / PL_SR; u++) {
                const int row = sr + PL_SR * u;
                const long p = p0 + row;
                const int z = z0 + sz;
                const bool in = p < ncol && z < nz;
                const size_t e = (size_t)p * (size_t)nz + (size_t)z;
                As[row * PL_LS + sz] = in ? fma(sa, A[e], a0) : 0.0;
                Bs[row * PL_LS + sz] = in ? fma(sb, B[e], b0) : 0.0;
            }
            __syncthreads();
            const int nzc = nz - z0 < PL_ZC ? nz - z0 : PL_ZC;
            if (nlive == PL_FC)
                pl_chunk<true>(As + lane * PL_LS, Bs + lane * PL_LS, nzc, xs, nlive, acc);
            else if (nlive > 0)
                pl_chunk<false>(As + lane * PL_LS, Bs + lane * PL_LS, nzc, xs, nlive, acc);
        }
        if (p0 + lane < ncol) {
#pragma unroll
            for (int j = 0; j < PL_FC; j++)
                if (j < nlive) out[(size_t)(f0 + j) * (size_t)ncol + (size_t)(p0 + lane)] = acc[j];
        }
    }
}

// ---- field moments ---------------------------------------------------------------------------------------------------

constexpr int FM_MAXB = 4096;     // partials_split gives at most this many

// a wave per column
__global__ void __launch_bounds__(256) fm_colsum_kernel(const double *__restrict__ f, long ncol, int nz, double *__restrict__ s) {
    const int lane = threadIdx.x & 63;
    const long p = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (p >= ncol) return;
    const double *col = f + (size_t)p * (size_t)nz;
    double a = 0.0;
    for (int z = lane; z < nz; z += 64) a += col[z];
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) a += __shfl_down(a, o, 64);
    if (lane == 0) s[p] = a;
}

// PASS 0: partial sum of v and partial max |v|.  PASS 1: partial sum of (v - m)^2, m = st[0] (second slot 0).
template <int PASS>
__global__ void __launch_bounds__(256)
fm_partial_kernel(const double *__restrict__ v, long count, long per, const double *__restrict__ st, double *__restrict__ work) {
#pragma clang fp contract(off)
    __shared__ double red[256];
    const long lo = (long)blockIdx.x * per;
    const long hi = lo + per < count ? lo + per : count;
    const double m = PASS ? st[0] : 0.0;
    double a = 0.0, b = 0.0;
    for (long i = lo + threadIdx.x; i < hi; i += 256) {
        const double t = v[i];
        if (PASS == 0) {
            a += t;
            b = fmax(b, fabs(t));
        } else {
            const double d = t - m;
            a += d * d;
        }
    }
    a = block_reduce<256>(a, red, [](double p, double q) { return p + q; });
    if (PASS == 0) b = block_reduce<256>(b, red, [](double p, double q) { return fmax(p, q); });
    if (threadIdx.x == 0) work[2 * (size_t)blockIdx.x] = a, work[2 * (size_t)blockIdx.x + 1] = b;
}

// PASS 0: st[0] = mean, *vmax (if given) = max.  PASS 1: *sd = sqrt(sum / count).
template <int PASS>
__global__ void __launch_bounds__(256)
fm_final_kernel(const double *__restrict__ work, int nb, long count, double *__restrict__ st, double *__restrict__ sd,
                double *__restrict__ vmax) {
    __shared__ double red[256];
    double a = 0.0, b = 0.0;
    for (int i = threadIdx.x; i < nb; i += 256) {
        a += work[2 * (size_t)i];
        b = fmax(b, work[2 * (size_t)i + 1]);
    }
    a = block_reduce<256>(a, red, [](double p, double q) { return p + q; });
    if (PASS == 0) b = block_reduce<256>(b, red, [](double p, double q) { return fmax(p, q); });
    if (threadIdx.x == 0) {
        if (PASS == 0) {
            st[0] = a / (double)count;
            if (vmax) *vmax = b;
        } else {
            *sd = sqrt(a / (double)count);
        }
    }
}

// population standard deviation of v [count] -> *sd, max |v| -> *vmax (if given); work [2 FM_MAXB], st [1]
int fm_std(corahip_ctx *ctx, const double *v, long count, double *work, double *st, double *sd, double *vmax) {
    int nb;
    long per;
    partials_split(count, 1, &nb, &per);
    hipLaunchKernelGGL(fm_partial_kernel<0>, dim3((unsigned)nb), dim3(256), 0, ctx->stream, v, count, per, st, work);
    LAUNCH_CHECK();
    hipLaunchKernelGGL(fm_final_kernel<0>, dim3(1), dim3(256), 0, ctx->stream, work, nb, count, st, sd, vmax);
    LAUNCH_CHECK();
    hipLaunchKernelGGL(fm_partial_kernel<1>, dim3((unsigned)nb), dim3(256), 0, ctx->stream, v, count, per, st, work);
    LAUNCH_CHECK();
    hipLaunchKernelGGL(fm_final_kernel<1>, dim3(1), dim3(256), 0, ctx->stream, work, nb, count, st, sd, vmax);
    LAUNCH_CHECK();
    return 0;
}

}  // namespace

extern "C" {

int corahip_powerlaw_los(corahip_ctx *ctx, const double *A, const double *beta, const double *x, double a0, double sa,
                         double b0, double sb, int nfreq, long ncol, int nz, double *out) {
    ARG_CHECK(ctx && A && beta && x && out);
    ARG_CHECK(nfreq >= 1 && ncol >= 1 && nz >= 1);
    ARG_CHECK(is_aligned(A, 8) && is_aligned(beta, 8) && is_aligned(x, 8) && is_aligned(out, 8));
    const size_t fbytes = (size_t)ncol * (size_t)nz * 8, obytes = (size_t)nfreq * (size_t)ncol * 8;
    ARG_CHECK(!overlaps(out, obytes, A, fbytes) && !overlaps(out, obytes, beta, fbytes));
    ARG_CHECK(!overlaps(out, obytes, x, (size_t)nfreq * 8));
    const long tiles = (ncol + PL_PT - 1) / PL_PT;
    ARG_CHECK(tiles <= 0x7fffffffL);
    const int nfb = (nfreq + PL_FB - 1) / PL_FB;
    // pixel tiles alone fill the device (4 workgroups per CU): a workgroup walks all channel blocks of its tile; fewer:
    // the blocks are spread over up to nfb workgroups per tile.  No sum depends on the choice.
    long gy = ((long)ctx->num_cu * 4 + tiles - 1) / tiles;
    gy = gy < 1 ? 1 : (gy > nfb ? nfb : gy);
    if (gy > 65535) gy = 65535;
    StageTimer t(ctx, "powerlaw_los");
    hipLaunchKernelGGL(powerlaw_los_kernel, dim3((unsigned)tiles, (unsigned)gy), dim3(PL_NT), 0, ctx->stream, A, beta, x, a0, sa,
                       b0, sb, nfreq, ncol, nz, nfb, out);
    LAUNCH_CHECK();
    return 0;
}

int corahip_field_moments(corahip_ctx *ctx, const double *f, long ncol, int nz, double *out3) {
    ARG_CHECK(ctx && f && out3 && ncol >= 1 && nz >= 1);
    ARG_CHECK(is_aligned(f, 8) && is_aligned(out3, 8));
    ARG_CHECK(!overlaps(out3, 3 * sizeof(double), f, (size_t)ncol * (size_t)nz * 8));
    ARG_CHECK((ncol + 3) / 4 <= 0x7fffffffL);
    // scratch slot 10: block partials [2 FM_MAXB] | mean [2] | column sums [ncol], all written before they are read
    void *scr = nullptr;
    int rc = corahip_ctx_scratch(ctx, 10, ((size_t)FM_MAXB * 2 + 2 + (size_t)ncol) * sizeof(double), &scr);
    if (rc != 0) return rc;
    double *work = (double *)scr, *st = work + 2 * FM_MAXB, *s = st + 2;
    StageTimer t(ctx, "field_moments");
    hipLaunchKernelGGL(fm_colsum_kernel, dim3((unsigned)((ncol + 3) / 4)), dim3(256), 0, ctx->stream, f, ncol, nz, s);
    LAUNCH_CHECK();
    rc = fm_std(ctx, s, ncol, work, st, out3, nullptr);
    if (rc != 0) return rc;
    return fm_std(ctx, f, ncol * (long)nz, work, st, out3 + 1, out3 + 2);
}

}  // extern "C"
