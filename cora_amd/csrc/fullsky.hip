// fullsky.hip - the exact curved-sky C_l(z, z') with redshift-space distortions (angular_powerspectrum_full of
// cora/signal/corr.py:777-868, dead code there), restated as a table of radial functions and one Gram product per l:
//   C_l[i, j] = sum_n g_n A_l[i, n] A_l[j, n],   A_l[i, n] = sum_a cb[i, a] j_l(k_n chi[i, a]) - cf[i, a] j_l''(k_n chi[i, a])
// with g_n = (2 / pi) w_n k_n^2 P(k_n) on one shared wavenumber grid; a runs over the sub-samples of channel i, whose
// average is linear and separable and so is taken before the product.
//
//   sphbessel_radial_kernel  A [lmax + 1, F, ld_k], k contiguous.  One lane per (n, i): for a fixed l a wave writes 512
//                          contiguous bytes.  l is the outer loop, the NS sub-samples the inner one; a sub-sample keeps two
//                          consecutive values, 1 / x, cb, cf and its normalisation in registers, the sum over a is formed in
//                          a register and stored once.  x = k_n chi is one product; j_l'' = (l (l - 1) / x^2 - 1) j_l +
//                          (2 / x) j_{l+1}.  Per sub-sample, with m = floor(x):
//                            l <= m      upward: j_{l+1} = (2l + 1) / x j_l - j_{l-1} from j_0 = sin x / x, j_1 =
//                                        (j_0 - cos x) / x.  Never above the turning point, where it amplifies rounding.
//                            l >  m      downward (Miller) from y_{L+1} = 0, y_L = 1 at L = lstart = top + ceil(sqrt(160
//                                        top)) + 30, top = lmax + 1 (j_{lmax+1} is needed for j'' at lmax); both values
//                                        are multiplied by 2^-256 whenever one passes 2^256; normalised to the upward
//                                        value at the larger of |j_m|, |j_{m+1}|.  x < 1: m = -1, normalised to j_0 (the
//                                        closed form of j_1 cancels there and is not used).
//                          A lane walks l = 0 .. L0 upward, L0 = min_a m_a: every sub-sample is below its turning point.
//                          If L0 < lmax it then (1) carries each sub-sample upward to its own m_a and runs the downward
//                          recurrence once to find the normalisation and the number R of rescalings, (2) runs it again
//                          from lstart down to L0 + 1, accumulating: the same arithmetic, so the rescalings fall on the
//                          same orders; a value with more than three rescalings still to come is below 2^-1024 times
//                          the normalisation and contributes an exact zero.  Between L0 and m_a the downward form runs
//                          through the oscillatory range, where neither solution grows.  A sub-sample with x >= top in
//                          such a lane enters pass (2) at l = lmax with its upward values.  Passes (1), (2) cost only
//                          where x < top.
//                          x < 2^-170 (x = 0 included): the leading terms j_l = t_l, j_0'' = -1/3, j_1'' = -3/5 t_1,
//                          j_l'' = l (l - 1) / ((2l - 1)(2l + 1)) t_{l-2}, t_l = x^l / (2l + 1)!! (the next terms are
//                          below 2^-340 of them); beyond l = 8 every one has underflowed.  x = 0 gives j_0 = 1, j_0'' =
//                          -1/3, j_2'' = 2/15 and zeros.  No NaN, no Inf for finite x >= 0: above 2^-170 no intermediate
//                          passes 2^450.
//                          Columns nk .. ld_k - 1 are written as zeros.
//   cl_gram_kernel         C[l, i, j] (+)= sum_n g_n A[l, i, n] A[l, j, n] on v_mfma_f64_16x16x4_f64 with the roles,
//                          accumulators and staged k-loop of mfma_tile.h: 128 x 128 tiles (a wave 64 x 64), k in chunks
//                          of 16, both operands read along k (64 lanes cover four 128-byte runs) into LDS as [row][k],
//                          pitch 17.  g multiplies the column operand on the way in.  Only tiles with ti <= tj, on a
//                          diagonal tile only the waves on or above the diagonal; every element (i <= j) is computed as
//                          row i times column j and written to [i, j] and [j, i]: symmetric bit for bit, one writer per
//                          element, no atomics.  The sum of an element runs over k = 0, 1, ... in MFMA steps of 4 from
//                          acc = 0 (or acc = C with accumulate): the order knows neither F nor the tile, so a subset of
//                          the channels gives the bits of the full call's sub-block.
// All element offsets are 64-bit.
#include "common.h"
#include "mfma_tile.h"
#include "sphbessel_lane.h"

namespace {

constexpr int SB_NT = 256;

template <int NS>
__global__ void __launch_bounds__(SB_NT)
sphbessel_radial_kernel(const double *__restrict__ k, int nk, const double *__restrict__ chi, const double *__restrict__ cb,
                        const double *__restrict__ cf, int nsub, int lmax, int lstart, long ld_k, double *__restrict__ A) {
    const long n = (long)blockIdx.x * SB_NT + threadIdx.x;
    const int i = blockIdx.y, F = gridDim.y;
    if (n >= ld_k) return;
    const size_t sl = (size_t)F * (size_t)ld_k;
    double *out = A + (size_t)i * (size_t)ld_k + (size_t)n;
    if (n >= nk) {
        for (int l = 0; l <= lmax; l++) out[(size_t)l * sl] = 0.0;
        return;
    }
    sb_lane<NS>(k[n], chi + (size_t)i * nsub, cb + (size_t)i * nsub, cf + (size_t)i * nsub, nsub, lmax, lstart, out, sl);
}

// ---- Gram product ----------------------------------------------------------------------------------------------------

constexpr int CG_NT = 256;
constexpr int CG_T = 128;                     // output tile edge (channels)
constexpr int CG_K = 16;                      // k per LDS chunk (4 MFMA steps)
constexpr int CG_AS = CG_K + 1;               // LDS pitch of a row
constexpr int CG_NA = CG_T * CG_K / CG_NT;    // staged elements per thread, operand and chunk

__global__ void __launch_bounds__(CG_NT)
cl_gram_kernel(const double *__restrict__ A, const double *__restrict__ g, int F, int nk, long ld_k, int ntiles, int accumulate,
               double *__restrict__ C) {
    __shared__ double As[2][CG_T * CG_AS];
    __shared__ double Bs[2][CG_T * CG_AS];
    const wave_roles<4, 4> w;
    const int tid = w.tid, ri = w.ri, kq = w.kq, wr = w.wr, wc = w.wc;
    const int l = (int)(blockIdx.x / (unsigned)ntiles);
    int t = (int)(blockIdx.x % (unsigned)ntiles), ti, tj = 0;
    while (t > tj) t -= ++tj;                 // tiles (ti <= tj) in column order
    ti = t;
    const bool diag = ti == tj;
    const int row0 = ti * CG_T, col0 = tj * CG_T;
    const bool active = !(diag && wr > wc);   // below the diagonal: written by the mirror of (wc, wr)
    const double *Al = A + (size_t)l * (size_t)F * (size_t)ld_k;
    double *Cl = C + (size_t)l * (size_t)F * (size_t)F;

    int msk = 0;                              // 16-blocks inside F: bits 0-3 rows, 4-7 columns
#pragma unroll
    for (int u = 0; u < 4; u++) {
        if (active && row0 + wr + 16 * u < F) msk |= 1 << u;
        if (col0 + wc + 16 * u < F) msk |= 16 << u;
    }
    msk = __builtin_amdgcn_readfirstlane(msk);
    bool ua[4], va[4];
#pragma unroll
    for (int u = 0; u < 4; u++) ua[u] = (msk >> u) & 1, va[u] = (msk >> (4 + u)) & 1;

    // an element of the tile is this lane's to write: inside F, and on or above the diagonal
    auto mine = [&](int gr, int gc) { return gr < F && gc < F && (!diag || gr <= gc); };

    acc_tile<4, 4> acc;
    acc.zero();
    if (accumulate) {
#pragma unroll
        for (int u = 0; u < 4; u++)
#pragma unroll
            for (int v = 0; v < 4; v++) {
                if (!(ua[u] && va[v])) continue;
                const int gc = col0 + wc + w.col(v);
#pragma unroll
                for (int rr = 0; rr < 4; rr++) {
                    const int gr = row0 + wr + w.row(u, rr);
                    if (mine(gr, gc)) acc.acc[u][v][rr] = Cl[(size_t)gr * (size_t)F + (size_t)gc];
                }
            }
    }

    const int nchunk = (nk + CG_K - 1) / CG_K;
    const int sk = tid % CG_K, sr = tid / CG_K;     // staging: k of the chunk, row (+ 16 u)
    double ra[CG_NA], rb[CG_NA];
    auto gload = [&](int c) {
        const int kk = c * CG_K + sk;
        const bool kin = kk < nk;
        const double gk = kin ? g[kk] : 0.0;
#pragma unroll
        for (int u = 0; u < CG_NA; u++) {
            const int rw = sr + (CG_NT / CG_K) * u;
            const int gr = row0 + rw, gc = col0 + rw;
            ra[u] = (kin && gr < F) ? Al[(size_t)gr * (size_t)ld_k + (size_t)kk] : 0.0;
            rb[u] = (kin && gc < F) ? gk * Al[(size_t)gc * (size_t)ld_k + (size_t)kk] : 0.0;
        }
    };
    auto lstore = [&](int buf, int) {
#pragma unroll
        for (int u = 0; u < CG_NA; u++) {
            const int rw = sr + (CG_NT / CG_K) * u;
            As[buf][rw * CG_AS + sk] = ra[u];
            Bs[buf][rw * CG_AS + sk] = rb[u];
        }
    };
    auto compute = [&](int, int buf) {
        const double *as = As[buf] + (wr + ri) * CG_AS + kq, *bs = Bs[buf] + (wc + ri) * CG_AS + kq;
#pragma unroll
        for (int ks = 0; ks < CG_K / 4; ks++) {
            const lds_rows af = {as + 4 * ks, CG_AS};
            double bv[4];
#pragma unroll
            for (int v = 0; v < 4; v++) bv[v] = bs[16 * v * CG_AS + 4 * ks];
            acc.mma_if(af, bv, ua, va);
        }
    };
    staged_k_loop(nchunk, gload, lstore, compute);

#pragma unroll
    for (int u = 0; u < 4; u++)
#pragma unroll
        for (int v = 0; v < 4; v++) {
            if (!(ua[u] && va[v])) continue;
            const int gc = col0 + wc + w.col(v);
#pragma unroll
            for (int rr = 0; rr < 4; rr++) {
                const int gr = row0 + wr + w.row(u, rr);
                if (mine(gr, gc)) {
                    const double x = acc.acc[u][v][rr];
                    Cl[(size_t)gr * (size_t)F + (size_t)gc] = x;
                    if (gr != gc) Cl[(size_t)gc * (size_t)F + (size_t)gr] = x;
                }
            }
        }
}

int launch_radial(corahip_ctx *ctx, const double *k, int nk, const double *chi, const double *cb, const double *cf, int F,
                  int nsub, int lmax, long ld_k, double *A) {
    const dim3 grid((unsigned)((ld_k + SB_NT - 1) / SB_NT), (unsigned)F), block(SB_NT);
    const int lstart = sb_lstart(lmax);
#define SB_LAUNCH(NS)                                                                                                   \
    hipLaunchKernelGGL(sphbessel_radial_kernel<NS>, grid, block, 0, ctx->stream, k, nk, chi, cb, cf, nsub, lmax, lstart, \
                       ld_k, A)
    if (nsub == 1)
        SB_LAUNCH(1);
    else if (nsub <= 3)
        SB_LAUNCH(3);
    else if (nsub <= 5)
        SB_LAUNCH(5);
    else if (nsub <= 9)
        SB_LAUNCH(9);
    else
        SB_LAUNCH(SB_MAXSUB);
#undef SB_LAUNCH
    LAUNCH_CHECK();
    return 0;
}

int launch_gram(corahip_ctx *ctx, const double *A, const double *g, int lmax, int F, int nk, long ld_k, double *C,
                int accumulate) {
    const long nt = (F + CG_T - 1) / CG_T, ntiles = nt * (nt + 1) / 2;
    hipLaunchKernelGGL(cl_gram_kernel, dim3((unsigned)(ntiles * (lmax + 1))), dim3(CG_NT), 0, ctx->stream, A, g, F, nk, ld_k,
                       (int)ntiles, accumulate, C);
    LAUNCH_CHECK();
    return 0;
}

// the shape limits shared by the entry points
bool shape_ok(int F, int nk, int lmax, long ld_k) {
    if (!(F >= 1 && F <= 65535 && nk >= 1 && lmax >= 0 && lmax <= (1 << 20) && ld_k >= nk)) return false;
    const long nt = (F + CG_T - 1) / CG_T;
    return nt * (nt + 1) / 2 * ((long)lmax + 1) <= 0x7fffffffL && (ld_k + SB_NT - 1) / SB_NT <= 0x7fffffffL;
}

long chunk_ld(int nk_chunk) { return ((long)nk_chunk + CG_K - 1) / CG_K * CG_K; }

}  // namespace

extern "C" {

int corahip_sphbessel_radial(corahip_ctx *ctx, const double *k, int nk, const double *chi, const double *cb, const double *cf,
                             int F, int nsub, int lmax, long ld_k, double *A) {
    ARG_CHECK(ctx && k && chi && cb && cf && A);
    ARG_CHECK(shape_ok(F, nk, lmax, ld_k) && nsub >= 1 && nsub <= SB_MAXSUB);
    ARG_CHECK(is_aligned(k, 8) && is_aligned(chi, 8) && is_aligned(cb, 8) && is_aligned(cf, 8) && is_aligned(A, 8));
    const size_t abytes = (size_t)(lmax + 1) * (size_t)F * (size_t)ld_k * 8, cbytes = (size_t)F * (size_t)nsub * 8;
    ARG_CHECK(!overlaps(A, abytes, k, (size_t)nk * 8) && !overlaps(A, abytes, chi, cbytes));
    ARG_CHECK(!overlaps(A, abytes, cb, cbytes) && !overlaps(A, abytes, cf, cbytes));
    StageTimer t(ctx, "sphbessel_radial");
    return launch_radial(ctx, k, nk, chi, cb, cf, F, nsub, lmax, ld_k, A);
}

int corahip_cl_gram(corahip_ctx *ctx, const double *A, const double *g, int lmax, int F, int nk, long ld_k, double *C,
                    int accumulate) {
    ARG_CHECK(ctx && A && g && C);
    ARG_CHECK(shape_ok(F, nk, lmax, ld_k) && (accumulate == 0 || accumulate == 1));
    ARG_CHECK(is_aligned(A, 8) && is_aligned(g, 8) && is_aligned(C, 8));
    const size_t abytes = (size_t)(lmax + 1) * (size_t)F * (size_t)ld_k * 8, cbytes = (size_t)(lmax + 1) * (size_t)F * (size_t)F * 8;
    ARG_CHECK(!overlaps(C, cbytes, A, abytes) && !overlaps(C, cbytes, g, (size_t)nk * 8));
    StageTimer t(ctx, "cl_gram");
    return launch_gram(ctx, A, g, lmax, F, nk, ld_k, C, accumulate);
}

int corahip_clarray_fullsky_workspace_bytes(int lmax, int F, int nk_chunk, size_t *bytes) {
    ARG_CHECK(bytes && nk_chunk >= 1 && shape_ok(F, nk_chunk, lmax, chunk_ld(nk_chunk)));
    *bytes = (size_t)(lmax + 1) * (size_t)F * (size_t)chunk_ld(nk_chunk) * 8;
    return 0;
}

int corahip_clarray_fullsky(corahip_ctx *ctx, const double *k, const double *g, int nk, const double *chi, const double *cb,
                            const double *cf, int F, int nsub, int lmax, int nk_chunk, void *workspace, double *C) {
    ARG_CHECK(ctx && k && g && chi && cb && cf && workspace && C);
    ARG_CHECK(nk >= 1 && nk_chunk >= 1 && nsub >= 1 && nsub <= SB_MAXSUB);
    const long ld = chunk_ld(nk_chunk);
    ARG_CHECK(shape_ok(F, nk_chunk, lmax, ld));
    ARG_CHECK(is_aligned(k, 8) && is_aligned(g, 8) && is_aligned(chi, 8) && is_aligned(cb, 8) && is_aligned(cf, 8));
    ARG_CHECK(is_aligned(workspace, 8) && is_aligned(C, 8));
    const size_t wbytes = (size_t)(lmax + 1) * (size_t)F * (size_t)ld * 8, cbytes = (size_t)(lmax + 1) * (size_t)F * (size_t)F * 8;
    const size_t sbytes = (size_t)F * (size_t)nsub * 8;
    ARG_CHECK(!overlaps(workspace, wbytes, C, cbytes));
    const void *in[5] = {k, g, chi, cb, cf};
    const size_t inb[5] = {(size_t)nk * 8, (size_t)nk * 8, sbytes, sbytes, sbytes};
    for (int q = 0; q < 5; q++) ARG_CHECK(!overlaps(workspace, wbytes, in[q], inb[q]) && !overlaps(C, cbytes, in[q], inb[q]));
    StageTimer t(ctx, "clarray_fullsky");
    double *A = (double *)workspace;
    for (long c0 = 0; c0 < nk; c0 += nk_chunk) {                  // ascending k: table, then Gram
        const int nc = nk - c0 < nk_chunk ? (int)(nk - c0) : nk_chunk;
        int rc = launch_radial(ctx, k + c0, nc, chi, cb, cf, F, nsub, lmax, ld, A);
        if (rc != 0) return rc;
        rc = launch_gram(ctx, A, g + c0, lmax, F, nc, ld, C, c0 > 0 ? 1 : 0);
        if (rc != 0) return rc;
    }
    return 0;
}

}  // extern "C"
