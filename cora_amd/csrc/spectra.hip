// spectra.hip - the multi-frequency angular power spectrum of a_lm in the device layout: per multipole l the Gram matrix
// of the channels,
//   out[l, i, j] = (1 / (2l+1)) sum_{m=0..l} c_m (Re a_i Re b_j + Im a_i Im b_j),   c_0 = 1, c_{m>0} = 2
// (healpy's alm2cl; Im a_l0 enters as stored).  The transpose of K3 (draw.hip): there a_l = T_l g_l, here a_l a_l^H.
//
//   cross_spectra_kernel   FP64 MFMA (v_mfma_f64_16x16x4_f64), M = channels of a, N = channels of b, K-dimension = the
//                          2 (l+1) real and imaginary values of one l (one MFMA takes (Re, Im) of two m).  A workgroup of
//                          4 waves owns a tile of 128 x 128 outputs of one l (a wave 64 x 64); 16 x 16 blocks beyond nx
//                          or ny are not multiplied.  Every (l, m) element of an operand is one contiguous row of 8 G
//                          doubles [G][2][4]; the 128 channels of a tile are 256 contiguous doubles of it, staged as they
//                          are: 16-byte loads (128 lanes cover the 2 KiB of a row), 16-byte LDS stores, CS_KM rows of m
//                          per chunk, on the schedule and the accumulator tile of mfma_tile.h.  LDS pitch 256 doubles,
//                          no padding: a fragment read (ds_read_b64) of lanes 0-31 = (16 channels) x (Re, Im) covers 32
//                          consecutive doubles = all 64 banks once, lanes 32-63 the same in the next row
//                          (tools/lds_bank_sim.py spectra).
//                          c_m: the chunks run over m = 1 .. l first, then every accumulator is doubled (exact), then one
//                          last MFMA adds m = 0 - no operand is scaled, so the symmetric case needs one staged operand on
//                          diagonal tiles.  1 / (2l+1): one correctly rounded division per output in the epilogue.
//                          Rounding: the 2 (l+1) products of an output are added in a fixed order by FMAs, + 1 division.
//                          Symmetric case (b = a): only tiles on or below the diagonal; an off-diagonal tile writes its
//                          mirror from the same accumulators; on a diagonal tile [i, j] and [j, i] are the commuted
//                          products a_i a_j, a_j a_i added in the same order (the 64 x 64 block above the diagonal is
//                          not computed but mirrored from the one below) - the result is bitwise symmetric.
//                          No atomics, no split of K: the sum order is fixed, repeat calls return identical bits.
//                          Work per item grows as l + 1: the grid runs over l in descending order.
//                          Padding channels (4 G > n) are staged like the others; they only ever reach rows / columns
//                          >= n of the MFMA result, which are not stored.  Groups beyond G are staged as zeros.
//   alm_gather_channels_kernel   the streaming copy that puts chosen channels of one a_lm buffer into a channel range of
//                          another (T, E, B, V of a polarised sky into one field-major operand of the Gram kernel);
//                          described at the kernel.
// All element offsets are 64-bit (nalm * 8 G exceeds 2^31 at 256 channels, lmax 2048).
#include "common.h"
#include "mfma_tile.h"

namespace {

constexpr int CS_WAVES = 4;
constexpr int CS_NT = 64 * CS_WAVES;    // threads per workgroup
constexpr int CS_T = 128;               // output tile edge (channels)
constexpr int CS_KM = 8;                // rows of m per LDS chunk (4 MFMA steps)
constexpr int CS_P = 2 * CS_T;          // doubles of a staged row: 32 groups x [2][4]
constexpr int CS_NV = CS_KM * CS_P / 2 / CS_NT;   // 16-byte loads per thread, operand and chunk

__global__ void __launch_bounds__(CS_NT, 2)
cross_spectra_kernel(const double *__restrict__ A, int nx, int Ga, const double *__restrict__ B, int ny, int Gb, int lmax,
                     int sym, int nty, int ntiles, double *__restrict__ out) {
    __shared__ __attribute__((aligned(16))) double As[2][CS_KM * CS_P];
    __shared__ __attribute__((aligned(16))) double Bs[2][CS_KM * CS_P];
    const wave_roles<4, 4> w;                                       // a wave owns 64 x 64 of the tile
    const int tid = w.tid, ri = w.ri, kq = w.kq, wr = w.wr, wc = w.wc;
    // descending l.  The quotient comes out of the VALU; the chunk loop it bounds is controlled by the SALU only if l is
    // in an SGPR.  __builtin_amdgcn_readfirstlane does not get it there: l is provably uniform, the compiler folds the
    // call away and then keeps l in a VGPR (v_cmp loop control, 6 more VGPRs).  The register constraint cannot be folded.
    int l = lmax - (int)(blockIdx.x / (unsigned)ntiles);
    asm("" : "+s"(l));
    int t = (int)(blockIdx.x % (unsigned)ntiles), ti, tj;
    if (sym) {
        ti = 0;
        while (t > ti) t -= ++ti;       // tiles (ti, tj <= ti) in row order
        tj = t;
    } else {
        ti = t / nty, tj = t % nty;
    }
    const bool diag = sym && ti == tj;
    const int row0 = ti * CS_T, col0 = tj * CS_T;
    const bool active = !(diag && wr < wc);                         // above the diagonal: mirrored from (wc, wr)
    const bool mirror = sym && (!diag || wr > wc);

    acc_tile<4, 4> acc;
    acc.zero();
    int msk = 0;                                                    // 16-blocks inside the operands: bits 0-3 rows, 4-7 columns
#pragma unroll
    for (int u = 0; u < 4; u++) {
        if (active && row0 + wr + 16 * u < nx) msk |= 1 << u;
        if (col0 + wc + 16 * u < ny) msk |= 16 << u;
    }
    msk = __builtin_amdgcn_readfirstlane(msk);                      // (wave-uniform)
    bool ua[4], va[4];
#pragma unroll
    for (int u = 0; u < 4; u++) ua[u] = (msk >> u) & 1, va[u] = (msk >> (4 + u)) & 1;

    // chunk c < nch holds m = 1 + c CS_KM + r (r = row of the chunk), chunk nch holds m = 0 in row 0; other rows zero
    const int nch = (l + CS_KM - 1) / CS_KM, ntot = nch + 1;
    const int sr = tid >> 7, sq = 2 * (tid & 127);                  // staging: row (+ 2 u), double offset in the row
    double2 ra[CS_NV], rb[CS_NV];
    auto gload1 = [&](double2(&rv)[CS_NV], const double *__restrict__ X, int G, int x0, int c) {
        const int d = 2 * x0 + sq;                                  // offset in the (l, m) row of 8 G doubles
#pragma unroll
        for (int u = 0; u < CS_NV; u++) {
            const int r = sr + 2 * u;
            const int m = c < nch ? 1 + c * CS_KM + r : (r == 0 ? 0 : l + 1);
            double2 x = make_double2(0.0, 0.0);
            if (m <= l && d < 8 * G)
                x = *reinterpret_cast<const double2 *>(X + ((size_t)alm_idx(l, m, lmax) * (size_t)G * 8 + (size_t)d));
            rv[u] = x;
        }
    };
    auto lstore1 = [&](double *S, const double2(&rv)[CS_NV]) {
#pragma unroll
        for (int u = 0; u < CS_NV; u++) *reinterpret_cast<double2 *>(&S[(sr + 2 * u) * CS_P + sq]) = rv[u];
    };
    // a diagonal tile stages one operand and reads both fragments from it
    auto gload = [&](int c) {
        gload1(ra, A, Ga, row0, c);
        if (!diag) gload1(rb, B, Gb, col0, c);
    };
    auto lstore = [&](int buf, int) {
        lstore1(As[buf], ra);
        if (!diag) lstore1(Bs[buf], rb);
    };
    // fragment position of channel c of the tile, value (Re, Im) = kq & 1: 8 (c / 4) + 4 (kq & 1) + c % 4
    const int fo = 8 * (ri >> 2) + 4 * (kq & 1) + (ri & 3) + (kq >> 1) * CS_P;
    auto compute = [&](int c, int buf) {
        const double *as = As[buf], *bs = diag ? As[buf] : Bs[buf];
        if (c == nch) acc.scale(2.0);                               // c_m = 2 of everything added so far
        const int nks = c == nch ? 1 : CS_KM / 2;                   // m = 0: one step (row 1 of that chunk is zero)
        for (int ks = 0; ks < nks; ks++) {                          // (not unrolled: 4 steps of fragments do not fit beside 128 accumulators)
            double a[4], b[4];
#pragma unroll
            for (int v = 0; v < 4; v++) {
                a[v] = as[2 * ks * CS_P + 2 * (wr + 16 * v) + fo];
                b[v] = bs[2 * ks * CS_P + 2 * (wc + 16 * v) + fo];
            }
            acc.mma_if(a, b, ua, va);
        }
    };
    staged_k_loop(ntot, gload, lstore, compute);

    const double dl = (double)(2 * l + 1);
    double *ol = out + (size_t)l * (size_t)nx * (size_t)ny;
#pragma unroll
    for (int u = 0; u < 4; u++)
#pragma unroll
        for (int v = 0; v < 4; v++) {
            if (!(ua[u] && va[v])) continue;
            const int gc = col0 + wc + w.col(v);
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int gr = row0 + wr + w.row(u, r);
                if (gr < nx && gc < ny) {
                    const double x = acc.acc[u][v][r] / dl;
                    ol[(size_t)gr * (size_t)ny + (size_t)gc] = x;
                    if (mirror) ol[(size_t)gc * (size_t)ny + (size_t)gr] = x;
                }
            }
        }
}

// ---- channel gather in the a_lm layout: dst channel dst_first + j = src channel idx[j] ------------------------------------
// Both buffers are [nalm][G][2][4]; channel c of an (l, m) row of 8 G doubles sits at 8 (c / 4) + 4 (Re, Im) + c % 4.  The
// unit of work is a destination pair: 16 bytes = the same component of the channels (4 g + 2 h, 4 g + 2 h + 1).  A thread
// owns one pair position of the row (group g, component, half h) for the whole call: it reads its (up to) two indices
// once, and then walks the rows a, a + stride, ... with GC_U rows of loads in flight before the stores.  Lanes run along
// the row (consecutive pairs = consecutive 16 bytes), and where the touched part of a row is shorter than the workgroup
// the remaining threads take the following rows, so a wave writes contiguous runs of the touched groups of consecutive
// rows.  A pair with both channels inside [dst_first, dst_first + n) takes one 16-byte store (and one 16-byte load when
// its two sources are an aligned neighbouring pair); at the ragged ends the one channel inside takes an 8-byte store;
// nothing else of dst is written: one writer per element, no atomics, no workspace.  An index outside [0, nsrc) writes
// nothing for its channel (the Python binding refuses it before the launch).  All element offsets are 64-bit.
constexpr int GC_NT = 256;
constexpr int GC_U = 4;                 // rows in flight per thread

__global__ void __launch_bounds__(GC_NT)
alm_gather_channels_kernel(const double *__restrict__ src, int nsrc, int Gs, const int32_t *__restrict__ idx, int n, long nalm,
                           double *__restrict__ dst, int Gd, int dst_first, int g0, int np, int W, int R) {
    const int tid = threadIdx.x;
    const int q = (int)blockIdx.x * W + tid % W, r = tid / W;       // pair position in the touched groups, row of the block
    if (r >= R || q >= np) return;
    const int g = g0 + (q >> 2), c = (q >> 1) & 1, h = q & 1;
    const int j0 = 4 * g + 2 * h - dst_first, j1 = j0 + 1;
    int s0 = -1, s1 = -1;
    if (j0 >= 0 && j0 < n) s0 = idx[j0];
    if (j1 >= 0 && j1 < n) s1 = idx[j1];
    const bool w0 = (unsigned)s0 < (unsigned)nsrc, w1 = (unsigned)s1 < (unsigned)nsrc;
    if (!w0 && !w1) return;
    const size_t so0 = w0 ? (size_t)(8 * (s0 >> 2) + 4 * c + (s0 & 3)) : 0, so1 = w1 ? (size_t)(8 * (s1 >> 2) + 4 * c + (s1 & 3)) : 0;
    const bool both = w0 && w1, wide = both && s1 == s0 + 1 && (s0 & 1) == 0;
    const size_t srow = (size_t)Gs * 8, drow = (size_t)Gd * 8, doff = (size_t)(8 * g + 4 * c + 2 * h);
    const long astep = (long)gridDim.y * R;
    for (long a = (long)blockIdx.y * R + r; a < nalm; a += GC_U * astep) {
        double2 v[GC_U];
#pragma unroll
        for (int u = 0; u < GC_U; u++) {
            const long au = a + u * astep;
            v[u] = make_double2(0.0, 0.0);
            if (au < nalm) {
                const double *sp = src + (size_t)au * srow;
                if (wide)
                    v[u] = *reinterpret_cast<const double2 *>(sp + so0);
                else {
                    if (w0) v[u].x = sp[so0];
                    if (w1) v[u].y = sp[so1];
                }
            }
        }
#pragma unroll
        for (int u = 0; u < GC_U; u++) {
            const long au = a + u * astep;
            if (au < nalm) {
                double *dp = dst + (size_t)au * drow + doff;
                if (both)
                    *reinterpret_cast<double2 *>(dp) = v[u];
                else if (w0)
                    dp[0] = v[u].x;
                else
                    dp[1] = v[u].y;
            }
        }
    }
}

}  // namespace

extern "C" {

int corahip_alm_cross_spectra(corahip_ctx *ctx, const double *alm_a, int nx, const double *alm_b, int ny, int lmax,
                              double *out) {
    ARG_CHECK(ctx && alm_a && out && nx >= 1 && ny >= 1 && lmax >= 0);
    const bool sym = alm_b == nullptr || alm_b == alm_a;
    ARG_CHECK(!sym || ny == nx);
    ARG_CHECK(is_aligned(alm_a, 16) && is_aligned(alm_b, 16) && is_aligned(out, 8));
    const int Ga = (nx + 3) / 4, Gb = (ny + 3) / 4;
    const size_t nalm = (size_t)nalm_of(lmax), obytes = (size_t)(lmax + 1) * (size_t)nx * (size_t)ny * 8;
    ARG_CHECK(!overlaps(out, obytes, alm_a, nalm * Ga * 64));
    ARG_CHECK(sym || !overlaps(out, obytes, alm_b, nalm * Gb * 64));
    const long ntx = (nx + CS_T - 1) / CS_T, nty = (ny + CS_T - 1) / CS_T;
    const long ntiles = sym ? ntx * (ntx + 1) / 2 : ntx * nty;
    ARG_CHECK(ntiles * (lmax + 1) <= 0x7fffffffL);
    StageTimer t(ctx, "alm_cross_spectra");
    hipLaunchKernelGGL(cross_spectra_kernel, dim3((unsigned)(ntiles * (lmax + 1))), dim3(CS_NT), 0, ctx->stream, alm_a, nx, Ga,
                       sym ? alm_a : alm_b, ny, Gb, lmax, sym ? 1 : 0, (int)nty, (int)ntiles, out);
    LAUNCH_CHECK();
    return 0;
}

int corahip_alm_gather_channels(corahip_ctx *ctx, const double *src, int nsrc, const int32_t *idx, int n, int lmax,
                                double *dst, int ndst, int dst_first) {
    ARG_CHECK(ctx && src && idx && dst && nsrc >= 1 && ndst >= 1 && n >= 1 && lmax >= 0);
    ARG_CHECK(dst_first >= 0 && dst_first <= ndst - n);
    ARG_CHECK(is_aligned(src, 16) && is_aligned(dst, 16) && is_aligned(idx, 4));
    const int Gs = (nsrc + 3) / 4, Gd = (ndst + 3) / 4;
    const long nalm = nalm_of(lmax);
    ARG_CHECK(!overlaps(dst, (size_t)nalm * Gd * 64, src, (size_t)nalm * Gs * 64));
    const int g0 = dst_first / 4, g1 = (dst_first + n - 1) / 4;
    const int np = 4 * (g1 - g0 + 1);                               // 16-byte pairs of a row in the touched groups
    const int W = np < GC_NT ? np : GC_NT, R = GC_NT / W;           // pairs and rows a workgroup covers
    const unsigned gx = (unsigned)((np + W - 1) / W);
    long gy = (nalm + (long)R * GC_U - 1) / ((long)R * GC_U);       // enough row blocks for GC_U rows per thread ...
    const long cap = (long)ctx->num_cu * 16 / gx;                   // ... at most 16 workgroups per CU in all
    if (gy > cap) gy = cap;
    if (gy < 1) gy = 1;
    StageTimer t(ctx, "alm_gather_channels");
    hipLaunchKernelGGL(alm_gather_channels_kernel, dim3(gx, (unsigned)gy), dim3(GC_NT), 0, ctx->stream, src, nsrc, Gs, idx, n,
                       nalm, dst, Gd, dst_first, g0, np, W, R);
    LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
