// sht_polana_native.hip - spin-2 ANALYSIS as ONE Legendre pass: the adjoint of legendre_pol_kernel (sht_legendre.hip).
//
//   E_lm = -(sum_rings W_lm Q~ - i X_lm U~),   B_lm = -(sum_rings W_lm U~ + i X_lm Q~)
// with W_lm = (g1 r1 + g2) lambda_l + g3 r2 lambda_{l-1},  X_lm = g4 r2 lambda_l - m g3 r1 lambda_{l-1} formed per ring and
// per l from the (A, B) recurrence, the plan's (g1..g4) table and r1 = 1/sin^2, r2 = cos/sin^2 - the expressions of
// legendre_pol_kernel, operation for operation, from the same seeds (lstart / d_seed: the 2^-70 start rule), so the two
// kernels are adjoints up to rounding and drop the same terms.  Against the composition of sht_polana.hip a (Q, U) pair
// costs two ring transforms instead of six, no scaled map copies, and four products (W Q~, W U~, X Q~, X U~) instead of
// six scalar contractions.
//
// Structure: K4^T (sht_analysis.hip) with another meaning of a row of the transposed tile.  W has the parity (-1)^{l+m}
// of lambda under theta -> pi - theta and X the opposite one, so W at even l - m and X at odd l - m both contract the
// N + S combination `ge` of the G tile, W at odd and X at even l - m the N - S combination `go`: a 16-row A tile holds
// 8 same-parity l of W stacked on the 8 l of the other parity of X, an l-block is 16 multipoles, and the transpose
// buffer (64 rings x 33 doubles per wave), the two accumulator sets per block and the register-resident G tile are
// those of K4^T.  The kernel writes S_W and S_X rows per ring tile; alm_reduce_rows_pol_kernel adds the tiles in fixed
// order (no atomics) and applies the exchange between columns c and c ^ 5 of a cell [ReQ ReU .. | ImQ ImU ..].
#include "sht_internal.h"

int sht_ensure_polc(corahip_ctx *ctx, corahip_sht_plan *p);

#define ADJP_LB 16       // l per block: 8 even + 8 odd (l - m), each with a W and an X row

template <int NCT>
__global__ void __launch_bounds__(512)
legendre_adj_pol_kernel(int lmax, int npair, int nring, int ncols, const double *__restrict__ z,
                        const double *__restrict__ sth, const double2 *__restrict__ coef,
                        const double *__restrict__ polc, const int32_t *__restrict__ lstart,
                        const double2 *__restrict__ seed, const int32_t *__restrict__ lmin_tab,
                        const int32_t *__restrict__ mcut, const double *__restrict__ inter, double *__restrict__ part,
                        unsigned *__restrict__ queue) {
    constexpr int TCOLS = 16 * NCT;
    constexpr int TRINGS = 64 * ADJ_WAVES;     // 512 ring pairs per workgroup
    constexpr int LB = ADJP_LB;
    constexpr int LSTR = 2 * LB + 1;           // LDS row stride of the transpose: conflict-free both ways
    constexpr int WREG = 64 * LSTR;            // doubles per wave
    extern __shared__ __attribute__((aligned(16))) double lds[];
    int &s_next = *reinterpret_cast<int *>(lds + ADJ_WAVES * WREG);

    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int ri = lane & 15, kq = lane >> 4;
    const int L = lmax + 1;
    const int G = ncols >> 3;
    const long nalm = nalm_of(lmax);
    const size_t slab = (size_t)nalm * ncols;  // one S_W or S_X slab of a ring tile
    const int ntile128 = (npair + LMIN_RINGS - 1) / LMIN_RINGS;
    const int ntile = (npair + TRINGS - 1) / TRINGS;
    const int ncg = ncols / TCOLS;
    const int nitems = L * ncg * ntile;
    double *lamw = lds + wave * WREG;

    int item = blockIdx.x;
    while (item < nitems) {
        if (tid == 0) s_next = (int)(gridDim.x + atomicAdd(queue, 1u));
        const int gidx = item / ntile;
        const int rtile = item - gidx * ntile;
        const int m = gidx / ncg;
        const int cg = gidx - m * ncg;
        const double mval = (double)m;
        int lmin = lmax + 1;
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const int t128 = rtile * 4 + q;
            if (t128 < ntile128) lmin = min(lmin, lmin_tab[m * ntile128 + t128]);
        }
        const long base_m = alm_idx(0, m, lmax);
        const int lb0 = lmin <= lmax ? m + ((lmin - m) & ~(LB - 1)) : lmax + 1;
        // slabs (2 rtile, 2 rtile + 1) = (S_W, S_X) of this ring tile; the rows below lb0 are neither written here nor
        // read by alm_reduce_rows_pol_kernel, which forms the same lb0
        double *pout = part + (size_t)(2 * rtile) * slab + (size_t)base_m * ncols + (size_t)cg * TCOLS;

        if (lb0 <= lmax) {
            // ---- this wave's G tile -> registers (B operand): k-step s covers rings 4s..4s+3 of the wave
            double ge[16][NCT], go[16][NCT];
#pragma unroll
            for (int s = 0; s < 16; s++) {
                const int ro = rtile * TRINGS + (4 * s + kq) * ADJ_WAVES + wave;
                const bool ok = ro < npair && m < mcut[min(ro, npair - 1)];
                const int rs = nring - 1 - ro;
#pragma unroll
                for (int t = 0; t < NCT; t++) {
                    const int col = cg * TCOLS + 16 * t + ri;
                    const size_t off = ((size_t)(col >> 3) * L + m) * 8 + (col & 7);
                    double gn = 0.0, gsv = 0.0;
                    if (ok) {
                        gn = inter[(size_t)ro * G * L * 8 + off];
                        if (rs != ro) gsv = inter[(size_t)rs * G * L * 8 + off];
                    }
                    ge[s][t] = gn + gsv;
                    go[s][t] = gn - gsv;
                }
            }
            // ---- recurrence state of this lane's ring
            const int ring = rtile * TRINGS + lane * ADJ_WAVES + wave;
            double x = 0.0, r1 = 0.0, r2 = 0.0, p0 = 0.0, p1 = 0.0;
            double2 sd = make_double2(0.0, 0.0);
            int my_ls = lmax + 1;
            if (ring < npair) {
                x = z[ring];
                const double s = sth[ring];
                r1 = 1.0 / (s * s);
                r2 = x * r1;
                const long o = (long)m * npair + ring;
                my_ls = lstart[o];
                sd = seed[o];
            }
            // first l of each group of 4 lanes (= one MFMA k-step): lets whole k-steps be skipped
            int ls4 = min(my_ls, __shfl_xor(my_ls, 1));
            ls4 = min(ls4, __shfl_xor(ls4, 2));
            const double2 *cf = coef + base_m;
            const double4 *gf = reinterpret_cast<const double4 *>(polc) + base_m;

            // 16 steps of this lane's ring: lambda_l, lambda_{l-1} as the recurrence sees it (the seed where the ring
            // starts) -> W, X -> transpose buffer, row = [W even l (8) | X odd l (8) || W odd l (8) | X even l (8)].
            // Coefficients are read unconditionally (both tables are padded past the last row; l is wave-uniform, so
            // they are scalar loads); rows past lmax are discarded at the reduction.
            auto steps = [&](auto with_inj, const int lb) __attribute__((always_inline)) {
                constexpr bool INJ = decltype(with_inj)::value != 0;
#pragma unroll 8
                for (int j = 0; j < LB; j++) {
                    const int l = lb + j;
                    const double2 c = cf[l];
                    const double4 g = gf[l];
                    double vv = fma(c.x * x, p1, -(c.y * p0));
                    if (INJ) {
                        const bool inj = (l == my_ls);
                        vv = inj ? sd.y : vv;
                        p0 = inj ? sd.x : p1;
                    } else {
                        p0 = p1;
                    }
                    p1 = vv;
                    const double W = fma(fma(g.x, r1, g.y), p1, (g.z * r2) * p0);
                    const double X = fma(g.w * r2, p1, -((mval * g.z) * r1) * p0);
                    lamw[lane * LSTR + (j & 1) * 16 + (j >> 1)] = W;
                    lamw[lane * LSTR + ((j & 1) ^ 1) * 16 + 8 + (j >> 1)] = X;
                }
            };
            // one 16-l block: recurrence -> transpose buffer -> MFMAs into `acc` (acc[0]: the `ge` tile, acc[1]: `go`)
            auto do_block = [&](const int lb, d4_t (&acc)[2][NCT]) __attribute__((always_inline)) {
                const unsigned long long act = __ballot(ls4 <= lb + LB - 1);   // bit 4s: k-step s has a started ring
                // the seed injection is only compiled into the blocks in which some ring of the wave starts
                if (__any(my_ls >= lb && my_ls < lb + LB)) steps(std::true_type{}, lb);
                else steps(std::false_type{}, lb);
                // A operands are read one k-step ahead of the MFMAs that use them (as in K4^T)
                double ae_n = lamw[kq * LSTR + ri], ao_n = lamw[kq * LSTR + 16 + ri];
                if (act == ~0ull) {
#pragma unroll
                    for (int s = 0; s < 16; s++) {
                        const double ae = ae_n, ao = ao_n;
                        if (s + 1 < 16) {
                            ae_n = lamw[(4 * (s + 1) + kq) * LSTR + ri];
                            ao_n = lamw[(4 * (s + 1) + kq) * LSTR + 16 + ri];
                        }
#pragma unroll
                        for (int t = 0; t < NCT; t++) {
                            acc[0][t] = __builtin_amdgcn_mfma_f64_16x16x4f64(ae, ge[s][t], acc[0][t], 0, 0, 0);
                            acc[1][t] = __builtin_amdgcn_mfma_f64_16x16x4f64(ao, go[s][t], acc[1][t], 0, 0, 0);
                        }
                    }
                } else {
#pragma unroll
                    for (int s = 0; s < 16; s++) {
                        const double ae = ae_n, ao = ao_n;
                        if (s + 1 < 16) {
                            ae_n = lamw[(4 * (s + 1) + kq) * LSTR + ri];
                            ao_n = lamw[(4 * (s + 1) + kq) * LSTR + 16 + ri];
                        }
                        if (!((act >> (4 * s)) & 1ull)) continue;
#pragma unroll
                        for (int t = 0; t < NCT; t++) {
                            acc[0][t] = __builtin_amdgcn_mfma_f64_16x16x4f64(ae, ge[s][t], acc[0][t], 0, 0, 0);
                            acc[1][t] = __builtin_amdgcn_mfma_f64_16x16x4f64(ao, go[s][t], acc[1][t], 0, 0, 0);
                        }
                    }
                }
            };
            // two blocks share one cross-wave reduction (the partial tiles of both fit the wave's transpose buffer)
            for (int lb = lb0; lb <= lmax; lb += 2 * LB) {
                d4_t acc0[2][NCT], acc1[2][NCT];
#pragma unroll
                for (int par = 0; par < 2; par++)
#pragma unroll
                    for (int t = 0; t < NCT; t++) acc0[par][t] = acc1[par][t] = (d4_t){0.0, 0.0, 0.0, 0.0};
                do_block(lb, acc0);
                const bool two = lb + LB <= lmax;
                if (two) do_block(lb + LB, acc1);
                // ---- add the eight waves' partial tiles through LDS (the wave's transpose buffer is free now:
                //      LDS operations of one wave are ordered)
#pragma unroll
                for (int par = 0; par < 2; par++)
#pragma unroll
                    for (int t = 0; t < NCT; t++)
#pragma unroll
                        for (int r = 0; r < 4; r++) {
                            lamw[((par * NCT + t) * 4 + r) * 64 + lane] = acc0[par][t][r];
                            if (two) lamw[(((2 + par) * NCT + t) * 4 + r) * 64 + lane] = acc1[par][t][r];
                        }
                __syncthreads();
#pragma unroll
                for (int u = 0; u < 2 * NCT; u++) {
                    if (u >= NCT && !two) break;
                    const int e = tid + 512 * u;          // element (block, par, t, r, lane) of the reduced tiles
                    double sum = 0.0;
#pragma unroll
                    for (int w = 0; w < ADJ_WAVES; w++) sum += lds[w * WREG + e];
                    const int el = e & 63, r = (e >> 6) & 3, q = e >> 8, t = q % NCT, par = (q / NCT) & 1, blk = q / (2 * NCT);
                    // tile row (el >> 4) + 4 r: rows 0..7 are W at l - lb = 2 row + par, rows 8..15 X at the other parity
                    const int isx = r >> 1;
                    const int l = lb + blk * LB + 2 * ((el >> 4) + 4 * (r & 1)) + (par ^ isx);
                    if (l <= lmax) pout[(size_t)isx * slab + (size_t)l * ncols + 16 * t + (el & 15)] = sum;
                }
                __syncthreads();
            }
        }
        __syncthreads();
        item = __builtin_amdgcn_readfirstlane(s_next);
        __syncthreads();
    }
}

// alm_eb[idx][col] from the per-ring-tile slabs part[2 t + (0: S_W, 1: S_X)][idx][col], by rows: block (chunk of 64
// multipoles, m).  Tiles are added in the order t = 0, 1, .. (ring tile t reaches row m from lb0_t(m) on -
// legendre_adj_pol_kernel's own expression; below that its slabs hold nothing and are not read), then
//   Re E = -(S_W[ReQ] + S_X[ImU]),  Im E = -(S_W[ImQ] - S_X[ReU]),  Re B = -(S_W[ReU] - S_X[ImQ]),  Im B = -(S_W[ImU] + S_X[ReQ]):
// column c of a cell takes S_X of column c ^ 5, so the thread of the column pair (c, c + 1), c even, reads the S_X
// pair at c ^ 4 and swaps it.  Rows l < 2 and the channels from nchan on are written as zeros.
__global__ void __launch_bounds__(256)
alm_reduce_rows_pol_kernel(const double *__restrict__ part, long nalm, int ntile, int ncols, int lmax, int ntile128,
                           const int32_t *__restrict__ lmin_tab, int nchan, double *__restrict__ alm) {
    __shared__ int s_lb0[16];
    const int m = blockIdx.y, l0 = m + 64 * (int)blockIdx.x;
    if (l0 > lmax) return;
    const int l1 = min(lmax + 1, l0 + 64), tid = threadIdx.x;
    if (tid < ntile) {
        int lmin = lmax + 1;
        for (int q = 0; q < 4; q++) {
            const int t128 = tid * 4 + q;
            if (t128 < ntile128) lmin = min(lmin, lmin_tab[m * ntile128 + t128]);
        }
        s_lb0[tid] = lmin <= lmax ? m + ((lmin - m) & ~(ADJP_LB - 1)) : lmax + 1;
    }
    __syncthreads();
    const long base_m = alm_idx(0, m, lmax);
    const int half = ncols >> 1;                       // double2 per row (ncols is a multiple of 16)
    const size_t slab2 = (size_t)nalm * half;          // double2 per slab
    const double2 *p2 = reinterpret_cast<const double2 *>(part);
    double2 *a2 = reinterpret_cast<double2 *>(alm);
    for (int e = tid; e < (l1 - l0) * half; e += 256) {
        const int lo = e / half, rem = e - lo * half;
        const int l = l0 + lo;
        const size_t row = (size_t)(base_m + l) * half;
        const int col = 2 * rem;                       // even column of the pair; channel = 4 (col / 8) + col % 4
        const int chan = ((col >> 3) << 2) + (col & 3);
        double2 out = make_double2(0.0, 0.0);
        if (l >= 2 && chan < nchan) {
            double2 sw = make_double2(0.0, 0.0), sx = make_double2(0.0, 0.0);
            for (int t = 0; t < ntile; t++)
                if (l >= s_lb0[t]) {
                    const double2 w = p2[(size_t)(2 * t) * slab2 + row + rem];
                    const double2 v = p2[(size_t)(2 * t + 1) * slab2 + row + (rem ^ 2)];
                    sw.x += w.x, sw.y += w.y;
                    sx.x += v.x, sx.y += v.y;
                }
            // (c, c + 1) = (Re Q, Re U) in the real half of the cell, (Im Q, Im U) in the imaginary half
            if (col & 4) out = make_double2(-(sw.x - sx.y), -(sw.y + sx.x));
            else out = make_double2(-(sw.x + sx.y), -(sw.y - sx.x));
        }
        a2[row + rem] = out;
    }
}

template <int NCT>
static int launch_legendre_adj_pol(corahip_ctx *ctx, const corahip_sht_plan *p, int ncols, const double *inter,
                                   double *part) {
    const size_t shm = sizeof(double) * (size_t)ADJ_WAVES * 64 * (2 * ADJP_LB + 1) + 16;
    HIP_TRY(hipFuncSetAttribute((const void *)legendre_adj_pol_kernel<NCT>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)shm));
    const int ntile = (p->npair + 64 * ADJ_WAVES - 1) / (64 * ADJ_WAVES);
    const long nitems = (long)p->L * (ncols / (16 * NCT)) * ntile;
    dim3 grid((unsigned)std::min<long>(nitems, (long)ctx->num_cu));
    HIP_TRY(hipMemsetAsync(p->d_queue, 0, 64, ctx->stream));
    legendre_adj_pol_kernel<NCT><<<grid, 512, shm, ctx->stream>>>(p->lmax, p->npair, p->nring, ncols, p->d_z, p->d_sth,
                                                                 p->d_coef, p->d_polc, p->d_lstart, p->d_seed, p->d_lmin,
                                                                 p->d_mcut, inter, part, p->d_queue);
    LAUNCH_CHECK();
    return 0;
}

// K4^T spin 2 + reduction over ring tiles: G_m cells of nchan interleaved (Q, U) channels -> (E, B) alm_dev
// (part: 2 slabs per ring tile)
int sht_legendre_adj_pol(corahip_ctx *ctx, corahip_sht_plan *p, int ncols, int nchan, const double *inter, double *part,
                         double *alm_dev) {
    int rc = sht_ensure_polc(ctx, p);
    if (rc) return rc;
    const int ntile = (p->npair + 64 * ADJ_WAVES - 1) / (64 * ADJ_WAVES);
    if (ntile > 16) return CORAHIP_EINVAL;      // (more than 16 ring tiles: nside > 16384)
    StageTimer t(ctx, "legendre_adj_pol");
    if ((ncols / 16) % 2 == 0) rc = launch_legendre_adj_pol<2>(ctx, p, ncols, inter, part);
    else rc = launch_legendre_adj_pol<1>(ctx, p, ncols, inter, part);
    if (rc) return rc;
    const int ntile128 = (p->npair + LMIN_RINGS - 1) / LMIN_RINGS;
    dim3 grid((unsigned)((p->L + 63) / 64), (unsigned)p->L);
    StageTimer tr(ctx, "alm_reduce_pol");       // (inside legendre_adj_pol: the reduction's share of it)
    alm_reduce_rows_pol_kernel<<<grid, 256, 0, ctx->stream>>>(part, p->nalm, ntile, ncols, p->lmax, ntile128, p->d_lmin,
                                                             nchan, alm_dev);
    LAUNCH_CHECK();
    return 0;
}
