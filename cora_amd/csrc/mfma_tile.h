// mfma_tile.h - the FP64 MFMA tile mainloop shared by the feature GEMM kernels (device code only): dgemm_nn_kernel
// (corrfunc.hip), slice_mix_kernel (lsschain.hip), cross_spectra_kernel (spectra.hip), faraday_mix_kernel (faraday.hip).
// The K1-K5 kernels are tuned one by one and do not use it.
//
// v_mfma_f64_16x16x4_f64 multiplies a 16 x 4 block of A by a 4 x 16 block of B into a 16 x 16 block of C/D.  Lane roles:
// with ri = lane & 15 and kq = lane >> 4 a lane holds A row ri at k-slot kq, B column ri at k-slot kq, and of C/D
// column ri at rows kq + 4 r (r = 0..3, the four doubles of a d4_t).
#pragma once
#include "common.h"

// A workgroup of 4 waves in a 2 x 2 arrangement; a wave owns U x V blocks of 16 x 16: sub-tile origin (wr, wc).
template <int U, int V>
struct wave_roles {
    int tid, lane, wave, ri, kq, wr, wc;
    __device__ wave_roles()
        : tid(threadIdx.x), lane(tid & 63), wave(tid >> 6), ri(lane & 15), kq(lane >> 4), wr((wave >> 1) * 16 * U),
          wc((wave & 1) * 16 * V) {}
    // the lane's C/D elements of block (u, v), inside the sub-tile: one column, four rows r = 0..3
    __device__ int row(int u, int r) const { return 16 * u + kq + 4 * r; }
    __device__ int col(int v) const { return 16 * v + ri; }
};

// The accumulators of a wave's sub-tile.  Every MFMA of these kernels is issued by fma16.  An epilogue walks acc[u][v][r]
// as a plain loop nest and takes the element's place from wave_roles::row(u, r) and col(v), the only statement of the
// C/D layout.  (A for_each(f) that handed every element to a callback gave the same bits, but a slower epilogue in each
// kernel: the per-block address arithmetic was no longer formed once per block.)
template <int U, int V>
struct acc_tile {
    d4_t acc[U][V];

    __device__ __forceinline__ void zero() {
#pragma unroll
        for (int u = 0; u < U; u++)
#pragma unroll
            for (int v = 0; v < V; v++) acc[u][v] = (d4_t){0.0, 0.0, 0.0, 0.0};
    }
    __device__ __forceinline__ void scale(double s) {
#pragma unroll
        for (int u = 0; u < U; u++)
#pragma unroll
            for (int v = 0; v < V; v++) acc[u][v] = acc[u][v] * s;
    }
    __device__ __forceinline__ void fma16(int u, int v, double a, double b) {
        acc[u][v] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[u][v], 0, 0, 0);
    }
    // one k-step of 4: block (u, v) += a[u] b[v], u outer, v inner
    __device__ __forceinline__ void mma(const double (&a)[U], const double (&b)[V]) {
#pragma unroll
        for (int u = 0; u < U; u++)
#pragma unroll
            for (int v = 0; v < V; v++) fma16(u, v, a[u], b[v]);
    }
    // the same for the blocks with rowp[u] && colp[v]; the predicates must be wave-uniform (an MFMA runs with EXEC full).
    // a[u] is evaluated under rowp[u]: an operand that reads its fragment in operator[] (lds_rows) is not read for a
    // skipped block of rows
    template <class A>
    __device__ __forceinline__ void mma_if(const A &a, const double (&b)[V], const bool (&rowp)[U], const bool (&colp)[V]) {
#pragma unroll
        for (int u = 0; u < U; u++)
            if (rowp[u]) {
                const double au = a[u];
#pragma unroll
                for (int v = 0; v < V; v++)
                    if (colp[v]) fma16(u, v, au, b[v]);
            }
    }
};

// A fragments still in LDS: [u] reads the lane's element of the u-th block of 16 rows (pitch doubles per row)
struct lds_rows {
    const double *p;
    int pitch;
    __device__ __forceinline__ double operator[](int u) const { return p[16 * u * pitch]; }
};

// complex k-step on (re, im) operand planes: (cr + i ci)(u, v) += (ar + i ai)[u] (br + i bi)[v], per block in the order
// ar br, (-ai) bi into cr, then ar bi, ai br into ci
template <int U, int V>
__device__ __forceinline__ void complex_mma(acc_tile<U, V> &cr, acc_tile<U, V> &ci, const double (&ar)[U],
                                            const double (&ai)[U], const double (&br)[V], const double (&bi)[V]) {
#pragma unroll
    for (int u = 0; u < U; u++) {
        const double nai = -ai[u];
#pragma unroll
        for (int v = 0; v < V; v++) {
            cr.fma16(u, v, ar[u], br[v]);
            cr.fma16(u, v, nai, bi[v]);
            ci.fma16(u, v, ar[u], bi[v]);
            ci.fma16(u, v, ai[u], br[v]);
        }
    }
}

// The K loop over nchunk chunks staged global -> registers -> LDS, LDS double-buffered:
//   gload(c)        chunk c from global memory into the staging registers
//   lstore(buf, c)  the staging registers (chunk c) into LDS buffer buf
//   compute(c, buf) the MFMAs of chunk c out of LDS buffer buf
// The loads of chunk c+1 are issued before chunk c is multiplied, so they are in flight under its MFMAs; their LDS
// stores follow it.  One barrier per chunk is enough: the stores of iteration c go to the buffer that compute(c - 1)
// read, and every wave finished that before it passed the barrier that ended iteration c - 1; the same barrier at the
// end of iteration c publishes them to compute(c + 1).  Chunk 0 is staged and its barrier runs even with nchunk == 0
// (gload must be safe to call then; nothing is multiplied).
template <class G, class L, class C>
__device__ __forceinline__ void staged_k_loop(int nchunk, G &&gload, L &&lstore, C &&compute) {
    gload(0);
    lstore(0, 0);
    __syncthreads();
    for (int c = 0; c < nchunk; c++) {
        const int buf = c & 1;
        if (c + 1 < nchunk) gload(c + 1);
        compute(c, buf);
        if (c + 1 < nchunk) lstore(buf ^ 1, c + 1);
        __syncthreads();
    }
}

// C[row0 .. +128, col0 .. +128) = A B over k in [kbeg, kbeg + 16 nchunk), row-major, for one workgroup of 256 threads:
// 4 waves of 64 x 64 = 4 x 4 MFMA blocks (128 accumulator VGPRs), K in 16-deep chunks through As[128][17] (row, k) and
// Bs[16][132] (k, column).  A is [Mr, Kd] (lda), B is [Kd, N] (ldb); rows >= Mr and columns >= N are staged as zeros and
// not stored.
// RANGES: klo[u], khi[u] (multiples of 4, wave-uniform) bound the k of the wave's u-th block of 16 rows; MFMAs outside
//         [klo, khi) are not issued.  The chunks follow the ranges, so they may reach past Kd: k >= Kd is staged as
//         zeros.  Without ranges the caller passes whole chunks inside Kd (kbeg and Kd multiples of 16) and k is not tested.
// IX:     the type of columns and leading dimensions (int, or long where n ncol passes 2^31); offsets are 64-bit.
// VECB:   with vec != 0 (N and ldb even, B 16-byte aligned; wave-uniform) the B tile is staged 16 bytes per lane.
constexpr int GT_T = 128, GT_K = 16, GT_NT = 256;
template <bool RANGES, bool VECB, class IX>
__device__ __forceinline__ void gemm_nn_128(const double *__restrict__ A, IX lda, const double *__restrict__ B, IX ldb,
                                            double *__restrict__ C, IX ldc, int row0, IX col0, int Mr, IX N, int Kd,
                                            int kbeg, int nchunk, const int *klo, const int *khi, int vec) {
    constexpr int AS = GT_K + 1, BS = GT_T + 4;
    constexpr int NA = GT_T * GT_K / GT_NT, NB = GT_K * GT_T / GT_NT;
    __shared__ double As[2][GT_T * AS];
    __shared__ __attribute__((aligned(16))) double Bs[2][GT_K * BS];
    const wave_roles<4, 4> w;
    const int tid = w.tid;
    acc_tile<4, 4> acc;
    acc.zero();

    double ra[NA], rb[NB];
    auto gload = [&](int c) {
        const int kc = kbeg + c * GT_K;
#pragma unroll
        for (int u = 0; u < NA; u++) {
            const int e = tid + GT_NT * u;
            const int r = e / GT_K, k = e % GT_K;     // A tile: 128 rows x 16 k (128-byte runs per row)
            const int gr = row0 + r;
            ra[u] = (gr < Mr && (!RANGES || kc + k < Kd)) ? A[(size_t)gr * (size_t)lda + kc + k] : 0.0;
        }
        if (VECB && vec) {
#pragma unroll
            for (int u = 0; u < NB / 2; u++) {
                const int e = tid + GT_NT * u;
                const int k = e / (GT_T / 2), cc = 2 * (e % (GT_T / 2));    // B tile: 16 k x 64 column pairs
                const IX gc = col0 + cc;                                  // even, N even: the pair is inside or outside
                double2 x = make_double2(0.0, 0.0);
                if ((!RANGES || kc + k < Kd) && gc < N) x = *reinterpret_cast<const double2 *>(B + (size_t)(kc + k) * (size_t)ldb + (size_t)gc);
                rb[2 * u] = x.x, rb[2 * u + 1] = x.y;
            }
        } else {
#pragma unroll
            for (int u = 0; u < NB; u++) {
                const int e = tid + GT_NT * u;
                const int k = e / GT_T, cc = e % GT_T;      // B tile: 16 k x 128 columns (coalesced along the columns)
                const IX gc = col0 + cc;
                rb[u] = ((!RANGES || kc + k < Kd) && gc < N) ? B[(size_t)(kc + k) * (size_t)ldb + (size_t)gc] : 0.0;
            }
        }
    };
    auto lstore = [&](int buf, int) {
#pragma unroll
        for (int u = 0; u < NA; u++) {
            const int e = tid + GT_NT * u;
            As[buf][(e / GT_K) * AS + e % GT_K] = ra[u];
        }
        if (VECB && vec) {
#pragma unroll
            for (int u = 0; u < NB / 2; u++) {
                const int e = tid + GT_NT * u;
                *reinterpret_cast<double2 *>(&Bs[buf][(e / (GT_T / 2)) * BS + 2 * (e % (GT_T / 2))]) =
                    make_double2(rb[2 * u], rb[2 * u + 1]);
            }
        } else {
#pragma unroll
            for (int u = 0; u < NB; u++) {
                const int e = tid + GT_NT * u;
                Bs[buf][(e / GT_T) * BS + e % GT_T] = rb[u];
            }
        }
    };
    auto compute = [&](int c, int buf) {
        const double *as = As[buf], *bs = Bs[buf];
#pragma unroll
        for (int ks = 0; ks < GT_K / 4; ks++) {
            if constexpr (RANGES) {
                // the A fragments stay in LDS: mma_if reads one under its block's range test
                const lds_rows af = {as + (w.wr + w.ri) * AS + 4 * ks + w.kq, AS};
                double b[4];
#pragma unroll
                for (int v = 0; v < 4; v++) b[v] = bs[(4 * ks + w.kq) * BS + w.wc + 16 * v + w.ri];
                const int k4 = kbeg + c * GT_K + 4 * ks;
                bool in[4];
#pragma unroll
                for (int u = 0; u < 4; u++) in[u] = k4 >= klo[u] && k4 < khi[u];
                acc.mma_if(af, b, in, {true, true, true, true});
            } else {
                double a[4], b[4];
#pragma unroll
                for (int u = 0; u < 4; u++) a[u] = as[(w.wr + 16 * u + w.ri) * AS + 4 * ks + w.kq];
#pragma unroll
                for (int v = 0; v < 4; v++) b[v] = bs[(4 * ks + w.kq) * BS + w.wc + 16 * v + w.ri];
                acc.mma(a, b);
            }
        }
    };
    staged_k_loop(nchunk, gload, lstore, compute);

#pragma unroll
    for (int u = 0; u < 4; u++)
#pragma unroll
        for (int v = 0; v < 4; v++) {
            const IX gc = col0 + w.wc + w.col(v);
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int gr = row0 + w.wr + w.row(u, r);
                if (gr < Mr && gc < N) C[(size_t)gr * (size_t)ldc + (size_t)gc] = acc.acc[u][v][r];
            }
        }
}
