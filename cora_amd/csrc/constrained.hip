// constrained.hip - mkconstrained (cora/core/skysim.py:139-201) without its host part: the eigenvectors of the k largest
// eigenvalues of every C_l, the weights W_l = V_k (V_k[f_ind, :])^-1 that turn the k constraint a_lm into all F channels,
// and their application to a_lm in the device layout.
//
//   eig_top_kernel   one workgroup of 256 threads per l: block orthogonal iteration on a block X of 16 columns (one
//                    v_mfma_f64_16x16x4 tile wide), X and Y = C X in LDS [F16][16], C_l streamed from global memory (only
//                    its lower triangle is read).  A product is 4 waves x row blocks of 16 x chunks of 16 k: a lane loads
//                    4 neighbouring k of its row (or, above the diagonal, of its column: 128-byte runs either way) and
//                    issues 4 MFMAs; the k-slots of the MFMA are permuted to fit the loads, in A and B alike.
//                    Orthogonalisation: classical Gram-Schmidt, every column twice, a thread owning rows tid + 256 n of
//                    all columns; a column whose norm falls to F u times the largest column norm of the block is DEFLATED
//                    (kept zero, which C X keeps zero) - the synchrotron covariance has numerical rank below 16 and plain
//                    Cholesky-QR breaks down on it.
//                    Rayleigh-Ritz after products 1, 2, every 4th and the last: G = X^T Y symmetrised, cyclic Jacobi on
//                    the 16 x 16 matrix in LDS, Ritz values in ascending algebraic order (deflated columns in front),
//                    X <- X Q, Y <- Y Q.  STOP: every one of the top k Ritz pairs has |Y_j - theta_j X_j|_2 <=
//                    8 F u |C|_inf (|C|_inf from the row sums of the first product).  With F <= 16 the start block is the
//                    identity and the first Rayleigh-Ritz step is the whole decomposition.
//                    The iteration finds the eigenvalues of largest MAGNITUDE; a block whose most negative Ritz value
//                    outweighs the k-th largest one is handed to the full decomposition, like one that has not met the
//                    stop rule after max_iter products (info = 1).
//   eig_full_kernel  the fallback: jacobi_sweeps (jacobi_sweep.h, the iteration of jacobi_root_kernel) on a symmetrised
//                    copy in global scratch, the k last columns in ascending order.  The list of such l is made on the
//                    host from info, as corahip_factor_batched makes its own.
//   cw_weights_kernel  per l >= 1: LU with partial pivoting of A = (V[f_ind, :])^T (k <= 8, one thread, LDS), then one
//                    thread per channel solves A w = V[f, :].  W[0] = 0 and V[0] is not read.
//   cw_mix_kernel    out[f, lm] = sum_j W[l, f, j] in[j, lm], j ascending, one thread per (packed index, group of 4
//                    output channels), 32-byte loads and stores; padding channels of the output are written as 0.
// No atomics, fixed reduction orders, the start block a hash of (F, row, column): identical bits from call to call.
#include "jacobi_sweep.h"
#include "mfma_tile.h"

#include <algorithm>
#include <vector>

namespace {

constexpr int ET_B = 16;       // block width: one MFMA tile
constexpr int ET_NT = 256;
constexpr int ET_KMAX = 8;     // most eigenpairs asked for
constexpr int ET_GP = 17;      // row pitch of the 16 x 16 matrices in LDS
// a cost setting (the stop rule decides correctness): at F = 258 on an MI355X a product with its share of the orthogonalisations and
// Rayleigh-Ritz steps takes 0.16 ms (Toeplitz exp(-|i-j|/3): about 120 products, 20 ms for six matrices side by side), the full
// decomposition 210 ms - the cap spends at most a fifth of a fallback before it gives up
constexpr int ET_DEFAULT_MAX_ITER = 256;
// LDS behind X and Y, in doubles: G, Q [16][17], cs [16], th [16], wred [4][16], order [16] ints
constexpr int ET_SMALL = 2 * ET_B * ET_GP + 16 + 16 + 4 * 16 + 8;
constexpr double ET_U = 1.1102230246251565e-16;   // 2^-53

size_t et_lds_bytes(int Fp) { return sizeof(double) * ((size_t)2 * Fp * ET_B + ET_SMALL) + 16; }

int et_max_f(corahip_ctx *ctx, int *max_f) {
    int lds = 0;
    HIP_TRY(hipDeviceGetAttribute(&lds, hipDeviceAttributeMaxSharedMemoryPerBlock, ctx->device));
    const long room = ((long)lds - 16) / (long)sizeof(double) - ET_SMALL;
    *max_f = room < 2 * ET_B * 16 ? 0 : (int)(room / (2 * ET_B) / 16 * 16);
    return 0;
}

// sums of the 256 threads' v[0 .. N) in a fixed order, returned to every thread: lanes by halving __shfl_down, then
// ((w0 + w1) + w2) + w3 through buf [4][N] (LDS).  The barrier in front frees buf of its earlier readers.
template <int N>
__device__ __forceinline__ void et_block_sum(double (&v)[N], double *buf) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1)
#pragma unroll
        for (int n = 0; n < N; n++) v[n] += __shfl_down(v[n], o, 64);
    __syncthreads();
    if (lane == 0)
#pragma unroll
        for (int n = 0; n < N; n++) buf[wave * N + n] = v[n];
    __syncthreads();
#pragma unroll
    for (int n = 0; n < N; n++) v[n] = ((buf[n] + buf[N + n]) + buf[2 * N + n]) + buf[3 * N + n];
}

// entry (i, j) of the start block: a fixed hash of (F, i, j) in [-1, 1)
__device__ __forceinline__ double et_start(int F, int i, int j) {
    unsigned h = (unsigned)F * 0x9E3779B1u ^ (unsigned)i * 0x85EBCA77u ^ (unsigned)j * 0xC2B2AE3Du;
    h ^= h >> 15;
    h *= 0x2C1B3C6Du;
    h ^= h >> 12;
    h *= 0x297A2D39u;
    h ^= h >> 15;
    return (double)(int)h * (1.0 / 2147483648.0);
}

// Y = C X for the symmetric C [F][F] of which the lower triangle is read; X, Y [Fp][16] in LDS, rows F .. Fp of X zero.
// NORM: returns the largest absolute row sum among the rows this lane met (the caller takes the maximum over the block).
template <bool NORM>
__device__ __forceinline__ double et_product(const double *__restrict__ A, int F, int Fp, const double *X, double *Y) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, ri = lane & 15, kq = lane >> 4;
    double nmax = 0.0;
    for (int row0 = 16 * wave; row0 < Fp; row0 += 64) {
        acc_tile<1, 1> acc;
        acc.zero();
        const int i = row0 + ri;
        double rs = 0.0;
        for (int kb = 0; kb < Fp; kb += 16) {
            double a[4];
#pragma unroll
            for (int s = 0; s < 4; s++) {
                const int j = kb + 4 * kq + s;
                double v = 0.0;
                if (i < F && j < F) v = j <= i ? A[(size_t)i * F + j] : A[(size_t)j * F + i];
                a[s] = v;
                if (NORM) rs += fabs(v);
            }
            // k-slot kq of step s is k = kb + 4 kq + s, for the A and the B fragment alike
#pragma unroll
            for (int s = 0; s < 4; s++) acc.fma16(0, 0, a[s], X[(kb + 4 * kq + s) * ET_B + ri]);
        }
#pragma unroll
        for (int r = 0; r < 4; r++) Y[(row0 + kq + 4 * r) * ET_B + ri] = acc.acc[0][0][r];
        if (NORM) {
            rs += __shfl_xor(rs, 16, 64);
            rs += __shfl_xor(rs, 32, 64);
            nmax = fmax(nmax, rs);
        }
    }
    return nmax;
}

// Orthonormalises the columns of M [..][16] (LDS) in place, left to right, by classical Gram-Schmidt applied twice; a
// column whose norm is not above F u times the largest column norm M came with is set to zero.  Returns the mask of the
// columns kept.  A thread owns the rows tid + 256 n of every column, so only the sums cross threads.
__device__ unsigned et_orth(double *M, int F, double *wred) {
    const int tid = threadIdx.x;
    double n2[ET_B];
#pragma unroll
    for (int c = 0; c < ET_B; c++) n2[c] = 0.0;
    for (int i = tid; i < F; i += ET_NT)
#pragma unroll
        for (int c = 0; c < ET_B; c++) {
            const double x = M[i * ET_B + c];
            n2[c] = fma(x, x, n2[c]);
        }
    et_block_sum<ET_B>(n2, wred);
    double maxn2 = 0.0;
#pragma unroll
    for (int c = 0; c < ET_B; c++) maxn2 = fmax(maxn2, n2[c]);
    const double fu = (double)F * ET_U, thr2 = fu * fu * maxn2;
    unsigned live = 0;
    for (int j = 0; j < ET_B; j++) {
        for (int pass = 0; pass < 2 && j > 0; pass++) {
            double d[ET_B];
#pragma unroll
            for (int g = 0; g < ET_B; g++) d[g] = 0.0;
            for (int i = tid; i < F; i += ET_NT) {
                const double yj = M[i * ET_B + j];
#pragma unroll
                for (int g = 0; g < ET_B; g++)
                    if (g < j) d[g] = fma(M[i * ET_B + g], yj, d[g]);
            }
            et_block_sum<ET_B>(d, wred);
            for (int i = tid; i < F; i += ET_NT) {
                double s = 0.0;
#pragma unroll
                for (int g = 0; g < ET_B; g++)
                    if (g < j) s = fma(d[g], M[i * ET_B + g], s);
                M[i * ET_B + j] -= s;
            }
        }
        double nn[1] = {0.0};
        for (int i = tid; i < F; i += ET_NT) {
            const double x = M[i * ET_B + j];
            nn[0] = fma(x, x, nn[0]);
        }
        et_block_sum<1>(nn, wred);
        const bool keep = nn[0] > thr2;          // (false for a NaN norm and for an all-zero block)
        const double inv = keep ? 1.0 / sqrt(nn[0]) : 0.0;
        for (int i = tid; i < F; i += ET_NT) M[i * ET_B + j] = keep ? M[i * ET_B + j] * inv : 0.0;
        if (keep) live |= 1u << j;
    }
    __syncthreads();
    return live;
}

// cyclic Jacobi on the symmetric G [16][ET_GP] in LDS, rotations accumulated in Q (the identity on entry): the rotation
// and the round-robin schedule of jacobi_sweeps, for 16 players
__device__ void et_jacobi16(double *G, double *Q, double *cs, double *wred) {
    const int tid = threadIdx.x, ga = tid >> 4, gc = tid & 15;
    auto pair_of = [](int k, int round, int &p, int &q) {
        const int m = ET_B - 1;
        p = k == 0 ? 0 : (k - 1 - round + m) % m + 1;
        q = (ET_B - 2 - k - round + m) % m + 1;
        if (p > q) { const int t = p; p = q; q = t; }
    };
    double prev = INFINITY;
    for (int sweep = 0; sweep < 30; sweep++) {
        const double x = G[ga * ET_GP + gc];
        double v[2] = {ga == gc ? 0.0 : x * x, ga == gc ? x * x : 0.0};
        et_block_sum<2>(v, wred);
        if (v[0] <= 1e-30 * v[1] || v[0] == 0.0 || v[0] >= prev) break;
        prev = v[0];
        for (int round = 0; round < ET_B - 1; round++) {
            if (tid < ET_B / 2) {
                int p, q;
                pair_of(tid, round, p, q);
                double c = 1.0, s = 0.0;
                const double apq = G[p * ET_GP + q];
                if (apq != 0.0) {
                    const double app = G[p * ET_GP + p], aqq = G[q * ET_GP + q];
                    const double tau = (aqq - app) / (2.0 * apq);
                    const double t = (tau >= 0.0 ? 1.0 : -1.0) / (fabs(tau) + sqrt(1.0 + tau * tau));
                    c = 1.0 / sqrt(1.0 + t * t);
                    s = t * c;
                }
                cs[2 * tid] = c;
                cs[2 * tid + 1] = s;
            }
            __syncthreads();
            if (tid < 128) {          // rows: G <- J^T G
                const int k = tid >> 4, j = tid & 15;
                int p, q;
                pair_of(k, round, p, q);
                const double c = cs[2 * k], s = cs[2 * k + 1];
                const double wp = G[p * ET_GP + j], wq = G[q * ET_GP + j];
                G[p * ET_GP + j] = c * wp - s * wq;
                G[q * ET_GP + j] = s * wp + c * wq;
            }
            __syncthreads();
            if (tid < 128) {          // columns: G <- G J, Q <- Q J
                const int k = tid & 7, i = tid >> 3;
                int p, q;
                pair_of(k, round, p, q);
                const double c = cs[2 * k], s = cs[2 * k + 1];
                const double wp = G[i * ET_GP + p], wq = G[i * ET_GP + q];
                G[i * ET_GP + p] = c * wp - s * wq;
                G[i * ET_GP + q] = s * wp + c * wq;
                const double vp = Q[i * ET_GP + p], vq = Q[i * ET_GP + q];
                Q[i * ET_GP + p] = c * vp - s * vq;
                Q[i * ET_GP + q] = s * vp + c * vq;
            }
            __syncthreads();
        }
    }
}

__global__ void __launch_bounds__(ET_NT)
eig_top_kernel(const double *__restrict__ C, int F, int Fp, int k, int max_iter, double *__restrict__ V,
               double *__restrict__ theta, int32_t *__restrict__ info) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    double *X = lds, *Y = X + (size_t)Fp * ET_B;
    double *G = Y + (size_t)Fp * ET_B, *Q = G + ET_B * ET_GP, *cs = Q + ET_B * ET_GP, *th = cs + 16, *wred = th + 16;
    int *order = reinterpret_cast<int *>(wred + 4 * 16);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l = blockIdx.x;
    const double *A = C + (size_t)l * F * F;
    const int b = F < ET_B ? F : ET_B;
    const bool whole = b == F;        // the block spans the space: identity start, the first Rayleigh-Ritz step decides

    for (int q = tid; q < Fp * ET_B; q += ET_NT) {
        const int i = q >> 4, j = q & 15;
        double v = 0.0;
        if (i < F && j < b) v = whole ? (i == j ? 1.0 : 0.0) : et_start(F, i, j);
        X[q] = v;
        Y[q] = 0.0;
    }
    __syncthreads();
    unsigned live = whole ? (1u << b) - 1u : et_orth(X, F, wred);

    double tol = 0.0;
    int nprod = 0;
    for (;;) {
        if (nprod == 0) {
            double nm = et_product<true>(A, F, Fp, X, Y);
#pragma unroll
            for (int o = 32; o >= 1; o >>= 1) nm = fmax(nm, __shfl_xor(nm, o, 64));
            if (lane == 0) th[wave] = nm;
            __syncthreads();
            tol = 8.0 * (double)F * ET_U * fmax(fmax(th[0], th[1]), fmax(th[2], th[3]));
        } else {
            et_product<false>(A, F, Fp, X, Y);
        }
        nprod++;
        __syncthreads();
        if (nprod <= 2 || (nprod & 3) == 0 || nprod >= max_iter || whole) {
            // ---- Rayleigh-Ritz: G = X^T Y, symmetrised
            {
                const int ga = tid >> 4, gc = tid & 15;
                double g = 0.0;
                for (int i = 0; i < F; i++) g = fma(X[i * ET_B + ga], Y[i * ET_B + gc], g);
                Q[ga * ET_GP + gc] = g;
                __syncthreads();
                G[ga * ET_GP + gc] = 0.5 * (Q[ga * ET_GP + gc] + Q[gc * ET_GP + ga]);
                __syncthreads();
                Q[ga * ET_GP + gc] = ga == gc ? 1.0 : 0.0;
                __syncthreads();
            }
            et_jacobi16(G, Q, cs, wred);
            __syncthreads();
            // Ritz values in ascending algebraic order, the deflated columns in front
            if (tid < ET_B) th[tid] = ((live >> tid) & 1u) ? G[tid * ET_GP + tid] : -INFINITY;
            __syncthreads();
            if (tid < ET_B) {
                int rank = 0;
                const double e = th[tid];
                for (int j = 0; j < ET_B; j++) {
                    const double f = th[j];
                    if (f < e || (f == e && j < tid)) rank++;
                }
                order[tid] = rank;
                cs[rank] = e;                       // (NaN Ritz values collide here: nothing converges, the fallback decides)
            }
            __syncthreads();
            // X <- X Q, Y <- Y Q, column c of the product to place order[c]
            for (int i = tid; i < F; i += ET_NT) {
                double xr[ET_B], yr[ET_B];
#pragma unroll
                for (int a = 0; a < ET_B; a++) xr[a] = X[i * ET_B + a], yr[a] = Y[i * ET_B + a];
                for (int c = 0; c < ET_B; c++) {
                    double sx = 0.0, sy = 0.0;
#pragma unroll
                    for (int a = 0; a < ET_B; a++) {
                        const double qa = Q[a * ET_GP + c];
                        sx = fma(xr[a], qa, sx);
                        sy = fma(yr[a], qa, sy);
                    }
                    const int o = order[c];
                    X[i * ET_B + o] = sx;
                    Y[i * ET_B + o] = sy;
                }
            }
            const int nlive = __popc(live);
            live = nlive >= ET_B ? 0xffffu : (((1u << nlive) - 1u) << (ET_B - nlive));
            __syncthreads();
            // residuals of the top k pairs
            double r[ET_KMAX];
#pragma unroll
            for (int c = 0; c < ET_KMAX; c++) r[c] = 0.0;
            for (int i = tid; i < F; i += ET_NT)
#pragma unroll
                for (int c = 0; c < ET_KMAX; c++)
                    if (c < k) {
                        const int col = ET_B - k + c;
                        const double d = fma(-cs[col], X[i * ET_B + col], Y[i * ET_B + col]);
                        r[c] = fma(d, d, r[c]);
                    }
            et_block_sum<ET_KMAX>(r, wred);
            bool ok = nlive >= k;
#pragma unroll
            for (int c = 0; c < ET_KMAX; c++)
                if (c < k) ok = ok && sqrt(r[c]) <= tol;
            if (ok) {
                for (int q = tid; q < F * k; q += ET_NT) {
                    const int i = q / k, c = q - i * k;
                    V[((size_t)l * F + i) * k + c] = X[i * ET_B + ET_B - k + c];
                }
                if (tid < k) theta[(size_t)l * k + tid] = cs[ET_B - k + tid];
                if (tid == 0) info[l] = 0;
                return;
            }
            if (nlive < k) break;
            // a negative eigenvalue that outweighs the k-th largest one: the iteration ranks by magnitude, not for this block
            if (!whole && -cs[ET_B - nlive] > cs[ET_B - k]) break;
        }
        if (nprod >= max_iter) break;
        live = et_orth(Y, F, wred);
        double *t = X;
        X = Y;
        Y = t;
    }
    if (tid == 0) info[l] = 1;
}

// the full decomposition of the listed matrices: the k last eigenpairs of the symmetrised lower triangle
__global__ void __launch_bounds__(JAC_NT)
eig_full_kernel(const double *__restrict__ C, const int32_t *__restrict__ list, int F, int k, double *__restrict__ Wall,
                double *__restrict__ Vall, double *__restrict__ Vout, double *__restrict__ theta) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    double *cs = lds;                      // [F/2+1][2]
    double *red = lds + 2 * (F / 2 + 1);   // [JAC_NT]
    double *ev = red + JAC_NT;             // [F]
    int *order = reinterpret_cast<int *>(ev + F);       // [F]
    const int tid = threadIdx.x;
    const int l = list[blockIdx.x];
    const double *A = C + (size_t)l * F * F;
    double *W = Wall + (size_t)blockIdx.x * F * F;
    double *V = Vall + (size_t)blockIdx.x * F * F;
    for (long q = tid; q < (long)F * F; q += JAC_NT) {
        const int i = (int)(q / F), j = (int)(q % F);
        W[q] = (j <= i) ? A[(size_t)i * F + j] : A[(size_t)j * F + i];
        V[q] = (i == j) ? 1.0 : 0.0;
    }
    jacobi_sweeps(W, V, F, cs, red);
    for (int i = tid; i < F; i += JAC_NT) ev[i] = W[(size_t)i * F + i];
    __syncthreads();
    jacobi_rank(ev, order, F);
    __syncthreads();
    for (long q = tid; q < (long)F * F; q += JAC_NT) {
        const int i = (int)(q / F), j = (int)(q % F);
        const int c = order[j] - (F - k);
        if (c >= 0) Vout[((size_t)l * F + i) * k + c] = V[q];
    }
    for (int j = tid; j < F; j += JAC_NT) {
        const int c = order[j] - (F - k);
        if (c >= 0) theta[(size_t)l * k + c] = ev[j];
    }
}

struct cw_index {
    int v[ET_KMAX];
};

// W_l = V_l (V_l[f_ind, :])^-1: row f of W solves A w = V_l[f, :] with A[a][c] = V_l[f_ind[c], a]
__global__ void __launch_bounds__(64)
cw_weights_kernel(const double *__restrict__ V, int F, int k, cw_index find, int dup, double *__restrict__ W,
                  int32_t *__restrict__ info) {
    __shared__ double A[ET_KMAX][ET_KMAX];
    __shared__ int perm[ET_KMAX];
    __shared__ int sing;
    const int tid = threadIdx.x, l = blockIdx.x;
    double *Wl = W + (size_t)l * F * k;
    if (l == 0) {                          // skysim.py:191-192: l = 0 carries nothing; V[0] is not read
        for (int q = tid; q < F * k; q += 64) Wl[q] = 0.0;
        if (tid == 0) info[0] = 0;
        return;
    }
    const double *Vl = V + (size_t)l * F * k;
    if (tid == 0) {
        int bad = dup;
        for (int a = 0; a < k; a++) {
            perm[a] = a;
            for (int c = 0; c < k; c++) A[a][c] = Vl[(size_t)find.v[c] * k + a];
        }
        for (int c = 0; c < k && !bad; c++) {
            int p = c;
            double best = fabs(A[c][c]);
            for (int r = c + 1; r < k; r++)
                if (fabs(A[r][c]) > best) best = fabs(A[r][c]), p = r;
            if (A[p][c] == 0.0) {          // LAPACK getrf's info > 0, on which scipy's solve raises
                bad = 1;
                break;
            }
            if (p != c) {
                for (int cc = 0; cc < k; cc++) {
                    const double t = A[c][cc];
                    A[c][cc] = A[p][cc];
                    A[p][cc] = t;
                }
                const int t = perm[c];
                perm[c] = perm[p];
                perm[p] = t;
            }
            for (int r = c + 1; r < k; r++) {
                const double m = A[r][c] / A[c][c];
                A[r][c] = m;
                for (int cc = c + 1; cc < k; cc++) A[r][cc] = fma(-m, A[c][cc], A[r][cc]);
            }
        }
        sing = bad;
    }
    __syncthreads();
    if (sing) {
        for (int q = tid; q < F * k; q += 64) Wl[q] = __builtin_nan("");
        if (tid == 0) info[l] = 2;
        return;
    }
    for (int f = tid; f < F; f += 64) {
        double y[ET_KMAX];
#pragma unroll
        for (int a = 0; a < ET_KMAX; a++) y[a] = a < k ? Vl[(size_t)f * k + perm[a]] : 0.0;
#pragma unroll
        for (int a = 0; a < ET_KMAX; a++)          // L y' = P y (unit diagonal)
#pragma unroll
            for (int c = 0; c < ET_KMAX; c++)
                if (c < a && a < k) y[a] = fma(-A[a][c], y[c], y[a]);
#pragma unroll
        for (int a = ET_KMAX - 1; a >= 0; a--) {   // U w = y'
#pragma unroll
            for (int c = ET_KMAX - 1; c >= 0; c--)
                if (c > a && c < k) y[a] = fma(-A[a][c], y[c], y[a]);
            if (a < k) y[a] = y[a] / A[a][a];
        }
#pragma unroll
        for (int a = 0; a < ET_KMAX; a++)
            if (a < k) Wl[(size_t)f * k + a] = y[a];
    }
    if (tid == 0) info[l] = 0;
}

// one thread per (packed index, group of 4 output channels)
__global__ void __launch_bounds__(256)
cw_mix_kernel(const double *__restrict__ in, int lmax, int k, int Gin, int F, int Gout, const double *__restrict__ W,
              double *__restrict__ out) {
    const long n = nalm_of(lmax) * Gout;
    for (long q = (long)blockIdx.x * blockDim.x + threadIdx.x; q < n; q += (long)gridDim.x * blockDim.x) {
        const long idx = q / Gout;
        const int g = (int)(q - idx * Gout);
        const long l = alm_l_of_idx(idx, lmax);
        const double *Wl = W + (size_t)l * F * k;
        d4_t ore = {0.0, 0.0, 0.0, 0.0}, oim = {0.0, 0.0, 0.0, 0.0};
        for (int gi = 0; gi < Gin; gi++) {
            const d4_t re = *reinterpret_cast<const d4_t *>(in + (idx * Gin + gi) * 8);
            const d4_t im = *reinterpret_cast<const d4_t *>(in + (idx * Gin + gi) * 8 + 4);
#pragma unroll
            for (int v = 0; v < 4; v++) {
                const int j = 4 * gi + v;
                if (j < k) {               // (the padding channels of the input take no part)
#pragma unroll
                    for (int u = 0; u < 4; u++) {
                        const int f = 4 * g + u;
                        if (f < F) {
                            const double w = Wl[(size_t)f * k + j];
                            ore[u] = fma(w, re[v], ore[u]);
                            oim[u] = fma(w, im[v], oim[u]);
                        }
                    }
                }
            }
        }
        *reinterpret_cast<d4_t *>(out + q * 8) = ore;
        *reinterpret_cast<d4_t *>(out + q * 8 + 4) = oim;
    }
}

}  // namespace

extern "C" {

int corahip_eig_top_max_f(corahip_ctx *ctx, int *max_f) {
    ARG_CHECK(ctx != nullptr && max_f != nullptr);
    return et_max_f(ctx, max_f);
}

int corahip_eig_top_batched(corahip_ctx *ctx, const double *C, int nl, int F, int k, int max_iter, double *V, double *theta,
                            int32_t *info) {
    ARG_CHECK(ctx != nullptr && C != nullptr && V != nullptr && theta != nullptr && info != nullptr);
    ARG_CHECK(nl >= 1 && F >= 1 && k >= 1 && k <= ET_KMAX && k <= F);
    int max_f = 0;
    if (int rc = et_max_f(ctx, &max_f)) return rc;
    if (F > max_f) {     // X and Y = C X live in the LDS of the workgroup: nothing is launched for a block that cannot
        corahip_set_error("invalid argument: F = %d channels exceed the limit of %d (two F x 16 blocks in the LDS of a workgroup) (%s:%d)",
                          F, max_f, __FILE__, __LINE__);
        return CORAHIP_EINVAL;
    }
    const size_t cbytes = (size_t)nl * F * F * 8, vbytes = (size_t)nl * F * k * 8, tbytes = (size_t)nl * k * 8, ibytes = (size_t)nl * 4;
    ARG_CHECK(!overlaps(V, vbytes, C, cbytes) && !overlaps(theta, tbytes, C, cbytes) && !overlaps(info, ibytes, C, cbytes));
    ARG_CHECK(!overlaps(V, vbytes, theta, tbytes) && !overlaps(V, vbytes, info, ibytes) && !overlaps(theta, tbytes, info, ibytes));
    if (max_iter <= 0) max_iter = ET_DEFAULT_MAX_ITER;
    StageTimer t(ctx, "eig_top");
    const int Fp = (F + 15) / 16 * 16;
    const size_t shm = et_lds_bytes(Fp);
    HIP_TRY(hipFuncSetAttribute((const void *)eig_top_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shm));
    eig_top_kernel<<<nl, ET_NT, shm, ctx->stream>>>(C, F, Fp, k, max_iter, V, theta, info);
    LAUNCH_CHECK();
    // the full decomposition for the blocks the iteration gave up on (host round trip, as in corahip_factor_batched)
    std::vector<int32_t> hinfo(nl);
    HIP_TRY(hipMemcpyAsync(hinfo.data(), info, sizeof(int32_t) * nl, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    std::vector<int32_t> list;
    for (int l = 0; l < nl; l++)
        if (hinfo[l] != 0) list.push_back(l);
    if (list.empty()) return 0;
    const size_t per = (size_t)2 * F * F * sizeof(double);
    const size_t batch = std::max<size_t>(1, std::min<size_t>(list.size(), ((size_t)1 << 31) / per));
    dev_buf<int32_t> dlist;
    dev_buf<double> scratch;
    HIP_TRY(dlist.alloc(list.size()));
    if (scratch.alloc(per * batch / sizeof(double)) != hipSuccess) {
        corahip_set_error("eig_top_batched: no memory for the scratch of the full decomposition (%zu bytes)", per * batch);
        return CORAHIP_ENOMEM;
    }
    {
        int rcf = corahip_debug_fill(ctx, dlist, sizeof(int32_t) * list.size());
        if (!rcf) rcf = corahip_debug_fill(ctx, scratch, per * batch);
        if (rcf) return rcf;
    }
    HIP_TRY(hipMemcpyAsync(dlist, list.data(), sizeof(int32_t) * list.size(), hipMemcpyHostToDevice, ctx->stream));
    const size_t shj = sizeof(double) * (2 * (F / 2 + 1) + JAC_NT + F) + sizeof(int) * (F + 4) + 16;
    for (size_t b0 = 0; b0 < list.size(); b0 += batch) {
        const int nb = (int)std::min(batch, list.size() - b0);
        eig_full_kernel<<<nb, JAC_NT, shj, ctx->stream>>>(C, dlist + b0, F, k, scratch, scratch + (size_t)nb * F * F, V, theta);
        LAUNCH_CHECK();
    }
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return 0;
}

int corahip_constrained_weights(corahip_ctx *ctx, const double *V, int nl, int F, int k, const int32_t *f_ind, double *W,
                                int32_t *info) {
    ARG_CHECK(ctx != nullptr && V != nullptr && f_ind != nullptr && W != nullptr && info != nullptr);
    ARG_CHECK(nl >= 1 && F >= 1 && k >= 1 && k <= ET_KMAX && k <= F);
    cw_index find = {};
    int dup = 0;
    for (int a = 0; a < k; a++) {
        if (f_ind[a] < 0 || f_ind[a] >= F) {
            corahip_set_error("invalid argument: f_ind[%d] = %d is not a channel of 0 .. %d (%s:%d)", a, (int)f_ind[a], F - 1, __FILE__,
                              __LINE__);
            return CORAHIP_EINVAL;
        }
        for (int c = 0; c < a; c++)
            if (f_ind[c] == f_ind[a]) dup = 1;       // two equal rows: singular for every l, reported as such (info = 2)
        find.v[a] = f_ind[a];
    }
    const size_t vbytes = (size_t)nl * F * k * 8;
    ARG_CHECK(!overlaps(W, vbytes, V, vbytes) && !overlaps(info, (size_t)nl * 4, V, vbytes) && !overlaps(info, (size_t)nl * 4, W, vbytes));
    StageTimer t(ctx, "constrained_weights");
    cw_weights_kernel<<<nl, 64, 0, ctx->stream>>>(V, F, k, find, dup, W, info);
    LAUNCH_CHECK();
    return 0;
}

int corahip_alm_mix_l(corahip_ctx *ctx, const double *alm_in, int lmax, int k, const double *W, int F, double *alm_out) {
    ARG_CHECK(ctx && alm_in && W && alm_out && lmax >= 0 && k >= 1 && F >= 1);
    const int Gin = (k + 3) / 4, Gout = (F + 3) / 4;
    const size_t ibytes = (size_t)nalm_of(lmax) * (size_t)Gin * 64, obytes = (size_t)nalm_of(lmax) * (size_t)Gout * 64;
    ARG_CHECK(!overlaps(alm_out, obytes, alm_in, ibytes));
    ARG_CHECK(!overlaps(alm_out, obytes, W, (size_t)(lmax + 1) * F * k * 8));
    ARG_CHECK(is_aligned(alm_in, 32) && is_aligned(alm_out, 32));
    StageTimer t(ctx, "alm_mix_l");
    hipLaunchKernelGGL(cw_mix_kernel, dim3(grid_blocks(ctx, nalm_of(lmax) * Gout)), dim3(256), 0, ctx->stream, alm_in, lmax, k, Gin, F,
                       Gout, W, alm_out);
    LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
