// jacobi_sweep.h - the parallel cyclic Jacobi iteration shared by jacobi_root_kernel (factor.hip) and the full
// decomposition behind corahip_eig_top_batched (constrained.hip); device code only.
#pragma once
#include "common.h"

#define JAC_NT 1024

// Diagonalises the symmetric W [F][F] in place by round-robin sweeps and accumulates the rotations in V [F][F], which the
// caller has set to the identity: on return the diagonal of W holds the eigenvalues and column j of V the eigenvector of
// W[j][j].  One workgroup of JAC_NT threads; W and V in global memory, written by the whole workgroup before the call
// (the function's first barrier publishes them).  cs [F/2+1][2] and red [JAC_NT] are LDS scratch.
// The iteration is a chain of L2 round trips (a rotation is two loads, two stores and a barrier away from the next one):
// 1024 threads keep four times as many of them in flight as 256 did, the column pass walks the pairs fastest so that a
// wave stays inside one row of W and V, and the round-robin schedule is computed, not rotated in LDS by one thread
// (F = 418: 3.2 -> 0.9 s per matrix, F = 256: 0.56 -> 0.15 s, the same bits).
__device__ __forceinline__ void jacobi_sweeps(double *W, double *V, int F, double *cs, double *red) {
    const int tid = threadIdx.x;
    const int np = (F + 1) / 2;      // pairs per round
    const int nplayers = 2 * np;     // a dummy player F when F is odd
    // round-robin schedule: player 0 stays at position 0, the others move up one position per round (and are back where
    // they started after the nplayers - 1 rounds of a sweep); the pairs of a round are positions (k, nplayers - 1 - k)
    auto pair_of = [&](int k, int round, int &p, int &q) {
        const int m = nplayers - 1;
        p = k == 0 ? 0 : (k - 1 - round + m) % m + 1;
        q = (nplayers - 2 - k - round + m) % m + 1;
        if (p > q) { const int t = p; p = q; q = t; }
    };
    __syncthreads();

    double prev_offs = INFINITY;
    for (int sweep = 0; sweep < 60; sweep++) {
        // convergence: off-diagonal Frobenius norm vs diagonal
        double offs = 0.0, dia = 0.0;
        for (long q = tid; q < (long)F * F; q += JAC_NT) {
            const int i = (int)(q / F), j = (int)(q % F);
            const double v = W[q];
            if (i == j) dia += v * v;
            else offs += v * v;
        }
        const auto plus = [](double a, double b) { return a + b; };
        offs = block_reduce<JAC_NT>(offs, red, plus);
        dia = block_reduce<JAC_NT>(dia, red, plus);
        if (offs <= 1e-30 * dia || offs == 0.0) break;
        // A rotation lowers the off-diagonal norm by 2 a_pq^2 in exact arithmetic, so a sweep that did not lower it has
        // reached rounding.  That floor is ~F u |W|: from F ~ 100 on it can lie ABOVE the relative rule of the line before,
        // which then never fires (measured at F = 384 - 418: all 60 sweeps, 10 - 12 s per matrix, against 2.6 - 3.6 s).
        if (offs >= prev_offs) break;
        prev_offs = offs;

        for (int round = 0; round < nplayers - 1; round++) {
            for (int k = tid; k < np; k += JAC_NT) {
                int p, q;
                pair_of(k, round, p, q);
                double c = 1.0, s = 0.0;
                if (q < F) {
                    const double apq = W[(size_t)p * F + q];
                    if (apq != 0.0) {
                        const double app = W[(size_t)p * F + p], aqq = W[(size_t)q * F + q];
                        const double tau = (aqq - app) / (2.0 * apq);
                        const double t = (tau >= 0.0 ? 1.0 : -1.0) / (fabs(tau) + sqrt(1.0 + tau * tau));
                        c = 1.0 / sqrt(1.0 + t * t);
                        s = t * c;
                    }
                }
                cs[2 * k] = c;
                cs[2 * k + 1] = s;
            }
            __syncthreads();
            // rows: W <- J^T W
            for (int it = tid; it < np * F; it += JAC_NT) {
                const int k = it / F, j = it % F;
                int p, q;
                pair_of(k, round, p, q);
                if (q >= F) continue;
                const double c = cs[2 * k], s = cs[2 * k + 1];
                const double wp = W[(size_t)p * F + j], wq = W[(size_t)q * F + j];
                W[(size_t)p * F + j] = c * wp - s * wq;
                W[(size_t)q * F + j] = s * wp + c * wq;
            }
            __syncthreads();
            // columns: W <- W J, V <- V J
            for (int it = tid; it < np * F; it += JAC_NT) {
                const int k = it % np, i = it / np;
                int p, q;
                pair_of(k, round, p, q);
                if (q >= F) continue;
                const double c = cs[2 * k], s = cs[2 * k + 1];
                const double wp = W[(size_t)i * F + p], wq = W[(size_t)i * F + q];
                W[(size_t)i * F + p] = c * wp - s * wq;
                W[(size_t)i * F + q] = s * wp + c * wq;
                const double vp = V[(size_t)i * F + p], vq = V[(size_t)i * F + q];
                V[(size_t)i * F + p] = c * vp - s * vq;
                V[(size_t)i * F + q] = s * vp + c * vq;
            }
            __syncthreads();
        }
    }
}

// ranks of ev[0 .. F) in ascending order, ties by index (stable): order[i] = the place of ev[i].  LDS arrays; the caller
// puts a barrier in front (ev complete) and behind (order complete)
__device__ __forceinline__ void jacobi_rank(const double *ev, int *order, int F) {
    for (int i = threadIdx.x; i < F; i += JAC_NT) {
        int rank = 0;
        const double e = ev[i];
        for (int j = 0; j < F; j++) {
            const double f = ev[j];
            if (f < e || (f == e && j < i)) rank++;
        }
        order[i] = rank;
    }
}
