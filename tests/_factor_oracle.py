"""Host oracle for K2 (csrc/factor.hip, corahip_factor_batched): numpy only, no reference factor needed.

Every expected value is defined by IEEE arithmetic on the host or by a published bound:

  * ``jittered``           the matrix the device factors: C (lower triangle) + fl(max(diag) * jitter_rel) on the diagonal;
  * ``chol_bound_ratio``   Higham's componentwise backward-error bound of a Cholesky factor (Accuracy and Stability of
                           Numerical Algorithms, 2nd ed., Thm 10.3), |T T^T - Cj| <= gamma_n |T| |T|^T, as the ratio of
                           the two sides, formed in extended precision;
  * ``eigen_root_checks``  the eigen route's root V sqrt(e+) through quantities that do not depend on the sign or the
                           choice of the eigenvectors: the product, the column norms IN ORDER, the columns' orthogonality
                           and the dropped columns;
  * ``planted``            matrices with a known factor and a pivot of a chosen sign and size at a chosen place;
  * ``spectrum_matrix``    symmetric matrices with a chosen spectrum.

np.longdouble is the x87 80-bit format here (64-bit mantissa, eps 1.08e-19): its own rounding is 2000 times below the
float64 bound it measures.
"""
import numpy as np

LD = np.longdouble
U = 2.0 ** -53          # unit roundoff of float64


def gamma(n):
    """Higham's gamma_n = n u / (1 - n u) for float64."""
    return LD(n) * LD(U) / (LD(1) - LD(n) * LD(U))


def symmetric_from_lower(C):
    """The symmetric matrix whose lower triangle is that of ``C`` (the strict upper triangle of ``C`` is never read)."""
    C = np.asarray(C, dtype=np.float64)
    lo = np.tril(C)
    return lo + np.tril(C, -1).T


def jittered(C, jitter_rel):
    """Cj exactly as the device forms it: jit = fl(max(diag C) * jitter_rel) in float64 (signed: a negative diagonal
    gives a negative jitter), then ONE rounded add per diagonal element.  Only the lower triangle of C is used."""
    Cj = symmetric_from_lower(C)
    d = np.diagonal(Cj).copy()
    jit = np.float64(d.max()) * np.float64(jitter_rel)
    Cj[np.diag_indices_from(Cj)] = d + jit
    return Cj


def _lower_product(T, blk=64):
    """The lower triangle (upper part left zero) of T T^T for a LOWER-TRIANGULAR longdouble T, by row blocks that
    skip the zero part: a third of the full product (numpy has no BLAS for longdouble)."""
    F = T.shape[0]
    out = np.zeros((F, F), dtype=LD)
    for i0 in range(0, F, blk):
        i1 = min(F, i0 + blk)
        out[i0:i1, :i1] = T[i0:i1, :i1] @ T[:i1, :i1].T
    return np.tril(out)


def chol_bound_ratio(Cj, T, extra=8):
    """max over i >= j of |T T^T - Cj|_ij / (gamma_n (|T| |T|^T)_ij), n = F + extra, in longdouble.

    Thm 10.3 gives gamma_{F+1} for any summation order, with or without FMA.  Seven more units cover the two
    operations K2 does not round correctly: sqrt(d) formed as d * (1 / sqrt(d)) with the reciprocal root from two
    Newton steps, and the division by L_jj done as a multiplication by that reciprocal - a few u each per entry.
    Only the lower triangle of T enters; entries with a zero bound must have a zero residual."""
    Cj = np.asarray(Cj, dtype=np.float64)
    F = Cj.shape[0]
    Tl = np.tril(np.asarray(T, dtype=np.float64)).astype(LD)
    R = np.abs(_lower_product(Tl) - np.tril(Cj).astype(LD))
    B = gamma(F + extra) * _lower_product(np.abs(Tl))
    low = np.tril(np.ones((F, F), dtype=bool))
    zero = low & (B == 0)
    assert np.all(R[zero] == 0), "non-zero residual where the bound is zero"
    use = low & (B > 0)
    if not use.any():
        return 0.0
    return float((R[use] / B[use]).max())


def has_cholesky_structure(T):
    """Strict upper triangle exactly zero, diagonal > 0 (NaN fails both)."""
    T = np.asarray(T)
    return bool(np.all(np.triu(T, 1) == 0) and np.all(np.diagonal(T) > 0))


def is_cholesky_factor(Cj, T, ratio=None):
    """T is THE Cholesky factor of Cj to working precision: lower triangular with a positive diagonal (the factor with
    these two properties is unique) and inside the backward-error bound.  ``ratio``: chol_bound_ratio(Cj, T) if the
    caller has it already."""
    if not has_cholesky_structure(T):
        return False
    if ratio is None:
        ratio = chol_bound_ratio(Cj, T)
    return bool(ratio <= 1.0)


def eigen_spectrum(Cj, eig_thresh):
    """(e, V, e+): numpy's eigh of Cj (lower triangle, ascending) and the eigenvalues kept by the reference's rule,
    e+ = where(e < e.max() * eig_thresh, 0, e)."""
    e, V = np.linalg.eigh(np.asarray(Cj, dtype=np.float64))
    ep = np.where(e < e.max() * eig_thresh, 0.0, e)
    return e, V, ep


def eigen_root_checks(Cj, T, eig_thresh):
    """The eigen route's root T = V sqrt(e+) (columns by ascending eigenvalue) against numpy's eigh of Cj.  Returns a
    dict, the quantities formed in longdouble:
      a         max |T T^T - V e+ V^T| / max |V e+ V^T|   (0 / 0 counts as 0)
      b         max_j | ||T[:, j]||^2 - e+_j | / e.max()   - the columns in the order they come
      c         max_{j != k} |(T^T T)_jk| / e.max()
      zero_cols every column with e+_j == 0 is exactly zero
      count     the number of non-zero columns equals count(e+ > 0)
    (an all-negative spectrum has e.max() < 0: its scale is taken as |e.max()|, T must be zero)."""
    T = np.asarray(T, dtype=np.float64)
    e, V, ep = eigen_spectrum(Cj, eig_thresh)
    scale = LD(abs(e.max())) if e.max() != 0 else LD(1)
    Tq, Vq = T.astype(LD), V.astype(LD)
    M = (Vq * ep.astype(LD)) @ Vq.T
    P = Tq @ Tq.T
    mmax = np.abs(M).max()
    da = np.abs(P - M).max()
    a = float(da / mmax) if mmax > 0 else float(da)
    G = Tq.T @ Tq
    b = float(np.abs(np.diagonal(G) - ep.astype(LD)).max() / scale)
    off = G - np.diag(np.diagonal(G))
    c = float(np.abs(off).max() / scale) if T.shape[0] > 1 else 0.0
    nonzero = np.any(T != 0, axis=0)
    return {"a": a, "b": b, "c": c,
            "zero_cols": bool(not np.any(nonzero[ep == 0])),
            "count": bool(int(nonzero.sum()) == int((ep > 0).sum()))}


def eig_tol(F):
    """The tolerance the existing tests of the Jacobi kernel use."""
    return 1e-13 if F <= 32 else (1e-12 if F <= 128 else 1e-11)


def eigen_root_ok(chk, F):
    return bool(chk["a"] <= eig_tol(F) and chk["b"] <= eig_tol(F) and chk["c"] <= eig_tol(F) and chk["zero_cols"]
                and chk["count"])


def planted(F, p, delta, seed, per_row=2):
    """(C, L0) with C = L0 diag(D) L0^T, D = 1 except D[p] = delta.

    L0 is lower triangular with a diagonal drawn from {1, 2, 4} and, below it, integer entries in [-3, 3]: at most
    ``per_row`` non-zero ones per row, at random places.  (A dense random triangular matrix has a condition number
    that grows exponentially with F; the sparse one keeps the leading blocks well enough conditioned that the sign of
    pivot p survives the rounding of ANY backward-stable factorisation, and the positive spectrum far above any
    eigenvalue threshold - tests/test_factor_oracle_host.py checks both with LAPACK.)
    Every product is an integer times a power of two, so for delta a power of two C is exact in float64 and the
    Cholesky recursion is exact up to pivot p, which is delta * L0[p, p]^2.  For delta > 0 the factor is
    T = L0 diag(sqrt D)."""
    rng = np.random.default_rng(seed)
    L0 = np.zeros((F, F))
    for i in range(1, F):
        cols = rng.choice(i, size=min(per_row, i), replace=False)
        vals = rng.integers(1, 4, size=cols.size) * rng.choice([-1, 1], size=cols.size)
        L0[i, cols] = vals
    L0[np.diag_indices(F)] = rng.choice([1.0, 2.0, 4.0], size=F)
    D = np.ones(F)
    D[p] = delta
    C = (L0 * D) @ L0.T
    return C, L0


def planted_factor(L0, p, delta):
    """T = L0 diag(sqrt D) for delta > 0."""
    D = np.ones(L0.shape[0])
    D[p] = delta
    return L0 * np.sqrt(D)


def spectrum_matrix(F, spec, seed):
    """Q diag(spec) Q^T, symmetrised, Q from the QR of a seeded normal matrix."""
    spec = np.asarray(spec, dtype=np.float64)
    assert spec.shape == (F,)
    rng = np.random.default_rng(seed)
    Q, _ = np.linalg.qr(rng.standard_normal((F, F)))
    M = (Q * spec) @ Q.T
    return 0.5 * (M + M.T)


# ---------------------------------------------------------------- the matrix families the host and the GPU tests share
def wishart(F, seed, nl=1):
    """[nl, F, F]: A A^T + 0.1 I with A of shape F x (F + 3), standard normal."""
    rng = np.random.default_rng(seed)
    out = np.empty((nl, F, F))
    for l in range(nl):
        A = rng.standard_normal((F, F + 3))
        out[l] = A @ A.T + 0.1 * np.identity(F)
    return out


def big_offdiag(F, imax, seed):
    """C with its largest diagonal entry m at index ``imax`` and ONE off-diagonal pair larger than every diagonal
    entry, such that C + 0.25 m I is positive definite (C itself is not: an off-diagonal entry above the diagonal
    rules that out).  M = G G^T / (F + 3) + 0.1 I + 50 (e_i + e_j)(e_i + e_j)^T + 2 e_i e_i^T is positive definite
    with M_ii ~ 53 its largest diagonal entry and M_ij ~ 50; C = M - 0.2 M_ii I has m = 0.8 M_ii ~ 42.5 < C_ij and
    C + 0.25 m I = M up to rounding."""
    rng = np.random.default_rng(seed)
    G = rng.standard_normal((F, F + 3))
    M = G @ G.T / (F + 3) + 0.1 * np.identity(F)
    j = (imax + F // 2) % F
    assert j != imax
    for a, b in ((imax, imax), (j, j), (imax, j), (j, imax)):
        M[a, b] += 50.0
    M[imax, imax] += 2.0
    C = M - 0.2 * M[imax, imax] * np.identity(F)
    d = np.diagonal(C)
    assert int(np.argmax(d)) == imax and abs(C[imax, j]) > d.max()
    return C


def negative_diagonal(F, seed):
    """Every diagonal entry negative (so max(diag) and the jitter are negative) and ONE large positive eigenvalue:
    w w^T with its diagonal replaced by -a, w in +-[1, 2], a in [1, 2].  The other eigenvalues lie near -(w_i^2 + a_i)."""
    rng = np.random.default_rng(seed)
    w = rng.uniform(1.0, 2.0, F) * rng.choice([-1.0, 1.0], F)
    C = np.outer(w, w)
    C[np.diag_indices(F)] = -rng.uniform(1.0, 2.0, F)
    return C


# the spectra of the eigen-route test: (F, spectrum, eig_thresh)
def eigen_cases():
    return [
        (6, [3, 2, 1, .5, -.2, -1e-3], 1e-16),
        (5, [1, 1, 1, 2, -.5], 1e-16),
        (33, [-.5] + 16 * [1.0] + 16 * [2.0], 1e-16),
        (65, list(np.linspace(1, 2, 64)) + [-1e-6], 1e-16),
        (96, list(10.0 ** np.linspace(-6, 0, 95)) + [-1e-9], 1e-16),
        (129, [0.0] * 125 + [-1e-3, 1, 2, 3], 1e-8),
        (256, [0.0] * 252 + [-1e-3, 1, 2, 3], 1e-8),
        (2, [1, -1], 1e-16),
        (1, [-1], 1e-16),
    ]


PIVOT_F = (33, 65, 66, 130, 386, 418, 384)


def pivot_positions(F):
    return sorted({p for p in (0, 1, 31, 32, 33, F // 2, F - 2, F - 1) if 0 <= p < F})


DELTA = 2.0 ** -20


def small_margin_delta(F, p, seed):
    """-2^k with 2^k the power of two nearest to 1e-10 max |C| of the planted matrix (a power of two keeps C exact)."""
    C1, _ = planted(F, p, 1.0, seed)
    return -(2.0 ** np.round(np.log2(1e-10 * np.abs(C1).max())))
