"""The K2 oracle (tests/_factor_oracle.py) checked on the host: LAPACK's own results must lie inside every cap the GPU
tests apply to csrc/factor.hip, for every matrix family and size they use; seeded mutants of a correct factor must be
rejected; and the planted matrices must fail, or not, where they were designed to.  No GPU."""
import numpy as np
import pytest
import scipy.linalg as la

import _factor_oracle as fo

# the sizes of tests/test_gpu_factor.py, by the kernel that takes them
F_GENERIC = (1, 2, 3, 31, 32, 33, 63, 65, 97, 129, 257)
F_LL = (64, 66, 94, 96, 98, 130, 258, 382)
F_TALL = (384, 386, 414, 416, 418, 450, 514)
F_COOP = (384, 416, 512)
F_ISSUE = (1, 2, 3, 31, 33, 65, 96, 130, 257, 400, 520)     # (the sizes the caps were first measured at)
F_ALL = sorted(set(F_GENERIC + F_LL + F_TALL + F_COOP + F_ISSUE))


def _lapack_root(Cj, eig_thresh):
    e, V, ep = fo.eigen_spectrum(Cj, eig_thresh)
    return V * np.sqrt(ep)


def _assert_gap(Cj, eig_thresh):
    """No eigenvalue within two decades of the threshold: which columns are dropped does not depend on rounding."""
    e = np.linalg.eigvalsh(Cj)
    t = e.max() * eig_thresh
    near = (e > min(t / 100, t * 100)) & (e < max(t / 100, t * 100))
    assert not near.any(), (e[near], t)


# ---------------------------------------------------------------------------------------- LAPACK inside every cap
@pytest.mark.parametrize("F", F_ALL)
def test_lapack_cholesky_inside_backward_error_bound(F):
    C = fo.wishart(F, 100 + F)[0]
    for rel in ((0.0, 1e-14) if F <= 130 else (1e-14,)):
        Cj = fo.jittered(C, rel)
        T = np.linalg.cholesky(Cj)
        ratio = fo.chol_bound_ratio(Cj, T)
        print("F=%d jitter %g: LAPACK bound ratio %.3f" % (F, rel, ratio))
        assert fo.is_cholesky_factor(Cj, T, ratio), (F, rel, ratio)


@pytest.mark.parametrize("F", fo.PIVOT_F)
def test_planted_matrices_behave_as_designed(F):
    """delta = +2^-20: LAPACK's factor is the closed form exactly.  delta = -2^-20 (and the small-margin delta): scipy's
    cholesky raises, the leading p x p block factors exactly, the matrix has exactly one negative eigenvalue and its
    positive spectrum is far above the eigenvalue threshold, LAPACK's eigen-route root passes the eigen checks."""
    ps = fo.pivot_positions(F)
    for p in ps:
        C, L0 = fo.planted(F, p, fo.DELTA, 1000 + F)
        Tp = fo.planted_factor(L0, p, fo.DELTA)
        T = np.linalg.cholesky(C)
        assert np.array_equal(T, Tp), (F, p)
        if F <= 130 or p in (ps[0], ps[-1]):
            assert fo.chol_bound_ratio(C, T) == 0.0 and fo.is_cholesky_factor(C, T)
        deltas = [-fo.DELTA] + ([fo.small_margin_delta(F, p, 1000 + F)] if F in (33, 130, 418) else [])
        for delta in deltas:
            Cm, L0m = fo.planted(F, p, delta, 1000 + F)
            assert np.array_equal(L0m, L0)
            with pytest.raises(la.LinAlgError):
                la.cholesky(Cm, lower=True)
            if p > 0:
                assert np.array_equal(np.linalg.cholesky(Cm[:p, :p]), L0[:p, :p]), (F, p)
            e = np.linalg.eigvalsh(Cm)
            assert (e < 0).sum() == 1 and e[e > 0].min() > 1e-12 * e.max(), (F, p, delta)
            _assert_gap(Cm, 1e-16)
            if delta == -fo.DELTA and (F <= 130 or p == F // 2):
                chk = fo.eigen_root_checks(Cm, _lapack_root(Cm, 1e-16), 1e-16)
                assert fo.eigen_root_ok(chk, F), (F, p, chk)
        if F in (33, 130, 418):
            # the first-pivot case: C[0, 0] = 0, the rest as it is
            Cz, _ = fo.planted(F, F // 2, fo.DELTA, 1000 + F)
            Cz[0, 0] = 0.0
            assert np.abs(Cz[1:, 0]).max() > 0
            with pytest.raises(la.LinAlgError):
                la.cholesky(Cz, lower=True)
            _assert_gap(Cz, 1e-16)


@pytest.mark.parametrize("F,spec,thresh", fo.eigen_cases(), ids=lambda v: str(v) if isinstance(v, int) else "")
def test_lapack_eigen_root_inside_tolerances(F, spec, thresh):
    C = fo.spectrum_matrix(F, spec, 300 + F)
    _assert_gap(C, thresh)
    T = _lapack_root(C, thresh)
    chk = fo.eigen_root_checks(C, T, thresh)
    print("F=%d: LAPACK eigen root a %.1e b %.1e c %.1e" % (F, chk["a"], chk["b"], chk["c"]))
    assert fo.eigen_root_ok(chk, F), chk
    if F == 1:
        assert T[0, 0] == 0.0


@pytest.mark.parametrize("F,imax", [(33, 0), (33, 32), (130, 0), (130, 129), (400, 0), (400, 399), (400, 300)])
def test_jitter_family_big_offdiagonal(F, imax):
    """Positive definite only WITH the jitter of max(diag); max |C| is an off-diagonal entry."""
    C = fo.big_offdiag(F, imax, 500 + F + imax)
    assert np.abs(C).max() > np.diagonal(C).max() and int(np.argmax(np.diagonal(C))) == imax
    with pytest.raises(la.LinAlgError):
        la.cholesky(C, lower=True)
    Cj = fo.jittered(C, 0.25)
    assert Cj[imax, imax] == C[imax, imax] + 0.25 * C[imax, imax]
    T = np.linalg.cholesky(Cj)
    assert fo.is_cholesky_factor(Cj, T)
    # mutants: no jitter is not even factorable; the jitter of max |C| is rejected
    Tw = np.linalg.cholesky(fo.symmetric_from_lower(C) + 0.25 * np.abs(C).max() * np.identity(F))
    assert fo.has_cholesky_structure(Tw) and not fo.is_cholesky_factor(Cj, Tw)


@pytest.mark.parametrize("F", [33, 130, 400])
def test_jitter_family_negative_diagonal(F):
    C = fo.negative_diagonal(F, 600 + F)
    assert np.diagonal(C).max() < 0
    Cj = fo.jittered(C, 0.25)
    assert np.all(np.diagonal(Cj) < np.diagonal(C))              # a NEGATIVE jitter
    e = np.linalg.eigvalsh(Cj)
    assert (e > 0).sum() == 1
    _assert_gap(Cj, 1e-16)
    chk = fo.eigen_root_checks(Cj, _lapack_root(Cj, 1e-16), 1e-16)
    assert fo.eigen_root_ok(chk, F), chk
    # mutants: the jitter left out, or added with the other sign
    for Cw in (fo.symmetric_from_lower(C), fo.symmetric_from_lower(C) - 0.25 * np.diagonal(C).max() * np.identity(F)):
        assert not fo.eigen_root_ok(fo.eigen_root_checks(Cj, _lapack_root(Cw, 1e-16), 1e-16), F)


def test_jittered_reads_lower_triangle_only_and_rounds_once():
    C = fo.wishart(7, 3)[0]
    G = C.copy()
    G[np.triu_indices(7, 1)] = np.nan
    assert np.array_equal(fo.jittered(G, 1e-14), fo.jittered(C, 1e-14))
    Cj = fo.jittered(C, 1e-14)
    jit = np.float64(np.diagonal(C).max()) * np.float64(1e-14)
    assert np.array_equal(np.diagonal(Cj), np.diagonal(C) + jit)
    assert np.array_equal(fo.jittered(C, 0.0), C)


# ---------------------------------------------------------------------------------------- mutants are rejected
@pytest.fixture(scope="module")
def good96():
    C = fo.wishart(96, 7)[0]
    Cj = fo.jittered(C, 1e-14)
    return Cj, np.linalg.cholesky(Cj)


def test_mutant_scaled_entry(good96):
    Cj, T = good96
    base = fo.chol_bound_ratio(Cj, T)
    assert fo.is_cholesky_factor(Cj, T, base)
    for (i, j) in ((48, 48), (95, 95), (60, 20), (95, 0)):
        M = T.copy()
        M[i, j] *= 1.0 + 1e-12
        r = fo.chol_bound_ratio(Cj, M)
        print("entry (%d, %d) scaled by 1 + 1e-12: ratio %.3f -> %.1f" % (i, j, base, r))
        assert r > 1.0 and not fo.is_cholesky_factor(Cj, M), (i, j, r)


def test_mutant_dropped_product(good96):
    Cj, T = good96
    for (i, j, k) in ((70, 40, 11), (95, 95, 94), (33, 32, 0)):
        M = T.copy()
        if i == j:
            M[i, i] = np.sqrt(T[i, i] ** 2 + T[i, k] ** 2)
        else:
            M[i, j] = T[i, j] + T[i, k] * T[j, k] / T[j, j]
        assert not fo.is_cholesky_factor(Cj, M), (i, j, k)


def test_mutant_jitter_omitted():
    for F in (33, 130):
        C = fo.wishart(F, 40 + F)[0]
        Cj = fo.jittered(C, 0.25)
        assert fo.is_cholesky_factor(Cj, np.linalg.cholesky(Cj))
        assert not fo.is_cholesky_factor(Cj, np.linalg.cholesky(C))


def test_mutant_structure():
    Cj, T = fo.jittered(fo.wishart(33, 9)[0], 0.0), None
    T = np.linalg.cholesky(Cj)
    M = T.copy()
    M[0, 1] = 1e-300
    assert not fo.is_cholesky_factor(Cj, M)
    M = T.copy()
    M[3, 5] = np.nan
    assert not fo.is_cholesky_factor(Cj, M)
    M = T.copy()
    M[:, 4] *= -1.0                      # T T^T unchanged: only the sign of the diagonal tells
    assert fo.chol_bound_ratio(Cj, M) <= 1.0 and not fo.is_cholesky_factor(Cj, M)


def test_mutant_eigen_columns():
    F, spec, thresh = fo.eigen_cases()[0]
    C = fo.spectrum_matrix(F, spec, 300 + F)
    e, V, ep = fo.eigen_spectrum(C, thresh)
    T = V * np.sqrt(ep)
    assert fo.eigen_root_ok(fo.eigen_root_checks(C, T, thresh), F)
    M = T.copy()
    M[:, [3, 4]] = M[:, [4, 3]]          # two kept columns swapped: T T^T is unchanged
    chk = fo.eigen_root_checks(C, M, thresh)
    assert chk["a"] <= fo.eig_tol(F) and chk["b"] > 0.1 and not fo.eigen_root_ok(chk, F)
    M = T[:, ::-1].copy()                # descending order
    assert not fo.eigen_root_ok(fo.eigen_root_checks(C, M, thresh), F)
    M = T.copy()
    M[:, 0] = V[:, 0] * 1e-9             # a dropped eigenvalue's column left non-zero, below every tolerance
    chk = fo.eigen_root_checks(C, M, thresh)
    assert chk["a"] <= fo.eig_tol(F) and not chk["zero_cols"] and not chk["count"] and not fo.eigen_root_ok(chk, F)
    M = T.copy()
    M[:, 5] = 0.5 * (T[:, 5] + T[:, 4])  # columns not orthogonal
    assert fo.eigen_root_checks(C, M, thresh)["c"] > 0.1
