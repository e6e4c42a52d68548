"""K2 (csrc/factor.hip, corahip_factor_batched) against the host oracle of tests/_factor_oracle.py, on every kernel
behind the entry point and at the sizes where each one's tiling has an edge:

  chol_kernel            F < 64 or odd F               panel width 32, 64 x 64 update tiles, 256-strided loops
  chol_ll_kernel<false>  even 64 <= F < 384            32 x 32 MFMA tiles, a ragged last block row for F % 32 != 0
  chol_ll_kernel<true>   even F >= 384                 64-row tiles (an odd number of block rows leaves half a tile)
  chol_coop_kernel       tall, F % 32 == 0, CORAHIP_K2_COOP=2 (every matrix; otherwise the stragglers of a big batch)
  jacobi_root_kernel     every matrix whose Cholesky met a pivot !(d > 0)

Every tolerance is one of: the componentwise backward-error bound gamma_{F+8} |T| |T|^T (derived in the oracle), the
three eigen-route tolerances the existing tests of the Jacobi kernel use (1e-13 / 1e-12 / 1e-11 by F), 1e-12 max |L0| on
a factor known in closed form, or bit equality.  tests/test_factor_oracle_host.py holds LAPACK to the same caps on the
same matrices.  The tests call the C entry point with their own T and info buffers.  Run with -m gpu."""
import numpy as np
import pytest

import _factor_oracle as fo

pytestmark = pytest.mark.gpu

F_GENERIC = (1, 2, 3, 31, 32, 33, 63, 65, 97, 129, 257)
F_LL = (64, 66, 94, 96, 98, 130, 258, 382)
F_TALL = (384, 386, 414, 416, 418, 450, 514)
F_COOP = (384, 416, 512)
CHECK_ALL_UP_TO = 258        # the extended-precision residual of larger matrices: first and last of the batch only


def _path(F, coop=False):
    if coop:
        assert F >= 384 and F % 32 == 0
        return "coop"
    if F < 64 or F % 2:
        return "generic"
    return "tall" if F >= 384 else "ll"


def _factor(ctx, C, rel, thresh=1e-16, fill=0x00):
    """corahip_factor_batched on the host array C [nl, F, F] with the caller's T and info filled with byte ``fill``
    -> (T, info) on the host."""
    import torch

    nl, F, _ = C.shape
    Cd = ctx.to_device(C)
    T = ctx.empty((nl, F, F))
    info = torch.empty((nl,), dtype=torch.int32, device=ctx.device)
    T.view(torch.uint8).fill_(fill)
    info.view(torch.uint8).fill_(fill)
    rc = ctx.lib.corahip_factor_batched(ctx.h, ctx._f64(Cd), nl, F, rel, thresh, ctx._f64(T), ctx._p(info))
    torch.cuda.synchronize()
    assert rc == 0, rc
    return T.cpu().numpy(), info.cpu().numpy()


def _set_coop(ctx, monkeypatch, coop, nl, F):
    """CORAHIP_K2_COOP=2 sends every matrix of a tall batch with F % 32 == 0 through the cooperative kernel IF its grid
    of ceil(nl / 8) * 8 * G workgroups fits the device, one per CU (G = ceil(F / 128)); a grid that does not fit goes
    through the batch kernel without a word.  The entry point reports which kernel ran only through info and the
    result, so the precondition is asserted here rather than assumed."""
    if not coop:
        monkeypatch.delenv("CORAHIP_K2_COOP", raising=False)
        return
    import torch

    G = ((F + 31) // 32 + 3) // 4
    ncu = torch.cuda.get_device_properties(ctx.device).multi_processor_count
    assert F >= 384 and F % 32 == 0 and (nl + 7) // 8 * 8 * G <= ncu, (F, nl, G, ncu)
    monkeypatch.setenv("CORAHIP_K2_COOP", "2")


def _which(nl, F):
    return range(nl) if F <= CHECK_ALL_UP_TO else sorted({0, nl - 1})


def _assert_eigen_root(Cj, T, thresh, label):
    F = Cj.shape[0]
    assert np.all(np.isfinite(T)), label
    chk = fo.eigen_root_checks(Cj, T, thresh)
    print("eigen route", label, "a %.2e b %.2e c %.2e (tol %.0e)" % (chk["a"], chk["b"], chk["c"], fo.eig_tol(F)))
    assert chk["zero_cols"] and chk["count"], (label, chk)
    assert max(chk["a"], chk["b"], chk["c"]) <= fo.eig_tol(F), (label, chk)
    return chk


def _assert_cholesky(Cj, T, label):
    assert np.all(np.isfinite(T)), label
    assert fo.has_cholesky_structure(T), label
    ratio = fo.chol_bound_ratio(Cj, T)
    print("bound ratio", label, "%.4f" % ratio)
    assert fo.is_cholesky_factor(Cj, T, ratio), (label, ratio)
    return ratio


# ---------------------------------------------------------------------------------------- backward error, every path
BACKWARD = ([(F, 3, False) for F in F_GENERIC + F_LL + F_TALL] + [(F, nl, True) for F in F_COOP for nl in (1, 9)])


@pytest.mark.parametrize("F,nl,coop", BACKWARD)
def test_backward_error_on_every_path(ctx, monkeypatch, F, nl, coop):
    """C = A A^T + 0.1 I, jitter 0 and 1e-14: info = 0 and T is the Cholesky factor of the jittered matrix inside
    Higham's componentwise bound gamma_{F+8} |T| |T|^T (LAPACK: 0.01 to 0.13 of it)."""
    C = fo.wishart(F, 100 + F, nl)
    _set_coop(ctx, monkeypatch, coop, nl, F)
    worst = 0.0
    for rel in (0.0, 1e-14):
        T, info = _factor(ctx, C, rel)
        assert np.array_equal(info, np.zeros(nl, dtype=np.int32)), (F, rel, info)
        for l in range(nl):
            assert np.all(np.isfinite(T[l])) and fo.has_cholesky_structure(T[l]), (F, rel, l)
        for l in _which(nl, F):
            worst = max(worst, _assert_cholesky(fo.jittered(C[l], rel), T[l], (_path(F, coop), F, nl, rel, l)))
    print("worst bound ratio path=%s F=%d nl=%d: %.4f" % (_path(F, coop), F, nl, worst))


# ---------------------------------------------------------------------------------------- cooperative = batch, bit for bit
@pytest.mark.parametrize("nl", (1, 9))
@pytest.mark.parametrize("F", F_COOP)
def test_cooperative_equals_batch_bits(ctx, monkeypatch, F, nl):
    """chol_coop_kernel states "same arithmetic per tile" as the batch kernel: the same batch (for nl = 9 with a planted
    +2^-20 pivot in matrix 4) through chol_ll_kernel<true> (CORAHIP_K2_COOP unset; nl is far below 2 x CUs, so no
    matrix is a straggler) and through the cooperative kernel gives the same bits of T, and info = 0 in both."""
    C = fo.wishart(F, 5000 + F, nl)
    if nl == 9:
        C[4] = fo.planted(F, F // 2, +fo.DELTA, 1000 + F)[0]
    _set_coop(ctx, monkeypatch, False, nl, F)
    Tb, ib = _factor(ctx, C, 1e-14)
    _set_coop(ctx, monkeypatch, True, nl, F)
    Tc, ic = _factor(ctx, C, 1e-14)
    assert np.array_equal(ib, np.zeros(nl, dtype=np.int32)), (F, nl, ib)
    assert np.array_equal(ic, np.zeros(nl, dtype=np.int32)), (F, nl, ic)
    assert np.array_equal(Tc, Tb), (F, nl, np.abs(Tc - Tb).max())


# ---------------------------------------------------------------------------------------- jitter semantics
@pytest.mark.parametrize("F,imax", [(33, 0), (33, 32), (130, 0), (130, 129), (400, 0), (400, 399), (400, 300)])
def test_jitter_is_quarter_of_max_diagonal(ctx, monkeypatch, F, imax):
    """jitter_rel = 0.25, far above rounding: the matrices are positive definite only WITH 0.25 max(diag) on the
    diagonal, their largest |entry| is off the diagonal, their largest diagonal entry sits at the first index, the
    last, or at 300 (the second pass of the 256-strided maximum)."""
    monkeypatch.delenv("CORAHIP_K2_COOP", raising=False)
    C = np.stack([fo.big_offdiag(F, imax, 500 + F + imax + 7 * k) for k in range(3)])
    T, info = _factor(ctx, C, 0.25)
    assert np.array_equal(info, np.zeros(3, dtype=np.int32)), info
    for l in _which(3, F):
        _assert_cholesky(fo.jittered(C[l], 0.25), T[l], ("jitter", F, imax, l))


@pytest.mark.parametrize("F", [33, 130, 400])
def test_negative_diagonal_gives_negative_jitter(ctx, monkeypatch, F):
    """Every diagonal entry negative: max(diag) * 0.25 is negative (as diag.max() * 1e-14 is in the reference's
    mkfullsky), the first pivot fails, and the eigen root is that of C MINUS |jitter| (one positive eigenvalue, which
    the jitter shifts by far more than the tolerance)."""
    monkeypatch.delenv("CORAHIP_K2_COOP", raising=False)
    C = np.stack([fo.negative_diagonal(F, 600 + F + 7 * k) for k in range(3)])
    T, info = _factor(ctx, C, 0.25)
    assert np.array_equal(info, np.ones(3, dtype=np.int32)), info
    for l in _which(3, F):
        _assert_eigen_root(fo.jittered(C[l], 0.25), T[l], 1e-16, ("negative diagonal", F, l))


# ---------------------------------------------------------------------------------------- where a pivot fails
_ALONE = {}


def _good_pair(ctx, F):
    """Two good matrices of size F and their factors, each factored alone (once per size and path)."""
    if F not in _ALONE:
        g = fo.wishart(F, 2000 + F, 2)
        _ALONE[F] = (g, [_factor(ctx, g[k:k + 1], 0.0)[0][0] for k in range(2)])
    return _ALONE[F]


PIVOT_CASES = [(F, p) for F in fo.PIVOT_F for p in fo.pivot_positions(F)]


@pytest.mark.parametrize("F,p", PIVOT_CASES)
def test_pivot_failure_location(ctx, monkeypatch, F, p):
    """[good, planted(-2^-20 at pivot p), planted(+2^-20 at pivot p), good], jitter 0; F = 384 through the cooperative
    kernel.  The planted matrices are exact in float64 and the recursion is exact up to pivot p, whose value is
    -+2^-20 L0[p, p]^2: at a 32-column block edge, inside the partial last block, at the first and the last row."""
    coop = F == 384
    _set_coop(ctx, monkeypatch, coop, 4, F)
    good, alone = _good_pair(ctx, F)
    Cm, L0 = fo.planted(F, p, -fo.DELTA, 1000 + F)
    Cp, L0p = fo.planted(F, p, fo.DELTA, 1000 + F)
    assert np.array_equal(L0, L0p)
    T, info = _factor(ctx, np.stack([good[0], Cm, Cp, good[1]]), 0.0)
    assert np.array_equal(info, np.array([0, 1, 0, 0], dtype=np.int32)), (F, p, info)
    assert np.array_equal(T[0], alone[0]) and np.array_equal(T[3], alone[1]), (F, p)
    _assert_cholesky(Cp, T[2], ("planted +", F, p))
    err = np.abs(T[2] - fo.planted_factor(L0, p, fo.DELTA)).max()
    assert err <= 1e-12 * np.abs(L0).max(), (F, p, err)
    _assert_eigen_root(Cm, T[1], 1e-16, ("planted -", F, p))


@pytest.mark.parametrize("F", [33, 130, 418])
def test_pivot_failure_by_small_margin_and_first_pivot(ctx, monkeypatch, F):
    """A pivot of -1e-10 max |C| (rounded to a power of two: the matrix stays exact) is far above rounding and must be
    flagged, in the middle and at the last row; C[0, 0] = 0 with a non-zero first column fails at the first pivot."""
    monkeypatch.delenv("CORAHIP_K2_COOP", raising=False)
    good = fo.wishart(F, 2000 + F, 2)
    fails = []
    for p in (F // 2, F - 1):
        delta = fo.small_margin_delta(F, p, 1000 + F)
        assert -4e-10 < delta / np.abs(fo.planted(F, p, 1.0, 1000 + F)[0]).max() < -2.5e-11
        fails.append(fo.planted(F, p, delta, 1000 + F)[0])
    Cz = fo.planted(F, F // 2, fo.DELTA, 1000 + F)[0]
    Cz[0, 0] = 0.0
    fails.append(Cz)
    T, info = _factor(ctx, np.stack([good[0]] + fails + [good[1]]), 0.0)
    assert np.array_equal(info, np.array([0, 1, 1, 1, 0], dtype=np.int32)), (F, info)
    for k, Cf in enumerate(fails):
        _assert_eigen_root(Cf, T[1 + k], 1e-16, ("small margin / first pivot", F, k))
    for k in (0, 4):
        assert np.all(np.isfinite(T[k])) and fo.has_cholesky_structure(T[k])


# ---------------------------------------------------------------------------------------- eigen route structure
@pytest.mark.parametrize("F,spec,thresh", fo.eigen_cases(), ids=lambda v: str(v) if isinstance(v, int) else "")
def test_eigen_route_structure(ctx, monkeypatch, F, spec, thresh):
    """T = V sqrt(e+) with the columns by ASCENDING eigenvalue (the order decides which normal multiplies which mode):
    product, column norms in order, orthogonality, and the dropped columns exactly zero.  Odd F (the round-robin's
    dummy player), F = 1 and 2, repeated eigenvalues, many nulls at F = 129 and 256."""
    monkeypatch.delenv("CORAHIP_K2_COOP", raising=False)
    C = np.stack([fo.spectrum_matrix(F, spec, 300 + F), fo.wishart(F, 2000 + F)[0], fo.spectrum_matrix(F, spec, 301 + F)])
    T, info = _factor(ctx, C, 0.0, thresh)
    assert np.array_equal(info, np.array([1, 0, 1], dtype=np.int32)), (F, info)
    for l in (0, 2):
        _assert_eigen_root(C[l], T[l], thresh, ("spectrum", F, l))
    if F == 1:
        assert T[0, 0, 0] == 0.0 and T[2, 0, 0] == 0.0
    assert fo.has_cholesky_structure(T[1])


# ---------------------------------------------------------------------------------------- read / write contract
CONTRACT = [(F, False) for F in (33, 66, 94, 130, 386, 418, 450)] + [(416, True)]


_CONTRACT = {}


def _contract_batch(ctx, F):
    """[good, planted -, good] and its result on zero-filled outputs (one run per size, shared by the two tests below;
    the eigen route costs seconds per matrix from F ~ 400 on)."""
    if F not in _CONTRACT:
        p = min(33, F - 1)
        good = fo.wishart(F, 2000 + F, 2)
        C = np.stack([good[0], fo.planted(F, p, -fo.DELTA, 1000 + F)[0], good[1]])
        T0, i0 = _factor(ctx, C, 1e-14, fill=0x00)
        assert np.array_equal(i0, np.array([0, 1, 0], dtype=np.int32)), i0
        assert np.all(np.isfinite(T0))
        _CONTRACT[F] = (C, T0, i0)
    return _CONTRACT[F]


@pytest.mark.parametrize("F,coop", CONTRACT)
def test_output_is_written_completely(ctx, monkeypatch, F, coop):
    """T and info zero-filled, then filled with NaN (bytes 0xFF) and with ~2^1000 (0x7E): K2 writes every element of T
    and info - the result is finite and bit-identical.  (chol_ll_kernel and chol_coop_kernel load "a row past the
    end" of a ragged F from row 0 of T and multiply it by 0.0.)"""
    _set_coop(ctx, monkeypatch, coop, 3, F)
    C, T0, i0 = _contract_batch(ctx, F)
    for byte in (0xFF, 0x7E):
        T1, i1 = _factor(ctx, C, 1e-14, fill=byte)
        assert np.array_equal(i1, i0), (F, hex(byte), i1)
        assert np.all(np.isfinite(T1)), (F, hex(byte))
        assert np.array_equal(T1, T0), (F, hex(byte), np.abs(T1 - T0).max())


@pytest.mark.parametrize("F,coop", CONTRACT)
def test_input_upper_triangle_is_never_read(ctx, monkeypatch, F, coop):
    """scipy's cholesky(lower=True) and eigh read the lower triangle only; so must K2, on the Cholesky and on the
    eigen route: the strict upper triangle of every C set to NaN, then to 2^1000, changes no bit of T or info."""
    _set_coop(ctx, monkeypatch, coop, 3, F)
    C, T0, i0 = _contract_batch(ctx, F)
    iu = np.triu_indices(F, 1)
    for junk in (np.nan, 2.0 ** 1000):
        G = C.copy()
        G[:, iu[0], iu[1]] = junk
        T1, i1 = _factor(ctx, G, 1e-14)
        assert np.array_equal(i1, i0), (F, junk, i1)
        assert np.array_equal(T1, T0), (F, junk)


# ---------------------------------------------------------------------------------------- scale covariance
def _scale_batch(F, route):
    if route == "cholesky":
        return fo.wishart(F, 3000 + F, 3), 1e-16
    _, spec, thresh = [c for c in fo.eigen_cases() if c[0] == F][0]
    return np.stack([fo.spectrum_matrix(F, spec, 300 + F), fo.wishart(F, 3000 + F)[0],
                     fo.spectrum_matrix(F, spec, 301 + F)]), thresh


@pytest.mark.parametrize("F,route", [(33, "cholesky"), (130, "cholesky"), (418, "cholesky"), (33, "eigen"), (96, "eigen")])
def test_scale_covariance(ctx, monkeypatch, F, route):
    """T(4^s C) = 2^s T(C) bit for bit, s = +-100, info equal: every operation of these kernels commutes with an even
    power of two (the jitter and the eigenvalue threshold are relative, 1 / sqrt(4^s d) = 2^-s / sqrt(d) in the
    hardware's reciprocal square root and in its Newton steps, Jacobi's angles are ratios and its stopping rule is
    relative), and nothing comes near the ends of the exponent range."""
    monkeypatch.delenv("CORAHIP_K2_COOP", raising=False)
    C, thresh = _scale_batch(F, route)
    T0, i0 = _factor(ctx, C, 1e-14, thresh)
    assert np.array_equal(i0, np.array([0, 0, 0] if route == "cholesky" else [1, 0, 1], dtype=np.int32)), i0
    assert np.all(np.isfinite(T0)) and np.abs(T0).max() > 0
    for s in (100, -100):
        T1, i1 = _factor(ctx, C * 4.0 ** s, 1e-14, thresh)
        assert np.array_equal(i1, i0), (F, s, i1)
        assert np.array_equal(T1, T0 * 2.0 ** s), (F, route, s, np.abs(T1 * 2.0 ** -s - T0).max())


# ---------------------------------------------------------------------------------------- batch independence
@pytest.mark.parametrize("F", [33, 130, 418])
def test_batch_independence(ctx, monkeypatch, F):
    """Nine matrices, the fifth one failing: every matrix gets the bits it gets when factored alone, info holds only
    0 and 1."""
    monkeypatch.delenv("CORAHIP_K2_COOP", raising=False)
    C = fo.wishart(F, 4000 + F, 9)
    C[4] = fo.planted(F, F // 2, -fo.DELTA, 1000 + F)[0]
    T, info = _factor(ctx, C, 1e-14)
    assert np.array_equal(info, np.array([0, 0, 0, 0, 1, 0, 0, 0, 0], dtype=np.int32)), info
    for l in range(9):
        Tl, il = _factor(ctx, C[l:l + 1], 1e-14)
        assert il[0] == info[l] and np.array_equal(Tl[0], T[l]), (F, l)
