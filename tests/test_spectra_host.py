"""Host side of the spectra estimators (no GPU): the pair order of ``hputil.anafast``, the call surface of the four
``lssutil`` estimators, and the parts of ``pk_flat`` and ``corrfunc`` that are not the device's Gram product - axes,
window, the Fourier contraction of the Gram matrix, the binning - against numpy restatements written here."""
import inspect

import numpy as np
import pytest

from cora_amd.signal import lssutil
from cora_amd.util import hputil

EPS = np.finfo(np.float64).eps


@pytest.mark.parametrize("n, want", [
    (1, [(0, 0)]),
    (2, [(0, 0), (1, 1), (0, 1)]),
    (3, [(0, 0), (1, 1), (2, 2), (0, 1), (1, 2), (0, 2)]),
    (5, [(0, 0), (1, 1), (2, 2), (3, 3), (4, 4), (0, 1), (1, 2), (2, 3), (3, 4), (0, 2), (1, 3), (2, 4), (0, 3), (1, 4),
         (0, 4)]),
])
def test_spectra_pair_order(n, want):
    i, j = hputil.spectra_pair_order(n)
    assert list(zip(i.tolist(), j.tolist())) == want
    assert i.dtype == np.int64 and j.dtype == np.int64


def _params(f):
    return [(p.name, p.default) for p in inspect.signature(f).parameters.values()]


def test_signatures():
    E = inspect.Parameter.empty
    assert _params(lssutil.pk_flat) == [("maps", E), ("chi", E), ("maps2", None), ("lmax", None), ("window", True)]
    assert _params(lssutil.corrfunc) == [("maps", E), ("chi", E), ("lmax", None), ("rmax", 1e3), ("numr", 1024)]
    assert _params(lssutil.ang_correlation) == [("x", E), ("y", E)]
    assert _params(lssutil.transfer) == [("x", E), ("y", E)]
    assert _params(hputil.anafast) == [("map1", E), ("map2", None), ("lmax", None), ("iter", 3), ("use_weights", False),
                                       ("pol", False)]
    assert _params(lssutil.pk_flat_device) == _params(lssutil.pk_flat)


def test_pk_flat_shape_mismatch():
    maps, maps2 = np.zeros((4, 48)), np.zeros((3, 48))
    with pytest.raises(ValueError) as e:
        lssutil.pk_flat(maps, np.arange(4.0) + 10, maps2=maps2)
    assert str(e.value) == "Shape of maps2 ((3, 48)) is not compatible with maps ((4, 48))"


def test_anafast_pol_not_implemented():
    with pytest.raises(NotImplementedError):
        hputil.anafast(np.zeros((3, 48)), pol=True)


def test_invert_no_zero():
    x = np.array([2.0, 0.0, -4.0, 0.0])
    assert np.array_equal(lssutil.invert_no_zero(x), np.array([0.5, 0.0, -0.25, 0.0]))


@pytest.mark.parametrize("N", [6, 5])
def test_pk_axes(N):
    """kpar = 2 pi n / (N dx), kperp = l / mean(chi), window sinc(kpar dx / 2 pi) = sin(pi n / N) / (pi n / N)."""
    lmax = 7
    chi = 1000.0 + 12.5 * np.arange(N)
    kpar, kperp, scale, Wk = lssutil._pk_axes(chi, lmax)
    n = np.arange(N // 2 + 1)
    assert kpar.shape == (N // 2 + 1,) and kperp.shape == (lmax + 1,) and Wk.shape == kpar.shape
    np.testing.assert_allclose(kpar, 2 * np.pi * n / (N * 12.5), rtol=4 * EPS, atol=0)
    np.testing.assert_allclose(kperp, np.arange(lmax + 1) / (1000.0 + 12.5 * (N - 1) / 2), rtol=4 * EPS, atol=0)
    np.testing.assert_allclose(scale, N * 12.5 * (1000.0 + 12.5 * (N - 1) / 2) ** 2, rtol=8 * EPS, atol=0)
    x = np.pi * n[1:] / N
    assert Wk[0] == 1.0
    np.testing.assert_allclose(Wk[1:], np.sin(x) / x, rtol=16 * EPS, atol=0)


@pytest.mark.parametrize("N", [6, 5, 1, 2])
def test_pk_contract_is_the_dft_of_the_gram_matrix(N):
    """The direct formula: N real fields with coefficients a_j(l, m), m >= 0 (a_j(l, 0) real), a_j(l, -m) =
    (-1)^m conj(a_j(l, m)); a^n(l, m) = sum_j w_nj a_j(l, m) for every m of both signs, w_nj = exp(-2 pi i n j / N) / N;
    out[n, l] = sum_{m=-l..l} |a^n(l, m)|^2 / (2l+1).  The contraction gets the Gram matrix the device kernel returns,
    S_l[j, k] = (a_j0 a_k0 + 2 Re sum_{m>0} a_jm conj(a_km)) / (2l+1), made symmetric and random here.
    Tolerance: N^2 terms of size |S_jk| / N^2, each with a cosine good to a few eps, against a reference with as many
    roundings again: 2 (N^2 + 2 l + 8) eps sum |S^abs| / N^2, S^abs the Gram matrix of absolute values."""
    import torch

    rng = np.random.default_rng(N)
    L = 4
    S, Sabs, direct = np.zeros((L, N, N)), np.zeros((L, N, N)), np.zeros((N // 2 + 1, L))
    w = np.exp(-2j * np.pi * np.outer(np.arange(N // 2 + 1), np.arange(N)) / N) / N
    for l in range(L):
        a0 = rng.standard_normal(N)
        am = rng.standard_normal((N, l)) + 1j * rng.standard_normal((N, l))
        S[l] = (np.outer(a0, a0) + 2 * (am @ am.conj().T).real) / (2 * l + 1)
        Sabs[l] = (np.outer(np.abs(a0), np.abs(a0)) + 2 * (np.abs(am) @ np.abs(am).T)) / (2 * l + 1)
        sign = (-1.0) ** np.arange(1, l + 1)
        full = np.concatenate([(sign * am.conj())[:, ::-1], a0[:, None], am], axis=1)      # m = -l .. l
        direct[:, l] = (np.abs(w @ full) ** 2).sum(axis=1) / (2 * l + 1)
    S = 0.5 * (S + S.transpose(0, 2, 1))                      # (numpy's product is symmetric to rounding only)
    out = lssutil._pk_contract(torch.from_numpy(S)).numpy()
    assert out.shape == (N // 2 + 1, L)
    tol = 2 * (N * N + 2 * np.arange(L) + 8) * EPS * Sabs.sum(axis=(1, 2)) / (N * N)
    assert np.all(np.abs(out - direct) <= tol[None, :]), (np.abs(out - direct) / tol[None, :]).max()


def _corrfunc_numpy(clxx, chi, lmax, rmax, numr):
    """The binning written out.  The pairs of distances come from the reference's own double loop, which appends
    (chi[j - i], chi[j]) for i in range(nx), j in range(i, nx): entry k of that list goes with spectrum k of anafast's
    diagonal order.  xi(theta) = sum_l (2l+1)/(4 pi) C_l P_l(cos theta) on 2048 angles; every (pair, angle) sample falls
    into the bin of its separation r, bins are averaged, empty bins are 0."""
    nx = len(chi)
    pairs = []
    for i in range(nx):
        for j in range(i, nx):
            pairs.append((chi[j - i], chi[j]))
    theta = np.linspace(0, np.pi, 2048)
    mu = np.cos(theta)
    P = np.polynomial.legendre.legvander(mu, lmax).T                   # [l, angle]
    xi = clxx @ (P * (2 * np.arange(lmax + 1) + 1)[:, None] / (4 * np.pi))
    edges = np.linspace(0, rmax, numr + 1)
    tot, cnt = np.zeros(numr), np.zeros(numr)
    for k, (x1, x2) in enumerate(pairs):
        r = np.sqrt((x1 - x2) ** 2 + 2 * x1 * x2 * (1 - mu))
        for t in range(2048):
            b_ = np.searchsorted(edges, r[t], side="right") - 1
            if 0 <= b_ < numr:
                tot[b_] += xi[k, t]
                cnt[b_] += 1
    return np.where(cnt > 0, tot / np.where(cnt > 0, cnt, 1), 0.0), 0.5 * (edges[1:] + edges[:-1])


def test_corrfunc_binning():
    rng = np.random.default_rng(3)
    nx, lmax, rmax, numr = 3, 12, 700.0, 16
    chi = np.array([200.0, 230.0, 275.0])
    clxx = rng.standard_normal((nx * (nx + 1) // 2, lmax + 1)) / (1 + np.arange(lmax + 1)) ** 2
    cf, r = lssutil._corrfunc_bin(clxx, chi, lmax, rmax, numr)
    ref, rref = _corrfunc_numpy(clxx, chi, lmax, rmax, numr)
    assert cf.shape == (numr,) and r.shape == (numr,)
    assert np.array_equal(r, rref)
    # sums of up to 3 * 2048 samples of size <= max |xi|, Legendre values by two different recurrences (1e-13)
    scale = np.abs(clxx).sum(axis=1).max() * (2 * lmax + 1) / (4 * np.pi)
    assert np.abs(cf - ref).max() <= 1e-12 * scale, np.abs(cf - ref).max()
    assert np.any(cf == 0.0) and np.any(cf != 0.0)             # (bins beyond the largest separation stay empty)
    # the auto spectra sit at zero lag: with only those non-zero, the first bin holds the mean of their xi(theta -> 0)
    only_auto = np.zeros_like(clxx)
    only_auto[:nx] = 1.0 / (2 * np.arange(lmax + 1) + 1)                         # xi(0) = (lmax + 1) / (4 pi) each
    cf0, _ = lssutil._corrfunc_bin(only_auto, chi, lmax, rmax, numr)
    ref0, _ = _corrfunc_numpy(only_auto, chi, lmax, rmax, numr)
    assert np.abs(cf0 - ref0).max() <= 1e-12 * (lmax + 1) and cf0[0] > 0.5 * (lmax + 1) / (4 * np.pi)
