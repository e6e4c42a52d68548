"""Spectra of a_lm on the device (csrc/spectra.hip through Context.alm_cross_spectra, hputil.cross_spectra_device /
anafast, skysim.clarray_from_maps and the estimators of cora_amd.signal.lssutil) against numpy on the same a_lm.

Tolerances are derived, not tuned:
  kernel      (2 (l+1) + 3) eps S^abs_l[i, j], S^abs = sum_m c_m (|Re a_i| |Re b_j| + |Im a_i| |Im b_j|) / (2l+1): the bound
              of an inner product of 2 (l+1) terms in any summation order, with FMA or without, plus the division.
  pk_flat     (N + 2 (l+1) + 4) eps / N^2 sum_jk S^abs_l[j, k] against the Fourier combination of the device's own a_lm.
  pk_flat against the literal route (transform along the shells first): measured on the CPU, stated at the test.
Every test prints its worst error over tolerance.  Run with -m gpu."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = np.finfo(np.float64).eps
CORAHIP_EINVAL = -1


def _lm(lmax):
    """(l, m) of every packed index m (2 lmax + 1 - m) / 2 + l (m-major)."""
    m = np.concatenate([np.full(lmax + 1 - mm, mm) for mm in range(lmax + 1)])
    l = np.concatenate([np.arange(mm, lmax + 1) for mm in range(lmax + 1)])
    return l, m


def _gram(a, b, lmax):
    """numpy Gram matrices of packed complex a [nx, nalm], b [ny, nalm]: (S, S^abs), [lmax+1, nx, ny] each."""
    l, m = _lm(lmax)
    S = np.zeros((lmax + 1, a.shape[0], b.shape[0]))
    Sabs = np.zeros_like(S)
    for ll in range(lmax + 1):
        idx = np.nonzero(l == ll)[0]
        c = np.where(m[idx] == 0, 1.0, 2.0) / (2 * ll + 1)
        x, y = a[:, idx], b[:, idx]
        S[ll] = (x.real * c) @ y.real.T + (x.imag * c) @ y.imag.T
        Sabs[ll] = (np.abs(x.real) * c) @ np.abs(y.real).T + (np.abs(x.imag) * c) @ np.abs(y.imag).T
    return S, Sabs


def _tol(Sabs):
    l = np.arange(Sabs.shape[0])[:, None, None]
    return (2 * (l + 1) + 3) * EPS * Sabs


def _ratio(err, tol):
    """worst err / tol; a non-zero error where the tolerance is zero counts as inf"""
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(tol > 0, err / np.where(tol > 0, tol, 1.0), np.where(err > 0, np.inf, 0.0))
    return float(np.max(r)) if r.size else 0.0


def _alm(n, lmax, seed):
    """random packed a_lm [n, nalm] (Im a_l0 left non-zero: it enters as stored), one channel 1e6 times larger, one zero"""
    rng = np.random.default_rng(seed)
    nalm = (lmax + 1) * (lmax + 2) // 2
    a = rng.standard_normal((n, nalm)) + 1j * rng.standard_normal((n, nalm))
    a[n // 2] *= 1e6
    if n > 1:
        a[0] = 0.0
    return a


def _to_dev(ctx, a, lmax):
    import torch

    return ctx.alm_packed_to_dev(torch.from_numpy(np.ascontiguousarray(a)).to(ctx.device), lmax)


def _hand_built(a, pad_value):
    """alm_dev [nalm, G, 2, 4] written out on the host: channel 4 g + v at [idx, g, c, v], c = (Re, Im); padding
    channels hold ``pad_value``."""
    n, nalm = a.shape
    G = (n + 3) // 4
    full = np.full((4 * G, nalm), pad_value + 1j * pad_value, dtype=np.complex128)
    full[:n] = a
    dev = np.empty((nalm, G, 2, 4))
    dev[:, :, 0, :] = full.real.T.reshape(nalm, G, 4)
    dev[:, :, 1, :] = full.imag.T.reshape(nalm, G, 4)
    return dev


LMAXES = (0, 1, 5, 33, 64)


@pytest.mark.parametrize("lmax", LMAXES)
@pytest.mark.parametrize("nx", (1, 3, 4, 5, 17, 129))
def test_symmetric_against_numpy(ctx, nx, lmax):
    import torch

    a = _alm(nx, lmax, 1000 * nx + lmax)
    dev = _to_dev(ctx, a, lmax)
    keep = dev.clone()
    out = ctx.alm_cross_spectra(dev, nx, lmax, out=torch.full((lmax + 1, nx, nx), float("nan"), dtype=torch.float64,
                                                              device=ctx.device))
    got = out.cpu().numpy()
    assert got.shape == (lmax + 1, nx, nx) and np.isfinite(got).all()          # every element of a NaN `out` is written
    S, Sabs = _gram(a, a, lmax)
    r = _ratio(np.abs(got - S), _tol(Sabs))
    print("symmetric nx %d lmax %d: worst err / tol %.3f" % (nx, lmax, r))
    assert r <= 1.0
    assert np.array_equal(got, got.transpose(0, 2, 1))                          # bitwise symmetric
    assert torch.equal(ctx.alm_cross_spectra(dev, nx, lmax), out)               # identical bits from call to call
    assert torch.equal(dev, keep)                                               # the input is not touched
    # the two-operand form with a copy of a as b: the same numbers within the bound (and b = a itself: the same bits)
    two = ctx.alm_cross_spectra(dev, nx, lmax, alm_b=keep, ny=nx).cpu().numpy()
    assert _ratio(np.abs(two - S), _tol(Sabs)) <= 1.0 and _ratio(np.abs(two - got), _tol(Sabs)) <= 1.0
    assert torch.equal(ctx.alm_cross_spectra(dev, nx, lmax, alm_b=dev, ny=nx), out)


@pytest.mark.parametrize("lmax", LMAXES)
@pytest.mark.parametrize("nx, ny", ((130, 3), (5, 129), (8, 8)))
def test_two_operands_against_numpy(ctx, nx, ny, lmax):
    import torch

    a, b = _alm(nx, lmax, 7 * nx + lmax), _alm(ny, lmax, 11 * ny + lmax + 1)
    da, db = _to_dev(ctx, a, lmax), _to_dev(ctx, b, lmax)
    ka, kb = da.clone(), db.clone()
    out = ctx.alm_cross_spectra(da, nx, lmax, alm_b=db, ny=ny,
                                out=torch.full((lmax + 1, nx, ny), float("nan"), dtype=torch.float64, device=ctx.device))
    got = out.cpu().numpy()
    assert got.shape == (lmax + 1, nx, ny) and np.isfinite(got).all()
    S, Sabs = _gram(a, b, lmax)
    r = _ratio(np.abs(got - S), _tol(Sabs))
    print("two operands (%d, %d) lmax %d: worst err / tol %.3f" % (nx, ny, lmax, r))
    assert r <= 1.0
    assert torch.equal(ctx.alm_cross_spectra(da, nx, lmax, alm_b=db, ny=ny), out)
    assert torch.equal(da, ka) and torch.equal(db, kb)
    # the transposed call gives the transposed numbers, bit for bit (commuted products in the same order)
    assert torch.equal(ctx.alm_cross_spectra(db, ny, lmax, alm_b=da, ny=nx), out.transpose(1, 2).contiguous())


@pytest.mark.parametrize("nx, ny", ((5, None), (17, None), (130, 3), (6, 129)))
def test_padding_channels_never_reach_out(ctx, nx, ny):
    """A layout test on a hand-built alm_dev: the channels between n and 4 ceil(n / 4) hold NaN on the host before the
    upload; the result is finite and has the bits of the result with zero padding (and of alm_packed_to_dev's)."""
    import torch

    lmax = 9
    a = _alm(nx, lmax, 5 * nx)
    b = None if ny is None else _alm(ny, lmax, 5 * ny + 1)

    def run(pad):
        da = torch.from_numpy(_hand_built(a, pad)).to(ctx.device)
        if b is None:
            return ctx.alm_cross_spectra(da, nx, lmax)
        return ctx.alm_cross_spectra(da, nx, lmax, alm_b=torch.from_numpy(_hand_built(b, pad)).to(ctx.device), ny=ny)

    clean, dirty = run(0.0), run(float("nan"))
    assert torch.isfinite(dirty).all() and torch.equal(clean, dirty)
    assert torch.equal(torch.from_numpy(_hand_built(a, 0.0)).to(ctx.device), _to_dev(ctx, a, lmax))
    S, Sabs = _gram(a, a if b is None else b, lmax)
    assert _ratio(np.abs(dirty.cpu().numpy() - S), _tol(Sabs)) <= 1.0


def test_invalid_arguments(ctx):
    import ctypes

    lmax, n = 4, 5
    dev = _to_dev(ctx, _alm(n, lmax, 1), lmax)
    out = ctx.empty((lmax + 1, n, n))
    f = ctx.lib.corahip_alm_cross_spectra
    p, o = ctypes.c_void_p(dev.data_ptr()), ctypes.c_void_p(out.data_ptr())
    assert f(ctx.h, p, n, None, n, lmax, o) == 0
    assert f(ctx.h, p, 0, None, 0, lmax, o) == CORAHIP_EINVAL
    assert f(ctx.h, p, n, p, 0, lmax, o) == CORAHIP_EINVAL
    assert f(ctx.h, p, n, None, n, -1, o) == CORAHIP_EINVAL
    assert f(ctx.h, None, n, None, n, lmax, o) == CORAHIP_EINVAL
    assert f(ctx.h, p, n, None, n, lmax, None) == CORAHIP_EINVAL
    assert f(ctx.h, p, n, None, n - 1, lmax, o) == CORAHIP_EINVAL              # the symmetric case is square
    assert f(ctx.h, p, n, p, n - 1, lmax, o) == CORAHIP_EINVAL
    assert f(ctx.h, p, n, None, n, lmax, p) == CORAHIP_EINVAL                  # out over the operand
    with pytest.raises(ValueError):
        ctx.alm_cross_spectra(dev, n + 4, lmax)
    with pytest.raises(ValueError):
        ctx.alm_cross_spectra(dev, n, lmax, out=ctx.empty((lmax + 1, n, n + 1)))


# ---- the API on maps --------------------------------------------------------------------------------------------
def _square_to_packed(sq, lmax):
    l, m = _lm(lmax)
    return np.ascontiguousarray(sq[:, l, m])


def _device_alm(ctx, maps, nside, lmax, use_weights=None, niter=None):
    """host copy (packed, [n, nalm]) of hputil.map2alm_device's own a_lm"""
    import torch

    from cora_amd.util import hputil

    alm = hputil.map2alm_device(torch.from_numpy(maps).to(ctx.device), nside, lmax, use_weights=use_weights, niter=niter)
    return _square_to_packed(ctx.alm_dev_to_square(alm, lmax, maps.shape[0]).cpu().numpy()[:, 0], lmax)


@pytest.fixture(scope="module")
def maps5():
    return np.random.default_rng(5).standard_normal((5, 12 * 16 * 16))


def test_api_on_maps(ctx, maps5):
    import torch

    from cora_amd.core import skysim
    from cora_amd.util import hputil

    nside, lmax, n = 16, 32, 5
    dmaps = torch.from_numpy(maps5).to(ctx.device)
    # hputil's defaults (use_weights=True, 2 refinements): cross_spectra_device and clarray_from_maps
    a = _device_alm(ctx, maps5, nside, lmax)
    S, Sabs = _gram(a, a, lmax)
    cs = hputil.cross_spectra_device(dmaps, lmax=lmax)
    assert cs.shape == (lmax + 1, n, n) and cs.device == dmaps.device
    r1 = _ratio(np.abs(cs.cpu().numpy() - S), _tol(Sabs))
    ch = skysim.clarray_from_maps(maps5, lmax=lmax)
    cd = skysim.clarray_from_maps(dmaps, lmax=lmax)
    assert isinstance(ch, np.ndarray) and isinstance(cd, torch.Tensor) and ch.shape == (lmax + 1, n, n)
    r2 = max(_ratio(np.abs(ch - S), _tol(Sabs)), _ratio(np.abs(cd.cpu().numpy() - S), _tol(Sabs)))
    # two stacks
    b = _device_alm(ctx, maps5[:3] * 2.0, nside, lmax)
    Sx, Sxabs = _gram(a, b, lmax)
    cx = hputil.cross_spectra_device(dmaps, dmaps[:3] * 2.0, lmax=lmax)
    assert cx.shape == (lmax + 1, n, 3)
    r3 = _ratio(np.abs(cx.cpu().numpy() - Sx), _tol(Sxabs))
    # healpy's defaults (no weights, 3 refinements): anafast, in the diagonal order
    a3 = _device_alm(ctx, maps5, nside, lmax, use_weights=False, niter=3)
    S3, S3abs = _gram(a3, a3, lmax)
    i, j = hputil.spectra_pair_order(n)
    cl = hputil.anafast(maps5, lmax=lmax)
    assert cl.shape == (n * (n + 1) // 2, lmax + 1)
    r4 = _ratio(np.abs(cl - S3[:, i, j].T), _tol(S3abs)[:, i, j].T)
    one = hputil.anafast(maps5[1], lmax=lmax)
    assert one.shape == (lmax + 1,)
    r5 = _ratio(np.abs(one - S3[:, 1, 1]), _tol(S3abs)[:, 1, 1])
    cross = hputil.anafast(maps5[1], maps5[3], lmax=lmax)
    assert cross.shape == (lmax + 1,)
    r6 = _ratio(np.abs(cross - S3[:, 1, 3]), _tol(S3abs)[:, 1, 3])
    assert hputil.anafast(maps5[:2]).shape == (3, 3 * nside)                     # default lmax = 3 nside - 1
    print("maps: cross_spectra_device %.3f, clarray_from_maps %.3f, two stacks %.3f, anafast %.3f / %.3f / %.3f"
          % (r1, r2, r3, r4, r5, r6))
    assert max(r1, r2, r3, r4, r5, r6) <= 1.0


def test_anafast_pair_against_sph_ps(ctx, maps5):
    """hputil.sph_ps (host product of two square a_lm arrays) and anafast with sph_ps's analysis settings"""
    from cora_amd.util import hputil

    nside, lmax = 16, 32
    ref = hputil.sph_ps(maps5[0], maps5[1], lmax=lmax)
    got = hputil.anafast(maps5[0], maps5[1], lmax=lmax, iter=hputil._iter, use_weights=hputil._weight)
    a = _device_alm(ctx, maps5[:2], nside, lmax)
    _, Sabs = _gram(a, a, lmax)
    r = _ratio(np.abs(got - np.real(ref)), _tol(Sabs)[:, 0, 1])
    print("anafast against sph_ps: worst err / tol %.3f" % r)
    assert r <= 1.0


# ---- pk_flat ------------------------------------------------------------------------------------------------------
def _full_m(a, lmax):
    """packed a [n, nalm] of real fields -> list over l of [n, 2l+1] coefficients for m = -l .. l"""
    l, m = _lm(lmax)
    out = []
    for ll in range(lmax + 1):
        idx = np.nonzero(l == ll)[0]                       # m = 0 .. ll
        x = a[:, idx]
        neg = ((-1.0) ** np.arange(1, ll + 1)) * x[:, 1:].conj()
        out.append(np.concatenate([neg[:, ::-1], x], axis=1))
    return out


def _cln_from_alm(a, b, lmax):
    """cln[n, l] = sum_{all m} a^n conj(b^n) / (2l+1), a^n = (1/N) sum_j exp(-2 pi i n j / N) a^j"""
    N = a.shape[0]
    w = np.exp(-2j * np.pi * np.outer(np.arange(N // 2 + 1), np.arange(N)) / N) / N
    fa, fb = _full_m(a, lmax), _full_m(b, lmax)
    return np.stack([((w @ fa[l]) * (w @ fb[l]).conj()).sum(axis=1).real / (2 * l + 1) for l in range(lmax + 1)], axis=1)


@pytest.mark.parametrize("cross", (False, True))
@pytest.mark.parametrize("N", (6, 5))
def test_pk_flat_against_combination_of_device_alm(ctx, N, cross):
    from cora_amd.signal import lssutil

    nside, lmax = 8, 16
    rng = np.random.default_rng(40 + N)
    maps = rng.standard_normal((N, 12 * nside * nside))
    maps2 = rng.standard_normal((N, 12 * nside * nside)) + 0.5 * maps if cross else None
    chi = 1500.0 + 7.0 * np.arange(N)
    pk, kpar, kperp = lssutil.pk_flat(maps, chi, maps2=maps2, lmax=lmax, window=False)
    pkw, _, _ = lssutil.pk_flat(maps, chi, maps2=maps2, lmax=lmax)
    assert pk.shape == (N // 2 + 1, lmax + 1) and kpar.shape == (N // 2 + 1,) and kperp.shape == (lmax + 1,)
    kp, kt, scale, Wk = lssutil._pk_axes(chi, lmax)
    assert np.array_equal(kpar, kp) and np.array_equal(kperp, kt)
    a = _device_alm(ctx, maps, nside, lmax)
    b = _device_alm(ctx, maps2, nside, lmax) if cross else a
    # the m = 0 coefficients of a real analysis are real up to the rounding of the ring FFT; the combination below
    # takes them as stored, like the kernel
    ref = _cln_from_alm(a, b, lmax)
    _, Sabs = _gram(a, b, lmax)
    l = np.arange(lmax + 1)
    tol = (N + 2 * (l + 1) + 4) * EPS / N**2 * Sabs.sum(axis=(1, 2))
    r = _ratio(np.abs(pk / scale - ref), np.broadcast_to(tol[None, :], ref.shape))
    rw = _ratio(np.abs(pkw * (Wk**2)[:, None] / scale - ref), np.broadcast_to(tol[None, :], ref.shape))
    print("pk_flat N %d %s: worst err / tol %.3f (with window %.3f)" % (N, "cross" if cross else "auto", r, rw))
    assert r <= 1.0 and rw <= 1.0


def _pk_inputs():
    nside, lmax, N = 8, 16, 6
    rng = np.random.default_rng(77)
    maps = rng.standard_normal((N, 12 * nside * nside))
    maps2 = rng.standard_normal((N, 12 * nside * nside)) + 0.5 * maps
    return nside, lmax, N, maps, maps2


def _oracle_alm(maps, nside, lmax):
    from oracle import sht

    return np.stack([sht.map2alm(m, nside, lmax, use_weights=True, niter=2) for m in maps])


def _literal_cln(maps, maps2, nside, lmax):
    """The reference's route with the oracle SHT: rfft along the shells, analysis of the real and imaginary part of
    every Fourier map, a = a(Re) + i a(Im) for both signs of m, |.|^2 summed over m."""
    N = maps.shape[0]

    def full(x):
        cn = np.fft.rfft(x, axis=0) / N
        re, im = _full_m(_oracle_alm(cn.real, nside, lmax), lmax), _full_m(_oracle_alm(cn.imag, nside, lmax), lmax)
        return [r + 1j * i for r, i in zip(re, im)]

    fa = full(maps)
    fb = fa if maps2 is None else full(maps2)
    return np.stack([(fa[l] * fb[l].conj()).sum(axis=1).real / (2 * l + 1) for l in range(lmax + 1)], axis=1)


def _commuted_cln(maps, maps2, nside, lmax):
    """The commuted route with the oracle SHT: analysis of the slices, Gram matrix, cosine sum (numpy)."""
    N = maps.shape[0]
    a = _oracle_alm(maps, nside, lmax)
    b = a if maps2 is None else _oracle_alm(maps2, nside, lmax)
    S, _ = _gram(a, b, lmax)
    d = np.arange(N)[:, None] - np.arange(N)[None, :]
    W = np.cos(2 * np.pi * ((np.arange(N // 2 + 1)[:, None, None] * d[None]) % N) / N) / N**2
    Sd, _ = _gram(a, a, lmax)
    Sd2 = Sd if maps2 is None else _gram(b, b, lmax)[0]
    dg = np.sqrt(np.einsum("lii->li", Sd))[:, :, None] * np.sqrt(np.einsum("lii->li", Sd2))[:, None, :]
    return np.einsum("njk,ljk->nl", W, S), dg.sum(axis=(1, 2)) / N**2


# measured on the CPU (both routes with oracle.sht, neither is the code under test), inputs of _pk_inputs():
#   largest |literal - commuted| / (sum_jk sqrt(S_jj S_kk) / N^2): auto 1.77e-16, cross 3.08e-16; allowed: 100 x the larger
PK_ROUTE_DIFF = 3.08e-16


@pytest.mark.parametrize("cross", (False, True))
def test_pk_flat_against_literal_route(ctx, cross):
    """pk_flat (slices analysed on the device, Fourier sum on their Gram matrix) against the literal route of the
    reference (np.fft.rfft along the shells first, then oracle.sht.map2alm of the real and imaginary parts, |.|^2).
    Tolerance: the two routes differ on the CPU, both with oracle.sht, by at most PK_ROUTE_DIFF = 3.08e-16 relative to
    sum_jk sqrt(S_jj S_kk) / N^2 (the rounding of two analyses that are linear only to rounding); 100 x that is
    allowed (3.08e-14) - the factor is for the device SHT's own 1e-11 / 1e-12 gates against the oracle, stacked twice."""
    from cora_amd.signal import lssutil

    nside, lmax, N, maps, maps2 = _pk_inputs()
    m2 = maps2 if cross else None
    lit = _literal_cln(maps, m2, nside, lmax)
    _, norm = _commuted_cln(maps, m2, nside, lmax)
    chi = 900.0 + 5.0 * np.arange(N)
    pk, _, _ = lssutil.pk_flat(maps, chi, maps2=m2, lmax=lmax, window=False)
    scale = lssutil._pk_axes(chi, lmax)[2]
    tol = 100 * PK_ROUTE_DIFF * norm
    r = _ratio(np.abs(pk / scale - lit), np.broadcast_to(tol[None, :], lit.shape))
    print("pk_flat against the literal route (%s): worst err / tol %.3g, worst err / norm %.3g"
          % ("cross" if cross else "auto", r, (np.abs(pk / scale - lit) / norm[None, :]).max()))
    assert r <= 1.0


# ---- the other estimators -------------------------------------------------------------------------------------
def test_corrfunc_ang_correlation_transfer(ctx):
    """numpy restatements fed with anafast's own output.  The spectra of two calls agree to the rounding of the analysis
    (its sums are not ordered the same way for every batch shape), far inside the SHT's 1e-11 gate; the estimators are
    smooth in them, so 1e-10 of the largest value is allowed."""
    from cora_amd.signal import lssutil
    from cora_amd.util import hputil

    nside, lmax, n = 8, 16, 3
    rng = np.random.default_rng(9)
    maps = rng.standard_normal((n, 12 * nside * nside))
    maps[1] += 0.7 * maps[0]
    chi = np.array([300.0, 340.0, 395.0])
    rmax, numr = 800.0, 32
    cf, r = lssutil.corrfunc(maps, chi, lmax=lmax, rmax=rmax, numr=numr)
    assert cf.shape == (numr,) and r.shape == (numr,)
    edges = np.linspace(0, rmax, numr + 1)
    assert np.array_equal(r, 0.5 * (edges[1:] + edges[:-1]))
    cl = hputil.anafast(maps, lmax=lmax)
    i, j = hputil.spectra_pair_order(n)
    mu = np.cos(np.linspace(0, np.pi, 2048))
    P = np.polynomial.legendre.legvander(mu, lmax).T * (2 * np.arange(lmax + 1) + 1)[:, None] / (4 * np.pi)
    xi = cl @ P
    xxp = []
    for a in range(n):                          # the reference's own double loop: entry k goes with spectrum k
        for b in range(a, n):
            xxp.append((chi[b - a], chi[b]))
    r1, r2 = (v[:, None] for v in np.array(xxp).T)
    assert np.array_equal(r1[:, 0], chi[i]) and np.array_equal(r2[:, 0], chi[j])
    sep = np.sqrt((r1 - r2) ** 2 + 2 * r1 * r2 * (1 - mu[None, :]))
    which = np.searchsorted(edges, sep.ravel(), side="right") - 1
    ok = (which >= 0) & (which < numr)
    tot = np.bincount(which[ok], weights=xi.ravel()[ok], minlength=numr)
    cnt = np.bincount(which[ok], minlength=numr)
    ref = np.where(cnt > 0, tot / np.maximum(cnt, 1), 0.0)
    e1 = np.abs(cf - ref).max() / np.abs(ref).max()
    assert np.array_equal(cf == 0.0, cnt == 0)

    x, y = maps[1], maps[0]
    c2 = hputil.anafast(np.stack([x, y]))
    rl, tl = lssutil.ang_correlation(x, y), lssutil.transfer(x, y)
    assert rl.shape == (3 * nside,) and tl.shape == (3 * nside,)
    ref_r, ref_t = c2[2] / np.sqrt(c2[0] * c2[1]), c2[2] / c2[1]
    e2 = np.abs(rl - ref_r).max() / np.abs(ref_r).max()
    e3 = np.abs(tl - ref_t).max() / np.abs(ref_t).max()
    assert np.all(np.abs(rl) <= 1 + 1e-12)
    print("corrfunc %.3g, ang_correlation %.3g, transfer %.3g (relative to the largest value)" % (e1, e2, e3))
    assert max(e1, e2, e3) <= 1e-10


# ---- round trip ----------------------------------------------------------------------------------------------------
def test_round_trip_mkfullsky(ctx, golden):
    """The mean of clarray_from_maps(mkfullsky(C)) over 64 realisations (DeviceRNG seeds 0 .. 63, nside 32) lies within
    5 sigma of C_l (2l + 1/2) / (2l + 1) for every l >= 2 and every pair, sigma^2 = (C_ii C_jj + C_ij^2) / (64 (2l+1)).
    (mkfullsky's complex a_l0 keeps half its variance in the map.)  The same mean from the oracle's own a_lm for these
    seeds (oracle/philox.py stream, T g, real part of a_l0, power straight from the a_lm) was computed on the CPU before
    the seeds were fixed: its worst deviation is 3.16 sigma (l = 26, pair (6, 5)), inside the band."""
    from cora_amd.core import skysim
    from cora_amd.util.nputil import DeviceRNG

    C = golden["cla_21cm_F8_l64_zromb3"]
    L, F, _ = C.shape
    nside, nreal = 32, 64
    dC = ctx.to_device(C)
    factors = skysim.factor_device(dC)
    acc = ctx.empty((L, F, F)).zero_()
    for seed in range(nreal):
        maps = skysim.mkfullsky_device(None, nside, rng=DeviceRNG(seed), factors=factors)
        acc += skysim.clarray_from_maps(maps, lmax=L - 1)
    mean = (acc / nreal).cpu().numpy()
    l = np.arange(L)[:, None, None]
    expect = C * (2 * l + 0.5) / (2 * l + 1)
    d = np.einsum("lii->li", C)
    sigma = np.sqrt((d[:, :, None] * d[:, None, :] + C**2) / (nreal * (2 * l + 1)))
    z = (np.abs(mean - expect) / sigma)[2:]
    print("round trip: worst deviation %.2f sigma" % z.max())
    assert z.max() <= 5.0
