"""numpy oracle of the polarised spectra (hputil.map2alm_sky_device / cross_spectra_pol_device / anafast_pol,
skysim.clarray_from_maps on [F, npol, npix], Context.alm_gather_channels).  Test infrastructure only; the transforms
come from ``oracle.sht``.

Layouts.  ``alm_dev`` is [nalm, G, 2, 4]: channel c of packed index k sits at [k, c // 4, (Re, Im), c % 4].  A
polarised sky is [F, npol, npix] with planes (T, Q, U[, V]); its coefficients are field-major: channel p F + f holds
field p of (T, E, B[, V]) of frequency channel f.

Bounds.
  gather      none: a copy, bit for bit.
  a_lm        1e-11 max|a| of the field against oracle.sht.map2alm / map2alm_spin2 on the same maps - the gate that
              tests/test_gpu_parity.py (sphtrans_real_pol) and tests/test_gpu_displacement.py (gradient) hold these
              transforms to.
  spectra     (2 (l + 1) + 3) eps S^abs_l[i, j] against the numpy Gram matrix of the device's own coefficients,
              S^abs = sum_m c_m (|Re a_i| |Re b_j| + |Im a_i| |Im b_j|) / (2l + 1): the bound of an inner product of
              2 (l + 1) terms in any summation order, with FMA or without, plus the division (tests/test_gpu_spectra.py).
  properties  ``norm_l(a) = sqrt(sum_m c_m |a_lm|^2 / (2l + 1))`` is a norm with ``sum_m c_m / (2l + 1) = 1``, so
              coefficients that lie within delta of the oracle's have ``|norm_l(dev) - norm_l(oracle)| <= delta``, and
              ``sqrt(2) delta`` for E and B stacked.  delta = 1e-11 max(|a^E|, |a^B|) of the (Q, U) pair: the spin-2
              analysis forms E and B from the same two maps, and its rounding scales with them, not with the smaller
              field (tests/test_gpu_parity.py takes the same scale for one pass).
"""
import numpy as np

from oracle import sht as osht

EPS = np.finfo(np.float64).eps
ALM_GATE = 1e-11


def lm(lmax):
    """(l, m) of every packed index m (2 lmax + 1 - m) / 2 + l (m-major)."""
    m = np.concatenate([np.full(lmax + 1 - mm, mm) for mm in range(lmax + 1)])
    l = np.concatenate([np.arange(mm, lmax + 1) for mm in range(lmax + 1)])
    return l, m


def gram(a, b, lmax):
    """numpy Gram matrices of packed complex a [nx, nalm], b [ny, nalm]: (S, S^abs), [lmax+1, nx, ny] each."""
    l, m = lm(lmax)
    S = np.zeros((lmax + 1, a.shape[0], b.shape[0]))
    Sabs = np.zeros_like(S)
    for ll in range(lmax + 1):
        idx = np.nonzero(l == ll)[0]
        c = np.where(m[idx] == 0, 1.0, 2.0) / (2 * ll + 1)
        x, y = a[:, idx], b[:, idx]
        S[ll] = (x.real * c) @ y.real.T + (x.imag * c) @ y.imag.T
        Sabs[ll] = (np.abs(x.real) * c) @ np.abs(y.real).T + (np.abs(x.imag) * c) @ np.abs(y.imag).T
    return S, Sabs


def gram_tol(Sabs):
    l = np.arange(Sabs.shape[0])[:, None, None]
    return (2 * (l + 1) + 3) * EPS * Sabs


def ratio(err, tol):
    """worst err / tol; a non-zero error where the tolerance is zero counts as inf"""
    err, tol = np.broadcast_arrays(np.asarray(err, dtype=np.float64), np.asarray(tol, dtype=np.float64))
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(tol > 0, err / np.where(tol > 0, tol, 1.0), np.where(err > 0, np.inf, 0.0))
    return float(np.max(r)) if r.size else 0.0


def norm_l(a, lmax):
    """sqrt(sum_m c_m |a_lm|^2 / (2l + 1)) per l of packed a [..., nalm] -> [..., lmax + 1]"""
    l, m = lm(lmax)
    w = np.where(m == 0, 1.0, 2.0) / (2 * l + 1)
    out = np.zeros(a.shape[:-1] + (lmax + 1,))
    np.add.at(out, (Ellipsis, l), w * np.abs(a) ** 2)
    return np.sqrt(out)


# ---- the a_lm layout ---------------------------------------------------------------------------------------------
def to_layout(a, pad=0.0):
    """packed complex a [n, nalm] -> alm_dev [nalm, ceil(n / 4), 2, 4] on the host; padding channels hold ``pad``"""
    n, nalm = a.shape
    G = (n + 3) // 4
    full = np.full((4 * G, nalm), pad + 1j * pad, dtype=np.complex128)
    full[:n] = a
    dev = np.empty((nalm, G, 2, 4))
    dev[:, :, 0, :] = full.real.T.reshape(nalm, G, 4)
    dev[:, :, 1, :] = full.imag.T.reshape(nalm, G, 4)
    return dev


def from_layout(dev):
    """alm_dev [nalm, G, 2, 4] (host) -> complex [4 G, nalm], padding channels included"""
    nalm, G = dev.shape[:2]
    return (dev[:, :, 0, :] + 1j * dev[:, :, 1, :]).reshape(nalm, 4 * G).T


def square_to_packed(sq, lmax):
    l, m = lm(lmax)
    return np.ascontiguousarray(sq[:, l, m])


def device_packed(ctx, alm_dev, lmax, n):
    """host copy, packed [n, nalm], of the first n channels of a device alm_dev"""
    return square_to_packed(ctx.alm_dev_to_square(alm_dev, lmax, n).cpu().numpy()[:, 0], lmax)


# ---- polarised skies ---------------------------------------------------------------------------------------------
def random_sky_alm(rng, lmax, F, npol, pure_e=False):
    """[npol, F, nalm] band-limited coefficients of (T, E, B[, V]): spectrum 1 / (1 + l), m = 0 real, E and B zero
    below l = 2 (``pure_e``: B zero everywhere)"""
    l, m = lm(lmax)
    nalm = l.size
    a = (rng.standard_normal((npol, F, nalm)) + 1j * rng.standard_normal((npol, F, nalm))) / (1.0 + l)
    a[..., m == 0] = a[..., m == 0].real
    a[1:3][..., l < 2] = 0.0
    if pure_e:
        a[2] = 0.0
    return a


def synth_sky(alm, nside, lmax):
    """[npol, F, nalm] -> maps [F, npol, npix] of (T, Q, U[, V]) with oracle.sht.alm2map / alm2map_spin2"""
    npol, F = alm.shape[:2]
    maps = np.empty((F, npol, 12 * nside * nside))
    for f in range(F):
        maps[f, 0] = osht.alm2map(alm[0, f], nside, lmax)
        maps[f, 1], maps[f, 2] = osht.alm2map_spin2(alm[1, f], alm[2, f], nside, lmax)
        if npol == 4:
            maps[f, 3] = osht.alm2map(alm[3, f], nside, lmax)
    return maps


def analyse_sky(maps, nside, lmax, use_weights=True, niter=2):
    """maps [F, npol, npix] -> field-major packed coefficients [npol F, nalm] with oracle.sht.map2alm / map2alm_spin2"""
    F, npol = maps.shape[:2]
    out = np.empty((npol * F, (lmax + 1) * (lmax + 2) // 2), dtype=np.complex128)
    for f in range(F):
        out[f] = osht.map2alm(maps[f, 0], nside, lmax, use_weights=use_weights, niter=niter)
        out[F + f], out[2 * F + f] = osht.map2alm_spin2(maps[f, 1], maps[f, 2], nside, lmax, use_weights=use_weights, niter=niter)
        if npol == 4:
            out[3 * F + f] = osht.map2alm(maps[f, 3], nside, lmax, use_weights=use_weights, niter=niter)
    return out


def rotate_polarisation(maps, psi):
    """Q' = Q cos 2 psi - U sin 2 psi, U' = Q sin 2 psi + U cos 2 psi on every pixel of maps [F, npol, npix]"""
    out = maps.copy()
    c, s = np.cos(2 * psi), np.sin(2 * psi)
    out[:, 1] = maps[:, 1] * c - maps[:, 2] * s
    out[:, 2] = maps[:, 1] * s + maps[:, 2] * c
    return out
