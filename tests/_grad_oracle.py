"""numpy oracle of the displacement-field step: first derivatives of a band-limited field on HEALPix rings and the
``lssutil.gradient`` composition (cora/signal/lssutil.py:225-261).  Test infrastructure only.

Three independent forms of ``[dT/dtheta, (1/sin theta) dT/dphi]`` for packed a_lm (healpy order), built on
``oracle.sht.lambda_lm`` (normalised Legendre functions, Condon-Shortley phase included) and
``oracle.sht.ring_synthesis``:

* ``der1_ladder``: the ladder identities, which contain NO division by sin theta - the yardstick of the tests:
    d lambda_lm / d theta = 1/2 [sqrt((l-m)(l+m+1)) lambda_{l,m+1} - sqrt((l+m)(l-m+1)) lambda_{l,m-1}],
    m lambda_lm / sin theta = -1/2 sqrt((2l+1)/(2l-1)) [sqrt((l-m)(l-m-1)) lambda_{l-1,m+1}
                                                       + sqrt((l+m)(l+m-1)) lambda_{l-1,m-1}],
  with lambda_{l,-1} = -lambda_{l,1};
* ``der1_composed``: the closed form the device evaluates, (x S[a1] - S[a2]) / sin theta and S[a3] / sin theta with
  a1 = l a_lm, a2_{l-1,m} = sqrt((2l+1)/(2l-1) (l^2 - m^2)) a_lm, a3 = i m a_lm, in numpy fp64 ring by ring;
* ``der1_bruteforce``: scipy.special.sph_harm_y(diff_n=1) for the theta component and i m Y_lm / sin theta for the
  phi component (tiny sizes).

Rings are numbered 0 .. 4 nside - 2 from the north (the index of ``oracle.healpix.ring_info``).  ``alm`` is [nalm]
or [nfields, nalm]; results carry the same leading axis.
"""
import numpy as np

from oracle import healpix
from oracle import sht as osht


def _as2d(alm):
    alm = np.asarray(alm, dtype=np.complex128)
    return (alm[None], True) if alm.ndim == 1 else (alm, False)


def _col(lmax, m):
    i0 = osht.alm_index(m, m, lmax)
    return slice(i0, i0 + lmax - m + 1)


def lam_table(lmax, x):
    """T[m, l] = lambda_lm(x) for 0 <= m <= l <= lmax; zero elsewhere (one extra zero row m = lmax + 1)."""
    T = np.zeros((lmax + 2, lmax + 1))
    for m in range(lmax + 1):
        T[m, m:] = osht.lambda_lm(lmax, m, float(x))
    return T


def ladder_tables(lmax, x):
    """(d lambda_lm / d theta, m lambda_lm / sin theta) as [m, l] tables from the ladder identities."""
    L = lmax + 1
    T = lam_table(lmax, x)
    l = np.arange(L, dtype=np.float64)[None, :]
    m = np.arange(L, dtype=np.float64)[:, None]
    ok = l >= m
    up = T[1:L + 1]                                         # lambda_{l, m+1}
    dn = np.empty((L, L))
    dn[1:] = T[:L - 1]                                      # lambda_{l, m-1}
    dn[0] = -T[1]                                           # lambda_{l,-1} = -lambda_{l,1}
    dlam = 0.5 * (np.sqrt(np.where(ok, (l - m) * (l + m + 1), 0.0)) * up
                  - np.sqrt(np.where(ok, (l + m) * (l - m + 1), 0.0)) * dn)
    dlam = np.where(ok, dlam, 0.0)
    # lambda_{l-1, m+-1}: shift the tables one step in l
    up1 = np.zeros((L, L))
    up1[:, 1:] = up[:, :-1]
    dn1 = np.zeros((L, L))
    dn1[1:, 1:] = T[:L - 1, :-1]
    ok1 = ok & (l >= 1) & (m >= 1)
    pref = np.sqrt((2 * l + 1) / np.where(l >= 1, 2 * l - 1, 1.0))
    mlam = -0.5 * pref * (np.sqrt(np.where(ok1, (l - m) * (l - m - 1), 0.0).clip(0)) * up1
                          + np.sqrt(np.where(ok1, (l + m) * (l + m - 1), 0.0)) * dn1)
    mlam = np.where(ok1, mlam, 0.0)
    return dlam, mlam


def _ring_list(nside, rings):
    nring = 4 * nside - 1
    return list(range(nring)) if rings is None else [int(r) for r in rings]


def _assemble(per_ring, nside, rings, nf, squeeze):
    """per_ring: list of ([nf, nphi], [nf, nphi]); full maps if rings is None, else the list (squeezed)."""
    if rings is not None:
        return [(a[0], b[0]) if squeeze else (a, b) for a, b in per_ring]
    ri = healpix.ring_info(nside)
    npix = healpix.nside2npix(nside)
    dth, dph = np.empty((nf, npix)), np.empty((nf, npix))
    for r, (a, b) in enumerate(per_ring):
        s, n = int(ri["start"][r]), int(ri["nphi"][r])
        dth[:, s:s + n], dph[:, s:s + n] = a, b
    return (dth[0], dph[0]) if squeeze else (dth, dph)


def der1_ladder(alm, nside, lmax, rings=None):
    """[dT/dtheta, (1/sin theta) dT/dphi] from the ladder identities.  ``rings=None``: two full RING maps;
    else a list of (dtheta, dphi) arrays, one pair per ring of ``rings`` (O(lmax^2) per ring)."""
    a, squeeze = _as2d(alm)
    nf = a.shape[0]
    ri = healpix.ring_info(nside)
    L = lmax + 1
    out = []
    for r in _ring_list(nside, rings):
        dlam, mlam = ladder_tables(lmax, ri["z"][r])
        ft = np.zeros((nf, L), dtype=np.complex128)
        fp = np.zeros((nf, L), dtype=np.complex128)
        for m in range(L):
            c = a[:, _col(lmax, m)]
            ft[:, m] = c @ dlam[m, m:]
            fp[:, m] = 1j * (c @ mlam[m, m:])
        n, p0 = int(ri["nphi"][r]), float(ri["phi0"][r])
        out.append((np.stack([osht.ring_synthesis(ft[k], n, p0) for k in range(nf)]),
                    np.stack([osht.ring_synthesis(fp[k], n, p0) for k in range(nf)])))
    return _assemble(out, nside, rings, nf, squeeze)


def der1_coefficients(alm, lmax):
    """(a1, a2, a3) of the closed form: a1 = l a_lm, a2_{l-1,m} = c_lm a_lm (a2_{lmax,m} = 0), a3 = i m a_lm."""
    a, squeeze = _as2d(alm)
    a1, a2, a3 = np.zeros_like(a), np.zeros_like(a), np.zeros_like(a)
    for m in range(lmax + 1):
        s = _col(lmax, m)
        l = np.arange(m, lmax + 1, dtype=np.float64)
        a1[:, s] = l * a[:, s]
        a3[:, s] = 1j * m * a[:, s]
        c = np.sqrt((2 * l[1:] + 1) / (2 * l[1:] - 1) * (l[1:] ** 2 - float(m) ** 2))
        a2[:, s.start:s.stop - 1] = c * a[:, s.start + 1:s.stop]
    return (a1[0], a2[0], a3[0]) if squeeze else (a1, a2, a3)


def der1_composed(alm, nside, lmax, rings=None):
    """The closed form handed to the device, in numpy fp64, ring by ring (same return convention as der1_ladder)."""
    a, squeeze = _as2d(alm)
    nf = a.shape[0]
    a1, a2, a3 = der1_coefficients(a, lmax)
    ri = healpix.ring_info(nside)
    L = lmax + 1
    out = []
    for r in _ring_list(nside, rings):
        z, sth = float(ri["z"][r]), float(ri["sth"][r])
        f1 = np.zeros((nf, L), dtype=np.complex128)
        f2, f3 = f1.copy(), f1.copy()
        for m in range(L):
            lam = osht.lambda_lm(lmax, m, z)
            s = _col(lmax, m)
            f1[:, m], f2[:, m], f3[:, m] = a1[:, s] @ lam, a2[:, s] @ lam, a3[:, s] @ lam
        n, p0 = int(ri["nphi"][r]), float(ri["phi0"][r])
        syn = lambda f: np.stack([osht.ring_synthesis(f[k], n, p0) for k in range(nf)])  # noqa: E731
        out.append(((z * syn(f1) - syn(f2)) / sth, syn(f3) / sth))
    return _assemble(out, nside, rings, nf, squeeze)


def der1_bruteforce(alm, nside, lmax):
    """Definition-level sums with scipy (nside <= 8): theta component from sph_harm_y(diff_n=1), phi component from
    i m Y_lm / sin theta."""
    from scipy.special import sph_harm_y

    alm = np.asarray(alm, dtype=np.complex128)
    theta, phi = healpix.pix2ang_ring(nside)
    dth, dph = np.zeros(theta.size), np.zeros(theta.size)
    for m in range(lmax + 1):
        cm = 1.0 if m == 0 else 2.0
        for l in range(m, lmax + 1):
            a = alm[osht.alm_index(l, m, lmax)]
            y, g = sph_harm_y(l, m, theta, phi, diff_n=1)
            if m == 0:
                dth += a.real * g[..., 0].real
            else:
                dth += cm * (a * g[..., 0]).real
                dph += cm * (a * 1j * m * y).real / np.sin(theta)
    return dth, dph


def map_rms(alm, lmax):
    """rms over the sphere of the real map with coefficients ``alm`` (Parseval): sqrt(sum_lm c_m |a_lm|^2 / 4 pi),
    c_0 = 1 on the real part, c_m = 2."""
    a, squeeze = _as2d(alm)
    n0 = lmax + 1
    p = (a[:, :n0].real ** 2).sum(axis=1) + 2.0 * (np.abs(a[:, n0:]) ** 2).sum(axis=1)
    r = np.sqrt(p / (4.0 * np.pi))
    return r[0] if squeeze else r


def tolerances(alm, nside, lmax):
    """Per-ring tolerances (theta, phi) [..., nring] of a derivative map against the ladder oracle, propagated from
    the project's gate for one scalar synthesis (1e-11 rms of the map) through the closed form:
    tol_theta = 1e-11 (|z| rms(S[a1]) + rms(S[a2])) / sin theta, tol_phi = 1e-11 rms(S[a3]) / sin theta."""
    a, squeeze = _as2d(alm)
    a1, a2, a3 = der1_coefficients(a, lmax)
    r1, r2, r3 = map_rms(a1, lmax), map_rms(a2, lmax), map_rms(a3, lmax)
    ri = healpix.ring_info(nside)
    z, sth = np.abs(ri["z"])[None, :], ri["sth"][None, :]
    tt = 1e-11 * (z * r1[:, None] + r2[:, None]) / sth
    tp = 1e-11 * r3[:, None] / sth
    return (tt[0], tp[0]) if squeeze else (tt, tp)


def per_pixel(nside, per_ring):
    """[..., nring] -> [..., npix]: the ring's value on each of its pixels."""
    return np.repeat(per_ring, healpix.ring_info(nside)["nphi"], axis=-1)


def gradient(maps, x, alm_of, nside, lmax, grad0=True):
    """The lssutil.gradient composition with the analysis passed in: ``alm_of(i)`` is the packed a_lm of map i;
    grad[1:, i] = der1_ladder(alm_of(i)) / x[i], grad[0] = np.gradient(maps, x, axis=0) or zeros."""
    maps = np.asarray(maps, dtype=np.float64)
    x = np.asarray(x, dtype=np.float64)
    grad = np.zeros((3,) + maps.shape)
    for i in range(maps.shape[0]):
        dth, dph = der1_ladder(alm_of(i), nside, lmax)
        grad[1, i], grad[2, i] = dth / x[i], dph / x[i]
    if grad0:
        grad[0] = np.gradient(maps, x, axis=0)
    return grad


def random_alm(rng, lmax, nf, power=0.0):
    """[nf, nalm] random a_lm with a real m = 0 column and spectrum l^-power (the monopole kept at 1)."""
    nalm = (lmax + 1) * (lmax + 2) // 2
    a = rng.normal(size=(nf, nalm)) + 1j * rng.normal(size=(nf, nalm))
    a[:, :lmax + 1] = a[:, :lmax + 1].real
    if power:
        for m in range(lmax + 1):
            l = np.arange(m, lmax + 1, dtype=np.float64)
            a[:, _col(lmax, m)] *= np.maximum(l, 1.0) ** (-power / 2.0)
    return a
