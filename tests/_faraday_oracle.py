"""numpy oracle of the polarised-galaxy steps (cora/foreground/galaxy.py:269-331) in the reference's statement order,
the reference's ``chunk_var`` (:58-83), and an "exact" inverse DFT along Faraday depth as a dense ``np.longdouble``
matrix product (small shapes only).  Used by tests/test_faraday_host.py and tests/test_gpu_faraday.py."""
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = np.finfo(np.float64).eps


def load_golden():
    """tests/golden/faraday_vectors.npz as {case: dict}, the quantised inputs turned into their float64 values."""
    g = np.load(os.path.join(ROOT, "tests", "golden", "faraday_vectors.npz"))
    q = float(g["q"])
    cases = {}
    for prefix in ("a_", "b_"):
        c = {k[len(prefix):]: g[k] for k in g.files if k.startswith(prefix)}
        c["base"] = c["base_q"][0] * q + 1.0j * (c["base_q"][1] * q)
        c["T"] = c["T_q"] * q
        c["faraday"] = c["faraday_q"] * q
        c["nside"], c["dphi"], c["maxphi"] = int(c["nside"]), float(c["dphi"]), float(c["maxphi"])
        cases[prefix[0]] = c
    return cases


def depth_grid(dphi, maxphi):
    nphi = 2 * int(maxphi / dphi)
    return np.fft.fftfreq(nphi, d=(1.0 / (dphi * nphi))), np.fft.fftfreq(nphi, d=dphi)


def taper(pcfreq, xiphi=1.0):
    return np.exp(-2 * (np.pi * xiphi * pcfreq[np.newaxis, :]) ** 2)


def chunk_var(a):
    nchunks = min(30, a.size)
    mean = a.mean()
    splits = np.array_split(a.ravel(), nchunks)
    t = 0.0
    for sec in splits:
        x = sec - mean
        x2 = np.sum(np.abs(x) ** 2)
        t += x2
    return t / a.size


def variance_exact(a):
    """(variance, mean) in long double."""
    a = np.asarray(a).ravel().astype(np.clongdouble)
    m = a.sum() / a.size
    d = a - m
    return float((d.real**2 + d.imag**2).sum() / a.size), complex(m)


def ptrans(phi, freq, dfreq):
    dx = dfreq / freq
    alpha = 2.0 * phi * 3e2**2 / freq**2
    return np.exp(1.0j * alpha) * np.sinc(alpha * dx / np.pi)


def transfer(phifreq, freq, dphi):
    """The reference's ``pta`` [nphi, nfreq] (:307-310)."""
    df = np.median(np.diff(freq))
    return ptrans(phifreq[:, np.newaxis], freq[np.newaxis, :], df) / dphi


def weights(phifreq, sigma_phi):
    w = np.exp(-0.25 * (phifreq[np.newaxis, :] / sigma_phi[:, np.newaxis]) ** 2)
    w /= w.sum(axis=1)[:, np.newaxis]
    return w


def saturate(map4):
    """:319-320 with the package's stated deviation: 0 where the sum is exactly 0 (the reference gives NaN)."""
    map4a = np.abs(map4)
    with np.errstate(invalid="ignore", divide="ignore"):
        out = map4 * np.tanh(map4a) / map4a
    return np.where(map4a == 0, 0.0, out)


def mix(y, scale, phifreq, sigma_phi, pta, T=None):
    """:286-331 from the depth cube after the inverse FFT: ``(map2, map4, map5 or None)``; ``scale`` = 1 / (2 sqrt(var))
    multiplies where the reference divides by ``2 chunk_var ** 0.5`` (see :func:`mix_reference`)."""
    map2 = y * scale
    map2 = map2 * weights(phifreq, sigma_phi)
    map4 = saturate(np.dot(map2, pta))
    return map2, map4, (None if T is None else to_map5(map4, T))


def to_map5(map4, T):
    map5 = np.zeros((T.shape[0], 4, T.shape[1]), dtype=np.float64)
    map5[:, 0] = T
    map5[:, 1] = map4.real.T
    map5[:, 2] = map4.imag.T
    map5[:, 1:3] *= map5[:, 0, np.newaxis, :]
    return map5


def mix_reference(base, sigma_phi, freq, T, dphi, maxphi, xiphi=1.0):
    """:269-331 statement by statement from the conj-depth maps ``base``: ``(map2, map4, w, pta, map5)``."""
    phifreq, pcfreq = depth_grid(dphi, maxphi)
    map2 = base * taper(pcfreq, xiphi)
    map2 = np.fft.ifft(map2, axis=1)
    map2 /= 2.0 * chunk_var(map2) ** 0.5
    w = weights(phifreq, sigma_phi)
    map2 *= w
    pta = transfer(phifreq, freq, dphi)
    map4 = np.dot(map2, pta)
    map4 = saturate(map4)
    return map2, map4, w, pta, to_map5(map4, T)


def idft_exact(x):
    """Inverse DFT along axis 1 as a long-double matrix product (twiddles from exactly reduced integer phases),
    rounded to complex128."""
    x = np.asarray(x)
    n = x.shape[1]
    jk = (np.arange(n)[:, None] * np.arange(n)[None, :]) % n
    ang = 8 * np.arctan(np.longdouble(1)) * jk.astype(np.longdouble) / n      # 2 pi in long double
    wr, wi = np.cos(ang), np.sin(ang)
    xr, xi = x.real.astype(np.longdouble), x.imag.astype(np.longdouble)
    yr = (xr @ wr - xi @ wi) / n
    yi = (xr @ wi + xi @ wr) / n
    return yr.astype(np.float64) + 1.0j * yi.astype(np.float64)


def mix_exact(y, scale, phifreq, sigma_phi, pta):
    """``(z, P)`` of :func:`mix` with the weights, the normaliser, the sum over depth and the saturation in long double,
    rounded to complex128 at the end: the reference of the device kernel (its own error is 2^-11 of a double's)."""
    ld = np.longdouble
    q = phifreq.astype(ld)[np.newaxis, :] / sigma_phi.astype(ld)[:, np.newaxis]
    w = np.exp(-0.25 * q * q)
    w /= w.sum(axis=1)[:, np.newaxis]
    br, bi = w * y.real.astype(ld), w * y.imag.astype(ld)
    ar, ai = pta.real.astype(ld), pta.imag.astype(ld)
    zr = (br @ ar - bi @ ai) * ld(scale)
    zi = (br @ ai + bi @ ar) * ld(scale)
    m = np.hypot(zr, zi)
    with np.errstate(invalid="ignore", divide="ignore"):
        s = np.where(m > 0, np.tanh(m) / m, 0)
    z = zr.astype(np.float64) + 1.0j * zi.astype(np.float64)
    return z, (zr * s).astype(np.float64) + 1.0j * (zi * s).astype(np.float64)


def variance_bound(count):
    """Relative bound of the device ``complex_variance`` for its own summation order, in units of eps.  The kernel
    cuts the array into nb = ceil(count / 8192) <= 4096 runs of per = ceil(count / nb) elements; in a run each of 256
    threads adds every 256th element in sequence (ceil(per / 256) additions), a wave folds its lanes in 6 halving
    steps, the 4 waves are added in order (3); the final pass does the same with the nb partials.  An element thus goes
    through D = ceil(per / 256) + ceil(nb / 256) + 18 additions, each rounding by u = eps / 2; the terms |y - m|^2 are
    positive, so the sum is within D u of itself; a term is two differences, two squares and a sum (4 u), the division
    by count one more: (D + 5) u.  Adding the zeros of idle lanes is exact, so D is at most count, the any-order bound.
    Returns ``(D, (D + 5) / 2)``."""
    nb = min(4096, max(1, -(-count // 8192)))
    per = -(-count // nb)
    nb = -(-count // per)
    D = min(count, -(-per // 256) + -(-nb // 256) + 18)
    return D, (D + 5) / 2.0


def z_bound(y, scale, phifreq, sigma_phi, pta, nphi_terms=None):
    """The per-element bound of z = scale sum_phi A w y stated in the issue: eps scale sum_phi (2 nphi + 16 + 3 t)
    |A| w |y|, t = 0.25 (phi / sigma)^2; [npix, nfreq]."""
    nphi = y.shape[1] if nphi_terms is None else nphi_terms
    t = 0.25 * (phifreq[np.newaxis, :] / sigma_phi[:, np.newaxis]) ** 2
    coef = (2 * nphi + 16 + 3 * t) * weights(phifreq, sigma_phi) * np.abs(y)
    return EPS * abs(scale) * (coef @ np.abs(pta))


# ---- the drawn path: statistics of the conj-depth maps ---------------------------------------------------------------

DRAWN = dict(nside=8, maxphi=8.0, nfreq=4, seed=20261018)     # the drawn-path case of tests/test_gpu_faraday.py


def flat_power_bound(nside):
    """``(mean, sigma)`` of ``mean_p |m_p|^2 / taper^2`` of one complex conj-depth map drawn with ``angular(l) = 1``:
    each real part has C_l = 1/2, so its mean square is (1/2) chi^2_N / (4 pi) with N = sum_l (2l+1) = (lmax+1)^2
    degrees of freedom: mean N / (8 pi), standard deviation (N / (8 pi)) sqrt(2 / N).  The two parts are independent:
    mean N / (4 pi), sigma sqrt(N) / (4 pi)."""
    N = (3 * nside) ** 2
    return N / (4 * np.pi), np.sqrt(N) / (4 * np.pi)


def pixel_power_sigma(nside, cl):
    """Mean and standard deviation of ``mean_p m_p^2`` for ONE real Gaussian field with spectrum ``cl`` synthesised at
    the pixel centres of ``nside``: the pixel covariance is K_pq = sum_l (2l+1)/(4 pi) C_l P_l(n_p . n_q) exactly (the
    synthesis evaluates the Y_lm at the centres), so the mean is K_pp and the variance 2 sum_pq K_pq^2 / npix^2 (a
    quadratic form of Gaussians).  For an exact quadrature this is the chi^2 with sum (2l+1) degrees of freedom."""
    from cora_amd.util import hputil

    npix = 12 * nside * nside
    v = np.stack(hputil.pix2vec(nside, np.arange(npix)), axis=1)
    mu = np.clip(v @ v.T, -1.0, 1.0)
    coef = (2 * np.arange(len(cl)) + 1) / (4 * np.pi) * np.asarray(cl, dtype=np.float64)
    K = np.polynomial.legendre.legval(mu, coef)
    return float(np.trace(K) / npix), float(np.sqrt(2.0 * np.sum(K * K)) / npix)
