"""Counterpart of the Gaussian part of cora/foreground/galaxy.py: the full-sky synchrotron
parameter sets (galaxy.py:20-40), and the body of ``ConstrainedGalaxy.getpolsky`` (galaxy.py:209-344) given its two
data-derived inputs, the Faraday-width map and the unpolarised sky: :func:`polarised_fraction_device`,
:func:`polarised_galaxy_device`, :func:`polarised_galaxy`.  ``ConstrainedGalaxy`` itself (``skydata.npz``, healpy
smoothing, ``getsky``) is not part of this package."""
import numpy as np

from . import gaussianfg


class FullSkySynchrotron(gaussianfg.Synchrotron):
    """Synchrotron amplitudes of La Porta et al. 2008 for |b| > 5 deg."""

    A = 6.6e-3
    beta = 2.8
    nu_0 = 408.0
    l_0 = 100.0


class FullSkyPolarisedSynchrotron(gaussianfg.Synchrotron):
    """Polarised synchrotron: same spectral shape, polarisation fraction 0.5 and a short
    frequency correlation length from Faraday rotation."""

    A = 1.65e-3
    beta = 2.8
    nu_0 = 408.0
    l_0 = 100.0
    zeta = 0.04


# ---- polarised emission: Faraday-depth synthesis (galaxy.py:209-344; csrc/faraday.hip) -------------------------------

DEPTH_CHUNK = 16     # depth channels drawn and synthesised at a time (2 * DEPTH_CHUNK real maps)


def faraday_depth_grid(dphi=1.0, maxphi=500.0):
    """``(phifreq, pcfreq)`` of galaxy.py:249-252 and :270: the Faraday-depth grid of ``nphi = 2 int(maxphi / dphi)``
    points in FFT order and its Fourier conjugate."""
    nphi = 2 * int(maxphi / dphi)
    if nphi < 2:
        raise ValueError("faraday_depth_grid: maxphi / dphi must be at least 1 (got %r / %r)" % (maxphi, dphi))
    phifreq = np.fft.fftfreq(nphi, d=(1.0 / (dphi * nphi)))
    pcfreq = np.fft.fftfreq(nphi, d=dphi)
    return phifreq, pcfreq


def faraday_transfer(phi, freq, dfreq):
    """The reference's ``ptrans`` (galaxy.py:300-305): rotation by Faraday depth ``phi`` at ``freq`` (MHz) averaged over
    a channel of width ``dfreq``."""
    dx = dfreq / freq

    alpha = 2.0 * phi * 3e2**2 / freq**2

    return np.exp(1.0j * alpha) * np.sinc(alpha * dx / np.pi)


def polarisation_angular_ps(l):
    """The angular power spectrum of the polarisation fluctuations (galaxy.py:244-246); l = 0 carries no power."""
    l = np.array(l, dtype=np.float64)
    l[np.where(l == 0)] = 1.0e16
    return (l / 100.0) ** -2.8


def _depth_taper(pcfreq, xiphi):
    return np.exp(-2 * (np.pi * xiphi * pcfreq) ** 2)


def _check_sigma(sigma_phi, npix):
    sigma = np.asarray(sigma_phi, dtype=np.float64)
    if sigma.shape != (npix,):
        raise ValueError("sigma_phi has shape %r, expected (%d,)" % (sigma.shape, npix))
    if not (np.all(np.isfinite(sigma)) and np.all(sigma > 0)):
        raise ValueError("sigma_phi must be finite and positive")
    return sigma


def _check_fits(nbytes, what):
    import torch

    free = torch.cuda.mem_get_info()[0]
    if nbytes > free:
        raise MemoryError("%s needs %.1f GB of device memory, %.1f GB are free: lower nside or maxphi / dphi"
                          % (what, nbytes / 1e9, free / 1e9))


def faraday_base_maps_device(nside, pcfreq, rng=None, xiphi=1.0, angular=None, chunk=None):
    """Random maps in the Fourier conjugate of Faraday depth with the depth taper applied (galaxy.py:260-271), drawn and
    synthesised on the device: complex128 ``[npix, nphi]``.

    The real and imaginary parts of the reference's complex field (full-m complex a_lm of variance ``angular(l) / 2``
    per part, galaxy.py:263-266) are ``2 nphi`` independent real Gaussian fields with ``C_l = angular(l) / 2``; the
    taper ``exp(-2 (pi xiphi pcfreq_k)^2)`` is a scalar per channel and goes into channel k's spectrum.  The fields
    come from :func:`cora_amd.core.skysim.mkfullsky_device` in chunks of ``chunk`` depth channels, each packed straight
    into the ``[npix, nphi]`` array.  Same distribution as the reference, not numpy's sequence of numbers."""
    import torch

    from .. import _lib
    from ..core import skysim

    ctx = _lib.get_context()
    nside = int(nside)
    npix, lmax = 12 * nside * nside, 3 * nside - 1
    nphi = len(pcfreq)
    chunk = DEPTH_CHUNK if chunk is None else int(chunk)
    cl = (polarisation_angular_ps if angular is None else angular)(np.arange(lmax + 1, dtype=np.float64))
    cl = np.broadcast_to(np.asarray(cl, dtype=np.float64), (lmax + 1,)) / 2.0
    taper2 = _depth_taper(np.asarray(pcfreq, dtype=np.float64), xiphi) ** 2
    _check_fits(npix * nphi * 16 + 3 * min(chunk, nphi) * 2 * npix * 8, "The [npix, nphi] depth cube")
    y = torch.empty((npix, nphi), dtype=torch.complex128, device=ctx.device)
    for k0 in range(0, nphi, chunk):
        nc = min(chunk, nphi - k0)
        corr = np.zeros((lmax + 1, 2 * nc, 2 * nc))
        i = np.arange(2 * nc)
        corr[:, i, i] = cl[:, None] * np.repeat(taper2[k0:k0 + nc], 2)[None, :]
        maps = skysim.mkfullsky_device(corr, nside, rng=rng)
        ctx.faraday_pack(maps, y, k0)
    return y


def _polarised(sigma_phi, freq, nside, rng, dphi, maxphi, xiphi, angular, base, debug, intensity):
    import torch

    from .. import _lib

    nside = int(nside)
    npix = 12 * nside * nside
    freq = np.asarray(freq, dtype=np.float64)
    if freq.ndim != 1 or freq.size < 1:
        raise ValueError("freq must be a 1-D array of channel centres")
    sigma = _check_sigma(sigma_phi, npix)
    phifreq, pcfreq = faraday_depth_grid(dphi, maxphi)
    nphi = len(phifreq)
    df = np.median(np.diff(freq)) if freq.size > 1 else 0.0
    A = np.ascontiguousarray((faraday_transfer(phifreq[:, np.newaxis], freq[np.newaxis, :], df) / dphi).T)
    if base is not None and tuple(base.shape) != (npix, nphi):
        raise ValueError("base has shape %r, expected %r" % (tuple(base.shape), (npix, nphi)))
    if intensity is not None and tuple(intensity.shape) != (freq.size, npix):
        raise ValueError("intensity has shape %r, expected %r" % (tuple(intensity.shape), (freq.size, npix)))

    ctx = _lib.get_context()
    if base is not None:
        _check_fits(npix * nphi * 16, "The [npix, nphi] depth cube")
        if isinstance(base, torch.Tensor):
            y = base.to(device=ctx.device, dtype=torch.complex128).clone().contiguous()
        else:
            y = torch.from_numpy(np.ascontiguousarray(base, dtype=np.complex128)).to(ctx.device)
        torch.view_as_real(y).mul_(ctx.to_device(_depth_taper(pcfreq, xiphi))[None, :, None])
    else:
        y = faraday_base_maps_device(nside, pcfreq, rng=rng, xiphi=xiphi, angular=angular)
    ctx.fft_c2c(y, axis=1, inverse=True)
    var, _ = ctx.complex_variance(y)
    scale = 1.0 / (2.0 * var**0.5)
    out = ctx.faraday_mix(y, phifreq, sigma, A, scale, intensity=intensity)
    if debug:
        return out, y, var, A
    return out


def polarised_fraction_device(sigma_phi, freq, nside, rng=None, dphi=1.0, maxphi=500.0, xiphi=1.0, angular=None,
                              base=None, debug=False):
    """The polarised fraction ``P = (Q + iU) / T`` of ``getpolsky`` (galaxy.py:236-320) on the device: complex128
    ``[nfreq, npix]``, ``|P| < 1``.

    sigma_phi : [npix] Faraday width of every pixel (the reference smooths ``|faraday|`` to get it); finite and
        positive, else ``ValueError``.
    freq : [nfreq] channel centres in MHz.
    base : optional complex ``[npix, nphi]``, the conj-depth maps of galaxy.py:260-267 (before the taper of :271): the
        call is then deterministic.  Without it they are drawn on the device (:func:`faraday_base_maps_device`) from
        ``rng``, a :class:`cora_amd.DeviceRNG` or a numpy generator as for ``mkfullsky_device``: the same distribution
        as the reference, not numpy's sequence of numbers (the reference draws ``nphi`` full-m complex a_lm arrays
        from the global numpy state).
    angular : optional ``C_l`` of the fluctuations, a function of an array of l (default: galaxy.py:244-246).
    debug : also return the device depth cube ``y`` after the inverse FFT, its variance and the host matrix ``A``.

    Steps: taper, inverse FFT along depth (``fft_c2c``), ``complex_variance``, then the fused ``faraday_mix``
    (weighting in depth, product with ``A = (ptrans / dphi).T``, tanh saturation).  Where the reference gives NaN
    (a pixel whose sum is exactly zero) P is 0.  A problem whose ``[npix, nphi]`` cube does not fit in free device
    memory raises ``MemoryError`` before anything is allocated."""
    return _polarised(sigma_phi, freq, nside, rng, dphi, maxphi, xiphi, angular, base, debug, None)


def polarised_galaxy_device(intensity, sigma_phi, freq, nside, rng=None, celestial=True, **kw):
    """The reference's ``map5`` (galaxy.py:324-339) on the device: float64 ``[nfreq, 4, npix]`` = (T, Re P T, Im P T, 0)
    for the unpolarised sky ``intensity`` = T ``[nfreq, npix]`` (galactic co-ordinates, host array or device tensor);
    ``celestial``: rotated into celestial co-ordinates with the existing map rotation, planes as scalars, as the
    reference does.  Other arguments as :func:`polarised_fraction_device`."""
    import torch

    from .. import _lib
    from ..util import hputil

    ctx = _lib.get_context()
    if not isinstance(intensity, torch.Tensor):
        intensity = ctx.to_device(np.asarray(intensity, dtype=np.float64))
    intensity = intensity.to(device=ctx.device, dtype=torch.float64).contiguous()
    debug = kw.pop("debug", False)
    res = _polarised(sigma_phi, freq, nside, rng, kw.pop("dphi", 1.0), kw.pop("maxphi", 500.0), kw.pop("xiphi", 1.0),
                     kw.pop("angular", None), kw.pop("base", None), debug, intensity)
    if kw:
        raise TypeError("unexpected arguments: %s" % ", ".join(sorted(kw)))
    out = res[0] if debug else res
    if celestial:
        nfreq, _, npix = out.shape
        out = hputil.rotate_map_device(out.reshape(nfreq * 4, npix), hputil.coord_matrix("C", "G")).reshape(nfreq, 4, npix)
    return (out,) + tuple(res[1:]) if debug else out


def polarised_galaxy(intensity, sigma_phi, freq, nside, rng=None, celestial=True, **kw):
    """:func:`polarised_galaxy_device` delivered to the host: ndarray ``[nfreq, 4, npix]``."""
    from .. import _lib

    res = polarised_galaxy_device(intensity, sigma_phi, freq, nside, rng=rng, celestial=celestial, **kw)
    if kw.get("debug", False):
        return (_lib.get_context().to_host(res[0]),) + tuple(res[1:])
    return _lib.get_context().to_host(res)
