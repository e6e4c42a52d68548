"""Counterpart of cora/foreground/galaxy.py: the full-sky synchrotron parameter sets (galaxy.py:20-40),
:func:`map_variance` and :func:`chunk_var` (:43-83) and :class:`ConstrainedGalaxy` (:86-344), the constrained realisation
of the galactic synchrotron emission.

``ConstrainedGalaxy.getsky`` runs on the device: the Gaussian maps (``skysim.mkfullsky_device``), the three beam
smoothings in one batch (``hputil.smoothing_device``), the variance chain (``Context.healpix_block_variance``), the
last third of the routine in one streaming launch (``Context.galaxy_combine``) and the rotation into celestial
co-ordinates; ``skysim.mkconstrained`` takes the smoothed maps as device tensors and stays on the device (csrc/constrained.hip).  ``getpolsky`` multiplies that sky by
the polarised fraction of :func:`polarised_fraction_device` (galaxy.py:209-344; csrc/faraday.hip).  The sky data
(``skydata.npz``: Haslam map, spectral-index maps, Faraday map) is not part of this package: the class takes the file's
path or the arrays."""
import numpy as np

from . import gaussianfg
from ..core import maps


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


# ---- variance maps (galaxy.py:43-83) -------------------------------------------------------------------------------------

def map_variance(input_map, nside):
    """Variance of ``input_map`` (RING, one map [npix] or maps [n, npix]) inside every pixel of the coarser resolution
    ``nside`` (galaxy.py:43-55), RING order.  numpy in, numpy out; a device tensor stays on the device.  One kernel
    (``Context.healpix_block_variance``: two passes, pairwise sums in NESTED child order) in place of the reference's two
    reordered copies."""
    from .. import _lib
    from ..util import hputil

    host = not hasattr(input_map, "data_ptr")
    shape = np.shape(input_map) if host else tuple(input_map.shape)
    if len(shape) not in (1, 2):
        raise ValueError("map_variance takes one map [npix] or maps [n, npix]")
    nside_in, nside = hputil.get_nside(input_map), int(nside)
    for ns in (nside_in, nside):
        if ns < 1 or ns & (ns - 1):
            raise ValueError("map_variance: nside must be a power of two (got %d)" % ns)
    if nside > nside_in or nside_in > 64 * nside:
        raise ValueError("map_variance takes a factor 1 to 64 in nside per call (got %d -> %d)" % (nside_in, nside))
    ctx = _lib.get_context()
    m = ctx.to_device(np.asarray(input_map, dtype=np.float64)) if host else input_map
    out = ctx.healpix_block_variance(m.reshape(-1, shape[-1]).contiguous(), nside)
    out = out[0] if len(shape) == 1 else out
    return out.cpu().numpy() if host else out


def chunk_var(a):
    """Variance of all elements of the (real or complex) host array ``a``, ``sum |a - mean|^2 / a.size``, accumulated
    over at most 30 pieces so that no temporary of the array's size is made (galaxy.py:58-83).  The device arrays of
    ``getpolsky`` go through the fixed-order ``Context.complex_variance`` instead."""
    a = np.asarray(a)
    mean = a.mean()
    total = 0.0
    for piece in np.array_split(a.ravel(), min(30, a.size)):
        total += np.sum(np.abs(piece - mean) ** 2)
    return total / a.size


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


# ---- the constrained galaxy (galaxy.py:86-344) ---------------------------------------------------------------------------

_SPECTRAL_KEYS = ("gsm", "md", "gd")


class ConstrainedGalaxy(maps.Sky3d):
    """Realistic simulations of the galactic synchrotron sky, constrained to the Haslam map (galaxy.py:86-344).

    Attributes
    ----------
    spectral_map : one of ['gsm', 'md', 'gd']
        Which spectral index map to use: ``gsm`` a GSM-derived map (two constraints, at 408 and 1420 MHz), ``md`` the
        map of Miville-Deschenes et al. 2008 (default), ``gd`` that of Giardino et al. 2002.

    Parameters
    ----------
    skydata : path of an ``.npz`` with the arrays ``haslam``, ``spectral_gsm``, ``spectral_md``, ``spectral_gd`` and
        ``faraday`` (the reference's ``skydata.npz``, which is not part of this package), or
    haslam, spectral, faraday : the arrays themselves, RING maps; ``spectral`` a dict keyed 'gsm' | 'md' | 'gd' or one map,
        used for whichever key ``spectral_map`` selects; ``faraday`` is needed by ``getpolsky`` only.
    amp_nside : resolution of the amplitude map (an extension: the reference hard-codes 512).
    """

    spectral_map = "md"

    _dphi = 1.0
    _maxphi = 500.0

    def __init__(self, skydata=None, haslam=None, spectral=None, faraday=None, amp_nside=512):
        from .. import _lib
        from ..util import hputil

        if skydata is not None:
            with np.load(skydata) as f:
                haslam = f["haslam"]
                spectral = {k: f["spectral_" + k] for k in _SPECTRAL_KEYS}
                faraday = f["faraday"]
        if haslam is None or spectral is None:
            raise ValueError("ConstrainedGalaxy: the sky data file is not part of cora_amd: pass skydata=FILE.npz "
                             "(arrays haslam, spectral_md, spectral_gsm, spectral_gd, faraday) or the arrays haslam, spectral")
        self._haslam = self._ring_map(haslam, "haslam")
        if not (np.all(np.isfinite(self._haslam)) and np.all(self._haslam > 0)):
            raise ValueError("haslam must be finite and positive")
        if isinstance(spectral, dict):
            bad = sorted(set(spectral) - set(_SPECTRAL_KEYS))
            if bad or not spectral:
                raise ValueError("spectral must be keyed by 'gsm', 'md', 'gd' (got %r)" % (sorted(spectral),))
            self._sp_ind = {k: self._ring_map(v, "spectral[%r]" % k) for k, v in spectral.items()}
        else:
            one = self._ring_map(spectral, "spectral")
            self._sp_ind = {k: one for k in _SPECTRAL_KEYS}
        self._faraday = None if faraday is None else self._ring_map(faraday, "faraday")
        amp_nside = int(amp_nside)
        if amp_nside < 1 or amp_nside & (amp_nside - 1):
            raise ValueError("amp_nside must be a power of two (got %d)" % amp_nside)
        if hputil.get_nside(self._haslam) < 16:
            raise ValueError("haslam must have nside >= 16: its variance is taken inside the pixels of nside 16")

        # galaxy.py:109-111
        ctx = _lib.get_context()
        vm = map_variance(hputil.smoothing_device(ctx.to_device(self._haslam[None]), sigma=np.radians(0.5)), 16)
        self._amp_map = hputil.smoothing_device(hputil.ud_grade(vm.sqrt(), amp_nside), sigma=np.radians(2.0))[0]

    @staticmethod
    def _ring_map(m, name):
        from ..util import hputil

        m = np.ascontiguousarray(m, dtype=np.float64)
        if m.ndim != 1:
            raise ValueError("%s must be one RING map [npix] (got shape %r)" % (name, m.shape))
        nside = hputil.get_nside(m)
        if nside & (nside - 1):
            raise ValueError("%s: nside must be a power of two (got %d)" % (name, nside))
        return m

    def _spectral(self):
        if self.spectral_map not in self._sp_ind:
            raise ValueError("spectral_map %r: no such spectral index map was given" % (self.spectral_map,))
        return self._sp_ind[self.spectral_map]

    def getsky_device(self, debug=False, celestial=True, rng=None):
        """A realisation of the unpolarised sky on the device, [nfreq, npix] (galaxy.py:133-207).

        debug : also return the intermediate products ``(fgt, fg, fgs, fgsmooth, am, mv)`` as the reference does.
        celestial : rotate the maps from galactic into celestial co-ordinates.
        rng : as for ``Sky3d.getsky`` (an extension): the maps have the reference's distribution, not numpy's sequence
            of numbers.
        """
        import torch

        from .. import _lib
        from ..core import skysim
        from ..util import hputil

        nside = int(self.nside)
        if nside < 32:
            raise ValueError("ConstrainedGalaxy needs nside >= 32 (got %d): the fluctuations are scaled by their variance "
                             "inside the pixels of nside 16, which is zero below" % nside)
        ctx = _lib.get_context()
        spectral = self._spectral()
        syn = FullSkySynchrotron()
        lmax = 3 * nside - 1
        efreq = np.concatenate((np.array([408.0, 1420.0]), np.asarray(self.nu_pixels, dtype=np.float64)))

        # the random fluctuations
        cla = skysim.clarray_device(syn.angular_powerspectrum, lmax, efreq, zromb=0)
        fg = skysim.mkfullsky_device(cla, nside, rng=rng)

        # the three smoothings of galaxy.py:160-161 and :176 in one batch: fg[0] at fwhm 1 deg, fg[1] at fwhm 5.8 deg,
        # fg[0] at sigma 0.5 deg
        beams = np.stack([hputil.gauss_beam(np.radians(1.0), lmax), hputil.gauss_beam(np.radians(5.8), lmax),
                          hputil.gauss_beam(np.radians(0.5) * np.sqrt(8.0 * np.log(2.0)), lmax)])
        sm = hputil.smoothing_device(fg[[0, 1, 0]], fl=beams)

        # maps constrained to the smoothed ones: at both frequencies (GSM) or at the Haslam frequency alone
        # (device tensors: mkconstrained stays on the device and returns a device tensor)
        cons = [(0, sm[0]), (1, sm[1])] if self.spectral_map == "gsm" else [(0, sm[0])]
        fgs = skysim.mkconstrained(cla, cons, nside)

        haslam = hputil.ud_grade(ctx.to_device(self._haslam), nside)
        sc = hputil.ud_grade(ctx.to_device(spectral), nside)
        am = hputil.ud_grade(self._amp_map, nside)

        # the variance of the fluctuations on the scale of the variance map; the mean over the sphere is the mean of the
        # 12 base-pixel means (ud_grade's fixed pairwise order), added up in order on the host
        vm = hputil.smoothing_device(map_variance(sm[2:3], 16).sqrt(), sigma=np.radians(2.0))
        mv = sum(ctx.to_host(hputil.ud_grade(vm, 1))[0].tolist()) / 12.0

        fgt = ctx.galaxy_combine(fg, fgs, haslam, sc, am, mv, efreq, skip=2)
        if celestial:
            fgt = hputil.rotate_map_device(fgt, hputil.coord_matrix("C", "G"))
        if debug:
            fgsmooth = haslam[None, :] * torch.pow(ctx.to_device(efreq / 408.0)[:, None], sc[None, :])
            return fgt, fg, fgs, fgsmooth, am, mv
        return fgt

    def getsky(self, debug=False, celestial=True, rng=None):
        """:meth:`getsky_device` delivered to the host: ndarray [nfreq, npix] (with ``debug`` the reference's tuple, its
        arrays on the host)."""
        from .. import _lib

        res = self.getsky_device(debug=debug, celestial=celestial, rng=rng)
        ctx = _lib.get_context()
        if debug:
            return tuple(ctx.to_host(r) for r in res[:5]) + (res[5],)
        return ctx.to_host(res)

    def getpolsky_device(self, debug=False, celestial=True, rng=None):
        """A realisation of the polarised sky on the device, [nfreq, 4, npix] (galaxy.py:209-344): the unpolarised sky
        times the polarised fraction of :func:`polarised_galaxy_device`, whose Faraday width is the smoothed ``|faraday|``
        map.  ``debug``: the tuple of :func:`polarised_galaxy_device`."""
        from .. import _lib
        from ..util import hputil

        if self._faraday is None:
            raise ValueError("getpolsky needs the Faraday rotation map: pass faraday= (or skydata=) to ConstrainedGalaxy")
        ctx = _lib.get_context()
        sigma_phi = hputil.ud_grade(
            hputil.smoothing_device(ctx.to_device(np.abs(self._faraday)[None]), fwhm=np.radians(10.0)), int(self.nside))[0]
        return polarised_galaxy_device(self.getsky_device(celestial=False, rng=rng), ctx.to_host(sigma_phi), self.nu_pixels,
                                       self.nside, rng=rng, celestial=celestial, dphi=self._dphi, maxphi=self._maxphi,
                                       debug=debug)

    def getpolsky(self, debug=False, celestial=True, rng=None):
        """:meth:`getpolsky_device` delivered to the host: ndarray [nfreq, 4, npix]."""
        from .. import _lib

        res = self.getpolsky_device(debug=debug, celestial=celestial, rng=rng)
        if debug:
            return (_lib.get_context().to_host(res[0]),) + tuple(res[1:])
        return _lib.get_context().to_host(res)
