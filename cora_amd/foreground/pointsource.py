"""Extra-galactic point sources (counterpart of cora/foreground/pointsource.py).

Three components, as in the reference: a Gaussian background below 0.1 Jy (``UnresolvedBackground``), a synthetic
population drawn from a source-count function (``PointSourceModel`` and its subclasses) and real sources from a
catalogue (``RealPointSources``); ``CombinedPointSources`` adds them up.

The reference forms the ``[N, F]`` array of every source's spectrum and adds its rows to pixels in a Python loop.  Here
the population is generated on the device (:func:`population_device`), sorted by pixel and painted straight into the
``[F, npix]`` map (:func:`paint_sources_device`, csrc/pointsource.hip); polarisation and Faraday rotation are one further
kernel.  The drawn maps have the reference's distribution, not numpy's sequence of numbers: the host quadrature, the
Poisson-distributed number of sources and the inverse-CDF spline are the reference's, the sources themselves come from a
counter-based stream keyed by a seed taken from the caller's generator.  Given ``(pix, flux, index)`` the map is the
reference's to rounding.

The two data files of the reference, the rotation-measure map of ``skydata.npz`` and the catalogue ``combinedps.dat``,
are not part of this package: they are the arguments ``faraday_map=`` and ``catalogue=``.
"""
import warnings

import numpy as np
import numpy.random as rnd

from .. import _lib
from ..core import maps
from ..util import constants, hputil
from ..util.nputil import DeviceRNG
from . import gaussianfg
from . import poisson as ps

CATALOGUE_FIELDS = ("RA", "DEC", "S600", "P600", "POLANG", "BETA", "GAMMA")


def _wavelengths(frequencies):
    return 1e-6 * constants.c / np.asarray(frequencies, dtype=np.float64)


def faraday_rotate(polmap, rm_map, frequencies):
    """Faraday rotate a set of sky maps, in place (pointsource.py:21-51); returns its argument.

    polmap : [freq, pol, pixel], packed as T, Q, U and optionally V: a numpy array or a float64 device tensor.
    rm_map : [pixel] rotation measure in rad / m^2.
    frequencies : [freq] in MHz.

    ``Q + iU`` is multiplied by ``exp(-2i wv rm)`` with ``wv = 1e-6 c / freq``: the wavelength, not its square.  That
    is the reference's own form (pointsource.py:43-45) and is kept, so that maps agree with it."""
    ctx = _lib.get_context()
    wv = _wavelengths(frequencies)
    if hasattr(polmap, "data_ptr"):
        ctx.faraday_rotate(polmap, rm_map, wv)
        return polmap
    if not isinstance(polmap, np.ndarray) or polmap.ndim != 3:
        raise ValueError("polmap must be a [freq, pol, pixel] array")
    dev = ctx.faraday_rotate(ctx.to_device(polmap), np.asarray(rm_map, dtype=np.float64), wv)
    polmap[:, 1:3] = dev[:, 1:3].cpu().numpy()
    return polmap


def _seed_and_generator(rng):
    """``(seed, draw)`` for one realisation: the 64-bit seed of the device stream and the host generator the few host
    draws (the Poisson count, the polarisation fractions) come from.  ``rng``: None (numpy's legacy global state, as
    the reference), a numpy ``Generator``, or a :class:`cora_amd.DeviceRNG`."""
    if rng is None:
        return None, rnd
    if isinstance(rng, DeviceRNG):
        seed = rng.next_seed()
        return seed, np.random.default_rng([seed & (2**64 - 1), 0x50535243])
    return None, rng


def _draw_seed(seed, draw):
    if seed is not None:
        return seed
    if draw is rnd:
        return int(rnd.randint(0, 2**63 - 1, dtype=np.int64))
    return int(draw.integers(0, 2**63 - 1))


def paint_sources_device(pix, flux, beta, frequencies, pivot, nside, gamma=None, polw=None, npol=1, out=None,
                         accumulate=False, check_pixels=True):
    """Paint sources into a brightness-temperature map on the device: ``[nfreq, npix]`` (``npol=1``) or
    ``[nfreq, 4, npix]`` in K.

    Source i adds ``flux_i exp(beta_i x + gamma_i x^2)`` Jy, ``x = log(freq / pivot)``, to pixel ``pix_i``: the power
    law ``flux (freq / pivot)^beta`` of the synthetic models with ``gamma=None``, the curved spectrum of the catalogue
    with it (pointsource.py:335, :495).  ``polw`` [N, 2] weights the same spectrum into Q and U.  The Jy -> K factor
    ``1e-26 c^2 / (2 k_B nu^2 1e12 pxarea)`` is applied per channel (:245-250).  Arguments are host arrays or device
    tensors; the sources are sorted by pixel here (stable).  A channel's map depends on that channel alone: painting a
    subset of ``frequencies`` gives, bit for bit, those rows of the full map, so frequency-sharded ranks paint their own
    rows of one population.  ``accumulate`` adds to ``out`` instead.  ``check_pixels=False`` skips the range check of ``pix``
    (two reductions and host synchronisations) for pixels that a kernel has just produced in range."""
    import torch

    ctx = _lib.get_context()
    nside = int(nside)
    npix = 12 * nside * nside
    freq = np.asarray(frequencies, dtype=np.float64)
    if freq.ndim != 1 or freq.size < 1:
        raise ValueError("frequencies must be a 1-D array of channel centres")

    def dev(a, dtype):
        if a is None:
            return None
        if not isinstance(a, torch.Tensor):
            a = torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64 if dtype == torch.int64 else np.float64))
        return a.to(device=ctx.device, dtype=dtype).contiguous()

    pix = dev(pix, torch.int64)
    if pix.dim() != 1:
        raise ValueError("pix must be one-dimensional")
    if check_pixels and pix.numel() and (int(pix.min()) < 0 or int(pix.max()) >= npix):
        raise ValueError("pixel index out of range for nside %d" % nside)
    pix, order = torch.sort(pix, stable=True)
    flux, beta, gamma, polw = (None if a is None else dev(a, torch.float64)[order].contiguous()
                               for a in (flux, beta, gamma, polw))
    pxarea = 4 * np.pi / npix
    x = np.log(freq / pivot)
    den = 2 * constants.k_B * freq**2 * 1e12 * pxarea
    return ctx.pointsource_paint(pix, flux, beta, x, den, constants.c**2, npix, gamma=gamma, polw=polw, npol=npol, out=out,
                                 accumulate=accumulate)


def population_device(model, area, seed, total=None):
    """The synthetic population of ``model`` over ``area`` (steradians) on the device: ``(pix, flux, index)`` tensors of
    one length, unsorted.

    The expected count (quadrature of the source-count function in log flux) and the inverse-CDF spline are formed on
    the host as the reference does (pointsource.py:163-171, poisson.py:191-204).  ``total`` is the number of sources:
    a number, a function of the expected count such as a generator's ``poisson``, or by default a Poisson draw keyed by
    ``seed``.  The sources are generated in one launch from counters that depend on ``(seed, i)`` alone: identical on
    every rank and for any number of GPUs.  Pixels are uniform over the model's ``12 nside^2``."""
    flux_max = model._flux_max(area)
    t = np.log(flux_max / model.flux_min)
    rate = model._log_rate(area)
    if total is None:
        total = np.random.default_rng([int(seed) & (2**64 - 1), 0x50535243]).poisson(ps.expected_events(t, rate))
    elif callable(total):
        total = total(ps.expected_events(t, rate))
    data, y2 = ps.inverse_cdf(t, rate).data()
    ctx = _lib.get_context()
    return ctx.pointsource_population(seed, int(total), data[:, 0], data[:, 1], y2, model.flux_min, model.spectral_mean,
                                      model.spectral_width, 12 * model.nside**2)


class PointSourceModel(maps.Map3d):
    r"""A population of astrophysical point sources described by a source-count function and a spectral function
    (pointsource.py:54-278).  A model implements ``source_count`` and ``spectral_realisation``; the device path needs
    the power-law spectrum of the two models below (``spectral_mean``, ``spectral_width``, ``spectral_pivot``).

    Attributes
    ----------
    flux_min : float
        The lower flux limit of sources to include (Jy).
    flux_max : {float, None}
        The upper flux limit; ``None``: the flux above which a source is improbable.
    faraday : boolean
        Whether to Faraday rotate polarisation maps (default True).  Needs ``faraday_map``.
    sigma_pol_frac : scalar
        The standard deviation of the polarisation fraction of sources.

    ``faraday_map`` : the rotation-measure map (rad / m^2, RING, any power-of-two nside); it is brought to the model's
    nside with :func:`cora_amd.util.hputil.ud_grade`.  The reference reads it from ``skydata.npz``.
    """

    flux_min = 1e-4
    flux_max = None

    faraday = True

    sigma_pol_frac = 0.03

    def __init__(self, faraday_map=None):
        self._faraday = None if faraday_map is None else np.asarray(faraday_map, dtype=np.float64)

    def source_count(self, flux):
        r"""The expected number of sources per unit flux (Jy) per steradian; implemented by a model."""
        pass

    def spectral_realisation(self, flux, frequencies):
        r"""The flux of sources of ``flux`` at each of ``frequencies`` (broadcasting); implemented by a model."""
        pass

    def _flux_max(self, area):
        if self.flux_max is not None:
            return self.flux_max
        from scipy.optimize import newton

        # the flux above which P(> S) is small (pointsource.py:147-157)
        flux_max = newton(lambda s: (s * area * self.source_count(s) - 5e-2), self.flux_min)
        print("Using maximum flux: %e Jy" % flux_max)
        return flux_max

    def _log_rate(self, area):
        return lambda s: self.flux_min * np.exp(s) * area * self.source_count(self.flux_min * np.exp(s))

    def generate_population(self, area):
        r"""The fluxes (Jy) of a population over ``area`` (steradians), on the host: the reference's numbers under
        ``np.random.seed`` (pointsource.py:131-173)."""
        flux_max = self._flux_max(area)
        return self.flux_min * np.exp(ps.inhomogeneous_process_approx(np.log(flux_max / self.flux_min), self._log_rate(area)))

    def _rm_device(self):
        if self._faraday is None:
            raise ValueError("faraday=True needs the rotation-measure map: pass faraday_map= (rad / m^2, RING order, any "
                             "power-of-two nside) to the constructor, or set faraday = False")
        ctx = _lib.get_context()
        return hputil.ud_grade(ctx.to_device(self._faraday), self.nside)

    def getsky_device(self, rng=None, out=None, accumulate=False, _state=None):
        """:meth:`getsky` as a device tensor; with ``out`` and ``accumulate`` the population is added to ``out``."""
        seed, draw = _state or _seed_and_generator(rng)
        pix, flux, index = population_device(self, 4 * np.pi, _draw_seed(seed, draw), total=draw.poisson)
        return paint_sources_device(pix, flux, index, self.nu_pixels, self.spectral_pivot, self.nside, out=out,
                                    accumulate=accumulate, check_pixels=False)

    def getsky(self, rng=None):
        """Simulate a map of point sources: ``[nfreq, npix]`` brightness temperature in K (pointsource.py:213-251).

        Order of work: host quadrature of the source count; the number of sources from ``rng`` (None: numpy's legacy
        global state, a numpy ``Generator``, or a :class:`cora_amd.DeviceRNG`); the inverse-CDF spline; the population
        on the device; a stable sort on pixel; the paint.  Same distribution as the reference, not numpy's sequence of
        numbers: the reference draws every source from the global numpy state."""
        return _lib.get_context().to_host(self.getsky_device(rng=rng))

    def getpolsky_device(self, rng=None):
        """:meth:`getpolsky` as a device tensor."""
        state = _seed_and_generator(rng)
        rm = self._rm_device() if self.faraday else None
        sky_I = self.getsky_device(_state=state)
        npix = sky_I.shape[1]
        draw = state[1]
        q_frac = self.sigma_pol_frac * draw.standard_normal(npix)
        u_frac = self.sigma_pol_frac * draw.standard_normal(npix)
        return _lib.get_context().polarise_rotate(sky_I, q_frac, u_frac, wv=_wavelengths(self.nu_pixels), rm=rm)

    def getpolsky(self, rng=None):
        """Simulate polarised point sources: ``[nfreq, 4, npix]`` (pointsource.py:253-278).  Every pixel gets Gaussian
        polarisation fractions of width ``sigma_pol_frac`` in Q and U, Faraday rotated with ``faraday_map`` when
        ``faraday`` is set.  ``rng`` and the distribution contract as :meth:`getsky`."""
        return _lib.get_context().to_host(self.getpolsky_device(rng=rng))


class PowerLawModel(PointSourceModel):
    r"""A power-law luminosity function and a power-law spectrum with a Gaussian-distributed index
    (pointsource.py:281-335; source counts loosely after the 6C survey, Hales et al. 1988).

    Attributes: ``source_index``, ``source_pivot`` (Jy), ``source_amplitude`` (sources / Jy / sr at the pivot),
    ``spectral_mean``, ``spectral_width``, ``spectral_pivot`` (MHz, the frequency the flux is defined at).
    """

    source_index = 2.5
    source_pivot = 1.0
    source_amplitude = 2.396e3

    spectral_mean = -0.7
    spectral_width = 0.1

    spectral_pivot = 151.0

    def source_count(self, flux):
        r"""Power law luminosity function."""
        return self.source_amplitude * (flux / self.source_pivot) ** (-self.source_index)

    def spectral_realisation(self, flux, freq):
        r"""Power-law spectral function with Gaussian distributed index (host, numpy's global state)."""
        ind = self.spectral_mean + self.spectral_width * rnd.standard_normal(flux.shape)
        return flux * (freq / self.spectral_pivot) ** ind


class DiMatteo(PointSourceModel):
    r"""Double power-law source counts of Di Matteo et al. 2002 (astro-ph/0109241), with the normalisation of Santos et
    al. 2005 (astro-ph/0408515, footnote 6): ``S_0`` is both pivot and normalising flux (pointsource.py:338-394).

    Attributes: ``gamma1``, ``gamma2``, ``S_0`` (Jy), ``k1`` (sources / Jy / sr at the pivot), ``spectral_mean``,
    ``spectral_width``, ``spectral_pivot`` (MHz).
    """

    gamma1 = 1.75
    gamma2 = 2.51
    S_0 = 0.88
    k1 = 1.52e3

    spectral_mean = -0.7
    spectral_width = 0.1

    spectral_pivot = 151.0

    def source_count(self, flux):
        r"""Double power law luminosity function."""
        s = flux / self.S_0
        return self.k1 / (s**self.gamma1 + s**self.gamma2)

    def spectral_realisation(self, flux, freq):
        r"""Power-law spectral function with Gaussian distributed index (host, numpy's global state)."""
        ind = self.spectral_mean + self.spectral_width * rnd.standard_normal(flux.shape)
        return flux * (freq / self.spectral_pivot) ** ind


def load_catalogue(catalogue):
    """The catalogue as a structured array with at least the fields RA, DEC (degrees), S600, P600 (Jy), POLANG
    (degrees), BETA, GAMMA: a path to a whitespace table with a header line (the reference's ``combinedps.dat``), or
    such an array."""
    if isinstance(catalogue, (str, bytes)) or hasattr(catalogue, "__fspath__"):
        with open(catalogue, "r") as f:
            catalogue = np.genfromtxt(f, names=True)
    catalogue = np.atleast_1d(np.asarray(catalogue))
    names = catalogue.dtype.names or ()
    missing = [k for k in CATALOGUE_FIELDS if k not in names]
    if missing:
        raise ValueError("catalogue lacks the field(s) %s" % ", ".join(missing))
    return catalogue


class RealPointSources(maps.Map3d):
    r"""Maps of real point sources from a catalogue at 600 MHz (the reference's comes from NVSS and VLSS,
    pointsource.py:397-523), each with the spectrum ``S600 exp(BETA x + GAMMA x^2)``, ``x = log(freq / 600)``.

    ``catalogue`` : a path or a structured array (:func:`load_catalogue`).  A source whose ``P600`` or ``POLANG`` is NaN
    contributes no Q / U.  ``faraday_map`` as for :class:`PointSourceModel`.

    Attributes: ``flux_min``, ``flux_max`` (Jy at 600 MHz, exclusive limits), ``faraday``, ``spectral_pivot``.
    """

    flux_min = 10.0
    flux_max = None

    spectral_pivot = 600.0

    faraday = True

    _rm_device = PointSourceModel._rm_device

    def __init__(self, catalogue=None, faraday_map=None):
        if catalogue is None:
            raise ValueError("RealPointSources needs the source catalogue: pass catalogue= (a path to a table with the "
                             "columns %s, or a structured array with those fields)" % " ".join(CATALOGUE_FIELDS))
        self._catalogue = load_catalogue(catalogue)
        self._faraday = None if faraday_map is None else np.asarray(faraday_map, dtype=np.float64)

    def _generate_catalogue(self):
        flux = self._catalogue["S600"]
        mask = np.ones_like(flux, dtype=bool)
        if self.flux_max is not None:
            mask &= flux < self.flux_max
        if self.flux_min is not None:
            mask &= flux > self.flux_min
        self._masked_catalogue = self._catalogue[np.where(mask)]

    def _sources(self):
        self._generate_catalogue()
        if self.flux_min < 2.0:
            print("Flux limit probably too low for reliable catalogue.")
        cat = self._masked_catalogue
        theta = np.pi / 2.0 - np.radians(cat["DEC"])
        phi = np.radians(cat["RA"])
        pix = np.atleast_1d(hputil.ang2pix(self.nside, theta, phi))
        flux = cat["S600"]
        # NVSS angles run from North to East, as HEALPix's do: no transformation
        polang = np.radians(cat["POLANG"])
        frac = cat["P600"] / flux
        polw = np.stack([frac * np.cos(2.0 * polang), frac * np.sin(2.0 * polang)], axis=1)
        polw[np.isnan(cat["P600"]) | np.isnan(polang)] = 0.0
        return pix, flux, cat["BETA"], cat["GAMMA"], polw

    def getsky_device(self, out=None, accumulate=False):
        pix, flux, beta, gamma, _ = self._sources()
        return paint_sources_device(pix, flux, beta, self.nu_pixels, self.spectral_pivot, self.nside, gamma=gamma, out=out,
                                    accumulate=accumulate)

    def getsky(self):
        """Stokes I of :meth:`getpolsky`: ``[nfreq, npix]`` in K."""
        return _lib.get_context().to_host(self.getsky_device())

    def getpolsky_device(self):
        rm = self._rm_device() if self.faraday else None
        pix, flux, beta, gamma, polw = self._sources()
        sky = paint_sources_device(pix, flux, beta, self.nu_pixels, self.spectral_pivot, self.nside, gamma=gamma, polw=polw,
                                   npol=4)
        if rm is not None:
            _lib.get_context().faraday_rotate(sky, rm, _wavelengths(self.nu_pixels))
        return sky

    def getpolsky(self):
        """``[nfreq, 4, npix]`` in K: the catalogue's sources with their measured polarisation, Faraday rotated when
        ``faraday`` is set (pointsource.py:464-523).  Deterministic."""
        return _lib.get_context().to_host(self.getpolsky_device())


class UnresolvedBackground(gaussianfg.PointSources):
    """``CombinedPointSources._UnresolvedBackground``: Gaussian approximation for S < 0.1 Jy."""

    A = 3.55e-5
    nu_0 = 408.0
    l_0 = 100.0

    oversample = 0


_warned_no_catalogue = False


class CombinedPointSources(maps.Map3d):
    """Full-sky point-source maps from three components (pointsource.py:526-578): a Gaussian realisation below
    0.1 Jy (at 151 MHz), a synthetic population up to 4 Jy at 600 MHz, and real sources above that.

    ``catalogue`` : the real sources (:class:`RealPointSources`); ``None`` leaves that component out, which is said
    once.  ``faraday_map`` : the rotation-measure map, needed by :meth:`getpolsky`.  ``flux_max`` caps the real and
    the synthetic sources.
    """

    flux_max = None

    _UnresolvedBackground = UnresolvedBackground

    class _RandomResolved(DiMatteo):
        flux_min = 0.1
        flux_max = 4.0 * (151.0 / 600.0) ** DiMatteo.spectral_mean     # the 600 MHz cut as a flux at 151 MHz

    class _RealResolved(RealPointSources):
        flux_min = 4.0

    def __init__(self, catalogue=None, faraday_map=None):
        self._catalogue = None if catalogue is None else load_catalogue(catalogue)
        self._faraday = faraday_map

    def _components(self):
        global _warned_no_catalogue
        obj_unresolved = self._UnresolvedBackground.like_map(self)
        obj_random = self._RandomResolved.like_map(self, faraday_map=self._faraday)
        obj_real = None
        if self._catalogue is not None:
            obj_real = self._RealResolved.like_map(self, catalogue=self._catalogue, faraday_map=self._faraday)
        elif not _warned_no_catalogue:
            _warned_no_catalogue = True
            warnings.warn("CombinedPointSources: no catalogue= given, the real sources above 4 Jy are left out")
        if self.flux_max is not None:
            if obj_real is not None:
                obj_real.flux_max = self.flux_max
            if self.flux_max < obj_random.flux_max:
                obj_random.flux_max = self.flux_max
        return obj_unresolved, obj_random, obj_real

    def getsky(self, rng=None):
        """Stokes I of the three components: ``[nfreq, npix]`` in K.  The resolved components are painted onto the
        Gaussian background in accumulate mode.  ``rng`` and the distribution contract as ``PointSourceModel.getsky``."""
        ctx = _lib.get_context()
        obj_unresolved, obj_random, obj_real = self._components()
        ps_all = ctx.to_device(obj_unresolved.getsky(rng=rng))
        obj_random.getsky_device(rng=rng, out=ps_all, accumulate=True)
        if obj_real is not None:
            obj_real.getsky_device(out=ps_all, accumulate=True)
        return ctx.to_host(ps_all)

    def getpolsky(self, rng=None):
        """``[nfreq, 4, npix]`` in K: the sum of the components' polarised maps (pointsource.py:561-578)."""
        ctx = _lib.get_context()
        obj_unresolved, obj_random, obj_real = self._components()
        if self._faraday is None and (obj_random.faraday or (obj_real is not None and obj_real.faraday)):
            obj_random._rm_device()      # raises with the sentence that says what to pass
        ps_all = ctx.to_device(obj_unresolved.getpolsky(rng=rng))
        ps_all += obj_random.getpolsky_device(rng=rng)
        if obj_real is not None:
            ps_all += obj_real.getpolsky_device()
        return ctx.to_host(ps_all)
