#!/usr/bin/env python3
"""Generate tests/golden/pointsource_vectors.npz from the reference's point-source code.

Run in the build container only (needs the reference tree and cython, as make_golden.py does).  The reference's
``cora.foreground.pointsource`` and ``cora.foreground.poisson`` are imported from where they lie, on the stand-ins of
``make_golden._install_shims()`` and the cythonised spline of ``make_golden._build_cython()``, plus, all part of THIS
script:

* ``healpy.ud_grade`` as the identity (the rotation-measure maps below are given at the model's nside),
  ``healpy.ang2pix`` as this package's ``hputil.ang2pix`` and ``healpy.nside2pixarea`` as ``4 pi / npix``;
* the module's ``rnd`` and ``np.random`` replaced by a recorder that hands every call on to numpy's global state and
  keeps what ``rand()`` and ``standard_normal()`` returned: the pixel draws, the spectral indices and the
  polarisation fractions of one ``getpolsky``;
* instances made with ``object.__new__`` and ``_faraday``, ``_catalogue``, ``nside``, ``frequencies`` set by hand
  (``__init__`` loads skydata.npz, which is not in the tree), ``generate_population`` wrapped to keep the fluxes.

Nothing of the reference is copied into the repository: the file holds inputs and outputs only.

* ``<case>_``: one ``getpolsky`` of DiMatteo / PowerLawModel under ``np.random.seed``: ``flux``, ``index``, ``pix`` of
  every source in drawing order, ``q_frac``, ``u_frac``, ``rm``, ``freq``, the model's scalars, and ``sky_pol`` planes
  0 - 2 (plane 3 is asserted zero; plane 0 is the reference's ``getsky`` output, assigned unchanged).
* ``cat_``: catalogue rows (the first 24, and two without polarisation as those 24 have none) as seven arrays, and the reference's cube with
  and without Faraday rotation.
* ``poi_``: ``inhomogeneous_process_approx`` for the DiMatteo rate under a seed: ``av``, ``total``, first / last 64 events.
* ``far_``: ``faraday_rotate`` on a small random cube.

Usage:  python tests/golden/make_golden_pointsource.py
"""
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.dont_write_bytecode = True

import make_golden  # noqa: E402  (tests/golden/make_golden.py: the shims)

REF = make_golden.REF
CAT_FIELDS = ("RA", "DEC", "S600", "P600", "POLANG", "BETA", "GAMMA")


class Recorder:
    """numpy.random with a memory: rand() without arguments and standard_normal() are kept in order."""

    def __init__(self):
        self.rand_values, self.normal_values = [], []

    def rand(self, *shape):
        v = np.random.rand(*shape)
        if not shape:
            self.rand_values.append(v)
        return v

    def standard_normal(self, *a, **k):
        v = np.random.standard_normal(*a, **k)
        self.normal_values.append(v)
        return v

    def __getattr__(self, name):
        return getattr(np.random, name)


class NumpyWithRecorder:
    def __init__(self, recorder):
        self.random = recorder

    def __getattr__(self, name):
        return getattr(np, name)


def _load_reference():
    from cora_amd.util import hputil

    make_golden._install_shims()
    sys.path.insert(0, REF)
    make_golden._build_cython(tempfile.mkdtemp())
    hp = sys.modules["healpy"]
    hp.ud_grade = lambda m, *a, **k: m
    hp.ang2pix = lambda nside, theta, phi: hputil.ang2pix(nside, theta, phi)
    hp.nside2pixarea = lambda nside: 4 * np.pi / (12 * nside * nside)
    from cora.foreground import pointsource, poisson

    return pointsource, poisson


def model_case(ps, cls, seed, nside, nfreq, flux_min, flux_max, rng):
    rec = Recorder()
    ps.rnd, ps.np = rec, NumpyWithRecorder(rec)
    try:
        npix = 12 * nside * nside
        freq = np.linspace(400.0, 800.0, nfreq)
        obj = object.__new__(cls)
        obj.nside, obj.frequencies = nside, freq
        obj.flux_min, obj.flux_max = flux_min, flux_max
        obj._faraday = rng.uniform(-2000.0, 2000.0, npix)
        kept = {}
        generate = obj.generate_population

        def generate_population(area):
            kept["flux"] = generate(area)
            return kept["flux"]

        obj.generate_population = generate_population
        np.random.seed(seed)
        sky_pol = obj.getpolsky()
    finally:
        ps.rnd, ps.np = np.random, np
    flux = kept["flux"]
    n = len(flux)
    z, q, u = rec.normal_values
    assert z.shape == (n, 1) and q.shape == u.shape == (npix,) and len(rec.rand_values) == n
    index = (obj.spectral_mean + obj.spectral_width * z)[:, 0]
    pix = np.array([int(v * npix) for v in rec.rand_values], dtype=np.int64)
    assert sky_pol.shape == (nfreq, 4, npix) and not sky_pol[:, 3].any() and np.all(np.isfinite(sky_pol))
    print("%s nside %d: %d sources, %d channels" % (cls.__name__, nside, n, nfreq))
    return dict(flux=flux, index=index, pix=pix, q_frac=obj.sigma_pol_frac * q, u_frac=obj.sigma_pol_frac * u,
                rm=obj._faraday, freq=freq, nside=nside, flux_min=flux_min, spectral_pivot=obj.spectral_pivot,
                spectral_mean=obj.spectral_mean, spectral_width=obj.spectral_width, sigma_pol_frac=obj.sigma_pol_frac,
                sky_pol=np.ascontiguousarray(sky_pol[:, :3]))


def catalogue_case(ps, rng):
    with open(os.path.join(REF, "cora/foreground/data/combinedps.dat"), "r") as f:
        cat = np.genfromtxt(f, names=True)
    nan = np.flatnonzero(np.isnan(cat["P600"]) | np.isnan(cat["POLANG"]))
    rows = np.arange(24)
    if not (nan < 24).any():
        rows = np.concatenate([rows, nan[:2]])
    cat = cat[rows]
    assert np.isnan(cat["POLANG"]).sum() >= 1
    nside, nfreq = 4, 5
    freq = np.linspace(400.0, 800.0, nfreq)
    out = {k: np.array(cat[k], dtype=np.float64) for k in CAT_FIELDS}
    out.update(freq=freq, nside=nside, flux_min=1.0, rm=rng.uniform(-2000.0, 2000.0, 12 * nside * nside))
    for key, faraday in (("cube", False), ("cube_rot", True)):
        obj = object.__new__(ps.RealPointSources)
        obj.nside, obj.frequencies = nside, freq
        obj._catalogue, obj._faraday = cat, out["rm"]
        obj.flux_min, obj.faraday = 1.0, faraday
        cube = obj.getpolsky()
        assert len(obj._masked_catalogue) == len(cat) and cube.shape == (nfreq, 4, 12 * nside * nside) and not cube[:, 3].any()
        out[key] = np.ascontiguousarray(cube[:, :3])
    return out


def poisson_case(ps, poi):
    from scipy.integrate import quad

    obj = object.__new__(ps.DiMatteo)
    flux_min, flux_max, area = 0.5, 300.0, 4 * np.pi
    t = np.log(flux_max / flux_min)

    def rate(s):
        return flux_min * np.exp(s) * area * obj.source_count(flux_min * np.exp(s))

    np.random.seed(777)
    events = poi.inhomogeneous_process_approx(t, rate)
    return dict(flux_min=flux_min, flux_max=flux_max, area=area, seed=777, av=quad(rate, 0.0, t)[0], total=len(events),
                first=events[:64].copy(), last=events[-64:].copy())


def faraday_case(ps, rng):
    nfreq, npix = 3, 48
    cube = rng.normal(size=(nfreq, 4, npix))
    rm = rng.uniform(-2000.0, 2000.0, npix)
    freq = np.array([400.0, 612.5, 800.0])
    return dict(cube=cube, rm=rm, freq=freq, rotated=ps.faraday_rotate(cube.copy(), rm, freq))


def main():
    ps, poi = _load_reference()
    rng = np.random.default_rng(20261018)
    g = {}
    cases = (("dm4", ps.DiMatteo, 11, 4, 3, 5.0, None), ("dm8", ps.DiMatteo, 12, 8, 17, 1.5, None),
             ("pl4", ps.PowerLawModel, 13, 4, 17, 10.0, 200.0), ("pl8", ps.PowerLawModel, 14, 8, 3, 4.0, None))
    for prefix, cls, seed, nside, nfreq, fmin, fmax in cases:
        for k, v in model_case(ps, cls, seed, nside, nfreq, fmin, fmax, rng).items():
            g["%s_%s" % (prefix, k)] = v
    for prefix, case in (("cat", catalogue_case(ps, rng)), ("poi", poisson_case(ps, poi)), ("far", faraday_case(ps, rng))):
        for k, v in case.items():
            g["%s_%s" % (prefix, k)] = v
    path = os.path.join(HERE, "pointsource_vectors.npz")
    np.savez_compressed(path, **g)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))
    assert os.path.getsize(path) < 900 * 1024


if __name__ == "__main__":
    main()
