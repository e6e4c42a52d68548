#!/usr/bin/env python3
"""Generate tests/golden/faraday_vectors.npz from the reference's ConstrainedGalaxy.getpolsky.

Run in the build container only (needs the reference tree, as make_golden.py does).  The reference's
cora/foreground/galaxy.py is loaded by path and its own ``getpolsky(debug=True, celestial=False)`` runs, under the
stand-ins of ``make_golden._install_shims()`` plus, all part of THIS script:

* empty modules for ``cora``, ``cora.core``, ``cora.util``, ``cora.foreground``, ``cora.core.maps``,
  ``cora.core.skysim``, ``cora.util.hputil`` and ``cora.foreground.gaussianfg``, with ``Sky3d`` / ``Synchrotron``
  placeholder classes (base classes only; nothing of them runs);
* ``healpy.smoothing`` and ``healpy.ud_grade`` as the identity, so that ``sigma_phi = |_faraday|``;
* ``hputil.sphtrans_inv_complex`` returning successive columns of a stored ``base`` (the spherical harmonic synthesis
  is not available here; the random a_lm the reference draws are ignored);
* ``getsky`` returning a stored ``T``;
* the instance made with ``object.__new__`` and ``_dphi``, ``_maxphi``, ``_faraday``, ``nside``, ``nu_pixels``,
  ``nu_num`` set by hand (``__init__`` loads skydata.npz, which is not in the tree).

Nothing of the reference is copied into the repository.  Stored per case (prefix ``a_``: nphi 32, ``b_``: nphi 6):
the inputs ``base_q`` (real, imaginary) / ``T_q`` / ``faraday_q`` as small integers (their float64 values are the
integers times ``q`` = 2^-10, exact), ``freq``, ``dphi``, ``maxphi``, ``nside``, and the reference's ``map2``, ``map4``,
``w``, ``sigma_phi``, ``pta``, ``map5``.

Usage:  python tests/golden/make_golden_faraday.py
"""
import importlib.util
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.dont_write_bytecode = True

import make_golden  # noqa: E402  (tests/golden/make_golden.py: the shims)

REF = make_golden.REF
Q = 2.0 ** -10


def _load_galaxy(state):
    make_golden._install_shims()
    for name in ("cora", "cora.core", "cora.util", "cora.foreground", "cora.core.maps", "cora.core.skysim",
                 "cora.util.hputil", "cora.foreground.gaussianfg"):
        mod = types.ModuleType(name)
        mod.__path__ = []
        sys.modules[name] = mod
        parent, _, leaf = name.rpartition(".")
        if parent:
            setattr(sys.modules[parent], leaf, mod)
    sys.modules["cora.core.maps"].Sky3d = type("Sky3d", (object,), {})
    sys.modules["cora.foreground.gaussianfg"].Synchrotron = type("Synchrotron", (object,), {})
    hp = sys.modules["healpy"]
    hp.smoothing = lambda m, *a, **k: m
    hp.ud_grade = lambda m, *a, **k: m

    def sphtrans_inv_complex(alm, nside):
        col = state["base"][:, state["next"]]
        state["next"] += 1
        return col

    sys.modules["cora.util.hputil"].sphtrans_inv_complex = sphtrans_inv_complex
    spec = importlib.util.spec_from_file_location("cora.foreground.galaxy", os.path.join(REF, "cora/foreground/galaxy.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def case(gal, state, rng, nside, maxphi, nfreq):
    npix = 12 * nside * nside
    nphi = 2 * int(maxphi / 1.0)
    base_q = np.rint(rng.normal(0.0, 1.0, (2, npix, nphi)) / Q).astype(np.int32)
    T_q = np.rint(rng.uniform(2.0, 30.0, (nfreq, npix)) / Q).astype(np.int32)
    # widths from well inside one depth bin to wider than the grid, either sign (the reference takes |.|)
    far_q = np.rint(np.exp(rng.uniform(np.log(0.2), np.log(3.0 * maxphi), npix)) / Q).astype(np.int32)
    far_q *= rng.choice([-1, 1], npix).astype(np.int32)
    freq = 400.0 + 2.0 * np.arange(nfreq)

    state["base"] = base_q[0] * Q + 1.0j * (base_q[1] * Q)
    state["next"] = 0
    T = T_q * Q
    obj = object.__new__(gal.ConstrainedGalaxy)
    obj._dphi, obj._maxphi = 1.0, float(maxphi)
    obj._faraday = far_q * Q
    obj.nside, obj.nu_pixels, obj.nu_num = nside, freq, nfreq
    obj.getsky = lambda debug=False, celestial=True: T.copy()
    map2, map4, w, sigma_phi, pta, map5 = obj.getpolsky(debug=True, celestial=False)
    assert state["next"] == nphi and map2.shape == (npix, nphi) and map5.shape == (nfreq, 4, npix)
    assert np.all(np.isfinite(map5))
    return dict(base_q=base_q, T_q=T_q, faraday_q=far_q, freq=freq, dphi=1.0, maxphi=float(maxphi), nside=nside,
                map2=map2, map4=map4, w=w, sigma_phi=sigma_phi, pta=pta, map5=map5)


def main():
    state = {}
    gal = _load_galaxy(state)
    rng = np.random.default_rng(20261018)
    g = dict(q=Q)
    for prefix, (nside, maxphi, nfreq) in (("a_", (2, 16, 5)), ("b_", (2, 3, 3))):
        for k, v in case(gal, state, rng, nside, maxphi, nfreq).items():
            g[prefix + k] = v
    path = os.path.join(HERE, "faraday_vectors.npz")
    np.savez_compressed(path, **g)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))
    assert os.path.getsize(path) < 400 * 1024


if __name__ == "__main__":
    main()
