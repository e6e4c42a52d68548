#!/usr/bin/env python3
"""Generate tests/golden/galaxy_vectors.npz from the reference's map_variance and ConstrainedGalaxy.getsky.

Run in the build container only (needs the reference tree, as make_golden.py does).  The reference's
cora/foreground/galaxy.py is loaded by path, the way make_golden_faraday.py loads it, and its own ``map_variance`` and
``getsky(debug=True, celestial=False)`` run under the stand-ins of ``make_golden._install_shims()`` plus, all part of
THIS script:

* empty modules for ``cora`` and its sub-packages with ``Sky3d`` / ``Synchrotron`` placeholder classes (base classes
  only; nothing of them runs);
* ``healpy.smoothing`` and ``healpy.ud_grade`` as the identity, ``healpy.get_nside`` from the pixel count and
  ``healpy.reorder`` from the numpy permutation of tests/_galaxy_oracle.py;
* ``skysim.clarray`` returning None and ``skysim.mkfullsky`` / ``skysim.mkconstrained`` returning stored ``fg`` / ``fgs``;
* the instance made with ``object.__new__`` and ``_haslam``, ``_sp_ind``, ``_amp_map``, ``nside``, ``nu_pixels`` set by
  hand (``__init__`` loads skydata.npz, which is not in the tree).

Nothing of the reference is copied into the repository.  Stored: for ``map_variance`` the cases ``v0_`` (nside 4 -> 1),
``v1_`` (8 -> 2), ``v2_`` (32 -> 16): ``map_q`` (small integers; the map is ``offset + map_q q``, exact in float64) and
the reference's ``var``; for ``getsky`` at nside 32 with two output channels the shared inputs ``in_fg_q``, ``in_fgs_q``,
``in_haslam_q``, ``in_am_q`` (integers; the float64 value is the integer times the power of two ``in_*_s``), ``in_freq``,
and per case (``md_``, ``gsm_``) the spectral-index map ``sc_q`` (times ``sc_s``) and the reference's ``fgt`` and ``mv`` in
full precision.

Usage:  python tests/golden/make_golden_galaxy.py
"""
import importlib.util
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.dont_write_bytecode = True

import make_golden  # noqa: E402  (tests/golden/make_golden.py: the shims)
import _galaxy_oracle as go  # noqa: E402

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
    sys.modules["cora.foreground.gaussianfg"].Synchrotron = type("Synchrotron", (object,), {"angular_powerspectrum": None})
    hp = sys.modules["healpy"]
    hp.smoothing = lambda m, *a, **k: m
    hp.ud_grade = lambda m, *a, **k: m
    hp.get_nside = lambda m: int(round((np.shape(m)[-1] / 12) ** 0.5))

    def reorder(m, r2n=None, n2r=None):
        assert bool(r2n) != bool(n2r)
        return go.reorder(np.asarray(m), bool(r2n))

    hp.reorder = reorder
    sk = sys.modules["cora.core.skysim"]
    sk.clarray = lambda *a, **k: None
    sk.mkfullsky = lambda cla, nside: state["fg"].copy()

    def mkconstrained(cla, constraints, nside):
        state["nconstraints"] = len(constraints)
        return state["fgs"].copy()

    sk.mkconstrained = mkconstrained
    spec = importlib.util.spec_from_file_location("cora.foreground.galaxy", os.path.join(REF, "cora/foreground/galaxy.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def variance_case(gal, rng, nside_in, nside_out, offset):
    map_q = rng.integers(-200, 201, 12 * nside_in * nside_in).astype(np.int16)
    var = gal.map_variance(offset + map_q * Q, nside_out)
    assert var.shape == (12 * nside_out * nside_out,)
    return dict(map_q=map_q, offset=offset, nside_out=nside_out, var=var)


def getsky_inputs(rng):
    """Inputs shared by the two getsky cases, as small integers times a power of two (``*_s`` the scale).  Rows 0, 1 of
    ``fgs`` and row 1 of ``fg`` do not reach the output (getsky drops the two constraint channels; row 0 of ``fg`` sets
    ``mv``): zeros."""
    nside, nfreq = 32, 2
    npix = 12 * nside * nside
    fg_q = np.rint(rng.normal(0.0, 6.0, (nfreq + 2, npix)) * 4).astype(np.int16)
    fgs_q = np.rint(rng.normal(0.0, 3.0, (nfreq + 2, npix)) * 4).astype(np.int16)
    fg_q[0] = rng.integers(-8, 9, npix)
    fg_q[1], fgs_q[:2] = 0, 0
    # a few pixels at x = 0 exactly (fg == fgs)
    fgs_q[2:, :16] = fg_q[2:, :16]
    return dict(nside=nside, freq=np.array([400.0, 800.0]), fg_q=fg_q, fg_s=2.0 ** -2, fgs_q=fgs_q, fgs_s=2.0 ** -2,
                haslam_q=rng.integers(5, 37, npix).astype(np.uint8), haslam_s=2.0,
                am_q=rng.integers(1, 33, npix).astype(np.uint8), am_s=2.0 ** -2)


def getsky_case(gal, state, rng, inp, spectral_map):
    npix = 12 * inp["nside"] ** 2
    sc_q = rng.integers(-28, -15, npix).astype(np.int8)             # -3.5 .. -2 in steps of 2^-3
    state["fg"], state["fgs"] = inp["fg_q"] * inp["fg_s"], inp["fgs_q"] * inp["fgs_s"]
    obj = object.__new__(gal.ConstrainedGalaxy)
    obj.spectral_map = spectral_map
    obj._haslam, obj._amp_map = inp["haslam_q"] * inp["haslam_s"], inp["am_q"] * inp["am_s"]
    obj._sp_ind = {spectral_map: sc_q * 2.0 ** -3}
    obj.nside, obj.nu_pixels = inp["nside"], inp["freq"]
    fgt, fg, fgs, fgsmooth, am, mv = obj.getsky(debug=True, celestial=False)
    assert state["nconstraints"] == (2 if spectral_map == "gsm" else 1)
    assert fgt.shape == (2, npix) and np.all(np.isfinite(fgt)) and np.all(fgt >= 0) and mv > 0
    assert np.array_equal(fg, state["fg"]) and np.array_equal(fgs, state["fgs"]) and np.array_equal(am, obj._amp_map)
    assert (fg[2:] < fgs[2:]).mean() > 0.3 and (fg[2:] > fgs[2:]).mean() > 0.3          # both branches of tanh_lin
    return dict(sc_q=sc_q, sc_s=2.0 ** -3, fgt=fgt, mv=mv)


def main():
    state = {}
    gal = _load_galaxy(state)
    rng = np.random.default_rng(20261018)
    g = dict(q=Q)
    for prefix, (ni, no, off) in (("v0_", (4, 1, 0.0)), ("v1_", (8, 2, 1024.0)), ("v2_", (32, 16, 0.0))):
        for k, v in variance_case(gal, rng, ni, no, off).items():
            g[prefix + k] = v
    inp = getsky_inputs(rng)
    for k, v in inp.items():
        g["in_" + k] = v
    for name in ("md", "gsm"):
        for k, v in getsky_case(gal, state, rng, inp, name).items():
            g[name + "_" + k] = v
    path = os.path.join(HERE, "galaxy_vectors.npz")
    np.savez_compressed(path, **g)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))
    assert os.path.getsize(path) < 500 * 1024


if __name__ == "__main__":
    main()
