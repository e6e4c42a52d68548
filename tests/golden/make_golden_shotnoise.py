#!/usr/bin/env python3
"""Generate tests/golden/shotnoise_vectors.npz from the reference's cora/signal/lssmodels.py, cora/util/cosmology.py and
cora/signal/lssutil.py.

Run in the build container only (needs the reference tree, as make_golden.py does).  The reference modules are loaded
by path with the stand-ins of ``make_golden._install_shims()`` plus empty modules for ``caput.algorithms``,
``caput.config``, ``cora.util.cubicspline`` and ``cora.util.hputil`` (untouched by what runs here); the stand-in for
``caput.astro.constants`` gets ``G`` and ``solar_mass`` set to this project's values (cora_amd/util/constants.py:
caput itself is not available to compare with).  Nothing of the reference is copied into the repository.

Stored (inputs as small integers times 2^-10, so that their float64 values are exact):
  z_q                               a 16-point redshift grid
  bias__* omega_HI__* sigma_P__*    every model of the three sets on that grid
  T_b__*                            mean_21cm_temperature with each omega_HI model
  n_eff__*                          log_M_HI_g_to_n_eff(log_M_HI_g = 9.5) with each omega_HI model
  growth_factor, growth_rate, H, chi    of the reference's default Cosmology
  dVdz                              differential_comoving_volume (lss.py:1584-1589 written out: that module needs caput's pipeline)
  chi6_q, z6_q, sn_std_scalar / sn_std_slices / sn_std_mass     AddCorrelatedShotNoise.process's std (lss.py:1289-1296
                                    written out with the reference's calculate_width) at nside 4 for a non-uniform 6-slice chi:
                                    n_eff = 2^-9, a per-slice n_eff, and log_M_HI_g = 9.5 at redshifts z6
  freq5, voxvol_fixed, voxvol_freq, central_redshift           GenerateFlatSpectrumMap.process's voxel volume (lss.py:1500-1516
                                    written out) at nside 4 for 5 channels, both settings of use_freq_dependent_voxel_volume

Usage:  python tests/golden/make_golden_shotnoise.py
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
ROOT = os.path.dirname(os.path.dirname(HERE))
Q = 2.0 ** -10
LOG_M = 9.5
NSIDE = 4


def _by_path(name, rel):
    spec = importlib.util.spec_from_file_location(name, os.path.join(REF, rel))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def _load():
    make_golden._install_shims()
    sys.path.insert(0, ROOT)
    from cora_amd.util import constants as ours

    const = sys.modules["caput.astro.constants"]
    const.G = ours.G
    const.solar_mass = ours.solar_mass
    for name in ("caput.algorithms", "caput.config", "cora.util.cubicspline", "cora.util.hputil"):
        mod = types.ModuleType(name)
        sys.modules[name] = mod
        parent, _, leaf = name.rpartition(".")
        if parent in sys.modules:
            setattr(sys.modules[parent], leaf, mod)
    sys.path.insert(0, REF)
    cosmology = _by_path("cora.util.cosmology", "cora/util/cosmology.py")
    lssutil = _by_path("cora.signal.lssutil", "cora/signal/lssutil.py")
    lssmodels = _by_path("cora.signal.lssmodels", "cora/signal/lssmodels.py")
    return cosmology, lssutil, lssmodels, const


def main():
    cosmology, lu, lm, const = _load()
    c = cosmology.Cosmology()
    g = dict(q=Q, log_M_HI_g=LOG_M, nside=NSIDE)

    z_q = (205 + 160 * np.arange(16) + np.array([0, 3, -7, 11, 2, -5, 9, 1, -4, 6, -2, 8, -9, 5, 7, -3])).astype(np.int64)
    z = z_q * Q                                                  # 0.2 .. 2.54
    g["z_q"] = z_q
    for cls in (lm.bias, lm.omega_HI, lm.sigma_P):
        for name in cls.models():
            g["%s__%s" % (cls.__name__, name)] = cls.evaluate(z, model=name)
    for name in lm.omega_HI.models():
        g["T_b__" + name] = lm.mean_21cm_temperature(c, z, lm.omega_HI.evaluate(z, model=name))
        g["n_eff__" + name] = lm.log_M_HI_g_to_n_eff(LOG_M, c, z, name)
    g["n_eff__default"] = lm.log_M_HI_g_to_n_eff(LOG_M, c, z)
    g["growth_factor"] = c.growth_factor(z)
    g["growth_factor_0"] = c.growth_factor(0)
    g["growth_rate"] = c.growth_rate(z)
    g["H"] = c.H(z)
    g["chi"] = c.comoving_distance(z)

    def dcv(zz):                                                 # lss.py:1584-1589
        H_z = c.H(zz) * (c._unit_distance / 1000.0)
        dm = c.comoving_distance(zz)
        return dm**2 * (const.c / 1e3) / H_z

    g["dVdz"] = dcv(z)

    # AddCorrelatedShotNoise.process, lss.py:1289-1296
    chi6_q = np.array([1843200, 1848100, 1853900, 1858300, 1864000, 1869700], dtype=np.int64)     # ~1800 + 5 i, jittered
    z6_q = np.array([620, 622, 625, 627, 630, 633], dtype=np.int64)
    ne6_q = np.array([2, 3, 2, 5, 4, 3], dtype=np.int64)                                          # times 2^-10
    g.update(chi6_q=chi6_q, z6_q=z6_q, ne6_q=ne6_q)
    ichi, z6 = chi6_q * Q, z6_q * Q
    pixarea = 4 * np.pi / (12 * NSIDE * NSIDE)                   # healpy.nside2pixarea
    volume = pixarea * (ichi**2) * lu.calculate_width(ichi)
    g["sn_std_scalar"] = (volume * (np.ones_like(ichi) * 2.0 ** -9)) ** -0.5
    g["sn_std_slices"] = (volume * (ne6_q * Q)) ** -0.5
    g["n_eff6_mass"] = lm.log_M_HI_g_to_n_eff(LOG_M, c, z6, "Crighton2015")
    g["sn_std_mass"] = (volume * g["n_eff6_mass"]) ** -0.5

    # GenerateFlatSpectrumMap.process, lss.py:1500-1516
    freq = np.array([600.0, 596.0, 592.0, 588.0, 584.0])
    g["freq5"] = freq
    redshift = const.nu21 / freq - 1
    ref_chan = int(len(freq) / 2.0)
    omega = pixarea
    dV = dcv(redshift)
    dz = lu.calculate_width(redshift)
    g["voxvol_freq"] = dV * dz * omega
    dV = dcv(redshift[ref_chan])
    dz = redshift[ref_chan + 1] - redshift[ref_chan]
    g["voxvol_fixed"] = dV * dz * omega
    g["central_redshift"] = redshift[ref_chan]

    path = os.path.join(HERE, "shotnoise_vectors.npz")
    np.savez_compressed(path, **g)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))
    assert os.path.getsize(path) < 200 * 1024


if __name__ == "__main__":
    main()
