#!/usr/bin/env python3
"""Golden vectors for the redshift-space correlation functions (cora/signal/corr.py:114-446, corr21cm.py:278-310):
outputs of the reference's own ``redshiftspace_correlation``, ``angular_correlation``, ``powerspectrum`` and
``powerspectrum_1D``, obtained by importing the reference with the shims and the Cython build of make_golden.py.

Stored (arrays only):
  table            the 1000 x 4 multipole table the reference's Corr21cm loads (data its program reads)
  table7           the same with three made-up columns dd0, dv0, dv2: smooth in r, small integers / 4096
  pi, sigma        the evaluation points (see ``points``), and per object x redshift form the reference's result, one
                   scalar call per point: with array arguments a vv-only object of the reference scales xdd_0, xdv_0 and
                   xvv_0 in place although they are one array (corr.py:291-326), so every one of them ends up times
                   b1 b2 (b1 f2 + b2 f1) / 2 f1 f2; scalars are not aliased and give the formula of its docstring
  theta, ang_*     angular_correlation(theta[16], 0.8, 1.1)
  kpar, kperp, ps_*  powerspectrum on a 7 x 5 grid: the vv-only, the three-spectrum and the ps_2d object (spectra restated
                   in tests/_rsdcorr_oracle.py: ``ps_vv``, ``ps_dd``, ``ps_dv``, ``ps_vv2d``)
  k1d, ps1d        powerspectrum_1D of the 21cm model

    python tests/golden/make_golden_rsdcorr.py
"""
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.dont_write_bytecode = True

import make_golden as mg  # noqa: E402
import _rsdcorr_oracle as ro  # noqa: E402

ZFORMS = (("none", None, None), ("z1", 0.8, None), ("z12", 0.8, 1.1))


def extra_columns(r):
    """dd0, dv0, dv2 of the 7-column file: smooth functions of r rounded to multiples of 1 / 4096."""
    lr = np.log10(r)
    cols = (3.0 / (1.0 + (r / 7.0) ** 2), 2.0 * np.cos(lr) / (1.0 + r / 50.0), -1.5 * lr / (1.0 + lr**2))
    return [np.round(c * 4096.0) / 4096.0 for c in cols]


def points(knots):
    """About 200 (pi, sigma) pairs, exact binary fractions: the origin, either component zero, negative pi, r below the
    first and above the last knot, r on a knot and one ulp to either side of it, and a spread of ordinary separations."""
    pi, sg = [0.0, 0.0, 0.0, 2.0**-14, -(2.0**-14), 0.0, 2.0**-15, 20480.0, -20480.0, 0.0, 16384.0],\
             [0.0, 2.0**-14, 2.0**-16, 0.0, 0.0, 2.0**-10, 2.0**-15, 0.0, 0.0, 20480.0, 16384.0]
    for j in (0, 1, 2, 333, 500, 998, 999):
        for x in (knots[j], np.nextafter(knots[j], 0.0), np.nextafter(knots[j], np.inf)):
            pi += [x, -x, 0.0]
            sg += [0.0, 0.0, x]
    rng = np.random.default_rng(20261020)
    m = 200 - len(pi)
    rr = 2.0 ** rng.uniform(-9, 13, m)
    ang = rng.uniform(0, np.pi, m)
    pi += list(np.round(rr * np.cos(ang) * 2.0**12) / 2.0**12)
    sg += list(np.round(rr * np.sin(ang) * 2.0**12) / 2.0**12)
    return np.array(pi), np.array(sg)


def main():
    mg._install_shims()
    sys.path.insert(0, mg.REF)
    tmp = tempfile.mkdtemp(prefix="cora_golden_")
    mg._build_cython(tmp)
    from cora.signal import corr, corr21cm

    g = {}
    table = np.loadtxt(os.path.join(mg.REF, "cora", "signal", "data", "corr_z1.5.dat"))
    assert table.shape == (1000, 4)
    g["table"] = table
    table7 = np.column_stack([table] + extra_columns(table[:, 0]))
    g["table7"] = table7
    f4, f7 = os.path.join(tmp, "t4.dat"), os.path.join(tmp, "t7.dat")
    np.savetxt(f4, table)
    np.savetxt(f7, table7)
    assert np.array_equal(np.loadtxt(f4), table) and np.array_equal(np.loadtxt(f7), table7)

    objs = {"c21": corr21cm.Corr21cm(),
            "mps": corr.RedshiftCorrelation.from_file_matterps(f4, redshift=1.5, bias=2.0),
            "fps": corr.RedshiftCorrelation.from_file_fullps(f7, redshift=1.5)}
    pi, sg = points(table[:, 0])
    g["pi"], g["sigma"] = pi, sg
    for name, o in objs.items():
        for tag, z1, z2 in ZFORMS:
            g["xi_%s_%s" % (name, tag)] = np.array([o.redshiftspace_correlation(float(a), float(b), z1, z2) for a, b in zip(pi, sg)])

    theta = np.arange(16) / 1024.0
    g["theta"] = theta
    for name in ("c21", "fps"):
        g["ang_" + name] = np.array([objs[name].angular_correlation(float(t), 0.8, 1.1) for t in theta])

    kpar = np.array([0.0, 0.015625, 0.0625, 0.25, 1.0, 2.5, 8.0])[:, None]
    kperp = np.array([0.0078125, 0.03125, 0.125, 0.75, 4.0])[None, :]
    g["kpar"], g["kperp"] = kpar, kperp
    vv = corr.RedshiftCorrelation(ps_vv=ro.ps_vv, redshift=1.5, bias=2.0)
    full = corr.RedshiftCorrelation(ps_vv=ro.ps_vv, ps_dd=ro.ps_dd, ps_dv=ro.ps_dv, redshift=1.5)
    two = corr.RedshiftCorrelation(ps_vv=ro.ps_vv2d, redshift=1.5, bias=2.0)
    two.ps_2d = True
    for name, o in (("vv", vv), ("full", full), ("2d", two)):
        for tag, z1, z2 in (("none", None, None), ("z12", 0.8, 1.1)):
            g["ps_%s_%s" % (name, tag)] = np.asarray(o.powerspectrum(kpar, kperp, z1, z2))

    k1d = 2.0 ** np.arange(-8, 3, dtype=np.float64)
    g["k1d"] = k1d
    g["ps1d"] = np.asarray(objs["c21"].powerspectrum_1D(k1d, 0.8, 1.1, 16))

    path = os.path.join(HERE, "rsdcorr_vectors.npz")
    np.savez_compressed(path, **g)
    print("wrote", path, {k: v.shape for k, v in g.items()}, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
