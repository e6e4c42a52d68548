#!/usr/bin/env python3
"""Golden vectors for the LOFAR synchrotron model: outputs of the reference's own ``LofarGDSE.getfield``
(cora/foreground/lofar.py:49-73), obtained by importing the reference in this container with the stand-ins of
make_golden.py (caput constants / mpiarray, healpy stub) plus empty stand-ins for the two Cython modules that
``cora.foreground`` imports but this path does not use (as make_golden_flatsky.py does).  Randomness: numpy's GLOBAL
state seeded with ``np.random.seed(7)`` - the reference draws from it (gaussianfield.py:115).

``getfield`` builds ``_LofarGDSE_3D(npix=list, wsize=list)``, whose ``npix != None`` test (gaussianfield.py:30) is
fine for a list, but the arrays made from them then meet ``self._n == None`` (gaussianfield.py:34), which current
numpy refuses to reduce to a truth value: the class is wrapped so that ``_n`` and ``_w`` are the ``LegacyArray`` of
make_golden_flatsky.py.  The same wrapper keeps the raw fields each ``getfield`` returns (A, then beta), which the
tests need for the error propagation.  No reference code is changed.

Per case: ``<tag>__Tb`` [nu_num, x_num, y_num], ``<tag>__A`` and ``<tag>__beta`` (the raw fields, beta absent when
correlated), ``<tag>__params`` = (nu_num, x_num, y_num, x_width, y_width, nu_lower, nu_upper, correlated).  ``attrs``:
the class attributes (nu_0, correlated, A_amp, A_std, beta_mean, beta_std, alpha, delta of the 3-d field class).

Commits data only: tests/golden/lofar_vectors.npz.      python tests/golden/make_golden_lofar.py
"""
import os
import sys
import types

import numpy as np

OUT = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, OUT)
import make_golden  # noqa: E402  (shims only)
from make_golden_flatsky import legacy  # noqa: E402

CASES = (
    ("c5_12_9", dict(nu_num=5, x_num=12, y_num=9, x_width=5.0, y_width=4.0, nu_lower=120.0, nu_upper=200.0), False),
    ("c5_12_9_corr", dict(nu_num=5, x_num=12, y_num=9, x_width=5.0, y_width=4.0, nu_lower=120.0, nu_upper=200.0), True),
    ("c3_8_7", dict(nu_num=3, x_num=8, y_num=7), False),           # numz = 7: field depth 6
    ("c4_6_6", dict(nu_num=4, x_num=6, y_num=6, nu_lower=300.0, nu_upper=350.0), False),   # channels straddle nu_0 = 325
)
ATTRS = ("nu_0", "correlated", "A_amp", "A_std", "beta_mean", "beta_std", "alpha")


def main():
    make_golden._install_shims()
    for name in ("cora.util.cubicspline", "cora.util.bilinearmap"):
        sys.modules[name] = types.ModuleType(name)
    sys.path.insert(0, make_golden.REF)
    import cora.util as cu

    cu.cubicspline = sys.modules["cora.util.cubicspline"]
    cu.bilinearmap = sys.modules["cora.util.bilinearmap"]
    from cora.foreground import lofar

    base = lofar._LofarGDSE_3D
    drawn = []

    class LegacyArgsField(base):
        def __init__(self, npix=None, wsize=None):
            base.__init__(self, npix=npix, wsize=wsize)
            self._n, self._w = legacy(self._n), legacy(self._w)

        def getfield(self):
            f = base.getfield(self)
            drawn.append(f.copy())
            return f

    g = {"attrs": np.array([float(getattr(lofar.LofarGDSE, a)) for a in ATTRS] + [float(base.delta)])}
    lofar._LofarGDSE_3D = LegacyArgsField
    try:
        for tag, kw, corr in CASES:
            m = lofar.LofarGDSE()
            for k, v in kw.items():
                setattr(m, k, v)
            m.correlated = corr
            del drawn[:]
            np.random.seed(7)
            with np.errstate(divide="ignore"):
                g[tag + "__Tb"] = m.getfield()
            assert len(drawn) == (1 if corr else 2)
            g[tag + "__A"] = drawn[0]
            if not corr:
                g[tag + "__beta"] = drawn[1]
            g[tag + "__params"] = np.array([m.nu_num, m.x_num, m.y_num, m.x_width, m.y_width, m.nu_lower, m.nu_upper,
                                            float(corr)], dtype=np.float64)
    finally:
        lofar._LofarGDSE_3D = base

    path = os.path.join(OUT, "lofar_vectors.npz")
    np.savez_compressed(path, **g)
    print("wrote", path, len(g), "arrays", {k: v.shape for k, v in g.items()})


if __name__ == "__main__":
    main()
