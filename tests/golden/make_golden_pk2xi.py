#!/usr/bin/env python3
"""Golden vectors for P(k) -> xi(r) (cora/signal/corrfunc.py:19-264, lssutil.py:264-290): outputs of the reference's own
``richardson``, ``_corr_direct``, ``ps_to_corr`` and ``lssutil.cutoff``, obtained by importing the reference in this
container with the stand-ins of make_golden_corrfunc.py, plus

  hankl.P2xi                   - ``hankl`` is an absent dependency: ``P2xi(k, P, 0, lowring=False)`` IS used by
                                 ``_corr_hankl_richardson`` and is restated by ``P2xi`` of tests/_pk2xi_oracle.py (f = P k^1.5,
                                 mu = 1/2, q = 0, r_j = 1 / k_{N-1-j}, xi = g (2 pi)^-1.5 r^-1.5).  The ``ps_to_corr`` run
                                 therefore pins the reference's grids, padding, decimation, trimming, Richardson table and
                                 concatenation, and its direct part; the FFTLog values themselves are UNPINNED (the analytic
                                 pair of tests/test_pk2xi_host.py holds them instead).
  healpy, caput.algorithms / .config, cora.util.cubicspline / .hputil
                               - imported at the top of lssutil.py, not used by ``cutoff``.

Commits data only: tests/golden/pk2xi_vectors.npz (a few hundred values).
    python tests/golden/make_golden_pk2xi.py [REFERENCE_ROOT]
"""
import importlib.util
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.dont_write_bytecode = True

import make_golden_corrfunc as mgc  # noqa: E402  (the shims)
import _pk2xi_oracle as po  # noqa: E402

REF = mgc.REF

PS_TO_CORR = dict(minlogr=-1, maxlogr=3, switchlogr=1, samples_per_decade=10, richardson_n=3, pad_low=2, pad_high=2)


def ps_model(k):
    """The test spectrum (restated in tests/_pk2xi_oracle.py as ``pk_pair``): P = k e^(-8 k)."""
    return k * np.exp(-8.0 * k)


def _load(name, *path):
    spec = importlib.util.spec_from_file_location(name, os.path.join(REF, *path))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def main():
    mgc._shims()
    sys.modules["hankl"].P2xi = po.P2xi
    cf = _load("cora.signal.corrfunc", "cora", "signal", "corrfunc.py")
    for name in ("healpy", "caput.algorithms", "caput.config", "cora.util.cubicspline", "cora.util.hputil"):
        mod = types.ModuleType(name)
        sys.modules[name] = mod
        parent, _, leaf = name.rpartition(".")
        if parent in sys.modules:
            setattr(sys.modules[parent], leaf, mod)
    lu = _load("cora.signal.lssutil", "cora", "signal", "lssutil.py")

    g = {}
    rng = np.random.default_rng(20261019)
    est = rng.standard_normal((4, 3))
    g["rich_est"] = est
    for bp in (1, 2):
        g["rich_t2_bp%d" % bp] = np.asarray(cf.richardson(list(est), 2.0, base_pow=bp))
        table = cf.richardson(list(est), 2.0, base_pow=bp, return_table=True)
        g["rich_t2_bp%d_table" % bp] = np.array([table[i][j] if j <= i else np.full(3, np.nan) for i in range(4) for j in range(4)])
    g["rich_t3"] = np.asarray(cf.richardson(list(est[:3]), 3.0))

    r = np.array([0.0, 0.1, 1.0, 7.5, 30.0, 100.0])
    g["direct_r"] = r
    for k in (4, 8, 16):
        g["direct_k%d" % k] = np.asarray(cf._corr_direct(ps_model, -5, 3, r, k=k))

    x = np.logspace(-6, 6, 25)
    g["cutoff_x"] = x
    g["cutoff_low"] = lu.cutoff(x, -4, 1, 0.5, 6)
    g["cutoff_high"] = lu.cutoff(x, 4, -1, 0.5, 4)
    g["cutoff_other"] = lu.cutoff(x, 0.3, -3, 0.25, 2.5)

    ra, fr = cf.ps_to_corr(ps_model, **PS_TO_CORR)
    g["ps_to_corr_r"], g["ps_to_corr_xi"] = ra, fr

    path = os.path.join(HERE, "pk2xi_vectors.npz")
    np.savez_compressed(path, **g)
    print("wrote", path, {k: v.shape for k, v in g.items()}, sum(v.size for v in g.values()), "values")


if __name__ == "__main__":
    main()
