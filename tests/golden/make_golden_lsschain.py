#!/usr/bin/env python3
"""Generate tests/golden/lsschain_vectors.npz from the reference's cora/signal/lssutil.py.

Run in the build container only (needs the reference tree, as make_golden.py does).  The reference module is loaded
by path with the stand-ins of ``make_golden._install_shims()`` plus empty modules for ``caput.algorithms``,
``caput.config``, ``cora.util.cubicspline`` and ``cora.util.hputil`` (none of them is touched by the four functions
that run); nothing of the reference is copied into the repository.

Stored (inputs as small integers times a power of two, so that their float64 values are exact):
  calculate_width            of a non-uniform 12-point chi
  exponential_FoG_kernel     for that chi with scalar sigmaP and D, with array sigmaP and D, and for a uniform
                             128-point chi (linspace(1800, 2400, 128), sigmaP 1.93, D 1)
  diff2                      of a [12, 48] field along axis 0 and of a [5, 12, 7] field along axis 1
  lognormal_transform        of a [12, 48] field with axis=1 and axis=None
  the three process formulas, written out below in the statement order of cora/signal/lss.py with the reference's own
  diff2 and exponential_FoG_kernel: bias (lss.py:565-592) with and without b2, linear dynamics (:902-914) with and
  without the velocity term, Fingers of God (:1198-1217) as K @ field for a [12, 48] and a [12, 4, 48] field.

Usage:  python tests/golden/make_golden_lsschain.py
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


def _load_lssutil():
    make_golden._install_shims()
    for name in ("caput.algorithms", "caput.config", "cora.util.cubicspline", "cora.util.hputil"):
        mod = types.ModuleType(name)
        sys.modules[name] = mod
        parent, _, leaf = name.rpartition(".")
        if parent in sys.modules:
            setattr(sys.modules[parent], leaf, mod)
    sys.path.insert(0, REF)
    spec = importlib.util.spec_from_file_location("cora.signal.lssutil", os.path.join(REF, "cora/signal/lssutil.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    lu = _load_lssutil()
    rng = np.random.default_rng(20261017)
    n, npix = 12, 48

    def q(scale, shape):
        return np.rint(rng.normal(0.0, scale, shape) / Q).astype(np.int32)

    g = dict(q=Q)
    # non-uniform chi: spacing ~ 5 with jitter, multiples of 2^-10
    chi_q = (np.arange(n) * 5120 + 1843200 + rng.integers(-900, 900, n)).astype(np.int64)
    chi = chi_q * Q
    g["chi_q"] = chi_q
    g["width"] = lu.calculate_width(chi)

    sig_q = (1976 + rng.integers(-300, 300, n)).astype(np.int64)        # ~1.93
    D_q = (800 - 12 * np.arange(n)).astype(np.int64)                    # 0.78 .. 0.65
    g["sigmaP_q"], g["D_q"] = sig_q, D_q
    sigmaP, D = sig_q * Q, D_q * Q
    g["fog_scalar"] = lu.exponential_FoG_kernel(chi, 1.93, 1.0)
    g["fog_array"] = lu.exponential_FoG_kernel(chi, sigmaP, D)
    g["fog_128"] = lu.exponential_FoG_kernel(np.linspace(1800.0, 2400.0, 128), 1.93, 1.0)

    phi_q, delta_q = q(3.0, (n, npix)), q(0.5, (n, npix))
    f3_q = q(2.0, (5, n, 7))
    g.update(phi_q=phi_q, delta_q=delta_q, f3_q=f3_q)
    phi, delta, f3 = phi_q * Q, delta_q * Q, f3_q * Q
    g["diff2_2d"] = lu.diff2(phi, chi, axis=0)
    g["diff2_3d"] = lu.diff2(f3, chi, axis=1)
    g["lognormal_axis1"] = lu.lognormal_transform(delta, axis=1)
    g["lognormal_none"] = lu.lognormal_transform(delta, axis=None)

    b1_q = (1024 + 40 * np.arange(n)).astype(np.int64)                  # 1.0 .. 1.43
    b2_q = (-300 + 55 * np.arange(n)).astype(np.int64)                  # -0.29 .. 0.30
    fr_q = (850 + 9 * np.arange(n)).astype(np.int64)                    # growth rate 0.83 .. 0.93
    g.update(b1_q=b1_q, b2_q=b2_q, fr_q=fr_q)
    b1, b2, fr = b1_q * Q, b2_q * Q, fr_q * Q

    # GenerateBiasedFieldBase.process, lss.py:565-592
    fd = delta
    bf = np.zeros_like(fd)
    bf[:] += (D * b1)[:, np.newaxis] * fd
    g["bias_b1"] = bf.copy()
    d2m = (fd**2).mean(axis=1)[:, np.newaxis]
    bf[:] += (D**2 * b2)[:, np.newaxis] * (fd**2 - d2m)
    g["bias_b1b2"] = bf.copy()
    g["bias_d2m"] = d2m[:, 0]
    g["bias_b1b2_lognormal"] = lu.lognormal_transform(bf.copy(), axis=1)

    # LinearDynamics.process, lss.py:902-914, on the biased field above
    fdelta = np.zeros_like(fd)
    fdelta[:] = g["bias_b1b2"]
    fdelta[:] += D[:, np.newaxis] * delta
    g["linear_real"] = fdelta.copy()
    vterm = lu.diff2(phi, chi, axis=0)
    vterm *= -(D * fr)[:, np.newaxis]
    fdelta[:] += vterm
    g["linear_rsd"] = fdelta.copy()

    # FingersOfGod.process, lss.py:1198-1217 (alpha_FoG 0.75, growth factor applied)
    g["alpha_fog"] = 0.75
    K = lu.exponential_FoG_kernel(chi, 0.75 * sigmaP, D)
    g["fog_K"] = K
    g["fog_2d"] = np.matmul(K, g["linear_rsd"])
    map_q = q(0.7, (n, 4, npix))
    g["map_q"] = map_q
    m = map_q * Q
    out = np.zeros_like(m)
    np.matmul(K, m.reshape(n, -1), out=out.reshape(n, -1))
    g["fog_map"] = out

    path = os.path.join(HERE, "lsschain_vectors.npz")
    np.savez_compressed(path, **g)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))
    assert os.path.getsize(path) < 200 * 1024


if __name__ == "__main__":
    main()
