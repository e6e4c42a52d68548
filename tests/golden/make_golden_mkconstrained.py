#!/usr/bin/env python3
"""Generate tests/golden/mkconstrained_vectors.npz from the reference's own ``skysim.mkconstrained``.

Run in the build container only (needs the reference tree, as make_golden.py does).  The reference's
cora/core/skysim.py is loaded by path under the stand-ins of ``make_golden._install_shims()`` plus, all part of THIS
script: empty modules for ``cora``, ``cora.util``, ``cora.util.hputil`` and ``cora.util.nputil`` (imported by the file,
not used by ``mkconstrained``) and a stand-in ``healpy`` that turns the two transforms into bookkeeping, so that what
the function returns is its own ``cv`` array:

* ``Alm.getlm(lmax)`` returns (l, m) in the published m-major order of the packed index;
* ``map2alm(map, lmax=...)`` returns the prepared a_lm of the constraint whose number the "map" holds;
* ``nside2npix(nside)`` returns ``2 nalm``;
* ``alm2map(alm, nside)`` returns the real parts followed by the imaginary parts.

Nothing of the reference is copied into the repository.  Two cases at lmax 8: ``a_`` F = 6 with one constraint and ``b_``
F = 18 with two.  Stored per case: ``corr`` [9, F, F] as small integers (G G^T of an integer G: symmetric, positive
definite, exact in float64), ``f_ind``, the constraint a_lm ``calm_re`` / ``calm_im`` [k, nalm] (integers times
``calm_s``, a power of two; m = 0 real) and the reference's ``cv`` [F, nalm] complex in full precision.

Usage:  python tests/golden/make_golden_mkconstrained.py
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
import _constrained_oracle as co  # noqa: E402

REF = make_golden.REF
LMAX = 8
NALM = (LMAX + 1) * (LMAX + 2) // 2


def _load_skysim(state):
    make_golden._install_shims()
    for name in ("cora", "cora.util", "cora.util.hputil", "cora.util.nputil"):
        mod = types.ModuleType(name)
        mod.__path__ = []
        sys.modules[name] = mod
        parent, _, leaf = name.rpartition(".")
        if parent:
            setattr(sys.modules[parent], leaf, mod)
    hp = sys.modules.get("healpy")
    if hp is None:
        hp = sys.modules["healpy"] = types.ModuleType("healpy")

    class Alm:
        @staticmethod
        def getlm(lmax):
            return co.getlm(lmax)

    hp.Alm = Alm
    hp.map2alm = lambda m, lmax=None, **kw: state["calm"][int(np.asarray(m).ravel()[0])].copy()
    hp.nside2npix = lambda nside: 2 * NALM
    hp.alm2map = lambda alm, nside, **kw: np.concatenate((np.asarray(alm).real, np.asarray(alm).imag))
    spec = importlib.util.spec_from_file_location("cora.core.skysim", os.path.join(REF, "cora/core/skysim.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def case(sk, state, rng, F, f_ind):
    k = len(f_ind)
    G = rng.integers(-8, 9, (LMAX + 1, F, F))
    corr = np.einsum("lij,lkj->lik", G, G).astype(np.int32)
    _, marr = co.getlm(LMAX)
    re = rng.integers(-512, 513, (k, NALM)).astype(np.int16)
    im = np.where(marr[None, :] == 0, 0, rng.integers(-512, 513, (k, NALM))).astype(np.int16)
    s = 2.0 ** -6
    state["calm"] = (re + 1j * im) * s
    out = sk.mkconstrained(corr.astype(np.float64), [[f, np.full(4, float(i))] for i, f in enumerate(f_ind)], 1)
    assert out.shape == (F, 2 * NALM)
    cv = out[:, :NALM] + 1j * out[:, NALM:]
    larr, _ = co.getlm(LMAX)
    assert np.all(cv[:, larr == 0] == 0) and np.all(np.isfinite(cv.view(np.float64)))
    return dict(corr=corr, f_ind=np.asarray(f_ind, dtype=np.int32), calm_re=re, calm_im=im, calm_s=s, cv=cv)


def main():
    state = {}
    sk = _load_skysim(state)
    rng = np.random.default_rng(20261019)
    g = dict(lmax=LMAX)
    for prefix, F, f_ind in (("a_", 6, [2]), ("b_", 18, [11, 3])):
        for key, v in case(sk, state, rng, F, f_ind).items():
            g[prefix + key] = v
    path = os.path.join(HERE, "mkconstrained_vectors.npz")
    np.savez_compressed(path, **g)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))
    assert os.path.getsize(path) < 500 * 1000


if __name__ == "__main__":
    main()
