#!/usr/bin/env python3
"""Generate tests/golden/zagrid_vectors.npz by running the reference's own ``za_density_grid``
(cora/signal/lss.py:996-1096) on small fixed inputs (nside 8, 6 slices).

Run in the build container only (needs the reference tree, as make_golden_lss.py does).  That one function is loaded
from the reference's source at generation time (``ast``: its FunctionDef is compiled on its own) into a namespace
that holds

  calculate_positions, _bin_delta   the reference's pmesh.pyx, compiled into a throw-away temp dir
                                    (make_golden_lss._build_pmesh);
  lssutil.assert_shape              this repository's;
  healpy                            a shim serving npix2nside, pix2ang (cora_amd.util.hputil) and get_interp_weights
                                    (tests/_interp_oracle.py): healpy is absent here, so healpy's own values are NOT
                                    held in this file.

Nothing of the reference is copied into the repository.

Stored:
  inputs   psi, delta_bias, delta_m as int16 multiples of 2^-6 (radial) / 2^-10 (angles, deltas), so that the f64
           values are exact; chi; out0 (the value ``out`` holds before the call).
  out      what the function returns when ``_bin_delta`` is the intended scatter, bin ri into out[ri, pix].
  bin_delta_ref  the reference's real ``_bin_delta`` accumulation over all slices into zeros: its C scatter uses a row
           stride of 4 (pmesh_util.c:38 with npix = len_pixel), so only the first (nchi - 1) 4 + npix elements are
           touched; that prefix is stored.  It pins the radial bins, weights and masks against the native.

Usage:  python tests/golden/make_golden_zagrid.py
"""
import ast
import os
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [HERE, os.path.join(ROOT, "tests"), ROOT]

import make_golden  # noqa: E402
import make_golden_lss  # noqa: E402  (OMP_NUM_THREADS=1 and the pmesh build recipe)

REF = make_golden.REF
NSIDE, NCHI = 8, 6
Q_R, Q_A = 2.0 ** -6, 2.0 ** -10


def _inputs():
    """Fixed fields with the edge cases of the tests: pole crossings, phi = 0 crossings, both radial ends pushed outside
    chi, one slice with zero radial displacement."""
    from cora_amd.util import hputil

    npix = 12 * NSIDE * NSIDE
    rng = np.random.default_rng(20261018)
    th, ph = hputil.pix2ang(NSIDE, np.arange(npix))
    q_r = np.rint(rng.normal(0.0, 6.0, (NCHI, npix)) / Q_R)                 # chi spacing ~10: about half a bin
    q_t = np.rint(rng.normal(0.0, 0.12, (NCHI, npix)) / Q_A)                # ~ one pixel (resol 0.128)
    q_p = np.rint(rng.normal(0.0, 0.12, (NCHI, npix)) / Q_A / np.maximum(np.sin(th), 0.2))
    q_b = np.rint(rng.normal(0.0, 0.5, (NCHI, npix)) / Q_A)
    q_m = np.rint(rng.normal(0.0, 0.6, (NCHI, npix)) / Q_A)
    # poles: the first / last 4 pixels move across them, their neighbours to just short of them
    q_t[:, 0:4] = np.rint(-0.3 / Q_A)
    q_t[:, npix - 4:] = np.rint(0.3 / Q_A)
    q_t[:, 4:12] = np.rint(-0.17 / Q_A)
    q_t[:, npix - 12:npix - 4] = np.rint(0.17 / Q_A)
    # phi = 0: pixels just east of it move west, pixels just west of it move east
    near0 = np.where((ph < 0.2) & (np.abs(th - np.pi / 2) < 1.0))[0]
    near2pi = np.where((ph > 2 * np.pi - 0.2) & (np.abs(th - np.pi / 2) < 1.0))[0]
    q_p[:, near0] = np.rint(-0.3 / Q_A)
    q_p[:, near2pi] = np.rint(0.3 / Q_A)
    # radial ends: slice 0 below chi[0] (some below the extrapolated cell too), the last slice beyond chi[-1]
    q_r[0, ::5] = np.rint(-6.0 / Q_R)
    q_r[0, 1::5] = np.rint(-25.0 / Q_R)
    q_r[-1, ::5] = np.rint(6.0 / Q_R)
    q_r[-1, 1::5] = np.rint(25.0 / Q_R)
    q_r[2] = 0                                                              # particles exactly on chi[2]
    psi_q = np.stack([q_r, q_t, q_p]).astype(np.int16)
    chi = 1000.0 + 10.0 * np.arange(NCHI) + np.array([0.0, 0.3, -0.2, 0.1, 0.0, 0.4])
    return psi_q, q_b.astype(np.int16), q_m.astype(np.int16), chi


def _reference_function(namespace):
    """The reference's za_density_grid, compiled from its FunctionDef alone into ``namespace``."""
    path = os.path.join(REF, "cora/signal/lss.py")
    with open(path) as fh:
        tree = ast.parse(fh.read(), path)
    node = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "za_density_grid"]
    assert len(node) == 1
    exec(compile(ast.Module(body=node, type_ignores=[]), path, "exec"), namespace)
    return namespace["za_density_grid"]


def main():
    make_golden._install_shims()
    sys.path.insert(0, REF)
    tmp = tempfile.mkdtemp(prefix="cora_golden_zagrid_")
    pm = make_golden_lss._build_pmesh(tmp)

    import _interp_oracle as io
    from cora_amd.signal import lssutil
    from cora_amd.util import hputil

    psi_q, db_q, dm_q, chi = _inputs()
    scale = np.array([Q_R, Q_A, Q_A])[:, None, None]
    psi = psi_q.astype(np.float64) * scale
    delta_bias = db_q.astype(np.float64) * Q_A
    delta_m = dm_q.astype(np.float64) * Q_A
    nchi, npix = delta_bias.shape
    out0 = 0.25

    healpy = types.SimpleNamespace(
        npix2nside=hputil._npix2nside, pix2ang=hputil.pix2ang,
        get_interp_weights=lambda nside, theta, phi: io.interp_weights(nside, theta, phi))
    bug = np.zeros((nchi, npix))

    def bin_delta(rho, pixel_ind, pixel_weight, radial_ind, radial_weight, out):
        pm._bin_delta(rho, pixel_ind, pixel_weight, radial_ind, radial_weight, bug)            # the native, stride 4
        out += io.scatter_stride(rho, pixel_ind, pixel_weight, radial_ind, radial_weight, npix,
                                 nchi * npix).reshape(nchi, npix)                                 # the intended one

    ns = dict(np=np, healpy=healpy, lssutil=types.SimpleNamespace(assert_shape=lssutil.assert_shape),
              calculate_positions=pm.calculate_positions, _bin_delta=bin_delta)
    ref = _reference_function(ns)
    out = ref(psi, delta_bias, delta_m, chi, np.full((nchi, npix), out0))

    touched = (nchi - 1) * 4 + npix
    flat = bug.ravel()
    assert not flat[touched:].any()
    g = dict(nside=NSIDE, q_r=Q_R, q_a=Q_A, psi_q=psi_q, delta_bias_q=db_q, delta_m_q=dm_q, chi=chi, out0=out0, out=out,
             bin_delta_ref=flat[:touched])
    path = os.path.join(HERE, "zagrid_vectors.npz")
    np.savez_compressed(path, **g)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
