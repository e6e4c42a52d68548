"""Counterpart of cora/util/pmesh.pyx: the particle positions of the Zel'dovich SPH scheme on the host.  The
weights and the mass deposit run on the device (csrc/pmesh.hip via cora_amd.signal.lss.za_density_sph)."""
import numpy as np


def calculate_positions(angpos, displacement):
    """Apply an angular displacement, wrapping through the poles and in longitude (pmesh.pyx:29-52).

    Parameters
    ----------
    angpos : np.ndarray[2, npix]
        The original angular positions ordered as theta, phi.
    displacement : np.ndarray[2, npix]
        The shift to apply to each coordinate.

    Returns
    -------
    new_angpos : np.ndarray[2, npix]
        theta outside [0, pi] becomes pi - (theta mod pi) and phi gains pi there; then phi becomes phi mod 2 pi.
        "mod" is numpy's floor remainder (the sign of the divisor, also for negative arguments).
    """
    new_angpos = np.asarray(angpos, dtype=np.float64) + displacement

    wrap = (new_angpos[0] > np.pi) | (new_angpos[0] < 0)
    new_angpos[0][wrap] = np.pi - new_angpos[0][wrap] % np.pi
    new_angpos[1][wrap] += np.pi

    new_angpos[1] = new_angpos[1] % (2 * np.pi)

    return new_angpos
