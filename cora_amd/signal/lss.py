"""Counterpart of the density step of cora/signal/lss.py: ``za_density_sph`` (lss.py:1305-1419), the Zel'dovich
SPH mass assignment behind ``ZeldovichDynamics(sph=True)``.  One fused HIP kernel (csrc/pmesh.hip) moves every
HEALPix voxel as a particle and spreads its mass over 9 pixels x 3 radial bins.

The reference's scatter (pmesh_util.c:37, called from pmesh.pyx:_bin_delta) indexes ``out`` with a row stride of 9
(the number of pixel weights) instead of the map's npix, so mass meant for radial bin ``ri`` lands ri (npix - 9)
elements early.  This port implements the intended ``out[ri, pix]`` (tests/test_lss_host.py).
"""
import numpy as np

from .. import _lib
from ..util import hputil


def _assert_shape(arr, shape, name):
    """lssutil.assert_shape (cora/signal/lssutil.py:630-640)."""
    if len(arr.shape) != len(shape):
        raise ValueError(
            f"Array {name} has wrong number of dimensions (got {len(arr.shape)}, expected {len(shape)}"
        )
    if tuple(arr.shape) != tuple(shape):
        raise ValueError(f"Array {name} has the wrong shape (got {tuple(arr.shape)}, expected {tuple(shape)}")


def _check(psi, delta_bias, delta_m, chi, out):
    if len(delta_bias.shape) != 2:
        raise ValueError("Array delta_bias must be [nchi, npix]")
    nchi, npix = delta_bias.shape
    nside = int(round(np.sqrt(npix / 12.0)))
    if nside < 1 or 12 * nside * nside != npix:
        raise ValueError("delta_bias has %d pixels, not a HEALPix map" % npix)
    _assert_shape(psi, (3, nchi, npix), "psi")
    _assert_shape(delta_m, (nchi, npix), "delta_m")
    _assert_shape(chi, (nchi,), "chi")
    _assert_shape(out, (nchi, npix), "out")
    if nchi < 3:
        raise ValueError("za_density_sph needs at least 3 radial slices (got %d)" % nchi)
    return nchi, nside


def _sigmas(chi_host, nside, sigma_chi):
    if sigma_chi is None:
        sigma_chi = np.mean(np.abs(np.diff(chi_host))) / 2
    sigma_ang = hputil.nside2resol(nside) / 2
    if not (sigma_chi > 0):
        raise ValueError("sigma_chi must be positive (got %r)" % (sigma_chi,))
    return float(sigma_ang), float(sigma_chi)


def za_density_sph_device(psi, delta_bias, delta_m, chi, out, sigma_chi=None):
    """``za_density_sph`` on device tensors (float64, contiguous, on the context's GPU): fields from
    ``mkfullsky_device`` stay on the device.  ``out`` [nchi, npix] is accumulated into, then 1 is subtracted from it;
    it is returned.  The inputs are left unchanged.  Sums use float atomics: two calls agree to rounding, not bit for
    bit."""
    nchi, nside = _check(psi, delta_bias, delta_m, chi, out)
    sigma_ang, sigma_chi = _sigmas(chi.detach().cpu().numpy(), nside, sigma_chi)
    ctx = _lib.get_context()
    return ctx.za_density_sph(psi, delta_bias, delta_m, chi, out, sigma_ang, sigma_chi)


def za_density_sph(psi, delta_bias, delta_m, chi, out, sigma_chi=None):
    """Calculate the density field under the Zel'dovich approximation (cora/signal/lss.py:1305-1419).

    Every voxel (slice ``ii``, RING pixel ``p``) is a particle of mass ``1 + delta_bias[ii, p]`` at the pixel
    centre and comoving distance ``chi[ii]``, displaced by ``psi[:, ii, p]`` (radial, theta, phi; positions wrap as
    ``cora_amd.util.pmesh.calculate_positions``).  Its mass is spread with Gaussian weights (normalised to 1) over
    the pixel of its new direction and that pixel's 8 neighbours, width ``nside2resol / 2 x s``, and over 3
    radial bins ``low .. low + 2`` (``low = min(max(0, searchsorted(chi, new_chi) - 1), nchi - 3)``), width
    ``sigma_chi x s``, where ``s = clip(1 + delta_m, 0.1, 3) ** (-1/3)``.  Bin ``ri`` of pixel ``pix`` receives
    into ``out[ri, pix]``: the intended placement, not the row stride of 9 the reference's C scatter uses.

    Parameters
    ----------
    psi : np.ndarray[3, nchi, npix]
        The vector displacement field.
    delta_bias : np.ndarray[nchi, npix]
        The biased density field.
    delta_m : np.ndarray[nchi, npix]
        The underlying matter density field, for the density dependent particle size.
    chi : np.ndarray[nchi]
        The comoving distance of each slice (ascending; nchi >= 3).
    out : np.ndarray[nchi, npix]
        Accumulated into in place (not zeroed), then 1 is subtracted.
    sigma_chi : float, optional
        Radial smoothing scale at mean density; default ``mean(|diff(chi)|) / 2``.

    Returns
    -------
    out
    """
    nchi, nside = _check(psi, delta_bias, delta_m, chi, out)
    sigma_ang, sigma_chi = _sigmas(np.asarray(chi, dtype=np.float64), nside, sigma_chi)
    ctx = _lib.get_context()
    dev = [ctx.to_device(a) for a in (psi, delta_bias, delta_m, chi, out)]
    res = ctx.za_density_sph(*dev, sigma_ang, sigma_chi)
    out[...] = res.cpu().numpy()
    return out
