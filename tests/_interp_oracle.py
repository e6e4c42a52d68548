"""Numpy oracle of the HEALPix RING bilinear interpolation (cora_amd.util.hputil.get_interp_weights, csrc/hpinterp.hip)
and of the grid form of the Zel'dovich density step built on it (cora_amd.signal.lss.za_density_grid,
cora/signal/lss.py:996-1096), for the tests.

The scheme is the published HEALPix one (``get_interpol``, Gorski et al. 2005), restated; healpy is not used and
its numbers are not held anywhere.  For a direction (theta, phi):

  * the two iso-latitude rings around theta: ``ir1`` the last ring (1 .. 4 nside - 1) whose centre colatitude is
    <= theta, ``ir2 = ir1 + 1``; ``ir1 = 0``: north of the first ring, ``ir2 = 4 nside``: south of the last one;
  * on each ring (``nr`` pixels from ``sp``, centres at ``(i + shifted / 2) 2 pi / nr``) the two nearest centres with
    weights linear in phi, wrapping round;
  * between the rings weights linear in theta; past the first / last ring the pole is a virtual sample whose value is
    the mean of the 4 pixels of that ring.

Ring colatitudes are ``arccos`` of the ring's z as ``hputil.pix2ang`` forms it, so a query at a pixel centre taken
from ``pix2ang`` sits exactly on its ring.
"""
import numpy as np

from cora_amd.util import hputil, pmesh

import _za_oracle as zo


def ring_theta(nside, ir):
    """Colatitude of ring ``ir`` (1 .. 4 nside - 1); 0 for ``ir <= 0`` and pi for ``ir >= 4 nside``."""
    ns = int(nside)
    ir = np.asarray(ir, dtype=np.int64)
    irc = np.clip(ir, 1, 4 * ns - 1)
    north, south = irc < ns, irc > 3 * ns
    i = np.where(south, 4 * ns - irc, irc)
    zc = 1.0 - i.astype(np.float64) ** 2 / (3.0 * ns * ns)
    zb = 4.0 / 3.0 - 2.0 * i / (3.0 * ns)
    z = np.where(north, zc, np.where(south, -zc, zb))
    return np.where(ir <= 0, 0.0, np.where(ir >= 4 * ns, np.pi, np.arccos(z)))


def ring_info(nside, ir):
    """(first pixel, pixel count, shifted as 0.0 / 1.0) of ring ``ir`` in 1 .. 4 nside - 1."""
    ns = int(nside)
    ir = np.asarray(ir, dtype=np.int64)
    npix, ncap = 12 * ns * ns, 2 * ns * (ns - 1)
    north, south = ir < ns, ir > 3 * ns
    j = 4 * ns - ir
    nr = np.where(north, 4 * ir, np.where(south, 4 * j, 4 * ns))
    sp = np.where(north, 2 * ir * (ir - 1), np.where(south, npix - 2 * j * (j + 1), ncap + (ir - ns) * 4 * ns))
    shifted = north | south | (((ir - ns) & 1) == 0)
    return sp, nr, shifted.astype(np.float64)


def ring_above(nside, theta):
    """``ir1``: the last ring whose centre colatitude is <= theta (0 .. 4 nside - 1)."""
    ns = int(nside)
    z = np.cos(theta)
    za = np.abs(z)
    belt = np.floor(ns * (2.0 - 1.5 * z))
    cap = np.floor(ns * np.sqrt(3.0 * (1.0 - za)))
    cap = np.where(z > 0, cap, 4 * ns - cap - 1)
    ir = np.clip(np.where(za <= 2.0 / 3.0, belt, cap), 0, 4 * ns - 1).astype(np.int64)
    # the formula in z is a first guess: the rings are compared in theta, where the weights are formed
    for _ in range(4 * ns):
        down = (ir > 0) & (theta < ring_theta(ns, ir))
        up = ~down & (ir < 4 * ns - 1) & (theta >= ring_theta(ns, ir + 1))
        if not (down.any() or up.any()):
            break
        ir = ir - down + up
    return ir


def _along_ring(nside, ir, phi):
    sp, nr, sh = ring_info(nside, ir)
    dphi = 2.0 * np.pi / nr
    i1 = np.floor(phi / dphi - 0.5 * sh)
    w = (phi - (i1 + 0.5 * sh) * dphi) / dphi
    i1 = i1.astype(np.int64)
    return sp + np.mod(i1, nr), sp + np.mod(i1 + 1, nr), w


def interp_weights(nside, theta, phi):
    """(pix [4, n] int64, weights [4, n]) of directions theta, phi (1-d arrays, 0 <= theta <= pi): the two pixels of
    the upper ring, then the two of the lower ring; north of the first ring the upper pair is the opposite pair of ring 1,
    south of the last ring the lower pair is the opposite pair of that ring."""
    ns = int(nside)
    npix = 12 * ns * ns
    theta = np.asarray(theta, dtype=np.float64).reshape(-1)
    phi = np.mod(np.asarray(phi, dtype=np.float64).reshape(-1), 2.0 * np.pi)
    ir1 = ring_above(ns, theta)
    ir2 = ir1 + 1
    npole, spole = ir1 == 0, ir2 == 4 * ns
    th1, th2 = ring_theta(ns, ir1), ring_theta(ns, ir2)
    a0, a1, wa = _along_ring(ns, np.where(npole, 1, ir1), phi)
    b0, b1, wb = _along_ring(ns, np.where(spole, 4 * ns - 1, ir2), phi)
    wt = (theta - th1) / (th2 - th1)
    pix = np.stack([a0, a1, b0, b1])
    w = np.stack([(1.0 - wa) * (1.0 - wt), wa * (1.0 - wt), (1.0 - wb) * wt, wb * wt])
    # north of ring 1: the pole, with weight 1 - wt, is the mean of the 4 pixels of ring 1
    fn = (1.0 - wt) * 0.25
    pix[0], pix[1] = np.where(npole, (b0 + 2) & 3, pix[0]), np.where(npole, (b1 + 2) & 3, pix[1])
    w[0], w[1] = np.where(npole, fn, w[0]), np.where(npole, fn, w[1])
    w[2], w[3] = np.where(npole, w[2] + fn, w[2]), np.where(npole, w[3] + fn, w[3])
    # south of the last ring: mirror image
    fs = wt * 0.25
    pix[2] = np.where(spole, ((a0 + 2) & 3) + npix - 4, pix[2])
    pix[3] = np.where(spole, ((a1 + 2) & 3) + npix - 4, pix[3])
    w[2], w[3] = np.where(spole, fs, w[2]), np.where(spole, fs, w[3])
    w[0], w[1] = np.where(spole, w[0] + fs, w[0]), np.where(spole, w[1] + fs, w[1])
    return pix, w


def interp_val(maps, theta, phi):
    """maps [nmap, npix] sampled at the directions: [nmap, n]."""
    maps = np.asarray(maps, dtype=np.float64)
    nside = int(round(np.sqrt(maps.shape[-1] / 12.0)))
    pix, w = interp_weights(nside, theta, phi)
    return (maps[:, pix] * w[None]).sum(axis=1)


def rotated_angles(nside, R):
    """(theta, phi) of ``R n_p`` for every pixel centre ``n_p``: where output pixel p of a rotation samples the input."""
    v = np.array(hputil.pix2vec(nside, np.arange(12 * int(nside) ** 2)))
    r = np.asarray(R, dtype=np.float64) @ v
    theta = np.arctan2(np.sqrt(r[0] * r[0] + r[1] * r[1]), r[2])
    phi = np.arctan2(r[1], r[0])
    return theta, np.where(phi < 0, phi + 2.0 * np.pi, phi)


def radial_bins(new_chi, chi):
    """The 2 radial bins [n, 2] and weights [n, 2] of cora/signal/lss.py:1041-1083: chi extended by one extrapolated
    cell at each end, np.digitize, |chi1 - x| / dchi and |x - chi0| / dchi; weight -1 marks a bin outside [0, nchi)."""
    nchi = chi.size
    ext = np.empty(nchi + 2)
    ext[1:-1] = chi
    ext[0] = chi[0] - (chi[1] - chi[0])
    ext[-1] = chi[-1] + (chi[-1] - chi[-2])
    ind = np.digitize(new_chi, ext)
    chi0 = ext[(ind - 1) % (nchi + 2)]
    chi1 = ext[ind % (nchi + 2)]
    dchi = chi1 - chi0
    w0 = np.abs((chi1 - new_chi) / dchi)
    w1 = np.abs((new_chi - chi0) / dchi)
    i0, i1 = ind - 2, ind - 1
    w0[(i0 < 0) | (i0 >= nchi)] = -1
    w1[(i1 < 0) | (i1 >= nchi)] = -1
    return np.stack([i0, i1], axis=1), np.stack([w0, w1], axis=1)


def scatter_stride(rho, pind, pw, rind, rw, stride, size):
    """The reference's C scatter (pmesh_util.c:17-41) with its row stride: flat[ri * stride + pi] += rho pw rw for
    rw >= 0, as a flat increment of ``size`` elements."""
    v = (rho[:, None] * pw)[:, :, None] * rw[:, None, :]
    idx = rind[:, None, :].astype(np.int64) * stride + pind[:, :, None].astype(np.int64)
    ok = np.broadcast_to(rw[:, None, :] >= 0, v.shape)
    return np.bincount(idx[ok], weights=v[ok], minlength=size)


def za_density_grid(psi, delta_bias, delta_m, chi, out, stride=None):
    """Oracle of lss.za_density_grid: every voxel's mass 1 + delta_bias goes to the 4 interpolation pixels of its new
    direction x the 2 radial bins around its new distance, into ``out[ri, pix]``; then minus 1.  ``delta_m`` is not
    used (as in the reference).  ``stride``: scatter with that row stride instead of npix into the flat ``out``
    (the reference's C scatter uses 4), without the final minus 1."""
    nchi, npix = delta_bias.shape
    nside = int(round(np.sqrt(npix / 12.0)))
    angpos = np.array(hputil.pix2ang(nside, np.arange(npix)))
    for ii in range(nchi):
        rho = 1 + delta_bias[ii]
        new_ang = pmesh.calculate_positions(angpos, psi[1:, ii])
        new_chi = chi[ii] + psi[0, ii]
        pix, w = interp_weights(nside, new_ang[0], new_ang[1])
        rind, rw = radial_bins(new_chi, chi)
        if stride is None:
            keep = np.where(rw >= 0, rw, 0.0)
            out += zo.scatter(rho, pix.T, w.T, np.where(rw >= 0, rind, 0), keep, nchi, npix)
        else:
            flat = out.reshape(-1)
            flat += scatter_stride(rho, pix.T, w.T, rind, rw, stride, flat.size)
    if stride is None:
        out -= 1.0
    return out
