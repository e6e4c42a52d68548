"""Counterpart of the density step of cora/signal/lss.py: ``za_density_sph`` (lss.py:1305-1419), the Zel'dovich
SPH mass assignment behind ``ZeldovichDynamics(sph=True)``.  One fused HIP kernel (csrc/pmesh.hip) moves every
HEALPix voxel as a particle and spreads its mass over 9 pixels x 3 radial bins.

``zeldovich_displacement`` makes the displacement field that kernel takes from the potential (lss.py:806-828:
iterated analysis, derivative synthesis and radial gradient, csrc/sht_der1.hip), and ``zeldovich_density`` is the
numerical content of ``ZeldovichDynamics.process(sph=True)`` (lss.py:777-856) from ``phi, delta`` to the final
density without leaving the device.

``za_density_grid`` (lss.py:996-1096) is the grid form behind ``ZeldovichDynamics(sph=False)``: the same particles,
their mass shared among the 4 bilinear-interpolation pixels of the new direction x 2 radial bins (csrc/hpinterp.hip);
``sph=False`` of ``zeldovich_density`` / ``tracer_map_device`` routes there.

The steps around it (csrc/lsschain.hip): ``biased_field`` (GenerateBiasedFieldBase.process, lss.py:556-603),
``linear_dynamics`` (LinearDynamics.process, :862-918), ``fingers_of_god`` (FingersOfGod.process, :1162-1220),
``biased_lss_to_map`` (BiasedLSSToMap.process, :944-993) and their composition ``tracer_map_device``: ``phi, delta``
in, map out, on the device.  ``multifrequency_aps_device`` and ``generate_initial_lss_device`` are the step before it
(CalculateMultiFrequencyAngularPowerSpectrum.process, :289-373, GenerateInitialLSSFromCl, :397-478): the three
correlation functions of ``calculate_correlations`` to C_l(chi, chi') in one pass, the extended covariance, the draw of
``phi, delta`` - so that P(k) -> xi -> C_l -> (phi, delta) -> tracer map is one device chain.  ``tracer_map_device`` takes ``b1``, ``b2``, ``sigmaP``, ``D``, ``f``, ``T_b`` as per-slice arrays (or scalars) the
caller supplies; ``tracer_models`` derives them from a redshift axis and the models of ``signal/lssmodels.py``, and
``tracer_map_from_models_device`` composes the chain with them and with ``add_correlated_shot_noise_device``
(``AddCorrelatedShotNoise``, lss.py:1223-1302).  ``generate_flat_spectrum_map_device`` (``GenerateFlatSpectrumMap``,
:1422-1552) draws through the same ``nputil.normal_rows_device``: numpy's scaled normals out of the device generator.

The reference's scatter (pmesh_util.c:37, called from pmesh.pyx:_bin_delta) indexes ``out`` with a row stride of 9
(the number of pixel weights) instead of the map's npix, so mass meant for radial bin ``ri`` lands ri (npix - 9)
elements early.  This port implements the intended ``out[ri, pix]`` (tests/test_lss_host.py).  The same
holds for the grid form, where that stride is 4 (the number of interpolation pixels).
"""
import numpy as np

from .. import _lib
from ..util import hputil
from . import lssutil

_assert_shape = lssutil.assert_shape


def _check(psi, delta_bias, delta_m, chi, out, min_slices=3, name="za_density_sph"):
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
    if nchi < min_slices:
        raise ValueError("%s needs at least %d radial slices (got %d)" % (name, min_slices, nchi))
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


# ------------------------------------------------------------------------------------
# the grid form (cora/signal/lss.py:996-1096)
# ------------------------------------------------------------------------------------
def _check_grid(psi, delta_bias, delta_m, chi, out):
    """``_check`` with the grid form's slice count, plus what its radial search needs: chi strictly ascending."""
    nchi, nside = _check(psi, delta_bias, delta_m, chi, out, min_slices=2, name="za_density_grid")
    chi_h = np.asarray(_host(chi), dtype=np.float64)
    if not (np.diff(chi_h) > 0).all():
        raise ValueError("za_density_grid needs chi ascending")
    return nchi, nside


def _check_device_f64(ctx, **tensors):
    """The kernels read raw float64 device memory: anything else is refused here, not by an assert further down."""
    import torch

    for name, t in tensors.items():
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float64 or t.device != ctx.device or not t.is_contiguous():
            raise ValueError("Array %s must be a contiguous float64 tensor on %s" % (name, ctx.device))


def za_density_grid_device(psi, delta_bias, delta_m, chi, out):
    """``za_density_grid`` on device tensors (float64, contiguous, on the context's GPU).  ``out`` [nchi, npix] is
    accumulated into, then 1 is subtracted from it; it is returned.  The inputs are left unchanged; ``delta_m`` is
    shape-checked and, as in the reference, not read.  Sums use float atomics: two calls agree to rounding, not bit for
    bit."""
    _check_grid(psi, delta_bias, delta_m, chi, out)
    ctx = _lib.get_context()
    _check_device_f64(ctx, psi=psi, delta_bias=delta_bias, chi=chi, out=out)
    return ctx.za_density_grid(psi, delta_bias, chi, out)


def za_density_grid(psi, delta_bias, delta_m, chi, out):
    """Calculate the density field under the Zel'dovich approximation, grid form (cora/signal/lss.py:996-1096).

    Every voxel (slice ``ii``, RING pixel ``p``) is a particle of mass ``1 + delta_bias[ii, p]`` moved exactly as in
    :func:`za_density_sph`.  Its mass is shared among the 4 pixels of the HEALPix bilinear interpolation at its new
    direction (``cora_amd.util.hputil.get_interp_weights``) and the 2 radial bins around its new distance: ``chi`` is
    extended by one extrapolated cell at each end, ``np.digitize`` picks the cell ``[chi0, chi1)``, the weights are
    ``|chi1 - x| / dchi`` and ``|x - chi0| / dchi``; a bin outside ``[0, nchi)`` drops its share (it is not
    redistributed, as in the reference).  Bin ``ri`` of pixel ``pix`` receives into ``out[ri, pix]``: the intended
    placement, not the row stride of 4 the reference's C scatter uses.

    Parameters
    ----------
    psi : np.ndarray[3, nchi, npix]
        The vector displacement field.
    delta_bias : np.ndarray[nchi, npix]
        The biased density field.
    delta_m : np.ndarray[nchi, npix]
        The underlying matter density field.  Shape-checked; not used (nor is it by the reference).
    chi : np.ndarray[nchi]
        The comoving distance of each slice (ascending; nchi >= 2).
    out : np.ndarray[nchi, npix]
        Accumulated into in place (not zeroed), then 1 is subtracted.

    Returns
    -------
    out
    """
    _check_grid(psi, delta_bias, delta_m, chi, out)
    ctx = _lib.get_context()
    dev = [ctx.to_device(a) for a in (psi, delta_bias, chi, out)]
    res = ctx.za_density_grid(*dev)
    out[...] = res.cpu().numpy()
    return out


# ------------------------------------------------------------------------------------
# the displacement field and the whole Zel'dovich step (cora/signal/lss.py:777-856)
# ------------------------------------------------------------------------------------
def _host(a):
    return a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)


def _check_displacement(phi, chi, D, f, nmin):
    nchi, nside = lssutil.check_maps(phi, chi, name="phi", xname="chi", nmin=nmin)
    _assert_shape(D, (nchi,), "D")
    if f is not None:
        _assert_shape(f, (nchi,), "f")
    return nchi, nside


def zeldovich_displacement_device(phi, chi, D, f=None, lmax=None, niter=3, out=None):
    """The Zel'dovich displacement field of cora/signal/lss.py:806-828 on device tensors.

    ``psi[0] = np.gradient(phi, chi, axis=0) * D * (1 + f)`` (no ``(1 + f)`` when ``f is None``, the reference's
    ``redshift_space=False``), ``psi[1] = D / chi * dphi/dtheta``, ``psi[2] = D / chi * (1/sin theta) dphi/dphi /
    sin theta``: the displacement in comoving distance, theta and phi that :func:`za_density_sph_device` takes.

    ``phi`` [nchi, npix] is a float64 device tensor (nchi >= 2); ``chi``, ``D`` (growth factor ratio) and ``f`` (growth
    rate) are [nchi] host or device arrays supplied by the caller.  ``lmax`` defaults to ``3 nside - 1``, ``niter``
    to healpy's 3 (see :func:`cora_amd.signal.lssutil.gradient`).  All three components are written by the kernels
    of csrc/sht_der1.hip with the factors fused; temporaries stay below
    ``lssutil.gradient_bytes(nside, lmax)`` (13.4e9 bytes at nside 1024, lmax 2048).  Returns ``psi``
    [3, nchi, npix] (``out`` if given)."""
    chi_h, D_h = _host(chi), _host(D)
    f_h = None if f is None else _host(f)
    _check_displacement(phi, chi_h, D_h, f_h, 2)
    D_h = np.asarray(D_h, dtype=np.float64)
    scale_r = D_h if f_h is None else D_h * (1.0 + np.asarray(f_h, dtype=np.float64))
    return lssutil.gradient_device(phi, np.asarray(chi_h, dtype=np.float64), grad0=True, out=out, lmax=lmax,
                                   niter=niter, scale_r=scale_r, scale_ang=D_h, phi_extra=1)


def zeldovich_displacement(phi, chi, D, f=None, lmax=None, niter=3):
    """:func:`zeldovich_displacement_device` for numpy arrays: ``phi`` [nchi, npix] -> ``psi`` [3, nchi, npix]."""
    phi, chi, D = np.asarray(phi), np.asarray(chi), np.asarray(D)
    f = None if f is None else np.asarray(f)
    _check_displacement(phi, chi, D, f, 2)
    ctx = _lib.get_context()
    return ctx.to_host(zeldovich_displacement_device(ctx.to_device(phi), chi, D, f, lmax=lmax, niter=niter))


def _check_density(phi, delta, delta_bias, chi, D, f):
    nchi, nside = _check_displacement(phi, chi, D, f, 3)
    _assert_shape(delta, tuple(phi.shape), "delta")
    _assert_shape(delta_bias, tuple(phi.shape), "delta_bias")
    return nchi, nside


def zeldovich_density_device(phi, delta, delta_bias, chi, D, f=None, sigma_chi=None, lmax=None, niter=3, sph=True):
    """The numerical content of ``ZeldovichDynamics.process(sph=True)`` (cora/signal/lss.py:777-856) on device tensors:
    ``psi = zeldovich_displacement_device(phi, chi, D, f)``, ``delta_m = delta * D[:, None]``, ``out = 0``, then
    ``za_density_sph_device(psi, delta_bias, delta_m, chi, out, sigma_chi)``.  ``phi``, ``delta`` (the matter
    density at the initial time) and ``delta_bias`` (the biased Lagrangian field) are [nchi, npix], nchi >= 3, ``chi``
    ascending.  Returns the final density contrast [nchi, npix].  Device memory beyond the three inputs: ``psi``,
    ``delta_m`` and the result (5 nchi npix doubles) plus ``lssutil.gradient_bytes(nside, lmax)``.  ``sph=False`` is
    the reference's ``sph=False``: the last step is ``za_density_grid_device(psi, delta_bias, delta_m, chi, out)``
    (``sigma_chi`` is not used there)."""
    import torch

    chi_h, D_h = _host(chi), _host(D)
    f_h = None if f is None else _host(f)
    _check_density(phi, delta, delta_bias, chi_h, D_h, f_h)
    ctx = _lib.get_context()
    psi = zeldovich_displacement_device(phi, chi_h, D_h, f_h, lmax=lmax, niter=niter)
    D_dev = ctx.to_device(np.asarray(D_h, dtype=np.float64))
    delta_m = delta * D_dev[:, None]
    out = torch.zeros_like(delta_bias)
    chi_dev = chi if isinstance(chi, torch.Tensor) else ctx.to_device(np.asarray(chi_h, dtype=np.float64))
    if not sph:
        return za_density_grid_device(psi, delta_bias, delta_m, chi_dev, out)
    return za_density_sph_device(psi, delta_bias, delta_m, chi_dev, out, sigma_chi)


def zeldovich_density(phi, delta, delta_bias, chi, D, f=None, sigma_chi=None, lmax=None, niter=3, sph=True):
    """:func:`zeldovich_density_device` for numpy arrays; returns the final density contrast [nchi, npix]."""
    phi, delta, delta_bias = np.asarray(phi), np.asarray(delta), np.asarray(delta_bias)
    chi, D = np.asarray(chi), np.asarray(D)
    f = None if f is None else np.asarray(f)
    _check_density(phi, delta, delta_bias, chi, D, f)
    ctx = _lib.get_context()
    res = zeldovich_density_device(ctx.to_device(phi), ctx.to_device(delta), ctx.to_device(delta_bias), chi, D, f,
                                   sigma_chi=sigma_chi, lmax=lmax, niter=niter, sph=sph)
    return ctx.to_host(res)


# ------------------------------------------------------------------------------------
# bias, linear dynamics, Fingers of God, map (cora/signal/lss.py:556-603, 862-918, 1162-1220, 944-993)
# ------------------------------------------------------------------------------------
_rows = lssutil.row_values


def _check_field(field, name, nmin=1):
    if len(field.shape) != 2:
        raise ValueError(f"Array {name} must be [nchi, npix] (got shape {tuple(field.shape)})")
    n = int(field.shape[0])
    if n < nmin:
        raise ValueError(f"{name} needs at least {nmin} slices (got {n})")
    return n, int(field.shape[1])


def biased_field_device(delta, D, b1=None, b2=None, lognormal=False, lightcone=True, out=None):
    """``GenerateBiasedFieldBase.process`` (cora/signal/lss.py:556-603) on a device tensor ``delta`` [nchi, npix]:
    ``(D b1)[:, None] delta + (D^2 b2)[:, None] (delta^2 - <delta^2>_slice)``, then the lognormal transform along
    axis 1 if ``lightcone`` else over the whole field.  ``D``, ``b1``, ``b2``: [nchi] arrays or scalars; a missing
    ``b1`` or ``b2`` skips that term.  Returns a new device tensor (``out`` if given; it may be ``delta``)."""
    n, npix = _check_field(delta, "delta")
    D = _rows(D, n, "D")
    ctx = _lib.get_context()
    c1 = np.zeros(n) if b1 is None else D * _rows(b1, n, "b1")
    if b2 is not None:
        c2 = D**2 * _rows(b2, n, "b2")
        _, s2 = ctx.slice_moments(delta)
        res = ctx.bias_field(delta, c1, c2, s2 / npix, out=out)
    else:
        res = ctx.bias_field(delta, c1, out=out)
    if lognormal:
        lssutil.lognormal_transform_device(res, out=res, axis=1 if lightcone else None)
    return res


def biased_field(delta, D, b1=None, b2=None, lognormal=False, lightcone=True):
    """:func:`biased_field_device` for numpy arrays."""
    delta = np.asarray(delta)
    n, _ = _check_field(delta, "delta")
    _rows(D, n, "D")
    ctx = _lib.get_context()
    return ctx.to_host(biased_field_device(ctx.to_device(delta), D, b1, b2, lognormal=lognormal, lightcone=lightcone))


def linear_dynamics_device(phi, delta, delta_bias, chi, D, f=None, out=None):
    """``LinearDynamics.process`` (cora/signal/lss.py:862-918) on device tensors [nchi, npix], nchi >= 4:
    ``(delta_bias + D[:, None] delta) + diff2(phi, chi, axis=0) (-(D f))[:, None]`` in one launch; ``f=None`` is the
    reference's ``redshift_space=False``: no velocity term.  ``out`` must not overlap ``phi``."""
    n, npix = _check_field(delta, "delta")
    _assert_shape(phi, (n, npix), "phi")
    _assert_shape(delta_bias, (n, npix), "delta_bias")
    chi_h = np.asarray(_host(chi), dtype=np.float64)
    _assert_shape(chi_h, (n,), "chi")
    D = _rows(D, n, "D")
    if n < 4:
        raise ValueError("linear_dynamics needs at least 4 slices (got %d)" % n)
    ctx = _lib.get_context()
    if f is None:
        return ctx.slice_diff2(None, None, g=delta, h=delta_bias, s=D, out=out)
    return ctx.slice_diff2(phi, chi_h, g=delta, h=delta_bias, s=D, t=-(D * _rows(f, n, "f")), out=out)


def linear_dynamics(phi, delta, delta_bias, chi, D, f=None):
    """:func:`linear_dynamics_device` for numpy arrays."""
    phi, delta, delta_bias = np.asarray(phi), np.asarray(delta), np.asarray(delta_bias)
    n, npix = _check_field(delta, "delta")
    _assert_shape(phi, (n, npix), "phi")
    _assert_shape(delta_bias, (n, npix), "delta_bias")
    if n < 4:
        raise ValueError("linear_dynamics needs at least 4 slices (got %d)" % n)
    ctx = _lib.get_context()
    return ctx.to_host(linear_dynamics_device(ctx.to_device(phi), ctx.to_device(delta), ctx.to_device(delta_bias), chi, D, f))


def _fog_kernel(n, chi, sigmaP, D, alpha_FoG):
    chi_h = np.asarray(_host(chi), dtype=np.float64)
    _assert_shape(chi_h, (n,), "chi")
    sig = alpha_FoG * _rows(sigmaP, n, "sigmaP")
    Dh = np.full(n, 1.0) if D is None else _rows(D, n, "D")
    return lssutil.exponential_FoG_kernel(chi_h, sig, Dh)


def fingers_of_god_device(field, chi, sigmaP, D=None, alpha_FoG=1.0, band_cut=None):
    """``FingersOfGod.process`` (cora/signal/lss.py:1162-1220) on a device tensor ``field`` [n, npix] or
    [n, npol, npix]: ``K @ field.reshape(n, -1)`` with ``K = exponential_FoG_kernel(chi, alpha_FoG sigmaP, D or 1)``.
    Returns ``field`` itself when ``alpha_FoG == 0``.  ``band_cut``: see :meth:`cora_amd._lib.Context.slice_mix`
    (default: exact)."""
    if alpha_FoG == 0.0:
        return field
    if len(field.shape) not in (2, 3):
        raise ValueError(f"Array field must be [n, npix] or [n, npol, npix] (got shape {tuple(field.shape)})")
    n = int(field.shape[0])
    K = _fog_kernel(n, chi, sigmaP, D, alpha_FoG)
    ctx = _lib.get_context()
    return ctx.slice_mix(K, field.reshape(n, -1), band_cut=band_cut).reshape(field.shape)


def fingers_of_god(field, chi, sigmaP, D=None, alpha_FoG=1.0, band_cut=None):
    """:func:`fingers_of_god_device` for numpy arrays."""
    if alpha_FoG == 0.0:
        return field
    field = np.asarray(field)
    if field.ndim not in (2, 3):
        raise ValueError(f"Array field must be [n, npix] or [n, npol, npix] (got shape {field.shape})")
    _fog_kernel(field.shape[0], chi, sigmaP, D, alpha_FoG)
    ctx = _lib.get_context()
    return ctx.to_host(fingers_of_god_device(ctx.to_device(field), chi, sigmaP, D, alpha_FoG, band_cut))


def biased_lss_to_map_device(delta, lognormal=False, map_prefactor=1.0, T_b=None, polarisation=True):
    """``BiasedLSSToMap.process`` (cora/signal/lss.py:944-993) on a device tensor ``delta`` [n, npix]: a map
    [n, 4 or 1, npix] whose plane 0 is the lognormal transform of ``delta`` along axis 1 (or a copy), times
    ``map_prefactor``, times ``T_b[:, None]`` (the mean 21 cm temperature per slice, supplied by the caller);
    the other planes are zero."""
    import torch

    n, npix = _check_field(delta, "delta")
    ctx = _lib.get_context()
    m = torch.zeros((n, 4 if polarisation else 1, npix), dtype=torch.float64, device=delta.device)
    hv = None
    if lognormal:
        _, var = lssutil.slice_moments_device(delta)
        hv = var * 0.5
    ctx.lognormal(delta, hv, out=m[:, 0], prefactor=map_prefactor, row_scale=None if T_b is None else _rows(T_b, n, "T_b"))
    return m


def biased_lss_to_map(delta, lognormal=False, map_prefactor=1.0, T_b=None, polarisation=True):
    """:func:`biased_lss_to_map_device` for numpy arrays."""
    delta = np.asarray(delta)
    _check_field(delta, "delta")
    ctx = _lib.get_context()
    return ctx.to_host(biased_lss_to_map_device(ctx.to_device(delta), lognormal, map_prefactor, T_b, polarisation))


def calculate_correlations(ps, minlogr=-1, maxlogr=5, switchlogr=1, samples_per_decade=1000, ksmooth=None,
                           logkcut_low=-4, logkcut_high=4):
    """The density, cross and potential correlation functions of a power spectrum: the body of
    ``CalculateCorrelations.process`` (lss.py:106-179) -> ``{"corr0", "corr2", "corr4"}``, each a
    ``cubicspline.SinhInterpolater`` ready for ``corrfunc.corr_to_clarray``.

    ps : P(k) at z = 0, a vectorised callable (the reference's ``powerspectrum(k, 0.0)``).  It is regularised by power-law
    cut-offs at ``logkcut_low`` / ``logkcut_high`` and a Gaussian of width ``ksmooth`` (None: none) and transformed with
    ``corrfunc.ps_to_corr`` (pads 4 / 6, nine Richardson levels) as P, P / k^2 and P / k^4.  ``ps`` is evaluated on the
    host, once per wavenumber grid: the three transforms share the samples."""
    from ..util import cubicspline
    from . import corrfunc

    ks = 1e10 if ksmooth is None else ksmooth
    plan = corrfunc._CorrPlan(minlogr, maxlogr, switchlogr, samples_per_decade, pad_low=4, pad_high=6, richardson_n=9)

    def _ps(k):
        return np.reshape(lssutil.cutoff(k, logkcut_low, 1, 0.5, 6) * lssutil.cutoff(k, logkcut_high, -1, 0.5, 4)
                          * np.exp(-0.5 * (k / ks) ** 2) * ps(k), -1)

    pd, pf = _ps(plan.kdirect), _ps(plan.kfine)
    out = {}
    for n, f_t in ((0, 1e-3), (2, 1e-6), (4, 1e2)):
        c = plan.run(pd * plan.kdirect**-n, pf * plan.kfine**-n).cpu().numpy()
        out["corr%d" % n] = cubicspline.SinhInterpolater(np.column_stack([plan.r, c]), x_t=plan.r[1], f_t=f_t)
    return out


# ------------------------------------------------------------------------------------
# xi(r) -> C_l(chi, chi') -> (phi, delta) (cora/signal/lss.py:246-478)
# ------------------------------------------------------------------------------------
_APS_SLOTS = ("Cl_delta_delta", "Cl_phi_delta", "Cl_phi_phi")     # function slots 0, 1, 2 of the packed spectra


def multifrequency_aps_device(correlations, nside, redshift=None, frequencies=None, cosmology=None, xromb=2, leg_q=4):
    """The body of ``CalculateMultiFrequencyAngularPowerSpectrum.process`` (lss.py:289-373) with the spectra left on the
    device.

    correlations : ``{"corr0", "corr2", "corr4"}`` of :func:`calculate_correlations`: the density, cross and potential
        correlation functions, interpolaters on the same knots.
    nside : ``lmax = 3 nside - 1``.
    redshift, frequencies : where to evaluate (arrays); ``frequencies`` (MHz) override ``redshift`` through ``nu21``.
        RuntimeError when neither is given.
    cosmology : its ``comoving_distance(redshift)`` gives ``chi``; default ``cora_amd.util.cosmology.Cosmology()``.
    xromb, leg_q : radial-bin quadrature order and Legendre accuracy parameter of ``corrfunc.corr_to_clarray``.

    Returns a dict: ``ell`` [lmax+1], ``chi``, ``redshift``, ``freq`` (None unless ``frequencies`` were given) as numpy
    arrays, ``Cl_delta_delta``, ``Cl_phi_delta``, ``Cl_phi_phi`` as device tensors [lmax+1, nz, nz], and ``cosmology``.
    The three functions are integrated in one pass (``corrfunc.corr_to_clarray_multi_device``)."""
    from ..util import constants
    from . import corrfunc

    if redshift is None and frequencies is None:
        raise RuntimeError("Redshifts or frequencies must be specified!")
    if cosmology is None:
        from ..util.cosmology import Cosmology

        cosmology = Cosmology()
    if frequencies is None:
        redshift = np.asarray(redshift, dtype=np.float64)
    else:
        frequencies = np.asarray(frequencies, dtype=np.float64)
        redshift = constants.nu21 / frequencies - 1.0
    xa = np.asarray(cosmology.comoving_distance(redshift), dtype=np.float64)
    # NOTE (the reference's): it is important not to set this any higher, or power aliases back down in the synthesis
    lmax = 3 * int(nside) - 1
    corrs = [correlations["corr0"], correlations["corr2"], correlations["corr4"]]
    full = corrfunc.corr_to_clarray_multi_device(corrs, lmax, xa, xromb=xromb, q=leg_q)
    aps = {"ell": np.arange(lmax + 1), "chi": xa, "redshift": redshift, "freq": frequencies, "cosmology": cosmology}
    for n, name in enumerate(_APS_SLOTS):
        aps[name] = full[n]
    return aps


def multifrequency_aps(correlations, nside, redshift=None, frequencies=None, cosmology=None, xromb=2, leg_q=4):
    """:func:`multifrequency_aps_device` with the three spectra as numpy arrays."""
    aps = multifrequency_aps_device(correlations, nside, redshift, frequencies, cosmology, xromb=xromb, leg_q=leg_q)
    ctx = _lib.get_context()
    for name in _APS_SLOTS:
        aps[name] = ctx.to_host(aps[name])
    return aps


def initial_lss_covariance_device(aps):
    """The extended covariance of ``GenerateInitialLSSFromCl.process`` (lss.py:439-445) -> device tensor
    [L, 2 nz, 2 nz]: phi phi at ``[:nz, :nz]``, delta delta at ``[nz:, nz:]``, phi delta at both off-diagonal blocks,
    symmetric bit for bit (``corahip_cl_blocks``).  ``aps``: the dict of :func:`multifrequency_aps_device` or
    :func:`multifrequency_aps`: the three spectra [L, nz, nz] as device tensors or arrays; their upper triangles
    (i, j >= i) are what is used, as they stand at the time of the call."""
    import torch

    ctx = _lib.get_context()
    cls = [c if isinstance(c, torch.Tensor) else ctx.to_device(c) for c in (aps[name] for name in _APS_SLOTS)]
    L, nz = int(cls[0].shape[0]), int(cls[0].shape[1])
    for name, c in zip(_APS_SLOTS, cls):
        _assert_shape(c, (L, nz, nz), name)
    iu = torch.triu_indices(nz, nz, device=ctx.device)
    packed = torch.stack([c[:, iu[0], iu[1]] for c in cls], dim=1).contiguous()
    return ctx.cl_blocks(packed, nz)


def generate_initial_lss_device(aps, nside=None, seed=0, rng=None):
    """``GenerateInitialLSSFromCl`` (lss.py:397-478): one realisation ``(phi, delta)``, device tensors [nz, npix], drawn
    from the extended covariance of :func:`initial_lss_covariance_device` by ``skysim.mkfullsky_device``.

    nside : default ``hputil.nside_for_lmax(L - 1, accuracy_boost=0)``; a larger one is a RuntimeError.
    seed, rng : ``rng`` defaults to ``numpy.random.default_rng(seed)``; the numpy stream is continued on the device, so
    the random numbers are the reference's."""
    from ..core import skysim

    nside_from_cl = hputil.nside_for_lmax(len(aps["ell"]) - 1, accuracy_boost=0)
    if nside is None:
        nside = nside_from_cl
    elif nside > nside_from_cl:
        raise RuntimeError(f"Requested nside ({nside}) cannot exceed nside used for input C_l ({nside_from_cl})")
    if rng is None:
        rng = np.random.default_rng(seed)
    nz = len(aps["chi"])
    sky = skysim.mkfullsky_device(initial_lss_covariance_device(aps), nside, rng=rng)
    return sky[:nz], sky[nz:]


def generate_initial_lss(aps, nside=None, seed=0, rng=None):
    """:func:`generate_initial_lss_device` with ``(phi, delta)`` as numpy arrays."""
    phi, delta = generate_initial_lss_device(aps, nside=nside, seed=seed, rng=rng)
    ctx = _lib.get_context()
    return ctx.to_host(phi), ctx.to_host(delta)


def tracer_map_device(phi, delta, chi, D, f, b1, b2=None, sigmaP=None, dynamics="zeldovich", lognormal=False,
                      lightcone=True, redshift_space=True, fog_D=None, alpha_FoG=1.0, band_cut=None,
                      map_lognormal=False, map_prefactor=1.0, T_b=None, polarisation=True, sigma_chi=None, lmax=None,
                      niter=3, sph=True):
    """``phi, delta`` [nchi, npix] (device, from ``mkfullsky_device``) -> tracer map [nchi, 4 or 1, npix] on the device:
    :func:`biased_field_device` -> :func:`zeldovich_density_device` (``dynamics="zeldovich"``) or
    :func:`linear_dynamics_device` (``"linear"``) -> :func:`fingers_of_god_device` (skipped when ``sigmaP`` is None)
    -> :func:`biased_lss_to_map_device`.  A composition only: every number comes from those four calls, with the
    arguments passed through (``redshift_space=False`` passes ``f=None`` to the dynamics; ``fog_D`` is the growth factor
    the FoG kernel divides out and re-applies, None = 1; ``sph`` goes to :func:`zeldovich_density_device`)."""
    if dynamics not in ("zeldovich", "linear"):
        raise ValueError("dynamics must be 'zeldovich' or 'linear' (got %r)" % (dynamics,))
    fd = f if redshift_space else None
    bias = biased_field_device(delta, D, b1, b2, lognormal=lognormal, lightcone=lightcone)
    if dynamics == "zeldovich":
        # the default call is the one made before the keyword existed, keyword for keyword
        # (tests/test_gpu_lsschain.py::test_tracer_map_is_the_composition compares them): only the grid form names sph
        grid = {} if sph else {"sph": False}
        final = zeldovich_density_device(phi, delta, bias, chi, D, fd, sigma_chi=sigma_chi, lmax=lmax, niter=niter, **grid)
    else:
        final = linear_dynamics_device(phi, delta, bias, chi, D, fd)
    del bias
    if sigmaP is not None:
        final = fingers_of_god_device(final, chi, sigmaP, fog_D, alpha_FoG, band_cut)
    return biased_lss_to_map_device(final, map_lognormal, map_prefactor, T_b, polarisation)


# ------------------------------------------------------------------------------------
# tracer models, correlated shot noise, flat-spectrum maps
# (cora/signal/lss.py:182-243, 676-684, 1223-1302, 1422-1589; the models: signal/lssmodels.py)
# ------------------------------------------------------------------------------------
def _default_cosmology(cosmology):
    if cosmology is None:
        from ..util.cosmology import Cosmology

        cosmology = Cosmology()
    return cosmology


def polynomial_bias(z, model=None, z_eff=None, bias_coeff=None, alpha_b=1.0):
    """``GeneratePolynomialBias._bias_1`` (lss.py:657-684): the first-order LAGRANGIAN bias at redshift ``z``, from
    ``z_eff`` and ``bias_coeff`` (``sum_n c_n (z - z_eff)^n``) when both are given, else from the named ``model`` of
    ``lssmodels.bias``; ValueError when neither is.  ``alpha_b`` scales the EULERIAN bias: ``alpha_b b + alpha_b - 1``."""
    from . import lssmodels

    if z_eff is not None and bias_coeff is not None:
        b = lssmodels.PolyModelSet.evaluate_poly(z, z_eff, bias_coeff)
    elif model is not None:
        b = lssmodels.bias[model](z)
    else:
        raise ValueError("Either `model` must be set, or `z_eff` and `bias_coeff`")
    return alpha_b * b + alpha_b - 1.0


def blend_power_spectrum(ps_linear, ps_nonlinear, alpha_NL=1.0):
    """The mix of ``BlendNonLinearPowerSpectrum.process`` (lss.py:233-238) for callables: returns
    ``k -> ps_linear(k) (1 - alpha_NL) + ps_nonlinear(k) alpha_NL`` (0: linear, 1: non-linear), a ``ps`` for
    :func:`calculate_correlations`."""

    def ps(k):
        return ps_linear(k) * (1 - alpha_NL) + ps_nonlinear(k) * alpha_NL

    return ps


def differential_comoving_volume(z, cosmo=None):
    """Comoving volume per unit redshift and steradian at ``z`` in (Mpc/h)^3, ``chi^2 c / H`` (lss.py:1555-1589);
    ``cosmo`` defaults to ``Cosmology()``."""
    from ..util import constants

    cosmo = _default_cosmology(cosmo)
    H_z = cosmo.H(z) * (cosmo._unit_distance / 1000.0)          # (km h) / (Mpc s)
    dm = cosmo.comoving_distance(z)
    return dm**2 * (constants.c / 1e3) / H_z


def shot_noise_seed(delta):
    """The seed ``AddCorrelatedShotNoise.setup`` derives from the initial field (lss.py:1259-1263): ``zlib.adler32`` of
    ``delta[:, :100]`` as contiguous float64 bytes.  For a device tensor that corner is copied to the host."""
    import zlib

    sub = delta[:, :100]
    sub = np.ascontiguousarray(_host(sub), dtype=np.float64)
    return zlib.adler32(sub.copy().tobytes())


def shot_noise_std(nside, chi, n_eff):
    """Standard deviation per slice of the shot noise of ``n_eff`` sources per (Mpc/h)^3 in a HEALPix voxel
    (lss.py:1289-1296): ``(pixarea chi^2 width(chi) n_eff) ** -0.5``."""
    pixarea = 4 * np.pi / hputil.nside2npix(nside)
    chi = np.asarray(chi, dtype=np.float64)
    volume = pixarea * (chi**2) * lssutil.calculate_width(chi)
    return (volume * n_eff) ** -0.5


def _shot_noise_n_eff(n, n_eff, log_M_HI_g, redshift, cosmology, omega_HI_model):
    from . import lssmodels

    if n_eff is not None:
        return np.ones(n) * _rows(n_eff, n, "n_eff")
    if log_M_HI_g is not None:
        if redshift is None:
            raise ValueError("log_M_HI_g needs the redshift of every slice")
        z = _rows(redshift, n, "redshift")
        return lssmodels.log_M_HI_g_to_n_eff(log_M_HI_g, _default_cosmology(cosmology), z, omega_HI_model)
    raise RuntimeError("One of `n_eff` or `log_M_HI_g` must be set.")


def _shot_noise_rng(rng, seed, seed_field):
    if rng is not None:
        return rng
    if seed is None:
        seed = shot_noise_seed(seed_field)
    return np.random.default_rng(seed)


def add_correlated_shot_noise_device(delta, chi, n_eff=None, log_M_HI_g=None, redshift=None, cosmology=None,
                                     omega_HI_model="Crighton2015", seed=None, rng=None, seed_from=None):
    """``AddCorrelatedShotNoise`` (lss.py:1223-1302) IN PLACE on a device tensor ``delta`` [nchi, npix]:
    ``delta += rng.normal(scale=std[:, None], size=delta.shape)`` with ``std = shot_noise_std(nside, chi, n_eff)``;
    returns ``delta``.

    n_eff : sources per (Mpc/h)^3, a scalar or one value per slice.  It wins over ``log_M_HI_g``, the log10 of the HI
        mass per tracer in solar masses, which needs the ``redshift`` of every slice (and ``cosmology``, default
        ``Cosmology()``, ``omega_HI_model``).  RuntimeError when neither is given.
    rng, seed, seed_from : the generator is ``rng`` if given, else ``numpy.random.default_rng(seed)``; with ``seed``
        None the seed is :func:`shot_noise_seed` of ``seed_from`` (the INITIAL field, as in the reference, so that
        every tracer of one realisation gets the same noise) or of ``delta`` itself.

    The draw equals the reference's statement bit for bit GIVEN THE SAME Generator: a PCG64 generator is continued on
    the device, the normals leave the generator's emit pass scaled and added (``nputil.normal_rows_device``).  How the
    reference's task builds its generator from the seed (caput's ``RandomTask``) is not restated here."""
    from ..util import nputil

    n, npix = _check_field(delta, "delta")
    chi_h = np.asarray(_host(chi), dtype=np.float64)
    _assert_shape(chi_h, (n,), "chi")
    nside = hputil._npix2nside(npix)
    ne = _shot_noise_n_eff(n, n_eff, log_M_HI_g, redshift, cosmology, omega_HI_model)
    std = shot_noise_std(nside, chi_h, ne)
    rng = _shot_noise_rng(rng, seed, delta if seed_from is None else seed_from)
    nputil.normal_rows_device(rng, std, npix, delta, accumulate=True)
    return delta


def add_correlated_shot_noise(delta, chi, n_eff=None, log_M_HI_g=None, redshift=None, cosmology=None,
                              omega_HI_model="Crighton2015", seed=None, rng=None, seed_from=None):
    """:func:`add_correlated_shot_noise_device` for a numpy array: returns a new array, ``delta`` is left as it is."""
    delta = np.asarray(delta, dtype=np.float64)
    n, npix = _check_field(delta, "delta")
    _assert_shape(np.asarray(chi), (n,), "chi")
    hputil._npix2nside(npix)
    _shot_noise_n_eff(n, n_eff, log_M_HI_g, redshift, cosmology, omega_HI_model)
    rng = _shot_noise_rng(rng, seed, delta if seed_from is None else seed_from)
    ctx = _lib.get_context()
    return ctx.to_host(add_correlated_shot_noise_device(ctx.to_device(delta), chi, n_eff, log_M_HI_g, redshift, cosmology,
                                                        omega_HI_model, rng=rng))


_STOKES = ("I", "Q", "U", "V")


def _flat_spectrum_plan(nside, frequencies, full_pol, pol, variance, P_SN, use_freq_dependent_voxel_volume, cosmology):
    """Everything of ``GenerateFlatSpectrumMap`` (lss.py:1476-1535) up to the draw, on the host:
    ``(nfreq, npol_total, ipol, scale_f [nfreq], attrs)``."""
    from ..util import constants

    if (variance is None) == (P_SN is None):
        raise ValueError("Only one of variance or P_SN can be specified.")
    pol = list(pol)
    if not full_pol and pol != ["I"]:
        raise RuntimeError("Must have full_pol=True if nonzero non-I maps are desired.")
    pol_axis = list(_STOKES) if full_pol else ["I"]
    ipol = [pol_axis.index(p) for p in pol]
    if len(set(ipol)) != len(ipol):
        raise ValueError("pol names a Stokes parameter twice: %r" % (pol,))
    freq = np.asarray(frequencies, dtype=np.float64)
    nfreq = len(freq)
    redshift = constants.nu21 / freq - 1
    ref_chan = int(nfreq / 2.0)
    omega = 4 * np.pi / hputil.nside2npix(nside)
    if use_freq_dependent_voxel_volume:
        dV = differential_comoving_volume(redshift, cosmology)
        dz = lssutil.calculate_width(redshift)
    else:
        dV = differential_comoving_volume(redshift[ref_chan], cosmology)
        dz = redshift[ref_chan + 1] - redshift[ref_chan]
    voxvol = dV * dz * omega
    if variance is not None:
        scale = variance**0.5
    else:
        scale = P_SN**0.5
        scale = scale / voxvol**0.5
    scale_f = np.ones(nfreq) * scale
    attrs = {"voxvol_ref": voxvol, "central_redshift": redshift[ref_chan]}
    return nfreq, len(pol_axis), ipol, scale_f, attrs


def generate_flat_spectrum_map_device(nside, frequencies, full_pol=True, pol=("I",), variance=None, P_SN=None,
                                      use_freq_dependent_voxel_volume=False, cosmology=None, seed=None, rng=None):
    """``GenerateFlatSpectrumMap`` (lss.py:1422-1552): a map [nfreq, 4 or 1, npix] on the device whose Stokes planes
    ``pol`` hold zero-mean Gaussian noise of standard deviation ``variance ** 0.5`` or ``(P_SN / V_voxel) ** 0.5``,
    the other planes zeros; returns ``(map, attrs)`` with ``attrs = {"voxvol_ref", "central_redshift"}``.

    frequencies : MHz.  ``V_voxel`` is that of the central channel ``nfreq // 2``, or per channel with
        ``use_freq_dependent_voxel_volume``.  Exactly one of ``variance`` and ``P_SN`` (ValueError); planes other than
        I need ``full_pol`` (RuntimeError).
    rng : default ``numpy.random.default_rng(seed)``.  The planes equal
        ``rng.normal(scale=scale, size=(nfreq, len(pol), npix))`` bit for bit given the same Generator: one
        ``nputil.normal_rows_device`` call whose rows are (channel, drawn plane) in C order."""
    import torch

    from ..util import nputil

    nfreq, npol, ipol, scale_f, attrs = _flat_spectrum_plan(nside, frequencies, full_pol, pol, variance, P_SN,
                                                            use_freq_dependent_voxel_volume, cosmology)
    npix = hputil.nside2npix(nside)
    if rng is None:
        rng = np.random.default_rng(seed)
    ctx = _lib.get_context()
    m = torch.zeros((nfreq, npol, npix), dtype=torch.float64, device=ctx.device)
    row_off = (np.arange(nfreq, dtype=np.int64)[:, np.newaxis] * npol + np.asarray(ipol, dtype=np.int64)[np.newaxis, :]) * npix
    nputil.normal_rows_device(rng, np.repeat(scale_f, len(ipol)), npix, m, row_off=row_off.reshape(-1), accumulate=False)
    return m, attrs


def generate_flat_spectrum_map(nside, frequencies, full_pol=True, pol=("I",), variance=None, P_SN=None,
                               use_freq_dependent_voxel_volume=False, cosmology=None, seed=None, rng=None):
    """:func:`generate_flat_spectrum_map_device` with the map as a numpy array."""
    _flat_spectrum_plan(nside, frequencies, full_pol, pol, variance, P_SN, use_freq_dependent_voxel_volume, cosmology)
    ctx = _lib.get_context()
    m, attrs = generate_flat_spectrum_map_device(nside, frequencies, full_pol, pol, variance, P_SN,
                                                 use_freq_dependent_voxel_volume, cosmology, seed, rng)
    return ctx.to_host(m), attrs


def tracer_models(redshift, cosmology=None, bias_model="HI", alpha_b=1.0, sigma_P_model=None, use_mean_21cmT=False,
                  omega_HI_model="Crighton2015"):
    """The per-slice numbers the reference's tasks derive from a redshift axis (lss.py:569-577, 1191-1196, 982-989 and
    the dynamics tasks): a dict of ``chi`` (``comoving_distance``), ``D`` (``growth_factor(z) / growth_factor(0)``),
    ``f`` (``growth_rate``), ``b1`` (:func:`polynomial_bias` of ``bias_model``), ``sigmaP`` (``lssmodels.sigma_P`` model,
    None without one), ``fog_D`` (``growth_factor(z)``, what ``FingersOfGod`` divides out) and ``T_b``
    (``mean_21cm_temperature`` of the ``omega_HI`` model, None unless ``use_mean_21cmT``)."""
    from . import lssmodels

    c = _default_cosmology(cosmology)
    z = np.asarray(redshift, dtype=np.float64)
    T_b = None
    if use_mean_21cmT:
        T_b = lssmodels.mean_21cm_temperature(c, z, lssmodels.omega_HI.evaluate(z, model=omega_HI_model))
    return {
        "chi": np.asarray(c.comoving_distance(z), dtype=np.float64),
        "D": c.growth_factor(z) / c.growth_factor(0),
        "f": c.growth_rate(z),
        "b1": polynomial_bias(z, model=bias_model, alpha_b=alpha_b),
        "sigmaP": None if sigma_P_model is None else lssmodels.sigma_P[sigma_P_model](z),
        "fog_D": c.growth_factor(z),
        "T_b": T_b,
    }


def tracer_map_from_models_device(phi, delta, redshift, cosmology=None, bias_model="HI", alpha_b=1.0, b2=None,
                                  sigma_P_model=None, n_eff=None, log_M_HI_g=None, use_mean_21cmT=False,
                                  omega_HI_model="Crighton2015", seed=None, rng=None, **kw):
    """:func:`tracer_map_device` with ``chi, D, f, b1, sigmaP, fog_D, T_b`` taken from :func:`tracer_models` of the
    redshift axis, and correlated shot noise added to the final field before it becomes a map:
    :func:`biased_field_device` -> the dynamics -> :func:`fingers_of_god_device` (with a ``sigma_P_model``) ->
    :func:`add_correlated_shot_noise_device` (skipped when ``n_eff`` and ``log_M_HI_g`` are both None; seeded from
    ``seed`` / ``rng``, else from the initial ``delta``) -> :func:`biased_lss_to_map_device`.  ``**kw``: the remaining
    keywords of :func:`tracer_map_device` (``dynamics``, ``lognormal``, ``lightcone``, ``redshift_space``, ``fog_D``,
    ``alpha_FoG``, ``band_cut``, ``map_lognormal``, ``map_prefactor``, ``polarisation``, ``sigma_chi``, ``lmax``,
    ``niter``, ``sph``).  A composition only: every number comes from those calls."""
    opt = dict(dynamics="zeldovich", lognormal=False, lightcone=True, redshift_space=True, alpha_FoG=1.0, band_cut=None,
               map_lognormal=False, map_prefactor=1.0, polarisation=True, sigma_chi=None, lmax=None, niter=3, sph=True)
    m = tracer_models(redshift, cosmology, bias_model, alpha_b, sigma_P_model, use_mean_21cmT, omega_HI_model)
    opt["fog_D"] = m["fog_D"]
    unknown = set(kw) - set(opt)
    if unknown:
        raise TypeError("tracer_map_from_models_device got unexpected keywords %s" % sorted(unknown))
    opt.update(kw)
    if opt["dynamics"] not in ("zeldovich", "linear"):
        raise ValueError("dynamics must be 'zeldovich' or 'linear' (got %r)" % (opt["dynamics"],))
    chi, D = m["chi"], m["D"]
    n, _ = _check_field(delta, "delta")
    noise = n_eff is not None or log_M_HI_g is not None
    if noise:
        _shot_noise_n_eff(n, n_eff, log_M_HI_g, redshift, cosmology, omega_HI_model)
        rng = _shot_noise_rng(rng, seed, delta)          # (the seed comes from the INITIAL field, before anything else runs)
    fd = m["f"] if opt["redshift_space"] else None
    bias = biased_field_device(delta, D, m["b1"], b2, lognormal=opt["lognormal"], lightcone=opt["lightcone"])
    if opt["dynamics"] == "zeldovich":
        grid = {} if opt["sph"] else {"sph": False}
        final = zeldovich_density_device(phi, delta, bias, chi, D, fd, sigma_chi=opt["sigma_chi"], lmax=opt["lmax"],
                                         niter=opt["niter"], **grid)
    else:
        final = linear_dynamics_device(phi, delta, bias, chi, D, fd)
    del bias
    if m["sigmaP"] is not None:
        final = fingers_of_god_device(final, chi, m["sigmaP"], opt["fog_D"], opt["alpha_FoG"], opt["band_cut"])
    if noise:
        add_correlated_shot_noise_device(final, chi, n_eff, log_M_HI_g, redshift, cosmology, omega_HI_model, rng=rng)
    return biased_lss_to_map_device(final, opt["map_lognormal"], opt["map_prefactor"], m["T_b"], opt["polarisation"])
