"""Counterpart of the functions of cora/signal/lssutil.py that the LSS steps use: ``linspace`` (lssutil.py:14-51), ``gradient``
(lssutil.py:225-261), ``assert_shape`` (lssutil.py:630-640), ``diff2`` (:99-185), ``calculate_width`` (:491-515),
``exponential_FoG_kernel`` (:518-589), ``lognormal_transform`` (:592-627); the last four with the kernels of
csrc/lsschain.hip.  The angular derivatives come from the derivative
synthesis (csrc/sht_der1.hip), the radial one from ``radial_gradient_kernel``; everything stays on the device in
the ``_device`` forms.  The estimators ``pk_flat`` (:293-376), ``corrfunc`` (:379-443), ``ang_correlation`` (:446-464) and
``transfer`` (:467-488) are read off the all-pairs spectra of the slices (csrc/spectra.hip).  ``laplacian`` (:188-222) is
composed from the iterated analysis, ``alm_scale_l``, the synthesis and one merged radial stencil."""
import numpy as np

from .. import _lib
from ..util import hputil

# slices that go through analysis + derivative synthesis together (a multiple of 4: whole channel groups)
SLICE_CHUNK = 16


def linspace(x):
    """Counterpart of lssutil.linspace (cora/signal/lssutil.py:14-51), the parser of the ``redshift`` / ``frequencies``
    settings: an ndarray is returned as it is; a dict with ``start``, ``stop``, ``num`` and optionally ``endpoint``, or a
    list ``[start, stop, num]`` / ``[start, stop, num, endpoint]``, becomes ``numpy.linspace`` of those.  Any other type
    is a TypeError (where the reference raises its configuration error)."""
    if isinstance(x, np.ndarray):
        return x
    if isinstance(x, dict):
        args = {k: x[k] for k in ("start", "stop", "num")}
        if "endpoint" in x:
            args["endpoint"] = x["endpoint"]
    elif isinstance(x, list):
        args = dict(zip(("start", "stop", "num", "endpoint"), x[:4]))
        for k in ("start", "stop", "num"):
            if k not in args:
                raise IndexError("linspace needs [start, stop, num] (got %d values)" % len(x))
    else:
        raise TypeError("linspace takes a dict, a list or an array (got %s)" % type(x).__name__)
    return np.linspace(**args)


def assert_shape(arr, shape, name):
    """lssutil.assert_shape (cora/signal/lssutil.py:630-640)."""
    if len(arr.shape) != len(shape):
        raise ValueError(
            f"Array {name} has wrong number of dimensions (got {len(arr.shape)}, expected {len(shape)}"
        )
    if tuple(arr.shape) != tuple(shape):
        raise ValueError(f"Array {name} has the wrong shape (got {tuple(arr.shape)}, expected {tuple(shape)}")


def check_maps(maps, x, name="maps", xname="x", nmin=1):
    """[nmaps, npix] HEALPix maps with ``len(x) == nmaps``: returns (nmaps, nside) or raises ValueError."""
    if len(maps.shape) != 2:
        raise ValueError(f"Array {name} must be [nmaps, npix] (got shape {tuple(maps.shape)})")
    nmaps, npix = (int(v) for v in maps.shape)
    nside = int(round(np.sqrt(npix / 12.0)))
    if nside < 1 or 12 * nside * nside != npix:
        raise ValueError(f"{name} has {npix} pixels, not a HEALPix map")
    assert_shape(x, (nmaps,), xname)
    if nmaps < nmin:
        raise ValueError(f"{name} needs at least {nmin} slices (got {nmaps})")
    return nmaps, nside


def gradient_bytes(nside, lmax, chunk=SLICE_CHUNK):
    """Upper bound of the temporary device memory of :func:`gradient_device` for slice chunks of ``chunk``, from the
    library's own workspace sizes: the coefficients of the chunk, plus the larger of the iterated analysis (three maps
    and two more coefficient sets) and the derivative synthesis (three coefficient sets and three maps per field),
    plus the shared transform workspace (the largest of the analysis pass, the synthesis of the chunk and the
    synthesis of 3 x ``chunk`` channels), plus 1 MiB of small tables."""
    ctx = _lib.get_context()
    nside, lmax, chunk = int(nside), int(lmax), max(4, int(chunk) // 4 * 4)
    plan = ctx.sht_plan(nside, lmax)
    npix = 12 * nside * nside
    nalm = (lmax + 1) * (lmax + 2) // 2
    g = chunk // 4
    alm = nalm * ((chunk + 7) // 8 * 2) * 64
    ws = max(ctx.map2alm_workspace_bytes(plan, chunk), ctx.alm2map_workspace_bytes(plan, chunk),
             ctx.alm2map_workspace_bytes(plan, 12 * g))
    ana = 3 * chunk * npix * 8 + 2 * alm
    der = nalm * 3 * g * 64 + 12 * g * npix * 8
    return alm + max(ana, der) + ws + (1 << 20)


def gradient_device(maps, x, grad0=True, out=None, lmax=None, niter=3, scale_r=None, scale_ang=None, phi_extra=0,
                    chunk=SLICE_CHUNK):
    """:func:`gradient` on device tensors: maps [nmaps, npix] (float64, contiguous), ``x`` [nmaps] (host or device) ->
    grad [3, nmaps, npix] (``out``: the tensor to write).  All slices of a chunk of ``chunk`` go through the analysis
    and the derivative synthesis in one batch; temporaries stay below :func:`gradient_bytes`.

    ``scale_r`` / ``scale_ang``: optional host [nmaps] factors multiplied into component 0 / components 1 and 2 (on
    top of ``1 / x``), ``phi_extra=1`` divides component 2 by sin theta once more - applied by the kernels that
    write the components (the Zel'dovich scaling of cora/signal/lss.py:815-828 costs no extra pass)."""
    import torch

    xh = x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
    nmaps, nside = check_maps(maps, xh)
    xh = np.asarray(xh, dtype=np.float64)
    if grad0 and nmaps < 2:
        raise ValueError("the radial gradient needs at least 2 slices (got %d)" % nmaps)
    lmax = 3 * nside - 1 if lmax is None else int(lmax)
    npix = 12 * nside * nside
    ctx = _lib.get_context()
    if out is None:
        out = ctx.empty((3, nmaps, npix))
    assert_shape(out, (3, nmaps, npix), "out")
    ang = 1.0 / xh if scale_ang is None else np.asarray(scale_ang, dtype=np.float64) / xh
    ang_dev = ctx.to_device(ang)
    chunk = max(4, int(chunk) // 4 * 4)
    for c0 in range(0, nmaps, chunk):
        n = min(chunk, nmaps - c0)
        alm = hputil.map2alm_device(maps[c0:c0 + n], nside, lmax, use_weights=True, niter=niter)
        ctx.alm2map_der1(alm, nside, lmax, n, scale_theta=ang_dev[c0:c0 + n], scale_phi=ang_dev[c0:c0 + n],
                         phi_extra=phi_extra, out=(out[1, c0:c0 + n], out[2, c0:c0 + n]))
        del alm
    if grad0:
        ctx.radial_gradient(maps, xh, scale=scale_r, out=out[0])
    else:
        out[0].zero_()
    return out


def gradient(maps, x, grad0=True, lmax=None, niter=3):
    """Take the gradient of a set of maps in spherical coordinates (cora/signal/lssutil.py:225-261).

    ``grad[1:, i] = alm2map_der1(map2alm(maps[i]))[1:] / x[i]`` and ``grad[0] = np.gradient(maps, x, axis=0)`` if
    ``grad0`` else zeros.  The analysis is ``hputil.map2alm_device(..., use_weights=True, niter=3)``: healpy's default
    ``iter=3`` with this package's ring weights (:func:`cora_amd.util.hputil.ring_weights`) standing in for the pixel
    weights the reference asks healpy for (``use_pixel_weights=True``) - those come from a data file of a dependency
    that is not available to this package.  With three refinements the result depends on the weights only through
    the starting point of the iteration.

    The device form runs the same kernels on the same batch shapes, so for up to ``SLICE_CHUNK`` maps this function
    returns exactly the host copy of :func:`gradient_device`'s result; the analysis itself is not guaranteed to be
    bitwise reproducible between batch shapes.

    Parameters
    ----------
    maps : np.ndarray[nmaps, npix]
        HEALPix maps (RING) at the radial positions ``x``.
    x : np.ndarray[nmaps]
        Radial coordinate of each map.
    grad0 : bool, optional
        Compute the radial component; if False ``grad[0]`` is zero.
    lmax : int, optional
        Band limit of the analysis, default ``3 nside - 1`` (healpy's).
    niter : int, optional
        Refinements of the analysis (healpy's ``iter``), default 3.

    Returns
    -------
    grad : np.ndarray[3, nmaps, npix]
        Components in the (r, theta, phi) directions.
    """
    maps = np.asarray(maps)
    x = np.asarray(x)
    check_maps(maps, x)
    if grad0 and maps.shape[0] < 2:
        raise ValueError("the radial gradient needs at least 2 slices (got %d)" % maps.shape[0])
    ctx = _lib.get_context()
    dev = ctx.to_device(maps)
    return ctx.to_host(gradient_device(dev, np.asarray(x, dtype=np.float64), grad0=grad0, lmax=lmax, niter=niter))


# ------------------------------------------------------------------------------------
# the Laplacian in spherical coordinates (cora/signal/lssutil.py:188-222)
# ------------------------------------------------------------------------------------
def laplacian_coefficients(x):
    """Host table [n, 4] of the radial part of :func:`laplacian` for coordinates ``x`` [n], n >= 4:
    ``diff2(f, x)_i + (2 / x_i) np.gradient(f, x)_i = sum_k coef[i, k] f[first[i] + k]`` over the four rows
    ``first[i] = min(max(i - 2, 0), n - 4)`` that ``corahip_slice_diff2`` reads.  ``Context.diff2_coefficients(x)`` plus
    ``2 / x_i`` times ``Context.gradient_coefficients(x)``, whose rows i - 1, i, i + 1 (the one-sided pair at the ends)
    always lie among those four: each entry is ``d_k + (2 / x_i) g_k`` with one product and one sum."""
    x = np.asarray(x, dtype=np.float64)
    coef, first = _lib.Context.diff2_coefficients(x)
    grad = _lib.Context.gradient_coefficients(x)
    n = x.size
    coef = coef.copy()
    for i in range(n):
        for k in range(3):
            row = i - 1 + k
            if 0 <= row < n:
                coef[i, row - first[i]] += (2.0 / x[i]) * grad[i, k]
    return coef


def laplacian_bytes(nside, lmax, chunk=SLICE_CHUNK):
    """Upper bound of the temporary device memory of :func:`laplacian_device` beyond its input and its output, for slice
    chunks of ``chunk``, from the library's own workspace sizes: the iterated analysis of a chunk (its synthesis and
    its residual, the coefficients, their update and the padded buffer of a pass: two maps and three coefficient sets
    per slice), the ``[chunk, lmax + 1]`` factors, the shared transform workspace (the larger of the analysis and the
    synthesis of a chunk), plus 1 MiB of small tables."""
    ctx = _lib.get_context()
    nside, lmax, chunk = int(nside), int(lmax), max(4, int(chunk) // 4 * 4)
    plan = ctx.sht_plan(nside, lmax)
    npix = 12 * nside * nside
    nalm = (lmax + 1) * (lmax + 2) // 2
    alm = nalm * ((chunk + 7) // 8 * 2) * 64
    ws = max(ctx.map2alm_workspace_bytes(plan, chunk), ctx.alm2map_workspace_bytes(plan, chunk))
    return 2 * chunk * npix * 8 + 3 * alm + chunk * (lmax + 1) * 8 + ws + (1 << 20)


def laplacian_device(maps, x, out=None, lmax=None, niter=3, chunk=SLICE_CHUNK):
    """:func:`laplacian` on device tensors: maps [nmaps, npix] (float64, contiguous), ``x`` [nmaps] (host or device) ->
    [nmaps, npix] (``out``: the tensor to write; it must not overlap ``maps``).

    Angular part, per chunk of ``chunk`` slices: ``hputil.map2alm_device(use_weights=False, niter)``, the factors
    ``fl[i, l] = -l (l + 1) / x_i^2`` applied by ``Context.alm_scale_l``, and ``Context.alm2map`` straight into ``out``.
    Radial part: both terms are stencils over the same four rows, merged on the host into one table
    (:func:`laplacian_coefficients`) and added to ``out`` in place by one ``Context.slice_diff2`` pass.  Temporaries
    stay below :func:`laplacian_bytes`.  Needs at least 4 slices (``diff2``'s one-sided ends)."""
    import torch

    xh = _host_x(x)
    nmaps, nside = check_maps(maps, xh)
    if nmaps < 4:
        raise ValueError("diff2 needs at least 4 samples along the axis (got %d)" % nmaps)
    lmax = 3 * nside - 1 if lmax is None else int(lmax)
    npix = 12 * nside * nside
    ctx = _lib.get_context()
    if out is None:
        out = ctx.empty((nmaps, npix))
    assert_shape(out, (nmaps, npix), "out")
    for t, name in ((maps, "maps"), (out, "out")):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float64 or not t.is_contiguous():
            raise ValueError("%s must be a contiguous float64 device tensor" % name)
    if ctx._overlap(out, nmaps * npix * 8, maps, nmaps * npix * 8):
        raise ValueError("laplacian: out overlaps maps")
    coef = laplacian_coefficients(xh)
    ll = np.arange(lmax + 1, dtype=np.float64)
    fl = -(ll * (ll + 1.0))[None, :] / (xh * xh)[:, None]
    chunk = max(4, int(chunk) // 4 * 4)
    for c0 in range(0, nmaps, chunk):
        n = min(chunk, nmaps - c0)
        alm = hputil.map2alm_device(maps[c0:c0 + n], nside, lmax, use_weights=False, niter=niter)
        ctx.alm_scale_l(alm, lmax, fl[c0:c0 + n], out=alm)
        ctx.alm2map(alm, nside, lmax, n, out=out[c0:c0 + n])
        del alm
    # out = (out + 0 * out) + stencil(maps) * 1: the kernel's epilogue with h = g = out
    ctx.slice_diff2(maps, xh, g=out, h=out, s=0.0, t=1.0, out=out, coef=coef)
    return out


def laplacian(maps, x, lmax=None, niter=3):
    """Take the Laplacian of a set of maps in spherical coordinates (cora/signal/lssutil.py:188-222).

    ``out_i = S[-l (l + 1) a_i] / x_i^2 + diff2(maps, x)_i + 2 np.gradient(maps, x, axis=0)_i / x_i`` with
    ``a_i = map2alm(maps_i)`` - three refinements and no weights, healpy's defaults, which is what the reference
    runs - and ``S`` the synthesis at the maps' nside.

    The two radial terms are evaluated as ONE four-point stencil with merged coefficients
    (:func:`laplacian_coefficients`) and added to the angular part, so the same terms are rounded in a different order
    than in the reference's three separate additions: the results agree to a few ulp of the sum of the terms'
    magnitudes, not bit for bit.  ``1 / x_i^2`` multiplies the coefficients before the synthesis, not the map after
    it.  The ends follow the reference: ``diff2`` is one-sided (4-point) on rows 0, 1 and
    N - 1, ``np.gradient`` first order on rows 0 and N - 1.

    For up to ``SLICE_CHUNK`` maps this function runs the same kernels on the same batch shapes as
    :func:`laplacian_device` and returns the host copy of its result.

    Parameters
    ----------
    maps : np.ndarray[nmaps, npix]
        HEALPix maps (RING) at the radial positions ``x``; at least 4.
    x : np.ndarray[nmaps]
        Radial coordinate of each map.
    lmax : int, optional
        Band limit of the analysis, default ``3 nside - 1`` (healpy's).
    niter : int, optional
        Refinements of the analysis (healpy's ``iter``), default 3.

    Returns
    -------
    lap : np.ndarray[nmaps, npix]
    """
    maps = np.asarray(maps)
    x = np.asarray(x)
    nmaps, _ = check_maps(maps, x)
    if nmaps < 4:
        raise ValueError("diff2 needs at least 4 samples along the axis (got %d)" % nmaps)
    ctx = _lib.get_context()
    dev = ctx.to_device(maps)
    return ctx.to_host(laplacian_device(dev, np.asarray(x, dtype=np.float64), lmax=lmax, niter=niter))


# ------------------------------------------------------------------------------------
# diff2, the Fingers-of-God kernel, slice products and moments, the lognormal transform (csrc/lsschain.hip)
# ------------------------------------------------------------------------------------
def row_values(v, n, name):
    """A per-slice argument: ``[n]`` array, or a scalar broadcast to ``[n]`` -> host float64 [n]."""
    h = v.detach().cpu().numpy() if hasattr(v, "detach") else np.asarray(v)
    h = np.asarray(h, dtype=np.float64)
    if h.ndim == 0:
        return np.full(n, float(h))
    assert_shape(h, (n,), name)
    return h


def calculate_width(centres):
    """Estimate the width of a set of contiguous bins from their centres (cora/signal/lssutil.py:491-515): interior
    widths are half the distance between the neighbours, the edge widths put the first boundary where the next bin's
    width says it is.  Host arithmetic; entries are always positive."""
    centres = np.asarray(centres, dtype=np.float64)
    if centres.ndim != 1 or centres.size < 3:
        raise ValueError("calculate_width needs at least 3 bin centres (got shape %r)" % (centres.shape,))
    widths = np.zeros(len(centres))
    widths[1:-1] = (centres[2:] - centres[:-2]) / 2.0
    widths[0] = 2 * (centres[1] - (widths[1] / 2.0) - centres[0])
    widths[-1] = 2 * (centres[-1] - (widths[-2] / 2.0) - centres[-2])
    return np.abs(widths)


def cutoff(x, cut, sign, width, index):
    """Roughly one, then a power-law drop-off (lssutil.py:264-290): ``(0.5 (1 + tanh(sign (log10 x - cut) / width)))^index``.

    cut : location of the cut in log10; sign : +1 cuts off lower values, -1 higher ones; width : width of the transition in
    decades; index : steepness, roughly the power-law index of the cut region.  Host arithmetic: it regularises the power
    spectrum that ``corrfunc.ps_to_corr`` evaluates on the host."""
    sign = np.sign(sign)
    return (0.5 * (1 + np.tanh(sign * (np.log10(x) - cut) / width))) ** index


def exponential_FoG_kernel(chi, sigmaP, D):
    """The ``len(chi) x len(chi)`` exponential smoothing matrix that approximates Fingers of God
    (cora/signal/lssutil.py:518-589): the Fourier conjugate of a Lorentzian ``(1 + k_par^2 sigmaP^2 / 2)^-1``,
    averaged over the width of each radial bin (the sinh(x)/x factors), rows normalised to 1, the growth factor
    ``D`` divided out before and re-applied after smoothing.  ``sigmaP`` and ``D``: scalars or [n] arrays.  Host
    numpy, the reference's operations in the reference's order."""
    chi = np.asarray(chi, dtype=np.float64)
    if chi.ndim != 1:
        raise ValueError("chi must be one-dimensional (got shape %r)" % (chi.shape,))
    sigmaP = row_values(sigmaP, chi.size, "sigmaP") if isinstance(sigmaP, np.ndarray) else np.ones_like(chi) * sigmaP
    D = row_values(D, chi.size, "D") if isinstance(D, np.ndarray) else np.ones_like(chi) * D
    a = 2**0.5 / sigmaP
    ar = a[:, np.newaxis]
    dchi = calculate_width(chi)[np.newaxis, :]
    chi_sep = np.abs(chi[:, np.newaxis] - chi[np.newaxis, :])

    def sinhc(x):
        return np.sinh(x) / x

    K = np.exp(-ar * chi_sep) * sinhc(ar * dchi / 2.0)
    np.fill_diagonal(K, np.diagonal(np.exp(-ar * dchi / 4) * sinhc(ar * dchi / 4)))
    K /= np.sum(K, axis=1)[:, np.newaxis]
    K /= D[np.newaxis, :]
    K *= D[:, np.newaxis]
    return K


def _host_x(x):
    return np.asarray(x.detach().cpu().numpy() if hasattr(x, "detach") else x, dtype=np.float64)


def diff2_device(f, x, out=None):
    """``diff2(f, x, axis=0)`` of a device tensor f [n, ncol] (float64, contiguous), n >= 4; ``x`` [n] host or device.
    Equal to the reference bit for bit.  ``out`` must not overlap ``f``."""
    if len(f.shape) != 2:
        raise ValueError(f"Array f must be [n, ncol] (got shape {tuple(f.shape)})")
    x = _host_x(x)
    assert_shape(x, (int(f.shape[0]),), "x")
    if f.shape[0] < 4:
        raise ValueError("diff2 needs at least 4 samples along the axis (got %d)" % f.shape[0])
    return _lib.get_context().slice_diff2(f, x, out=out)


def diff2(f, x, axis=-1):
    """Take a non-uniform second order derivative along ``axis`` (cora/signal/lssutil.py:99-185): the three-point
    scheme of doi:10.1016/0307-904X(94)00020-7 on rows 2 .. N-2, one-sided 4-point schemes on rows 0, 1 and N-1
    (the reference's code fills them, whatever its docstring says).  Same shape as ``f``; needs N >= 4."""
    f = np.asarray(f, dtype=np.float64)
    x = np.asarray(x, dtype=np.float64)
    if f.ndim < 1:
        raise ValueError("diff2 needs an array")
    axis = axis % f.ndim
    n = f.shape[axis]
    assert_shape(x, (n,), "x")
    if n < 4:
        raise ValueError("diff2 needs at least 4 samples along the axis (got %d)" % n)
    fm = np.moveaxis(f, axis, 0)
    ctx = _lib.get_context()
    res = ctx.to_host(diff2_device(ctx.to_device(fm.reshape(n, -1)), x))
    return np.ascontiguousarray(np.moveaxis(res.reshape(fm.shape), 0, axis))


def slice_mix_device(K, f, out=None, band_cut=None):
    """``K @ f`` for a device field f [n, ncol] and K [n, n] (host or device) with FP64 MFMA
    (:meth:`cora_amd._lib.Context.slice_mix`: the skipping rule and the bound of ``band_cut`` are stated there)."""
    if len(f.shape) != 2:
        raise ValueError(f"Array f must be [n, ncol] (got shape {tuple(f.shape)})")
    assert_shape(K, (int(f.shape[0]), int(f.shape[0])), "K")
    return _lib.get_context().slice_mix(K, f, out=out, band_cut=band_cut)


def slice_moments_device(f):
    """``(f.mean(axis=1), f.var(axis=1))`` of a device field [n, ncol] (a view with a larger row stride is fine) as
    numpy forms them: the mean first, then the mean of the centred squares.  Device tensors [n]; fixed summation
    order, identical bits from call to call."""
    ctx = _lib.get_context()
    ncol = int(f.shape[1])
    s1, _ = ctx.slice_moments(f)
    mean = s1 / ncol
    _, s2 = ctx.slice_moments(f, mean)
    return mean, s2 / ncol


def _lognormal_axis(field, axis):
    if axis is None:
        return None
    if len(field.shape) == 2 and axis in (1, -1):
        return 1
    raise ValueError("lognormal_transform takes axis=None or the last axis of a 2-D field (got axis=%r for %d-D)"
                     % (axis, len(field.shape)))


def lognormal_transform_device(field, out=None, axis=None):
    """:func:`lognormal_transform` on a device tensor.  ``out`` may be ``field`` itself, or (2-D fields) a view with a
    larger row stride such as plane 0 of a [n, 4, npix] map."""
    import torch

    axis = _lognormal_axis(field, axis)
    ctx = _lib.get_context()
    if not isinstance(field, torch.Tensor) or field.dtype != torch.float64 or not field.is_contiguous():
        raise ValueError("field must be a contiguous float64 device tensor")
    if out is not None and (not isinstance(out, torch.Tensor) or tuple(out.shape) != tuple(field.shape)
                            or out.dtype != field.dtype):
        raise ValueError("Given output array is incompatible.")
    if axis == 1:
        _, var = slice_moments_device(field)
        return ctx.lognormal(field, var * 0.5, out=out)
    _, var = slice_moments_device(field.reshape(1, -1))
    if field.dim() == 2:
        return ctx.lognormal(field, (var * 0.5).expand(field.shape[0]), out=out)
    if out is None:
        out = torch.empty_like(field)
    if not out.is_contiguous():
        raise ValueError("Given output array is incompatible.")
    ctx.lognormal(field.reshape(1, -1), var * 0.5, out=out.view(1, -1))
    return out


def lognormal_transform(field, out=None, axis=None):
    """Transform to a lognormal field with the same first order two point statistics
    (cora/signal/lssutil.py:592-627): ``exp(field - var / 2) - 1`` with ``var = field.var(axis=axis, keepdims=True)``.
    ``axis``: None (one variance over everything) or the last axis of a 2-D field.  ``out``: array to write into
    (may be ``field``); a new one if None."""
    field = np.asarray(field)
    axis = _lognormal_axis(field, axis)
    if out is None:
        out = np.zeros_like(field, dtype=np.float64)
    elif not isinstance(out, np.ndarray) or field.shape != out.shape or field.dtype != out.dtype:
        raise ValueError("Given output array is incompatible.")
    if field.dtype != np.float64:
        raise ValueError("lognormal_transform takes float64 fields (got %s)" % field.dtype)
    ctx = _lib.get_context()
    res = lognormal_transform_device(ctx.to_device(field), axis=axis)
    out[...] = ctx.to_host(res)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# estimators (cora/signal/lssutil.py:293-488): all of them are read off the Gram matrix of the slices' a_lm per l,
# S_l[j, k] = sum_m a_j(l,m) conj(a_k(l,m)) / (2l + 1)  (hputil.cross_spectra_device, csrc/spectra.hip)
# ---------------------------------------------------------------------------------------------------------------------
def invert_no_zero(x):
    """``1 / x`` where ``x != 0``, else 0 (what the reference takes from ``caput.algorithms.invert_no_zero``)."""
    x = np.asarray(x, dtype=np.float64)
    out = np.zeros_like(x)
    np.divide(1.0, x, out=out, where=x != 0)
    return out


def _pk_axes(chi, lmax, nkpar=None):
    """``(kpar, kperp, scale, Wk)`` of :func:`pk_flat` for shell distances ``chi``: the shells are ``dx = ptp(chi) /
    (N - 1)`` apart and span ``L = N dx`` (the range plus one channel width), ``kpar = 2 pi n / L`` for the
    ``N // 2 + 1`` modes of a real transform, ``kperp = l / mean(chi)``, ``scale = L mean(chi)^2`` and the window of a
    shell of width dx, ``Wk = sinc(kpar dx / 2 pi)`` (numpy's sinc)."""
    chi = np.asarray(chi, dtype=np.float64)
    N = len(chi)
    chi_mean = chi.mean()
    dx = np.ptp(chi) / (N - 1)
    L = N * dx
    n = np.arange(N // 2 + 1 if nkpar is None else nkpar)
    kpar = 2 * np.pi * n / L
    kperp = np.arange(lmax + 1) / chi_mean
    return kpar, kperp, L * chi_mean**2, np.sinc(kpar * dx / (2 * np.pi))


def _pk_contract(S):
    """``[L, N, N]`` Gram matrices (torch tensor, any device) -> ``[N // 2 + 1, L]``:
    ``out[n, l] = (1 / N^2) sum_jk cos(2 pi n (j - k) / N) S[l, j, k]``.

    This is ``sum_m |a^n_lm|^2 / (2l + 1)`` over both signs of m for ``a^n = rfft(a^j, axis=j)[n] / N``: the analysis
    is linear, so the transform along the slices commutes with it, and ``|sum_j w_nj a^j|^2`` summed over +-m keeps
    only the real part ``cos`` of ``w_nj conj(w_nk)``.  The phases are reduced exactly (``n (j - k) mod N`` in
    integers); the small contraction is a torch matmul."""
    import torch

    L, N = int(S.shape[0]), int(S.shape[1])
    if tuple(S.shape) != (L, N, N):
        raise ValueError("S must be [L, N, N]")
    n = np.arange(N // 2 + 1)[:, None, None]
    d = np.arange(N)[None, :, None] - np.arange(N)[None, None, :]
    W = np.cos(2 * np.pi * ((n * d) % N) / N) / float(N * N)
    W = torch.from_numpy(W.reshape(N // 2 + 1, N * N)).to(S.device)
    return torch.matmul(W, S.reshape(L, N * N).t())


def pk_flat_device(maps, chi, maps2=None, lmax=None, window=True):
    """:func:`pk_flat` on device maps ``[N, npix]`` (float64); ``chi`` a host array.  Returns ``(pk, kpar, kperp)``
    with ``pk`` a device tensor ``[N // 2 + 1, lmax + 1]`` and the axes host arrays."""
    import torch

    if maps2 is not None and tuple(maps.shape) != tuple(maps2.shape):
        raise ValueError(
            f"Shape of maps2 ({tuple(maps2.shape)}) is not compatible with maps ({tuple(maps.shape)})"
        )
    chi = np.asarray(chi, dtype=np.float64)
    nmaps, nside = check_maps(maps, chi, xname="chi", nmin=2)
    lmax = 3 * nside if lmax is None else int(lmax)
    S = hputil.cross_spectra_device(maps, maps2, lmax=lmax)       # hputil._weight / _iter: sphtrans_complex's analysis
    kpar, kperp, scale, Wk = _pk_axes(chi, lmax)
    pk = _pk_contract(S)
    fac = np.full(kpar.shape, scale) / (Wk**2 if window else 1.0)
    pk = pk * torch.from_numpy(fac).to(pk.device)[:, None]
    return pk, kpar, kperp


def pk_flat(maps, chi, maps2=None, lmax=None, window=True):
    """Estimate a 2D kpar, kperp power spectrum from a set of spherical maps (cora/signal/lssutil.py:293-376).

    Flat-sky, thin-shell approximation: the angular transform stands for the k_perp direction and the shells are
    taken as equally spaced.  The reference transforms along the shells first and then analyses every complex
    Fourier map; here the slices are analysed once and the Fourier sum is taken on their Gram matrix
    (:func:`_pk_contract`), which is the same number by linearity of the analysis
    (``hputil.map2alm_device`` with the ``_weight`` / ``_iter`` the reference configures for ``sphtrans_complex``).

    Parameters
    ----------
    maps : np.ndarray[N, npix]
        The Healpix maps at each distance.
    chi : np.ndarray[N]
        The distance to each shell in comoving Mpc/h.
    maps2 : np.ndarray[N, npix], optional
        A second set of maps: the cross-power spectrum is calculated instead.
    lmax : int, optional
        Maximum l to use (sets the maximum k_perp); default ``3 nside``, the reference's.
    window : bool, optional
        Undo the effective window function caused by the finite shell width.

    Returns
    -------
    pk : np.ndarray[N // 2 + 1, lmax + 1]
        The 2D power spectrum as k_par, k_perp.
    k_par, k_perp : np.ndarray
        The wavenumber along each axis.
    """
    import torch

    maps = np.asarray(maps)
    if maps2 is not None:
        maps2 = np.asarray(maps2)
        if maps.shape != maps2.shape:
            raise ValueError(
                f"Shape of maps2 ({maps2.shape}) is not compatible with maps ({maps.shape})"
            )
    check_maps(maps, np.asarray(chi), xname="chi", nmin=2)
    ctx = _lib.get_context()
    dev = torch.from_numpy(np.ascontiguousarray(maps, dtype=np.float64)).to(ctx.device)
    dev2 = None if maps2 is None else torch.from_numpy(np.ascontiguousarray(maps2, dtype=np.float64)).to(ctx.device)
    pk, kpar, kperp = pk_flat_device(dev, chi, dev2, lmax=lmax, window=window)
    return pk.cpu().numpy(), kpar, kperp


def _corrfunc_bin(clxx, chi, lmax, rmax, numr):
    """The host part of :func:`corrfunc`: spectra ``[n (n + 1) / 2, lmax + 1]`` in healpy's pair order -> ``(cf, r)``."""
    from .corrfunc import legendre_array

    chi = np.asarray(chi, dtype=np.float64)
    i, j = hputil.spectra_pair_order(len(chi))
    # spectrum k belongs to maps (i_k, j_k), at distances (chi[i_k], chi[j_k]): the reference's loop `for i: for j in
    # range(i, nx): (chi[j - i], chi[j])` runs in row order, and its (j - i, j) is what turns that into the diagonal order
    r1, r2 = chi[i][:, None], chi[j][:, None]
    mu = np.cos(np.linspace(0, np.pi, 2048))
    Pl = legendre_array(lmax, mu) * ((2 * np.arange(lmax + 1)[:, None] + 1) / (4 * np.pi))
    ctheta = np.dot(clxx, Pl)
    rc = ((r1 - r2) ** 2 + 2 * r1 * r2 * (1 - mu[None, :])) ** 0.5
    rbins = np.linspace(0, rmax, numr + 1)
    ind = np.digitize(rc.ravel(), rbins)
    norm = np.bincount(ind, minlength=numr + 2)
    csum = np.bincount(ind, weights=ctheta.ravel(), minlength=numr + 2)
    return (csum * invert_no_zero(norm))[1:-1].copy(), 0.5 * (rbins[1:] + rbins[:-1])


def corrfunc(maps, chi, lmax=None, rmax=1e3, numr=1024):
    """Estimate a 1D correlation function from a set of spherical maps (cora/signal/lssutil.py:379-443).

    The spectra of all pairs of slices (``hputil.anafast``, one Gram product on the device) are turned into angular
    correlations on 2048 angles by a Legendre sum and binned in the separation of the two shell points.

    Parameters
    ----------
    maps : np.ndarray[N, npix]
        The Healpix maps at each distance.
    chi : np.ndarray[N]
        The distance to each shell in comoving Mpc/h.
    lmax : int, optional
        Maximum l of the intermediate spectra (default ``3 nside - 1``, ``anafast``'s).
    rmax : float, optional
        The maximum r to bin up to.
    numr : int, optional
        The number of r bins.

    Returns
    -------
    cr : np.ndarray[numr]
        The 1D correlation function.
    r : np.ndarray[numr]
        The centres of the bins.
    """
    maps = np.asarray(maps)
    _, nside = check_maps(maps, np.asarray(chi), xname="chi")
    lmax = 3 * nside - 1 if lmax is None else int(lmax)
    clxx = hputil.anafast(maps, pol=False, lmax=lmax)
    return _corrfunc_bin(clxx, chi, lmax, rmax, numr)


def _pair_spectra(x, y):
    """(cl_xx, cl_yy, cl_xy) of two maps from one 2-map call (``anafast``'s defaults)."""
    cl = hputil.anafast(np.stack([np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)]), pol=False)
    return cl[0], cl[1], cl[2]


def ang_correlation(x, y):
    """The angular correlation ``r_l = C_l^xy / sqrt(C_l^xx C_l^yy)`` between two Healpix maps
    (cora/signal/lssutil.py:446-464)."""
    cl_xx, cl_yy, cl_xy = _pair_spectra(x, y)
    return cl_xy / (cl_xx * cl_yy) ** 0.5


def transfer(x, y):
    """The angular transfer function ``T_l = C_l^xy / C_l^yy``: the amount of the power in ``x`` that comes from the
    reference field ``y`` (cora/signal/lssutil.py:467-488)."""
    _, cl_yy, cl_xy = _pair_spectra(x, y)
    return cl_xy / cl_yy
