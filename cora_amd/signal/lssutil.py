"""Counterpart of the functions of cora/signal/lssutil.py that the LSS steps use: ``gradient``
(lssutil.py:225-261), ``assert_shape`` (lssutil.py:630-640), ``diff2`` (:99-185), ``calculate_width`` (:491-515),
``exponential_FoG_kernel`` (:518-589), ``lognormal_transform`` (:592-627); the last four with the kernels of
csrc/lsschain.hip.  The angular derivatives come from the derivative
synthesis (csrc/sht_der1.hip), the radial one from ``radial_gradient_kernel``; everything stays on the device in
the ``_device`` forms."""
import numpy as np

from .. import _lib
from ..util import hputil

# slices that go through analysis + derivative synthesis together (a multiple of 4: whole channel groups)
SLICE_CHUNK = 16


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
