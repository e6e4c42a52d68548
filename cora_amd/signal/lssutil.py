"""Counterpart of the functions of cora/signal/lssutil.py that the Zel'dovich step uses: ``gradient``
(lssutil.py:225-261), ``assert_shape`` (lssutil.py:630-640).  The angular derivatives come from the derivative
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
