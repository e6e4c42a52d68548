"""Counterpart of cora/util/nputil.py on the hot path: matrix root + normal draws.

``matrix_root_manynull`` runs the library's batched factor kernel (K2) on a batch of one;
``complex_std_normal`` consumes a numpy generator exactly as the reference does (that IS
the definition of the seeded stream); ``DeviceRNG`` is this package's
counter-based alternative that never leaves the GPU; ``normal_rows_device`` is
``rng.normal(scale=s[:, None], size=(nrow, ncol))`` stored or added in place on the device,
for a PCG64 generator straight out of the device generator's emit pass.
"""
import numpy as np

from .. import _lib


class DeviceRNG:
    """Counter-based (Philox4x32-10 + Box-Muller) N(0,1) stream generated on the GPU.

    Pass an instance as ``rng`` to ``skysim.mkfullsky`` to keep the draw on the device.
    Element k of the stream (in the order of cora/core/skysim.py:114-121, see
    include/corahip.h "stream order") depends only on (seed, k): reproducible for any
    number of GPUs.  Each ``mkfullsky`` call advances ``seed`` by one.
    """

    def __init__(self, seed=0):
        self.seed = int(seed)

    def next_seed(self):
        s = self.seed
        self.seed += 1
        return s


def matrix_root_manynull(mat, threshold=1e-16, truncate=True):
    """Square root of a symmetric PSD matrix (cora/util/nputil.py:51-101).

    Cholesky first; if a pivot is not positive, eigen-decomposition with eigenvalues
    below ``max * threshold`` zeroed.  With ``truncate`` the root keeps only the columns
    of the non-zero eigenvalues and ``(root, num_pos)`` is returned.
    """
    mat = np.ascontiguousarray(mat, dtype=np.float64)
    if mat.ndim != 2 or mat.shape[0] != mat.shape[1]:
        raise ValueError("expected square matrix")
    ctx = _lib.get_context()
    n = mat.shape[0]
    T, info = ctx.factor_batched(ctx.to_device(mat[np.newaxis]), jitter_rel=0.0, eig_thresh=threshold)
    root = T[0].cpu().numpy()
    branch = int(info[0].item())
    if branch == 0:
        num_pos = n
    else:
        nz = np.flatnonzero(np.abs(root).sum(axis=0) > 0)
        num_pos = len(nz)
        if truncate:
            # columns are in ascending-eigenvalue order (scipy.linalg.eigh order): keep the last num_pos
            root = root[:, n - num_pos:] if num_pos > 0 else root[:, n:]
            root = root[np.newaxis]  # the reference returns [1, N, num_pos] here (nputil.py:92-96 quirk)
    if truncate:
        return root, num_pos
    return root


def complex_std_normal(shape, rng=None):
    """Complex standard normals (cora/util/nputil.py:104-125): the real block is drawn
    first, then the imaginary block; ``rng=None`` uses numpy's legacy global state."""
    if rng is None:
        re = np.random.standard_normal(shape)
        im = np.random.standard_normal(shape)
    else:
        re = rng.standard_normal(shape)
        im = rng.standard_normal(shape)
    return (re + 1.0j * im) / 2**0.5


_HOST_CHUNK = 1 << 22          # values per rng.normal call of the host route of normal_rows_device


def normal_rows_device(rng, scale, ncol, out, row_off=None, accumulate=False):
    """``rng.normal(scale=scale[:, None], size=(len(scale), ncol))`` written (``accumulate=False``) or added in place to
    the device tensor ``out`` - what ``AddCorrelatedShotNoise`` and ``GenerateFlatSpectrumMap`` draw
    (cora/signal/lss.py:1297-1300, 1538-1540) - with the bits numpy gives for the same generator.

    Row ``r`` goes to ``out.view(-1)[row_off[r] : row_off[r] + ncol]`` (``row_off`` None: ``r * ncol``); ``scale`` is a
    host array [nrow], ``row_off`` host integers [nrow], ``out`` a contiguous device float64 tensor.

    A ``Generator`` on PCG64 is continued on the device (``corahip_normal_rows_pcg64``: the values leave the
    generator's emit pass scaled and placed, no buffer of normals exists) under ``bit_generator.lock``, and is left
    where numpy would leave it.  Any other ``Generator`` - and a PCG64 one while a draw session holds the context's
    tables (``CORAHIP_ESTATE``) - takes the host route: ``rng.normal`` in chunks of rows, each uploaded and stored or
    added.  ``rng`` must be a ``numpy.random.Generator``: there is no legacy global stream here, the reference's tasks
    always hold a generator; pass ``numpy.random.default_rng(seed)``.  Returns ``out``."""
    from ..core import skysim

    if not isinstance(rng, np.random.Generator):
        raise TypeError("rng must be a numpy.random.Generator (got %s); use numpy.random.default_rng(seed)" % type(rng).__name__)
    scale = np.ascontiguousarray(scale, dtype=np.float64)
    if scale.ndim != 1:
        raise ValueError("scale must be one value per row (got shape %s)" % (scale.shape,))
    nrow, ncol = len(scale), int(ncol)
    ctx = _lib.get_context()
    if skysim._is_pcg64_generator(rng):
        bg = rng.bit_generator
        with bg.lock:                                          # the lock numpy's own draws hold
            st = bg.state
            s, inc = int(st["state"]["state"]), int(st["state"]["inc"])
            try:
                nraw = ctx.normal_rows_pcg64(s, inc, scale, ncol, out, row_off=row_off, accumulate=accumulate)
            except _lib.CoraHipError as e:
                if e.status != _lib.CORAHIP_ESTATE:
                    raise
                nraw = None                                    # a draw session is pending: the host route, outside the lock
            else:
                st["state"]["state"] = _lib.pcg64_advance(s, inc, nraw)
                bg.state = st                                  # (has_uint32 / uinteger untouched, as normal leaves them)
        if nraw is not None:
            return out
    # the host route (the wrapper's argument checks first: nothing is drawn for a call that is refused)
    _, offs = _lib.Context.check_rows(scale, ncol, out, row_off)
    if nrow == 0 or ncol == 0:
        return out
    if offs is None:
        offs = np.arange(nrow, dtype=np.int64) * ncol
    flat = out.view(-1)
    per = max(1, _HOST_CHUNK // ncol)
    for r0 in range(0, nrow, per):
        r1 = min(nrow, r0 + per)
        chunk = ctx.to_device(rng.normal(scale=scale[r0:r1, np.newaxis], size=(r1 - r0, ncol)))
        for r in range(r0, r1):
            dst = flat[int(offs[r]):int(offs[r]) + ncol]
            if accumulate:
                dst.add_(chunk[r - r0])
            else:
                dst.copy_(chunk[r - r0])
    return out


def save_ndarray_list(fname, la):
    """cora/util/nputil.py:12-27."""
    np.savez(fname, **{repr(i): v for i, v in enumerate(la)})


def load_ndarray_list(fname):
    """cora/util/nputil.py:30-48."""
    d = np.load(fname)
    return [v for _, v in sorted(d.items(), key=lambda kv: int(kv[0]))]
