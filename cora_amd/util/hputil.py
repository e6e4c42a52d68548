"""Counterpart of the part of cora/util/hputil.py on the hot path.

``sphtrans_inv_real`` / ``sphtrans_inv_sky`` call the library's HEALPix synthesis
(K4 Legendre MFMA contraction + K5 ring FFT) where the reference calls
``healpy.alm2map`` (cora/util/hputil.py:388-391); all channels go through in one batch.
``sphtrans_real`` / ``sphtrans_sky`` / ``sph_ps`` call the adjoint kernels where the reference
calls ``healpy.map2alm(use_weights=True, iter=2)`` (cora/util/hputil.py:46-47,195-234,460-497,607-619).
"""
import contextlib

import numpy as np

from .. import _lib


def nside2npix(nside):
    return 12 * int(nside) * int(nside)


def ang2pix(nside, theta, phi, lonlat=False):
    """RING pixel index of a direction (what the reference takes from ``healpy.ang2pix`` in
    scripts/makesky.py:412-420): colatitude/longitude in radians, or (lon, lat) in degrees with
    ``lonlat=True``.  Standard HEALPix geometry (Gorski et al. 2005, eqs. 2-9)."""
    nside = int(nside)
    theta = np.asarray(theta, dtype=np.float64)
    phi = np.asarray(phi, dtype=np.float64)
    if lonlat:
        theta, phi = np.pi / 2.0 - np.radians(phi), np.radians(theta)
    z = np.cos(theta)
    za = np.abs(z)
    tt = np.mod(phi, 2.0 * np.pi) / (np.pi / 2.0)          # [0, 4)
    npix = 12 * nside * nside
    ncap = 2 * nside * (nside - 1)
    # equatorial belt
    t1 = nside * (0.5 + tt)
    t2 = nside * z * 0.75
    jp = np.floor(t1 - t2).astype(np.int64)
    jm = np.floor(t1 + t2).astype(np.int64)
    ir = nside + 1 + jp - jm
    kshift = 1 - (ir & 1)
    ip = np.mod((jp + jm - nside + kshift + 1) // 2, 4 * nside)
    belt = ncap + (ir - 1) * 4 * nside + ip
    # polar caps
    tp = tt - np.floor(tt)
    tmp = nside * np.sqrt(3.0 * (1.0 - za))
    jp = np.floor(tp * tmp).astype(np.int64)
    jm = np.floor((1.0 - tp) * tmp).astype(np.int64)
    irc = jp + jm + 1
    ipc = np.mod(np.floor(tt * irc).astype(np.int64), 4 * irc)
    cap = np.where(z > 0, 2 * irc * (irc - 1) + ipc, npix - 2 * irc * (irc + 1) + ipc)
    out = np.where(za <= 2.0 / 3.0, belt, cap)
    return out if out.ndim else int(out)


def pix2ang(nside, ipix):
    """(theta, phi) of RING pixel centres (what the reference takes from ``healpy.pix2ang``): caps
    z = 1 - i^2/(3 nside^2), phi = (j + 1/2) pi/(2 i); belt z = 4/3 - 2 i/(3 nside), phi = (j + s/2) pi/(2 nside)."""
    z, phi = _pix2zphi(nside, ipix)
    return np.arccos(z), phi


def _pix2zphi(nside, ipix):
    """(z, phi) of RING pixel centres; csrc/pmesh.hip repeats this arithmetic operation for operation."""
    nside = int(nside)
    ipix = np.asarray(ipix, dtype=np.int64)
    npix = 12 * nside * nside
    ncap = 2 * nside * (nside - 1)
    p = np.where(ipix >= npix - ncap, npix - 1 - ipix, ipix)             # mirror the south cap onto the north
    # north cap: ring i (1-based) holds pixels 2 i (i - 1) .. 2 i (i + 1) - 1
    i_cap = ((1 + np.sqrt(1 + 2 * np.minimum(p, max(ncap - 1, 0)).astype(np.float64))) / 2).astype(np.int64)
    i_cap = np.where(2 * i_cap * (i_cap - 1) > p, i_cap - 1, i_cap)
    i_cap = np.where(2 * i_cap * (i_cap + 1) <= p, i_cap + 1, i_cap)
    i_cap = np.maximum(i_cap, 1)
    j_cap = p - 2 * i_cap * (i_cap - 1)
    z_cap = 1.0 - i_cap.astype(np.float64) ** 2 / (3.0 * nside * nside)
    phi_cap = (j_cap + 0.5) * np.pi / (2.0 * i_cap)
    # equatorial belt
    pb = ipix - ncap
    i_b = pb // (4 * nside) + nside
    j_b = pb % (4 * nside)
    s_b = (i_b - nside + 1) & 1
    z_b = 4.0 / 3.0 - 2.0 * i_b / (3.0 * nside)
    phi_b = (j_b + 0.5 * s_b) * np.pi / (2.0 * nside)
    in_n = ipix < ncap
    in_s = ipix >= npix - ncap
    z = np.where(in_n, z_cap, np.where(in_s, -z_cap, z_b))
    # a mirrored south-cap pixel runs backwards in phi on its ring
    phi = np.where(in_n, phi_cap, np.where(in_s, 2.0 * np.pi - phi_cap, phi_b))
    return z, phi


def pix2vec(nside, ipix):
    """Unit vectors (x, y, z) of RING pixel centres, as ``healpy.pix2vec``: sin(theta) = sqrt((1 - z)(1 + z))."""
    z, phi = _pix2zphi(nside, ipix)
    st = np.sqrt((1.0 - z) * (1.0 + z))
    return st * np.cos(phi), st * np.sin(phi), z


def ang2vec(theta, phi):
    """Unit vectors [..., 3] of directions (colatitude, longitude in radians), as ``healpy.ang2vec``."""
    theta = np.asarray(theta, dtype=np.float64)
    phi = np.asarray(phi, dtype=np.float64)
    st = np.sin(theta)
    return np.stack([st * np.cos(phi), st * np.sin(phi), np.cos(theta)], axis=-1)


def nside2resol(nside):
    """Approximate pixel size in radians, sqrt(4 pi / npix) (``healpy.nside2resol``)."""
    return np.sqrt(4.0 * np.pi / nside2npix(nside))


def get_all_neighbours(nside, ipix):
    """The 8 RING neighbours of each pixel of ``ipix`` as ``healpy.get_all_neighbours(nside, ipix)`` gives them:
    [8, n] (or [8] for a scalar) in the order SW, W, NW, N, NE, E, SE, S, -1 where a pixel has none.  The table comes
    from the device (corahip_healpix_neighbours)."""
    ipix = np.asarray(ipix, dtype=np.int64)
    npix = nside2npix(nside)
    if ipix.size and (ipix.min() < 0 or ipix.max() >= npix):
        raise ValueError("pixel index out of range for nside %d" % int(nside))
    ctx = _lib.get_context()
    table = ctx.healpix_neighbours(int(nside))
    rows = ctx.to_device(ipix.reshape(-1), dtype=np.int64)
    nb = table[rows, 1:].cpu().numpy()
    return nb.T.astype(np.int64).reshape((8,) + ipix.shape)


def ang_positions(nside):
    """Angular position [theta, phi] of every pixel: [npix, 2] (cora/util/hputil.py:53-73)."""
    npix = nside2npix(int(nside))
    angpos = np.empty([npix, 2], dtype=np.float64)
    angpos[:, 0], angpos[:, 1] = pix2ang(nside, np.arange(npix))
    return angpos


def nside_for_lmax(lmax, accuracy_boost=1):
    """cora/util/hputil.py:76-90."""
    return int(2 ** (accuracy_boost + np.ceil(np.log((lmax + 1) / 3.0) / np.log(2.0))))


def _make_full_alm(alm_half, centered=False):
    """a_lm for m >= 0 -> both signs of m, using a_{l,-m} = (-1)^m conj(a_lm) (cora/util/hputil.py:155-174).
    Output [..., l, 2 mmax - 1]: FFT order (m >= 0 first, then m = -(mmax-1)..-1) or, ``centered``, m ascending."""
    lmax, mmax = alm_half.shape[-2:]
    alm = np.zeros(alm_half.shape[:-2] + (lmax, 2 * mmax - 1), dtype=alm_half.dtype)
    neg = ((-1) ** np.arange(mmax)[:0:-1]) * alm_half[..., :, :0:-1].conj()
    if not centered:
        alm[..., :mmax] = alm_half
        alm[..., mmax:] = neg
    else:
        alm[..., (mmax - 1):] = alm_half
        alm[..., : (mmax - 1)] = neg
    return alm


def _make_half_alm(alm_full):
    """[l, 2 lside - 1] (FFT order in m) -> the m >= 0 coefficients of its REAL part: the projection
    (a_lm + (-1)^m conj(a_{l,-m})) / 2 (cora/util/hputil.py:177-192)."""
    lside = alm_full.shape[-2]
    alm = np.zeros(alm_full.shape[:-2] + (lside, lside), dtype=alm_full.dtype)
    alm[..., 0] = alm_full[..., :, 0]
    for mi in range(1, lside):
        alm[..., mi] = 0.5 * (alm_full[..., mi] + (-1) ** mi * alm_full[..., -mi].conj())
    return alm


def unpack_alm(alm, lmax, fullm=False):
    """Healpix-packed a_lm -> 2D [l, m] (cora/util/hputil.py:93-121)."""
    almarray = np.zeros((lmax + 1, lmax + 1), dtype=alm.dtype)
    (almarray.T)[np.triu_indices(lmax + 1)] = alm
    if fullm:
        full = np.zeros((lmax + 1, 2 * lmax + 1), dtype=alm.dtype)
        full[:, : lmax + 1] = almarray
        mm = np.arange(1, lmax + 1)
        full[:, -mm] = ((-1.0) ** mm) * almarray[:, mm].conj()
        almarray = full
    return almarray


def pack_alm(almarray, lmax=None):
    """2D [l, m] a_lm -> Healpix packing, idx(l,m) = m(2 lmax+1-m)/2 + l (hputil.py:124-152)."""
    if (2 * almarray.shape[1] - 1) == almarray.shape[0]:
        almarray = _make_half_alm(almarray)
    if not lmax:
        lmax = almarray.shape[0] - 1
    return (almarray.T)[np.triu_indices(lmax + 1)]


def _synth(alm_list, nside):
    """alm_list: [n, L, L] complex -> [n, npix] maps on the GPU."""
    n, L, _ = alm_list.shape
    lmax = L - 1
    packed = np.stack([pack_alm(a) for a in alm_list]).astype(np.complex128)
    ctx = _lib.get_context()
    import torch

    alm_dev = ctx.alm_packed_to_dev(torch.from_numpy(np.ascontiguousarray(packed)).to(ctx.device), lmax)
    maps = ctx.alm2map(alm_dev, int(nside), lmax, n)
    return _lib.get_context().to_host(maps)


def sphtrans_inv_real(alm, nside):
    """Inverse SHT onto a real field (cora/util/hputil.py:369-391)."""
    if alm.shape[1] != alm.shape[0]:
        raise Exception("a_lm array wrong shape.")
    return _synth(np.asarray(alm)[np.newaxis], nside)[0]


def _synth_pol(alm_e, alm_b, nside):
    """alm_e, alm_b: [n, L, L] complex -> (Q, U) maps [n, npix] each (spin-2 synthesis on the GPU)."""
    import torch

    n, L, _ = alm_e.shape
    lmax = L - 1
    packed = np.empty((2 * n, L * (L + 1) // 2), dtype=np.complex128)
    for i in range(n):
        packed[2 * i] = pack_alm(alm_e[i])
        packed[2 * i + 1] = pack_alm(alm_b[i])
    ctx = _lib.get_context()
    out = np.empty((2 * n, nside2npix(nside)))
    # the spin-2 entry point wants its channel count in whole groups of 8 (or 5..7 mod 8): chunks of 4 fields
    for c0 in range(0, 2 * n, 8):
        c1 = min(c0 + 8, 2 * n)
        blk = packed[c0:c1]
        if (c1 - c0) % 8 not in (0, 6):          # pad with zero fields to 8 channels
            blk = np.concatenate([blk, np.zeros((8 - (c1 - c0), packed.shape[1]), dtype=np.complex128)])
        dev = ctx.alm_packed_to_dev(torch.from_numpy(np.ascontiguousarray(blk)).to(ctx.device), lmax)
        maps = ctx.alm2map_spin2(dev, int(nside), lmax, blk.shape[0])
        out[c0:c1] = maps[: c1 - c0].cpu().numpy()
    return out[0::2], out[1::2]


def sphtrans_inv_real_pol(alm, nside):
    """Inverse transform onto a real polarised field: alm [npol, L, L] for T, E, B (and V) -> T, Q, U (and V) maps
    [npol, npix] (cora/util/hputil.py:394-432; healpy.alm2map of the three packed arrays).  Q and U come from the
    spin-2 synthesis kernel (convention: Zaldarriaga & Seljak 1997, the one HEALPix documents), T and V from the
    scalar one."""
    alm = np.asarray(alm)
    npol = alm.shape[0]
    if alm.shape[1] != alm.shape[2] or not (npol == 3 or npol == 4):
        raise Exception("a_lm array wrong shape.")
    maps = np.zeros((npol, nside2npix(nside)), dtype=np.float64)
    scal = _synth(alm[[0] + ([3] if npol == 4 else [])], nside)
    maps[0] = scal[0]
    q, u = _synth_pol(alm[1:2], alm[2:3], nside)
    maps[1], maps[2] = q[0], u[0]
    if npol == 4:
        maps[3] = scal[1]
    return maps


def sphtrans_inv_sky(alm, nside):
    """[freq, pol, l, m] a_lm -> [freq, pol, npix] sky (cora/util/hputil.py:500-531): the polarised transform when
    the pol axis has 3 or 4 entries (T, E, B[, V] -> T, Q, U[, V]), else the scalar one; all frequencies in batches."""
    alm = np.asarray(alm)
    nfreq, npol = alm.shape[0], alm.shape[1]
    if alm.shape[3] != alm.shape[2]:
        raise Exception("a_lm array wrong shape.")
    sky = np.empty((nfreq, npol, nside2npix(nside)), dtype=np.float64)
    if npol >= 3:
        if npol > 4:
            raise Exception("a_lm array wrong shape.")
        sky[:, 0] = _synth(alm[:, 0], nside)
        sky[:, 1], sky[:, 2] = _synth_pol(alm[:, 1], alm[:, 2], nside)
        if npol == 4:
            sky[:, 3] = _synth(alm[:, 3], nside)
        return sky
    for p in range(npol):
        sky[:, p] = _synth(np.asarray(alm[:, p]), nside)
    return sky


# ------------------------------------------------------------------------------------
# analysis: healpy.map2alm(use_weights=_weight, iter=_iter) as the reference configures it
# ------------------------------------------------------------------------------------
_weight = True   # cora/util/hputil.py:46
_iter = 2        # cora/util/hputil.py:47
_spin2_method = "composed"   # quadrature pass of the (Q, U) analysis: "composed" (six scalar passes, csrc/sht_polana.hip)
                             # or "native" (one spin-2 Legendre pass, csrc/sht_polana_native.hip)
_ring_weight_cache = {}


def ring_weights(nside, lmax_exact=None):
    """Quadrature weights of the 2 nside north rings (equator included).

    healpy reads these from the HEALPix data file weight_ring_n<nside>.fits; that file is data of a
    dependency which is not available to this package, so the defining property is used: the
    minimum-norm correction to uniform weights that integrates the zonal P_l(z), even l <= lmax_exact
    (default 3 nside), exactly.  Host numpy, once per nside (cached)."""
    key = (int(nside), lmax_exact)
    if key not in _ring_weight_cache:
        nside = int(nside)
        npair = 2 * nside
        npix = nside2npix(nside)
        i = np.arange(1, npair + 1, dtype=np.float64)
        cap = i < nside
        z = np.where(cap, 1.0 - i * i / (3.0 * nside * nside), 4.0 / 3.0 - 2.0 * i / (3.0 * nside))
        cnt = np.where(cap, 4.0 * i, 4.0 * nside) * 2.0
        cnt[-1] = 4.0 * nside                       # the equator ring has no mirror
        lx = 3 * nside if lmax_exact is None else int(lmax_exact)
        P = np.empty((lx + 1, npair))
        P[0] = 1.0
        if lx >= 1:
            P[1] = z
        for l in range(2, lx + 1):
            P[l] = ((2 * l - 1) * z * P[l - 1] - (l - 1) * P[l - 2]) / l
        M = P[0::2] * (cnt * 4.0 * np.pi / npix)[None, :]
        rhs = np.zeros(M.shape[0])
        rhs[0] = 4.0 * np.pi
        _ring_weight_cache[key] = 1.0 + np.linalg.lstsq(M, rhs - M.sum(axis=1), rcond=None)[0]
    return _ring_weight_cache[key]


def map2alm_device(maps, nside, lmax, use_weights=None, niter=None):
    """Device maps [n, npix] -> alm_dev: quadrature pass + `niter` Jacobi refinements
    alm <- alm + A(map - S alm), i.e. healpy.map2alm(..., use_weights, iter) for all maps at once."""
    ctx = _lib.get_context()
    use_weights = _weight if use_weights is None else use_weights
    niter = _iter if niter is None else niter
    w = ctx.to_device(ring_weights(nside)) if use_weights else None
    n = maps.shape[0]
    alm = ctx.map2alm(maps, int(nside), int(lmax), w)
    for _ in range(niter):
        resid = maps - ctx.alm2map(alm, int(nside), int(lmax), n)
        alm = alm + ctx.map2alm(resid, int(nside), int(lmax), w)
        del resid
    return alm


def _resolve_spin2_method(method=None):
    """``method`` of the (Q, U) analysis: None = the module's ``_spin2_method``; checked before any device work."""
    method = _spin2_method if method is None else method
    if method not in ("composed", "native"):
        raise ValueError("method must be 'composed' or 'native' (got %r)" % (method,))
    return method


@contextlib.contextmanager
def spin2_method(method):
    """``with hputil.spin2_method("native"): ...`` - the module's ``_spin2_method`` for the duration of the block: the
    route of :func:`map2alm_sky_device`, :func:`map2alm_sky_bytes`, :func:`cross_spectra_pol_device`,
    :func:`anafast_pol` and everything built on them (``skysim.clarray_from_maps`` on polarised stacks), and of
    :func:`map2alm_pol_device` called without ``method``.  Any value but "composed" / "native" raises ``ValueError``."""
    global _spin2_method
    method = _resolve_spin2_method(method)
    saved, _spin2_method = _spin2_method, method
    try:
        yield method
    finally:
        _spin2_method = saved


def map2alm_pol_device(maps_qu, nside, lmax, use_weights=None, niter=None, method=None):
    """Device maps [2 n, npix], (Q_f, U_f) interleaved -> alm_dev with (E_f, B_f) interleaved: the (Q, U) half of
    healpy.map2alm([T, Q, U], use_weights, iter) - a quadrature pass composed of scalar passes over ring-scaled
    maps (csrc/sht_polana.hip) plus `niter` refinements alm <- alm + A(map - S alm) with the spin-2 synthesis.
    ``method="native"`` runs every quadrature pass as one spin-2 Legendre pass (``Context.map2alm_spin2_native``) on the
    maps as they are; None = the module's ``_spin2_method``, any other value raises ``ValueError``."""
    method = _resolve_spin2_method(method)
    ctx = _lib.get_context()
    analyse = ctx.map2alm_spin2_native if method == "native" else ctx.map2alm_spin2
    use_weights = _weight if use_weights is None else use_weights
    niter = _iter if niter is None else niter
    w = ctx.to_device(ring_weights(nside)) if use_weights else None
    n2 = maps_qu.shape[0]
    alm = analyse(maps_qu, int(nside), int(lmax), w)
    nnu_pad = 4 * alm.shape[1]
    for _ in range(niter):
        back = ctx.alm2map_spin2(alm, int(nside), int(lmax), nnu_pad)[:n2]
        alm = alm + analyse(maps_qu - back, int(nside), int(lmax), w)
        del back
    return alm


def _analyse_pol(q, u, lmax):
    """Host (Q, U) maps [n, npix] each -> (E, B) alm[l, m] arrays [n, lmax+1, lmax+1] each."""
    import torch

    q = np.ascontiguousarray(q, dtype=np.float64)
    n, npix = q.shape
    nside = int(round(np.sqrt(npix / 12.0)))
    if 12 * nside * nside != npix:
        raise ValueError("Wrong pixel number (it is not 12*nside**2)")   # healpy.npix2nside
    qu = np.empty((2 * n, npix))
    qu[0::2], qu[1::2] = q, u
    ctx = _lib.get_context()
    alm = map2alm_pol_device(torch.from_numpy(qu).to(ctx.device), nside, lmax)
    sq = ctx.alm_dev_to_square(alm, lmax, 4 * alm.shape[1]).cpu().numpy()[: 2 * n, 0]   # (padding channels dropped)
    return sq[0::2], sq[1::2]


def _analyse(hpmaps, lmax):
    """[n, npix] host maps -> [n, lmax+1, lmax+1] complex alm[l, m] (m > l entries zero)."""
    import torch

    hpmaps = np.ascontiguousarray(hpmaps, dtype=np.float64)
    n, npix = hpmaps.shape
    nside = int(round(np.sqrt(npix / 12.0)))
    if 12 * nside * nside != npix:
        raise ValueError("Wrong pixel number (it is not 12*nside**2)")   # healpy.npix2nside
    ctx = _lib.get_context()
    alm = map2alm_device(torch.from_numpy(hpmaps).to(ctx.device), nside, lmax)
    return ctx.alm_dev_to_square(alm, lmax, n).cpu().numpy()[:, 0]


def sphtrans_real(hpmap, lmax=None, lside=None):
    """Spherical harmonic transform of a real map -> alm[l, m], m >= 0 (cora/util/hputil.py:195-234)."""
    hpmap = np.asarray(hpmap)
    if lmax is None:
        lmax = 3 * int(round(np.sqrt(hpmap.size / 12.0))) - 1
    if lside is None or lside < lmax:
        lside = lmax
    alm = np.zeros([lside + 1, lside + 1], dtype=np.complex128)
    alm[: lmax + 1, : lmax + 1] = _analyse(hpmap.reshape(1, -1), lmax)[0]
    return alm


def sphtrans_real_pol(hpmaps, lmax=None, lside=None):
    """T, Q, U (and V) maps [npol, npix] -> a^T, a^E, a^B (and a^V) as alm[pol, l, m], m >= 0
    (cora/util/hputil.py:274-323: healpy.map2alm of the T, Q, U triple, V on its own)."""
    hpmaps = np.ascontiguousarray(hpmaps, dtype=np.float64)
    npol = len(hpmaps)
    if lmax is None:
        lmax = 3 * int(round(np.sqrt(hpmaps[0].size / 12.0))) - 1
    if lside is None or lside < lmax:
        lside = lmax
    alms = np.zeros([npol, lside + 1, lside + 1], dtype=np.complex128)
    scal = _analyse(hpmaps[[0] + ([3] if npol == 4 else [])], lmax)
    alms[0, : lmax + 1, : lmax + 1] = scal[0]
    e, b = _analyse_pol(hpmaps[1:2], hpmaps[2:3], lmax)
    alms[1, : lmax + 1, : lmax + 1], alms[2, : lmax + 1, : lmax + 1] = e[0], b[0]
    if npol == 4:
        alms[3, : lmax + 1, : lmax + 1] = scal[1]
    return alms


def sphtrans_complex_pol(hpmaps, lmax=None, centered=False, lside=None):
    """Complex T, Q, U (and V) maps -> a_lm for both signs of m (cora/util/hputil.py:326-366)."""
    hpmaps = np.asarray(hpmaps)
    if lmax is None:
        lmax = 3 * int(round(np.sqrt(hpmaps[0].size / 12.0))) - 1
    alm = _make_full_alm(sphtrans_real_pol(hpmaps.real, lmax=lmax, lside=lside), centered=centered)
    alm += 1.0j * _make_full_alm(sphtrans_real_pol(hpmaps.imag, lmax=lmax, lside=lside), centered=centered)
    return alm


def sphtrans_sky(skymap, lmax=None):
    """[freq, npix] (or [freq, pol, npix]) sky -> alm [freq, (pol,) l, m] (cora/util/hputil.py:460-497).
    All frequency slices go through the GPU in one batch; with 3 or 4 polarisation components the
    (Q, U) planes take the spin-2 analysis, T (and V) the scalar one."""
    skymap = np.asarray(skymap)
    if skymap.ndim == 3 and skymap.shape[1] >= 3:
        if skymap.shape[1] > 4:
            raise Exception("Wrong number of polarisation components.")
        if lmax is None:
            lmax = 3 * int(round(np.sqrt(skymap.shape[-1] / 12.0))) - 1
        nfreq, npol = skymap.shape[:2]
        alm = np.zeros((nfreq, npol, lmax + 1, lmax + 1), dtype=np.complex128)
        alm[:, 0] = _analyse(skymap[:, 0].astype(np.float64), lmax)
        alm[:, 1], alm[:, 2] = _analyse_pol(skymap[:, 1], skymap[:, 2], lmax)
        if npol == 4:
            alm[:, 3] = _analyse(skymap[:, 3].astype(np.float64), lmax)
        return alm
    if lmax is None:
        lmax = 3 * int(round(np.sqrt(skymap.shape[-1] / 12.0))) - 1
    flat = skymap.reshape(-1, skymap.shape[-1]).astype(np.float64)
    alm = _analyse(flat, lmax)
    return alm.reshape(skymap.shape[:-1] + (lmax + 1, lmax + 1))


def sphtrans_complex(hpmap, lmax=None, centered=False, lside=None):
    """Spherical harmonic transform of a complex map: a_lm for both signs of m (cora/util/hputil.py:237-263)."""
    hpmap = np.asarray(hpmap)
    if lmax is None:
        lmax = 3 * int(round(np.sqrt(hpmap.size / 12.0))) - 1
    both = _analyse(np.stack([hpmap.real, hpmap.imag]), lmax)
    if lside is not None and lside > lmax:
        pad = np.zeros((2, lside + 1, lside + 1), dtype=np.complex128)
        pad[:, : lmax + 1, : lmax + 1] = both
        both = pad
    return _make_full_alm(both[0], centered=centered) + 1.0j * _make_full_alm(both[1], centered=centered)


def sphtrans_inv_complex(alm, nside):
    """Inverse transform onto a complex field from a_lm with both signs of m (cora/util/hputil.py:435-457).

    Mirrors the reference formula exactly, including its sign: the imaginary part is built from
    ``1j * (a - a_real)`` = minus the coefficients of Im f, so the result is the complex CONJUGATE of the field
    whose :func:`sphtrans_complex` is ``alm``; and all of a_l0 goes to the real part (m = 0 modes of Im f drop)."""
    alm = np.asarray(alm)
    if alm.shape[1] != (2 * alm.shape[0] - 1):
        raise Exception("a_lm array wrong shape: " + repr(alm.shape))
    almr = _make_half_alm(alm)
    almi = 1.0j * (alm[:, : almr.shape[1]] - almr)
    both = _synth(np.stack([almr, almi]), nside)
    return both[0] + 1.0j * both[1]


def sph_ps(map1, map2=None, lmax=None):
    """Angular (cross) power spectrum of maps (cora/util/hputil.py:607-619).

    The reference's test ``if map is not None`` looks at the builtin ``map`` and is always true, so its
    auto-spectrum branch never runs and ``map2=None`` fails inside healpy; here ``map2=None`` means the
    auto spectrum, which is what the signature documents."""
    map1 = np.asarray(map1)
    lmax = lmax if lmax is not None else (3 * int(round(np.sqrt(map1.size / 12.0))) - 1)
    if map2 is None:
        alm1 = alm2 = sphtrans_real(map1, lmax)
    else:
        both = _analyse(np.stack([map1, np.asarray(map2)]), lmax)
        alm1, alm2 = both[0], both[1]
    prod = alm1 * alm2.conj()
    s = prod[:, 0] + 2 * prod[:, 1:].sum(axis=1).real
    return s / (2.0 * np.arange(lmax + 1) + 1.0)


# ------------------------------------------------------------------------------------
# derivative synthesis: healpy.alm2map_der1 (cora/signal/lssutil.py:225-261)
# ------------------------------------------------------------------------------------
def alm2map_der1_device(alm_dev, nside, lmax, nnu, **scales):
    """alm_dev [nalm, G, 2, 4] of ``nnu`` fields -> device ``(dT/dtheta, (1/sin theta) dT/dphi)``, [nnu, npix] each:
    rows 1 and 2 of ``healpy.alm2map_der1`` for all fields at once (``Context.alm2map_der1``; keywords
    ``scale_theta``, ``scale_phi``, ``phi_extra``, ``out``, ``max_bytes`` are passed through)."""
    return _lib.get_context().alm2map_der1(alm_dev, int(nside), int(lmax), int(nnu), **scales)


def alm2map_der1(alm, nside):
    """``healpy.alm2map_der1(alm, nside)`` for one packed complex ``alm`` (lmax from its length): host
    ``ndarray[3, npix]`` = ``[T, dT/dtheta, (1/sin theta) dT/dphi]``, RING order.  The derivatives are composed from
    three scalar syntheses per field (csrc/sht_der1.hip)."""
    import torch

    alm = np.ascontiguousarray(alm, dtype=np.complex128)
    if alm.ndim != 1:
        raise ValueError("alm2map_der1 takes one packed alm array (got shape %r)" % (alm.shape,))
    lmax = int(round((-3 + np.sqrt(1 + 8 * alm.size)) / 2))
    if (lmax + 1) * (lmax + 2) // 2 != alm.size:
        raise ValueError("alm has %d entries, not (lmax + 1)(lmax + 2) / 2 for any lmax" % alm.size)
    nside = int(nside)
    ctx = _lib.get_context()
    dev = ctx.alm_packed_to_dev(torch.from_numpy(alm[None]).to(ctx.device), lmax)
    out = np.empty((3, nside2npix(nside)))
    out[0] = ctx.alm2map(dev, nside, lmax, 1)[0].cpu().numpy()
    dth, dph = ctx.alm2map_der1(dev, nside, lmax, 1)
    out[1], out[2] = dth[0].cpu().numpy(), dph[0].cpu().numpy()
    return out


# ------------------------------------------------------------------------------------
# spectra of maps: healpy.anafast for every pair of a stack at once (csrc/spectra.hip)
# ------------------------------------------------------------------------------------
def spectra_pair_order(n):
    """Index arrays ``(i, j)`` of the ``n (n + 1) / 2`` spectra of ``n`` maps in healpy's order: the diagonals one after
    the other, (0,0), (1,1), ..., (0,1), (1,2), ..., (0,2), ... (``healpy.anafast`` / ``alm2cl`` of several maps)."""
    n = int(n)
    i = np.concatenate([np.arange(n - d) for d in range(n)]) if n > 0 else np.zeros(0, dtype=np.int64)
    j = np.concatenate([np.arange(d, n) for d in range(n)]) if n > 0 else np.zeros(0, dtype=np.int64)
    return i.astype(np.int64), j.astype(np.int64)


def _npix2nside(npix):
    nside = int(round(np.sqrt(int(npix) / 12.0)))
    if nside < 1 or 12 * nside * nside != int(npix):
        raise ValueError("Wrong pixel number (it is not 12*nside**2)")   # healpy.npix2nside
    return nside


def cross_spectra_device(maps, maps2=None, lmax=None, use_weights=None, niter=None):
    """Device maps [n, npix] (and ``maps2`` [n2, npix]) -> device ``[lmax + 1, n, n2]``: the spectrum
    ``C_l[i, j] = sum_m a_i(l,m) conj(b_j(l,m)) / (2l + 1)`` of every pair (``maps2=None``: of ``maps`` with itself,
    bitwise symmetric).  :func:`map2alm_device` (``use_weights``, ``niter`` as there) followed by
    ``Context.alm_cross_spectra``; the a_lm never leave the device.  Default ``lmax = 3 nside - 1``."""
    ctx = _lib.get_context()
    if maps.dim() != 2 or (maps2 is not None and (maps2.dim() != 2 or maps2.shape[1] != maps.shape[1])):
        raise ValueError("maps must be [n, npix] (and maps2 [n2, npix] of the same nside)")
    nside = _npix2nside(maps.shape[1])
    lmax = 3 * nside - 1 if lmax is None else int(lmax)
    n = int(maps.shape[0])
    alm = map2alm_device(maps.contiguous(), nside, lmax, use_weights=use_weights, niter=niter)
    if maps2 is None:
        return ctx.alm_cross_spectra(alm, n, lmax)
    n2 = int(maps2.shape[0])
    alm2 = map2alm_device(maps2.contiguous(), nside, lmax, use_weights=use_weights, niter=niter)
    return ctx.alm_cross_spectra(alm, n, lmax, alm_b=alm2, ny=n2)


def anafast(map1, map2=None, lmax=None, iter=3, use_weights=False, pol=False):
    """``healpy.anafast`` for temperature maps, with healpy's shapes and defaults (``iter=3``, ``use_weights=False``,
    ``lmax = 3 nside - 1``): one map -> ``[lmax + 1]``; maps ``[n, npix]`` -> ``[n (n + 1) / 2, lmax + 1]`` in the
    order of :func:`spectra_pair_order`; with ``map2`` (same shape) the cross spectra only, entry (i, j) from map i of
    ``map1`` and map j of ``map2``.  All pairs come from one call of the Gram kernel (:func:`cross_spectra_device`).
    ``pol=True`` on more than one map (healpy: T, Q, U) is not implemented here: the polarised spectra of a (T, Q, U)
    triple are :func:`anafast_pol`."""
    import torch

    map1 = np.asarray(map1, dtype=np.float64)
    single = map1.ndim == 1
    if pol and not single:
        raise NotImplementedError("anafast: polarised (spin-2) spectra of [T, Q, U] are hputil.anafast_pol; "
                                  "anafast takes pol=False")
    m1 = np.ascontiguousarray(map1.reshape(1, -1) if single else map1)
    if m1.ndim != 2:
        raise ValueError("anafast takes one map or maps [n, npix]")
    ctx = _lib.get_context()
    d2 = None
    if map2 is not None:
        m2 = np.asarray(map2, dtype=np.float64)
        m2 = np.ascontiguousarray(m2.reshape(1, -1) if m2.ndim == 1 else m2)
        if m2.shape != m1.shape:
            raise ValueError("anafast: map2 must have the shape of map1")
        d2 = torch.from_numpy(m2).to(ctx.device)
    cl = cross_spectra_device(torch.from_numpy(m1).to(ctx.device), d2, lmax=lmax, use_weights=use_weights, niter=iter)
    cl = cl.cpu().numpy()
    if single:
        return cl[:, 0, 0].copy()
    i, j = spectra_pair_order(m1.shape[0])
    return np.ascontiguousarray(cl[:, i, j].T)


# ------------------------------------------------------------------------------------
# polarised skies: maps [F, npol, npix] of (T, Q, U[, V]) -> a_lm of (T, E, B[, V]) in one field-major buffer and the
# spectra C_l^{pq}(nu, nu') of all of them from one Gram product (csrc/spectra.hip)
# ------------------------------------------------------------------------------------
SKY_CHUNK = 16      # frequency channels that go through the analysis together in map2alm_sky_device


def sky_channel(p, f, nfreq):
    """The field-major rule of :func:`map2alm_sky_device`: field ``p`` (0 = T, 1 = E, 2 = B, 3 = V) of frequency channel
    ``f`` of ``nfreq`` is channel ``p * nfreq + f`` (scalars or arrays)."""
    return np.asarray(p) * int(nfreq) + np.asarray(f)


def _check_sky(maps, name="maps"):
    """(F, npol, nside) of a polarised stack [F, npol, npix], npol 3 or 4 - decided on the shape alone."""
    shape = tuple(maps.shape)
    if len(shape) != 3:
        raise ValueError("%s must be [nfreq, npol, npix] (got shape %r)" % (name, shape))
    if shape[1] not in (3, 4):
        raise Exception("Wrong number of polarisation components.")
    if shape[0] < 1:
        raise ValueError("%s holds no frequency channel" % name)
    return int(shape[0]), int(shape[1]), _npix2nside(shape[2])


def map2alm_sky_bytes(nside, lmax, npol, chunk=SKY_CHUNK):
    """Upper bound of the temporary device memory of :func:`map2alm_sky_device` beyond its input and its output, for
    chunks of ``chunk`` frequency channels, from the library's own workspace sizes.  With ``M`` the bytes of one map,
    ``A(n) = nalm * 2 ceil(n / 8) * 64`` those of the coefficients of n channels padded to 8, ``c = chunk``,
    ``s = (npol - 2) c`` scalar maps and ``p = 8 ceil(2 c / 8)``, the larger of

    * the scalar planes: their contiguous copy, the synthesis and the residual of a refinement (``3 s M``), the
      coefficients, their update and the padded buffer of a pass (``3 A(s)``);
    * the (Q, U) planes: their copy ``2 c M``, the synthesis of the padded (E, B) set ``p M``, the residual ``2 c M``
      and its six ring-scaled maps ``6 c M``, three (E, B) sets ``3 A(2 c)`` and the six-fold set of a pass twice
      (``2 A(6 c)``: as :meth:`Context.map2alm` returns it and padded to 8),

    plus the shared transform workspace (the largest of the analysis of ``s`` and ``6 c`` channels and the synthesis of
    ``s`` and ``p``) and 1 MiB of small tables.

    With the module's ``_spin2_method`` at "native" (:func:`spin2_method`) the (Q, U) side is that of the one-pass analysis: no
    ring-scaled maps and no six-fold coefficient sets, ``(4 c + p) M + 3 A(2 c)``, and the workspace of the spin-2
    analysis of ``c`` fields (``Context.map2alm_spin2_workspace_bytes``) in place of that of ``6 c`` scalar channels."""
    method = _resolve_spin2_method()
    ctx = _lib.get_context()
    nside, lmax, npol, c = int(nside), int(lmax), int(npol), max(1, int(chunk))
    if npol not in (3, 4):
        raise Exception("Wrong number of polarisation components.")
    plan = ctx.sht_plan(nside, lmax)
    m = 12 * nside * nside * 8
    nalm = (lmax + 1) * (lmax + 2) // 2

    def a8(n):
        return nalm * ((n + 7) // 8 * 2) * 64

    s, p = (npol - 2) * c, (2 * c + 7) // 8 * 8
    scal = 3 * s * m + 3 * a8(s)
    if method == "native":
        pol = (4 * c + p) * m + 3 * a8(2 * c)
        ana = ctx.map2alm_spin2_workspace_bytes(plan, c)
    else:
        pol = (10 * c + p) * m + 3 * a8(2 * c) + 2 * a8(6 * c)
        ana = ctx.map2alm_workspace_bytes(plan, 6 * c)
    ws = max(ctx.map2alm_workspace_bytes(plan, s), ctx.alm2map_workspace_bytes(plan, s),
             ana, ctx.alm2map_workspace_bytes(plan, p))
    return max(scal, pol) + ws + (1 << 20)


def map2alm_sky_device(maps, lmax=None, use_weights=None, niter=None, chunk=SKY_CHUNK):
    """Analysis of a polarised sky: device maps ``[F, npol, npix]`` with planes (T, Q, U) or (T, Q, U, V) - what
    ``getpolsky`` returns and :func:`sphtrans_sky` takes - -> one ``alm_dev [nalm, ceil(P F / 4), 2, 4]`` of ``P F``
    channels, **field-major**: channel ``p F + f`` (:func:`sky_channel`) holds field p of frequency channel f, fields
    in the order (T, E, B[, V]), ``P = npol``.  Any other ``npol`` raises ``Exception("Wrong number of polarisation
    components.")`` as :func:`sphtrans_sky` does.  ``lmax`` defaults to ``3 nside - 1``, ``use_weights`` and ``niter``
    to the module's ``_weight`` / ``_iter`` as in :func:`map2alm_device`.

    E and B follow the convention documented at ``corahip_alm2map_spin2`` (HEALPix's: ``Q +- iU = - sum (a^E +- i a^B)
    (+-2)Y_lm``); their ``l < 2`` coefficients are zero.  Padding channels of the last group are zero.

    The channels go through in chunks of ``chunk`` frequencies: T (and V) of a chunk through :func:`map2alm_device`,
    its (Q_f, U_f) pairs - adjacent rows ``npol f + 1``, ``npol f + 2`` of the flattened stack - through
    :func:`map2alm_pol_device`, and each set of coefficients is put into the output by
    ``Context.alm_gather_channels``, which also takes E and B apart (the spin-2 analysis returns them interleaved).
    Temporaries stay below :func:`map2alm_sky_bytes`.

    The default chunk of 16: at nside 1024 (lmax 3071, nalm 4 720 128, M = 100.7 MB) the (Q, U) side of the bound is
    ``(160 + 32) M + 3 A(32) + 2 A(96)`` = 19.3 + 7.2 + 14.5 = 41.1 GB plus the workspace of a 96-channel analysis -
    beside 77.3 GB of input and 58.0 GB of output for 256 channels x 3 planes on a 288 GB device - where the analysis
    of all pairs at once takes six ring-scaled maps per pair alone, 155 GB.

    The (Q, U) pairs take the route of the module's ``_spin2_method`` ("composed" / "native", :func:`spin2_method`),
    read once at entry and checked before any device work; the bound is :func:`map2alm_sky_bytes` under the same setting."""
    import torch

    method = _resolve_spin2_method()
    F, npol, nside = _check_sky(maps)
    if not isinstance(maps, torch.Tensor) or maps.dtype != torch.float64:
        raise ValueError("maps must be a float64 device tensor")
    ctx = _lib.get_context()
    if maps.device != ctx.device:
        raise ValueError("maps must be on %s (got %s)" % (ctx.device, maps.device))
    lmax = 3 * nside - 1 if lmax is None else int(lmax)
    chunk = max(1, int(chunk))
    npix = int(maps.shape[2])
    nout = npol * F
    out = ctx._alm_out(lmax, nout)
    if nout % 4:
        out[:, -1].zero_()                                  # the padding channels share this group; the gather keeps them
    for f0 in range(0, F, chunk):
        c = min(chunk, F - f0)
        ar = np.arange(c, dtype=np.int32)
        planes = [0] + ([3] if npol == 4 else [])
        scal = torch.cat([maps[f0:f0 + c, p] for p in planes]) if len(planes) > 1 else maps[f0:f0 + c, 0].contiguous()
        alm = map2alm_device(scal, nside, lmax, use_weights=use_weights, niter=niter)
        del scal
        for k, p in enumerate(planes):
            ctx.alm_gather_channels(alm, 4 * alm.shape[1], k * c + ar, out, nout, dst_first=p * F + f0)
        del alm
        qu = maps[f0:f0 + c, 1:3].contiguous().view(2 * c, npix)
        alm = map2alm_pol_device(qu, nside, lmax, use_weights=use_weights, niter=niter, method=method)
        del qu
        for k in (0, 1):                                    # E_f, B_f = channels 2 f, 2 f + 1 of the spin-2 result
            ctx.alm_gather_channels(alm, 4 * alm.shape[1], 2 * ar + k, out, nout, dst_first=(1 + k) * F + f0)
        del alm
    return out


def cross_spectra_pol_device(maps, maps2=None, lmax=None, use_weights=None, niter=None):
    """Device maps ``[F, npol, npix]`` (and ``maps2 [F2, npol2, npix]``) of (T, Q, U[, V]) -> device
    ``[lmax + 1, P F, P2 F2]``: ``C.reshape(L, P, F, P2, F2)[l, p, i, q, j]`` is ``C_l^{pq}(nu_i, nu_j)`` with p, q over
    (T, E, B[, V]) - TT, EE, BB, TE, EB, TB and their frequency cross terms at once.  :func:`map2alm_sky_device`
    (``use_weights``, ``niter`` as there) and one ``Context.alm_cross_spectra`` call on the field-major buffers; with
    ``maps2=None`` the result equals its transpose bit for bit.  Default ``lmax = 3 nside - 1``.  The route of the
    (Q, U) analysis is the module's ``_spin2_method`` (:func:`spin2_method`)."""
    _resolve_spin2_method()
    F, npol, nside = _check_sky(maps)
    if maps2 is not None:
        F2, npol2, nside2 = _check_sky(maps2, "maps2")
        if nside2 != nside:
            raise ValueError("maps2 must have the nside of maps")
    ctx = _lib.get_context()
    lmax = 3 * nside - 1 if lmax is None else int(lmax)
    alm = map2alm_sky_device(maps, lmax, use_weights=use_weights, niter=niter)
    if maps2 is None:
        return ctx.alm_cross_spectra(alm, npol * F, lmax)
    alm2 = map2alm_sky_device(maps2, lmax, use_weights=use_weights, niter=niter)
    return ctx.alm_cross_spectra(alm, npol * F, lmax, alm_b=alm2, ny=npol2 * F2)


def anafast_pol(map1, map2=None, lmax=None, iter=3, use_weights=False):
    """``healpy.anafast(map1, map2, pol=True)`` for one polarised map ``[3, npix]`` (T, Q, U), with healpy's defaults
    (``iter=3``, ``use_weights=False``, ``lmax = 3 nside - 1``): ``[6, lmax + 1]`` in healpy's order TT, EE, BB, TE, EB,
    TB - :func:`spectra_pair_order` of 3 over (T, E, B).  With ``map2`` (same shape) entry (X, Y) takes X from ``map1``
    and Y from ``map2``.  Any other shape raises ``ValueError``.  (:func:`cross_spectra_pol_device` underneath.)"""
    import torch

    _resolve_spin2_method()
    m1 = np.asarray(map1, dtype=np.float64)
    if m1.ndim != 2 or m1.shape[0] != 3:
        raise ValueError("anafast_pol takes one polarised map [3, npix] of (T, Q, U) (got shape %r)" % (m1.shape,))
    _npix2nside(m1.shape[1])
    m2 = None
    if map2 is not None:
        m2 = np.asarray(map2, dtype=np.float64)
        if m2.shape != m1.shape:
            raise ValueError("anafast_pol: map2 must have the shape of map1")
    ctx = _lib.get_context()
    d1 = torch.from_numpy(np.ascontiguousarray(m1[None])).to(ctx.device)
    d2 = None if m2 is None else torch.from_numpy(np.ascontiguousarray(m2[None])).to(ctx.device)
    cl = cross_spectra_pol_device(d1, d2, lmax=lmax, use_weights=use_weights, niter=iter).cpu().numpy()
    i, j = spectra_pair_order(3)
    return np.ascontiguousarray(cl[:, i, j].T)


# ------------------------------------------------------------------------------------
# bilinear interpolation and coordinate rotation: healpy.get_interp_weights / get_interp_val and
# cora/util/hputil.py:534-604 (csrc/hpinterp.hip)
# ------------------------------------------------------------------------------------
# The interpolation scheme is the published HEALPix one (get_interpol, Gorski et al. 2005), restated; healpy is not a
# dependency of this package and its own numbers are neither used nor tested against.
def _query(nside, theta, phi, nest, lonlat):
    if nest:
        raise NotImplementedError("NEST ordering is not implemented; pass nest=False")
    if phi is None:
        ipix = np.asarray(theta, dtype=np.int64)
        if ipix.size and (ipix.min() < 0 or ipix.max() >= nside2npix(nside)):
            raise ValueError("pixel index out of range for nside %d" % int(nside))
        theta, phi = pix2ang(nside, ipix)
    else:
        theta, phi = np.broadcast_arrays(np.asarray(theta, dtype=np.float64), np.asarray(phi, dtype=np.float64))
        if lonlat:
            theta, phi = np.pi / 2.0 - np.radians(phi), np.radians(theta)
    if theta.size and not ((theta >= 0).all() and (theta <= np.pi).all()):
        raise ValueError("THETA is out of range [0,pi]")
    ctx = _lib.get_context()
    return ctx, theta.shape, ctx.to_device(theta.reshape(-1)), ctx.to_device(phi.reshape(-1))


def get_interp_weights(nside, theta, phi=None, nest=False, lonlat=False):
    """``healpy.get_interp_weights`` in RING order: the 4 pixels and bilinear weights around each direction, host
    arrays ``(pix [4, ...] int64, weights [4, ...] float64)`` of the arguments' (broadcast) shape, the two pixels of
    the upper ring first.  ``theta``, ``phi``: scalars or arrays (colatitude and longitude in radians; with
    ``lonlat=True`` longitude and latitude in degrees); ``phi=None``: ``theta`` holds pixel indices, whose centres are
    taken.  North of the first ring (south of the last) the pole is a virtual sample, the mean of the ring's 4 pixels:
    the ring's two pixels and their opposites are returned.  ``nest=True`` raises NotImplementedError.

    The scheme is HEALPix's published one, computed on the device (corahip_healpix_interp_weights); it is pinned by its
    properties and an independent numpy oracle (tests/_interp_oracle.py), not by healpy's output.  Ring colatitudes are
    those of :func:`pix2ang`, so a pixel centre taken from there gets weight 1 on its own pixel in theta."""
    ctx, shape, th, ph = _query(int(nside), theta, phi, nest, lonlat)
    pix, w = ctx.healpix_interp_weights(int(nside), th, ph)
    return pix.cpu().numpy().reshape((4,) + shape), w.cpu().numpy().reshape((4,) + shape)


def get_interp_val_device(maps, theta, phi):
    """Device maps [n, npix] sampled at the directions ``theta``, ``phi`` (1-d float64 device tensors, theta in
    [0, pi], not checked) -> device [n, len(theta)].  The weights are formed once per direction and applied to every
    map in one launch; no atomics, identical bits from call to call."""
    return _lib.get_context().healpix_interp_val(maps, theta, phi)


def get_interp_val(m, theta, phi, nest=False, lonlat=False):
    """``healpy.get_interp_val`` in RING order: the bilinear interpolation of the map ``m`` [npix], or of each map of
    ``m`` [n, npix], at the directions (scalars or arrays, as :func:`get_interp_weights`).  Host result of the
    directions' shape, with a leading axis ``n`` for several maps."""
    m = np.asarray(m, dtype=np.float64)
    if m.ndim not in (1, 2):
        raise ValueError("get_interp_val takes one map [npix] or maps [n, npix]")
    nside = _npix2nside(m.shape[-1])
    ctx, shape, th, ph = _query(nside, theta, phi, nest, lonlat)
    val = ctx.healpix_interp_val(ctx.to_device(m.reshape(-1, m.shape[-1])), th, ph).cpu().numpy()
    if m.ndim == 1:
        val = val[0].reshape(shape)
        return val if val.ndim else float(val)
    return val.reshape((m.shape[0],) + shape)


def rotate_map_device(maps, R, out=None):
    """Device maps [n, npix] rotated by the 3 x 3 host matrix ``R``: ``out[i, p] = interp(maps[i], R n_p)`` with
    ``n_p`` the centre of pixel p, i.e. output pixel p samples the input at ``R n_p``.  One fused kernel
    (corahip_healpix_rotate_maps): no angle arrays in memory, the weights of a pixel serve all n maps.  ``out`` must not
    overlap ``maps`` (ValueError).  No atomics: identical bits from call to call."""
    return _lib.get_context().healpix_rotate_maps(maps, R, out=out)


def ud_grade(map_in, nside_out):
    """``healpy.ud_grade(map_in, nside_out)`` with its defaults (``power=None``, RING in and out) for one map [npix] or
    maps [n, npix], between two power-of-two resolutions: degrading takes the arithmetic mean of the ``4^k`` children,
    upgrading replicates the parent.  numpy in, numpy out; a device tensor stays on the device.  No ``UNSEEN`` handling.
    Restated from the NESTED hierarchy of Gorski et al. 2005 (corahip_healpix_ud_grade) and pinned by its properties and
    a numpy oracle (tests/_pointsource_oracle.py), not by healpy's output."""
    ctx = _lib.get_context()
    host = not hasattr(map_in, "data_ptr")
    m = ctx.to_device(np.asarray(map_in, dtype=np.float64)) if host else map_in
    if m.dim() not in (1, 2):
        raise ValueError("ud_grade takes one map [npix] or maps [n, npix]")
    out = ctx.healpix_ud_grade(m.reshape(-1, m.shape[-1]).contiguous(), nside_out)
    out = out[0] if m.dim() == 1 else out
    return out.cpu().numpy() if host else out


# ------------------------------------------------------------------------------------
# RING <-> NESTED, Gaussian-beam smoothing: healpy.reorder / ring2nest / nest2ring / gauss_beam / smoothing
# (csrc/galaxy.hip).  Restated from the published definitions (Gorski et al. 2005, section 4.1; a Gaussian beam of
# width sigma multiplies a_lm by exp(-l (l + 1) sigma^2 / 2)) and pinned by their properties and a numpy oracle
# (tests/_galaxy_oracle.py), not by healpy's output.
# ------------------------------------------------------------------------------------
_FACE_RING = np.array([2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4])       # ring of a base pixel's northern corner, in nside
_FACE_PHI = np.array([1, 3, 5, 7, 0, 2, 4, 6, 1, 3, 5, 7])        # its longitude, in units of pi / 4


def get_nside(m):
    """``healpy.get_nside``: the nside of one map [npix] or of maps [n, npix]."""
    return _npix2nside(np.shape(m)[-1])


def _order_of(nside, what):
    nside = int(nside)
    if nside < 1 or nside & (nside - 1) or nside > 8192:
        raise ValueError("%s: nside must be a power of two up to 8192 (got %d)" % (what, nside))
    return nside, nside.bit_length() - 1


def _index_array(nside, ipix, what):
    ipix = np.asarray(ipix)
    if ipix.dtype.kind not in "iu":
        raise ValueError("%s takes integer pixel indices" % what)
    ipix = ipix.astype(np.int64)
    if ipix.size and (ipix.min() < 0 or ipix.max() >= nside2npix(nside)):
        raise ValueError("pixel index out of range for nside %d" % nside)
    return ipix


def _bits(v, k, src_step, dst_step):
    """Bit ``src_step b`` of ``v`` moved to place ``dst_step b``, b < k."""
    out = np.zeros_like(v)
    for b in range(k):
        out |= ((v >> (src_step * b)) & 1) << (dst_step * b)
    return out


def nest2ring(nside, ipix):
    """``healpy.nest2ring``: RING index of NESTED pixels (host index arrays).  A NESTED index is
    ``face nside^2 + (bits of x on the even places, bits of y on the odd places)``; the pixel (x, y) of a face lies on
    ring ``jr = face_ring nside - x - y - 1`` at the position that ``x - y`` fixes."""
    nside, k = _order_of(nside, "nest2ring")
    ipix = _index_array(nside, ipix, "nest2ring")
    face, rest = ipix >> (2 * k), ipix & (nside * nside - 1)
    ix, iy = _bits(rest, k, 2, 1), _bits(rest >> 1, k, 2, 1)
    jr = _FACE_RING[face] * nside - ix - iy - 1
    nr = np.where(jr < nside, jr, np.where(jr > 3 * nside, 4 * nside - jr, nside))           # pixels per quarter ring
    first = np.where(jr < nside, 2 * nr * (nr - 1),
                     np.where(jr > 3 * nside, 12 * nside * nside - 2 * nr * (nr + 1), 2 * nside * (nside - 1) + (jr - nside) * 4 * nside))
    shift = np.where((jr >= nside) & (jr <= 3 * nside), (jr - nside) & 1, 0)
    jp = (_FACE_PHI[face] * nr + ix - iy + 1 + shift) // 2
    jp = np.where(jp > 4 * nside, jp - 4 * nside, np.where(jp < 1, jp + 4 * nside, jp))
    out = first + jp - 1
    return out if out.ndim else int(out)


_r2n_cache = {}


def ring2nest(nside, ipix):
    """``healpy.ring2nest``: NESTED index of RING pixels (host index arrays): the inverse permutation of
    :func:`nest2ring`, tabulated once per nside."""
    nside, _ = _order_of(nside, "ring2nest")
    ipix = _index_array(nside, ipix, "ring2nest")
    table = _r2n_cache.get(nside)
    if table is None:
        npix = nside2npix(nside)
        table = np.empty(npix, dtype=np.int64)
        table[nest2ring(nside, np.arange(npix))] = np.arange(npix)
        if nside <= 256:                                   # 6 MB at most; larger tables are rebuilt per call
            _r2n_cache[nside] = table
    out = table[ipix]
    return out if out.ndim else int(out)


def reorder(map_in, inp=None, out=None, r2n=None, n2r=None):
    """``healpy.reorder`` for one map [npix] or maps [n, npix]: ``r2n=True`` (or ``inp='RING', out='NESTED'``) RING ->
    NESTED, ``n2r=True`` (or ``inp='NESTED', out='RING'``) the other way; equal orderings return a copy.  numpy in,
    numpy out; a device tensor stays on the device (corahip_healpix_reorder).  nside a power of two."""
    if r2n and n2r:
        raise ValueError("reorder: r2n and n2r are exclusive")
    if r2n:
        inp, out = "RING", "NESTED"
    if n2r:
        inp, out = "NESTED", "RING"
    names = {"RING": "RING", "NEST": "NESTED", "NESTED": "NESTED"}
    if not isinstance(inp, str) or not isinstance(out, str) or inp.upper() not in names or out.upper() not in names:
        raise ValueError("reorder: inp and out must be 'RING' or 'NESTED' (or pass r2n / n2r)")
    inp, out = names[inp.upper()], names[out.upper()]
    host = not hasattr(map_in, "data_ptr")
    shape = np.shape(map_in) if host else tuple(map_in.shape)
    if len(shape) not in (1, 2):
        raise ValueError("reorder takes one map [npix] or maps [n, npix]")
    _order_of(_npix2nside(shape[-1]), "reorder")
    if inp == out:
        return np.array(map_in, dtype=np.float64) if host else map_in.clone()
    ctx = _lib.get_context()
    m = ctx.to_device(np.asarray(map_in, dtype=np.float64)) if host else map_in
    res = ctx.healpix_reorder(m.reshape(-1, shape[-1]).contiguous(), inp == "RING").reshape(shape)
    return res.cpu().numpy() if host else res


def gauss_beam(fwhm, lmax):
    """``healpy.gauss_beam(fwhm, lmax)`` for temperature: ``exp(-l (l + 1) sigma^2 / 2)``, ``sigma = fwhm / sqrt(8 ln 2)``,
    l = 0 .. lmax (fwhm in radians)."""
    sigma = float(fwhm) / np.sqrt(8.0 * np.log(2.0))
    ell = np.arange(int(lmax) + 1, dtype=np.float64)
    return np.exp(-0.5 * ell * (ell + 1.0) * (sigma * sigma))


def _beams(n, lmax, fl, fwhm, sigma):
    """[n, lmax + 1] transfer functions of ``smoothing_device`` from ``fl``, or ``sigma``, or ``fwhm`` (in that order)."""
    if fl is not None:
        fl = np.asarray(fl, dtype=np.float64)
        if fl.shape != (n, lmax + 1):
            raise ValueError("fl has shape %r, expected %r" % (fl.shape, (n, lmax + 1)))
        return fl
    width = np.asarray(0.0 if fwhm is None else fwhm, dtype=np.float64) if sigma is None \
        else np.asarray(sigma, dtype=np.float64) * np.sqrt(8.0 * np.log(2.0))
    if width.ndim > 1 or (width.ndim == 1 and width.shape[0] != n):
        raise ValueError("fwhm / sigma must be a scalar or one value per map (%d)" % n)
    return np.stack([gauss_beam(w, lmax) for w in np.broadcast_to(width, (n,))])


def smoothing_device(maps, fl=None, fwhm=None, sigma=None, lmax=None, niter=3, use_weights=False):
    """``healpy.smoothing`` with its defaults (``iter=3``, no ring weights, ``lmax = 3 nside - 1``) for device maps
    [n, npix]: :func:`map2alm_device`, ``Context.alm_scale_l`` and ``Context.alm2map``, all maps in one batch.  ``fwhm``
    or ``sigma`` (radians): a scalar, or one value per map; ``fl`` [n, lmax + 1] overrides both."""
    if maps.dim() != 2:
        raise ValueError("maps must be [n, npix]")
    n, nside = int(maps.shape[0]), _npix2nside(maps.shape[1])
    lmax = 3 * nside - 1 if lmax is None else int(lmax)
    beams = _beams(n, lmax, fl, fwhm, sigma)
    ctx = _lib.get_context()
    alm = map2alm_device(maps.contiguous(), nside, lmax, use_weights=use_weights, niter=niter)
    ctx.alm_scale_l(alm, lmax, beams, out=alm)
    return ctx.alm2map(alm, nside, lmax, n)


def smoothing(map_in, fwhm=0.0, sigma=None, lmax=None, iter=3, use_weights=False):
    """``healpy.smoothing`` for one temperature map [npix] or maps [n, npix]: numpy in, numpy out
    (:func:`smoothing_device`)."""
    m = np.asarray(map_in, dtype=np.float64)
    if m.ndim not in (1, 2):
        raise ValueError("smoothing takes one map [npix] or maps [n, npix]")
    _npix2nside(m.shape[-1])
    ctx = _lib.get_context()
    out = smoothing_device(ctx.to_device(m.reshape(-1, m.shape[-1])), fwhm=fwhm, sigma=sigma, lmax=lmax, niter=iter,
                           use_weights=use_weights)
    return ctx.to_host(out).reshape(m.shape)


# J2000 constants of the coordinate systems (IAU 1958 galactic system transformed to J2000, as in the Hipparcos
# catalogue vol. 1 sec. 1.5.3; mean obliquity of the IAU 1976 system): degrees
GAL_POLE_RA, GAL_POLE_DEC, GAL_LON_NCP = 192.85948, 27.12825, 122.93192
ECL_OBLIQUITY = 23.4392911


def _rot(axis, angle_deg):
    """Active rotation by ``angle_deg`` about coordinate axis 0, 1 or 2."""
    a = np.radians(angle_deg)
    c, s = np.cos(a), np.sin(a)
    i, j = [(1, 2), (2, 0), (0, 1)][axis]
    r = np.eye(3)
    r[i, i], r[i, j], r[j, i], r[j, j] = c, -s, s, c
    return r


def _mm(a, b):
    """3 x 3 product with a fixed order of the sums, so that ``_mm(a, b.T) == _mm(b, a.T).T`` bit for bit."""
    return np.array([[(a[i, 0] * b[0, j] + a[i, 1] * b[1, j]) + a[i, 2] * b[2, j] for j in range(3)] for i in range(3)])


def _from_celestial(y):
    if y == "G":
        # turn about z to the pole's right ascension, tip the pole onto z, then turn the celestial pole (now at
        # longitude 180 deg) to its galactic longitude
        return _mm(_rot(2, GAL_LON_NCP - 180.0), _mm(_rot(1, GAL_POLE_DEC - 90.0), _rot(2, -GAL_POLE_RA)))
    if y == "E":
        return _rot(0, -ECL_OBLIQUITY)
    return np.eye(3)


def coord_matrix(x, y):
    """The 3 x 3 matrix taking a unit vector given in system ``x`` to system ``y``; 'C' celestial (equatorial J2000),
    'G' galactic, 'E' ecliptic.  Composed from elementary rotations by the defining angles, so it is orthonormal to
    rounding, ``coord_matrix(x, y) == coord_matrix(y, x).T`` exactly and ``coord_matrix(x, x)`` is the identity.

    Galactic (J2000): north pole at RA 192.85948 deg, Dec 27.12825 deg, galactic longitude of the celestial pole
    122.93192 deg; ecliptic: J2000 obliquity 23.4392911 deg.  These are the project's own constants; healpy composes
    its matrices from slightly different ones, and agreement with healpy below about 1e-5 rad is neither claimed nor
    tested."""
    if x not in ["C", "G", "E"] or y not in ["C", "G", "E"]:
        raise Exception("Co-ordinate system invalid.")
    if x == y:
        return np.eye(3)
    return _mm(_from_celestial(y), _from_celestial(x).T)


ROTATE_MAX_BYTES = 1 << 31     # device bytes (input + output chunk) coord_x2y uses at a time


def coord_x2y(map, x, y, max_bytes=None):
    """Rotate maps [..., npix] from co-ordinate system ``x`` into system ``y`` ('C', 'G' or 'E';
    cora/util/hputil.py:534-566): output pixel p is the bilinear interpolation of the input at
    ``coord_matrix(y, x) n_p``, the position in ``x`` of the point whose ``y`` co-ordinates are the pixel centre.
    Polarisation planes are rotated as scalars, as the reference does (no rotation of the polarisation angle).

    Returns a NEW array of the input's shape; the reference overwrites its argument and returns it.  The maps go to
    the device in chunks of channels whose input and output together stay within ``max_bytes`` (default
    ``ROTATE_MAX_BYTES``, 2 GiB; never less than one map); chunking does not change a bit of the result.  The rotation
    matrix is :func:`coord_matrix`: see there for the constants."""
    if x not in ["C", "G", "E"] or y not in ["C", "G", "E"]:
        raise Exception("Co-ordinate system invalid.")
    map = np.asarray(map, dtype=np.float64)
    npix = map.shape[-1]
    _npix2nside(npix)
    R = coord_matrix(y, x)
    flat = np.ascontiguousarray(map.reshape((-1, npix)))
    out = np.empty_like(flat)
    budget = ROTATE_MAX_BYTES if max_bytes is None else int(max_bytes)
    chunk = max(1, budget // (2 * npix * 8))
    ctx = _lib.get_context()
    for c0 in range(0, flat.shape[0], chunk):
        out[c0:c0 + chunk] = ctx.to_host(rotate_map_device(ctx.to_device(flat[c0:c0 + chunk]), R))
    return out.reshape(map.shape)


def coord_g2c(map_):
    """Rotate maps [..., npix] from galactic into celestial co-ordinates (cora/util/hputil.py:569-585)."""
    return coord_x2y(map_, "G", "C")


def coord_c2g(map_):
    """Rotate maps [..., npix] from celestial into galactic co-ordinates (cora/util/hputil.py:588-604)."""
    return coord_x2y(map_, "C", "G")
