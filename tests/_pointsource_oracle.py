"""Oracles and bounds of the point-source kernels (csrc/pointsource.hip; test infrastructure only).

Stream.  Source i of a population takes two Philox4x32-10 blocks (oracle/philox.py) under key = seed:

    A = philox(counter (i & 0xffffffff, i >> 32, 0, 0x50535243), key (seed & 0xffffffff, seed >> 32))
    B = philox(counter (i & 0xffffffff, i >> 32, 1, 0x50535243), key ...)
    u1 = ((A0 << 21) | (A1 >> 11)) 2^-53        u2 = ((A2 << 21) | (A3 >> 11)) 2^-53        (53 bits, exact, [0, 1))
    z  = the first normal of block B under the Box-Muller mapping of oracle/philox.py, written out in first_normal()
    flux = flux_min exp(spline(u1)),  index = mean + width z,  pix = min(int(u2 npix), npix - 1)

The a_lm and flat-sky streams use counter words 2 and 3 = 0; word 3 = "PSRC" here, so under no seed does a block of
this stream coincide with one of theirs.  The spline is cubicspline.Interpolater's (NR form): interval lo = the last
knot <= u1 (searchsorted side="right" minus 1), a = (x_hi - u) / h, b = (u - x_lo) / h,
value = a y_lo + b y_hi + (a^3 - a) h^2 / 6 y2_lo + (b^3 - b) h^2 / 6 y2_hi.

Bounds, with eps = 2^-52 and u = eps / 2 (one rounding is <= u relative; the library functions exp, sincos are taken
as <= 1 ulp <= eps relative):

Spline value.  The four terms t_k are each a product of at most 6 rounded operations on top of a, b, h (one rounding
    each for the difference and one for the quotient: the differences of knots are of exactly representable inputs);
    a^3 - a loses no more than the roundings of a^3 (2) and the subtraction: each term carries <= 8 roundings, i.e.
    <= 8 u |t_k| (1 + O(u)), and the three additions <= 3 u sum |t_k|: in total < 8 eps sum_k |t_k|.
Flux.  exp turns the absolute error d <= 8 eps sum |t_k| of its argument t into a relative error of the same size; on
    top of it exp's own error (eps), the product with flux_min (u) and, for an oracle that rounds t to a double before
    its exp, u |t|: relative tolerance 8 eps sum |t_k| + (|t| + 3) eps.
Index.  mean + width z: the package's Box-Muller bound |z - z_oracle| <= 4e-15 max(1, |z|) (tests/test_gpu_parity.py),
    scaled by |width|, plus the two roundings u (|width z| + |index|).
Pixel.  u2 npix is one rounding of an exact product: it can cross an integer only when the exact product lies within
    npix u of it.  Sources with |u2 npix - round(u2 npix)| <= npix eps are left out of the exact comparison.

Paint, per output element, n sources in the pixel, t_i = S_i exp(y_i), y_i = beta_i x + gamma_i x^2:
    y_i is formed with the roundings of beta x (u |beta x|), x^2 and gamma x^2 (2 u |gamma| x^2) and the sum
    (u |y_i| <= u (|beta x| + |gamma| x^2)): an absolute error <= eps (|beta x| + 2 |gamma| x^2) (generous by a third),
    which exp turns into a relative one of t_i; exp itself eps, the product u: <= eps (|beta x| + 2 |gamma| x^2 + 4) |t_i|
    with room for the reference's pow in place of exp(index log(.)) (<= 1 ulp, and x = log(freq / pivot) rounded once:
    u |beta x|).  A sum of n terms in ANY order is within (n - 1) u sum |t_i| (1 + O(n u)).  The unit conversion is two
    products and a quotient: 3 u, allowed 3 eps relative of the result.  The polarised planes multiply each term by
    polw (u) where the reference multiplies by P / S and by the cosine separately (2 u): 2 eps |t_i polw_i| per term.

        tol = (eps sum_i (|beta_i x| + 2 |gamma_i| x^2 + 4) |t_i w_i| + (n - 1) u sum_i |t_i w_i| + 2 eps sum_i |t_i w_i| [w != 1])
              1e-26 c2 / den + 3 eps |out|

Rotation, per component of (Q + iU) exp(-i a), a = 2 wv rm: the angle is the rounded product (-2 wv) rm: an absolute
    error u |a|, which moves the result by u |a| |Q + iU|; sincos <= 1 ulp per component (eps |Q + iU| together with
    the other component's), the two products and the sum 3 u (|Q| + |U|) <= 3 u sqrt2 |Q + iU|; the reference's own
    complex exp and product err by as much again.  tol = eps (|a| + 8) |Q + iU|.  In polarise_rotate Q = I q and U = I u
    carry one more rounding each (u |Q + iU|), inside the 8.

ud_grade: replication is exact; the m = 4^k children are summed pairwise in NESTED order (a balanced binary tree, so
    that m equal children sum exactly and upgrading followed by degrading returns the input bits); any order is within
    (m - 1) u sum |child| / m of the mean.
"""
import os

import numpy as np

from oracle import philox

EPS = 2.0 ** -52
U = EPS / 2
DOMAIN = 0x50535243
LD = np.longdouble
K_B = 1.3806503e-23
C_LIGHT = 299792458.0
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pointsource_vectors.npz")


def load_golden():
    g = np.load(GOLDEN)
    cases = {}
    for key in g.files:
        prefix, _, name = key.partition("_")
        v = g[key]
        cases.setdefault(prefix, {})[name] = v if v.ndim else v.item()
    return cases


# ---- stream ------------------------------------------------------------------------------------------------------------

def population_words(seed, i, block):
    i = np.asarray(i, dtype=np.uint64)
    seed = int(seed) & (2**64 - 1)
    return philox.philox4x32_10(i & np.uint64(0xFFFFFFFF), i >> np.uint64(32), block, DOMAIN, seed & 0xFFFFFFFF, seed >> 32)


def _uniform53(hi, lo):
    k = (hi.astype(np.uint64) << np.uint64(21)) | (lo.astype(np.uint64) >> np.uint64(11))
    return k.astype(np.float64) * 2.0 ** -53           # k < 2^53: exact


def first_normal(r0, r1, r2, r3):
    """The first Box-Muller normal of one Philox block, the mapping of oracle/philox.py (boxmuller_counter) word for word:

        k = r0 << 20 | r1 >> 12 (52 bits),  u = (k + 1/2) 2^-52,  radius = sqrt(-2 ln u)
        j = r2 >> 24,  w = (r2 & 0xffffff) << 28 | r3 >> 4 (52 bits),  theta = 2 pi (j + (w + 1/2) 2^-52) / 256
        z = radius cos(theta)

    The angle is evaluated in long double about the centre of sector j: theta = (2 j + 1) pi / 256 + x with
    x = ((w + 1/2) 2^-52 - 1/2) 2 pi / 256, the centre reduced as an integer multiple of pi / 256."""
    r0, r1, r2, r3 = (np.asarray(v).astype(np.uint64) for v in (r0, r1, r2, r3))
    k = (r0 << np.uint64(20)) | (r1 >> np.uint64(12))
    u = (k.astype(np.float64) + 0.5) * 2.0 ** -52                   # exact: 2 k + 1 < 2^53
    radius = np.sqrt(-2.0 * np.log1p(-(1.0 - u)))                   # 1 - u exact; log1p keeps u -> 1 accurate
    j = (r2 >> np.uint64(24)).astype(np.int64)
    w = ((r2 & np.uint64(0xFFFFFF)) << np.uint64(28)) | (r3 >> np.uint64(4))
    two_pi = 2 * LD(np.pi) + LD(2.4492935982947064e-16)             # 2 pi beyond the double
    x = ((w.astype(np.float64) * 2.0 ** -52 - 0.5) + 2.0 ** -53).astype(LD) * (two_pi / 256)      # offset exact in a double
    jj = 2 * j + 1                                                  # centre = jj pi / 256, jj odd in [1, 511]
    quadrant = jj // 128
    rem = (jj - 128 * quadrant).astype(LD) * (two_pi / 512)
    cr, sr = np.cos(rem), np.sin(rem)
    c0 = np.where(quadrant == 0, cr, np.where(quadrant == 1, -sr, np.where(quadrant == 2, -cr, sr)))
    s0 = np.where(quadrant == 0, sr, np.where(quadrant == 1, cr, np.where(quadrant == 2, -sr, -cr)))
    return radius * (c0 * np.cos(x) - s0 * np.sin(x)).astype(np.float64)


def population_draws(seed, n):
    """(u1, u2, z) of sources 0 .. n - 1."""
    i = np.arange(n, dtype=np.uint64)
    a = population_words(seed, i, 0)
    b = population_words(seed, i, 1)
    return _uniform53(a[0], a[1]), _uniform53(a[2], a[3]), first_normal(*b).reshape(n)


def spline_eval(xs, ys, y2, u, dtype=np.float64):
    """(interval, value, sum of the moduli of the four terms), in the kernel's statement order."""
    lo = np.searchsorted(xs, u, side="right") - 1
    lo = np.clip(lo, 0, len(xs) - 2)
    hi = lo + 1
    xs_, ys_, y2_, u_ = (np.asarray(v, dtype=dtype) for v in (xs, ys, y2, u))
    h = xs_[hi] - xs_[lo]
    a, b = (xs_[hi] - u_) / h, (u_ - xs_[lo]) / h
    h26 = h * h / dtype(6.0)
    t = [a * ys_[lo], b * ys_[hi], (a * a * a - a) * h26 * y2_[lo], (b * b * b - b) * h26 * y2_[hi]]
    return lo, ((t[0] + t[1]) + t[2]) + t[3], sum(np.abs(np.asarray(v, dtype=np.float64)) for v in t)


def population(seed, n, xs, ys, y2, flux_min, mean, width, npix, dtype=np.float64):
    """The population as the kernel forms it (dtype float64) or in long double: dict of arrays."""
    u1, u2, z = population_draws(seed, n)
    lo, t, tabs = spline_eval(xs, ys, y2, u1, dtype)
    flux = dtype(flux_min) * np.exp(t)
    index = dtype(mean) + dtype(width) * z.astype(dtype)
    prod = u2 * float(npix)
    pix = np.minimum(prod.astype(np.int64), npix - 1)
    exact = u2.astype(LD) * LD(npix)
    safe = np.abs(exact - np.rint(exact)).astype(np.float64) > npix * EPS
    return dict(u1=u1, u2=u2, z=z, interval=lo, t=t, tabs=tabs, flux=flux, index=index, pix=pix, pix_safe=safe)


# ---- paint -------------------------------------------------------------------------------------------------------------

def conversion(freq, nside):
    """(den [F], c2) as the host forms them (pointsource.py:245-250)."""
    npix = 12 * nside * nside
    pxarea = 4 * np.pi / npix
    freq = np.asarray(freq, dtype=np.float64)
    return 2 * K_B * freq**2 * 1e12 * pxarea, C_LIGHT**2


def paint(pix, flux, beta, gamma, polw, x, den, c2, npix, npol=1, dtype=LD, base=None, rel=None, relx=None):
    """out [F, npol, npix] (npol 1: [F, npix]) summed in source order, and the tolerance of every element.

    dtype long double: the oracle the kernels are held to.  dtype float64: the kernel's statement order for a pixel of
    at most 16 sources, which is also the reference's order.  ``base``: accumulate onto it (occupied pixels only).
    ``rel``, ``relx`` [n]: bounds on the relative error of the fluxes and the absolute error of the indices handed to
    the kernel (a population that was itself computed): term i then carries (rel_i + relx_i |x|) |t_i| more."""
    pix = np.asarray(pix, dtype=np.int64)
    n, F = len(pix), len(x)
    xd, dd = np.asarray(x, dtype=dtype), np.asarray(den, dtype=dtype)
    S, b = np.asarray(flux, dtype=dtype), np.asarray(beta, dtype=dtype)
    g = np.zeros(n, dtype=dtype) if gamma is None else np.asarray(gamma, dtype=dtype)
    nplane = 3 if polw is not None else 1
    out = np.zeros((F, 4 if npol == 4 else 1, npix), dtype=dtype)
    tol = np.zeros((F, 4 if npol == 4 else 1, npix))
    count = np.bincount(pix, minlength=npix)
    xf = np.asarray(x, dtype=np.float64)
    for f in range(F):
        y = b * xd[f] + g * (xd[f] * xd[f]) if gamma is not None else b * xd[f]
        t = S * np.exp(y)
        arg = np.abs(np.asarray(beta) * xf[f]) + (2 * np.abs(np.asarray(gamma)) * xf[f] ** 2 if gamma is not None else 0.0) + 4
        if rel is not None:
            arg = arg + (np.asarray(rel) + np.asarray(relx) * abs(xf[f])) / EPS
        conv = float(1e-26 * c2 / den[f])
        for k in range(nplane):
            tw = t if k == 0 else t * np.asarray(polw, dtype=dtype)[:, k - 1]
            s = np.zeros(npix, dtype=dtype)
            np.add.at(s, pix, tw)
            out[f, k] = ((s * dtype(1e-26)) * dtype(c2)) / dd[f]
            ta = np.abs(tw).astype(np.float64)
            e1, e2 = np.zeros(npix), np.zeros(npix)
            np.add.at(e1, pix, arg * ta)
            np.add.at(e2, pix, ta)
            tol[f, k] = (EPS * e1 + np.maximum(count - 1, 0) * U * e2 + (2 * EPS * e2 if k else 0.0)) * conv
    tol += 3 * EPS * np.abs(out).astype(np.float64)
    if base is not None:
        occupied = count > 0
        full = np.array(base, dtype=dtype).reshape(out.shape)
        full[:, :nplane, occupied] += out[:, :nplane, occupied]
        tol = np.where(occupied[None, None, :], tol + U * np.abs(full).astype(np.float64), 0.0)
        if nplane < tol.shape[1]:
            tol[:, nplane:] = 0.0
        out = full
    if npol == 1:
        out, tol = out[:, 0], tol[:, 0]
    return out, tol


def power_law_inputs(case):
    """(x, den, c2, npix) of a golden model case."""
    freq, nside = case["freq"], int(case["nside"])
    den, c2 = conversion(freq, nside)
    return np.log(freq / case["spectral_pivot"]), den, c2, 12 * nside * nside


def catalogue_inputs(cat, pix):
    """(flux, beta, gamma, polw) of the golden catalogue rows: NaN polarisation gives no Q / U."""
    polang = np.radians(cat["POLANG"])
    frac = cat["P600"] / cat["S600"]
    polw = np.stack([frac * np.cos(2.0 * polang), frac * np.sin(2.0 * polang)], axis=1)
    polw[np.isnan(cat["P600"]) | np.isnan(polang)] = 0.0
    return cat["S600"], cat["BETA"], cat["GAMMA"], polw


# ---- rotation ----------------------------------------------------------------------------------------------------------

def wavelengths(freq):
    return 1e-6 * C_LIGHT / np.asarray(freq, dtype=np.float64)


def rotate(q, u, wv, rm, dtype=LD):
    """(Q', U', tol) for Q, U [F, npix]: (Q + iU) exp(-2i wv rm), the angle the rounded double product (-2 wv) rm."""
    ang = ((-2.0 * np.asarray(wv, dtype=np.float64))[:, None] * np.asarray(rm, dtype=np.float64)[None, :])
    c, s = np.cos(ang.astype(dtype)), np.sin(ang.astype(dtype))
    qd, ud = np.asarray(q, dtype=dtype), np.asarray(u, dtype=dtype)
    tol = EPS * (np.abs(ang) + 8) * np.hypot(np.asarray(q, dtype=np.float64), np.asarray(u, dtype=np.float64))
    return qd * c - ud * s, qd * s + ud * c, tol


# ---- ud_grade ----------------------------------------------------------------------------------------------------------

_JRLL = np.array([2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4])
_JPLL = np.array([1, 3, 5, 7, 0, 2, 4, 6, 1, 3, 5, 7])


def _isqrt(v):
    r = np.sqrt(v.astype(np.float64)).astype(np.int64)
    r = np.where(r * r > v, r - 1, r)
    return np.where((r + 1) * (r + 1) <= v, r + 1, r)


def ring2xyf(nside, pix):
    """RING pixel -> (x, y, face) of the NESTED hierarchy (Gorski et al. 2005, section 4.1)."""
    pix = np.asarray(pix, dtype=np.int64)
    npix, ncap, nl2 = 12 * nside * nside, 2 * nside * (nside - 1), 2 * nside
    # north cap
    ir_n = (1 + _isqrt(1 + 2 * np.clip(pix, 0, None))) >> 1
    ip_n = pix + 1 - 2 * ir_n * (ir_n - 1)
    fa_n = (ip_n - 1) // np.maximum(ir_n, 1)
    # belt
    ipb = pix - ncap
    tmp = ipb // (4 * nside)
    ir_b = tmp + nside
    ip_b = ipb - tmp * 4 * nside + 1
    ks_b = (ir_b + nside) & 1
    ire, irm = tmp + 1, nl2 + 1 - tmp
    ifm, ifp = (ip_b - (ire >> 1) + nside - 1) // nside, (ip_b - (irm >> 1) + nside - 1) // nside
    fa_b = np.where(ifp == ifm, ifp | 4, np.where(ifp < ifm, ifp, ifm + 8))
    # south cap
    ips = npix - pix
    ir_s = (1 + _isqrt(np.clip(2 * ips - 1, 0, None))) >> 1
    ip_s = 4 * ir_s + 1 - (ips - 2 * ir_s * (ir_s - 1))
    fa_s = 8 + (ip_s - 1) // np.maximum(ir_s, 1)
    north, south = pix < ncap, pix >= npix - ncap
    iring = np.where(north, ir_n, np.where(south, 2 * nl2 - ir_s, ir_b))
    iphi = np.where(north, ip_n, np.where(south, ip_s, ip_b))
    nr = np.where(north, ir_n, np.where(south, ir_s, nside))
    kshift = np.where(north | south, 0, ks_b)
    face = np.clip(np.where(north, fa_n, np.where(south, fa_s, fa_b)), 0, 11)
    irt = iring - _JRLL[face] * nside + 1
    ipt = 2 * iphi - _JPLL[face] * nr - kshift - 1
    ipt = np.where(ipt >= nl2, ipt - 8 * nside, ipt)
    return (ipt - irt) >> 1, (-ipt - irt) >> 1, face


def xyf2ring(nside, ix, iy, face):
    npix, ncap, nl4 = 12 * nside * nside, 2 * nside * (nside - 1), 4 * nside
    jr = _JRLL[face] * nside - ix - iy - 1
    north, south = jr < nside, jr > 3 * nside
    nr = np.where(north, jr, np.where(south, nl4 - jr, nside))
    before = np.where(north, 2 * nr * (nr - 1), np.where(south, npix - 2 * (nr + 1) * nr, ncap + (jr - nside) * nl4))
    kshift = np.where(north | south, 0, (jr - nside) & 1)
    jp = (_JPLL[face] * nr + ix - iy + 1 + kshift) // 2
    jp = np.where(jp > nl4, jp - nl4, np.where(jp < 1, jp + nl4, jp))
    return before + jp - 1


def _spread(v, k):
    out = np.zeros_like(v)
    for b in range(k):
        out |= ((v >> b) & 1) << (2 * b)
    return out


def _compress(v, k):
    out = np.zeros_like(v)
    for b in range(k):
        out |= ((v >> (2 * b)) & 1) << b
    return out


def ring2nest(nside, pix):
    k = int(np.log2(nside))
    ix, iy, face = ring2xyf(nside, pix)
    return face * nside * nside + _spread(ix, k) + 2 * _spread(iy, k)


def nest2ring(nside, pnest):
    k = int(np.log2(nside))
    pnest = np.asarray(pnest, dtype=np.int64)
    face, rest = pnest // (nside * nside), pnest % (nside * nside)
    return xyf2ring(nside, _compress(rest, k), _compress(rest >> 1, k), face)


def parent(nside_hi, nside_lo, pix):
    """RING index at nside_lo of the pixel that holds RING pixel ``pix`` of nside_hi."""
    return nest2ring(nside_lo, ring2nest(nside_hi, pix) // (nside_hi // nside_lo) ** 2)


def ud_grade(maps, nside_out, dtype=np.float64):
    """RING maps [nmap, npix_in] -> [nmap, npix_out]: the children, in NESTED order, summed pairwise (a balanced binary
    tree: equal children sum exactly), then divided."""
    maps = np.asarray(maps, dtype=dtype)
    nside_in = int(round((maps.shape[1] / 12) ** 0.5))
    npo = 12 * nside_out * nside_out
    if nside_out == nside_in:
        return maps.copy()
    if nside_out > nside_in:
        return maps[:, parent(nside_out, nside_in, np.arange(npo))]
    m = (nside_in // nside_out) ** 2
    nest_o = ring2nest(nside_out, np.arange(npo))
    v = np.stack([maps[:, nest2ring(nside_in, nest_o * m + j)] for j in range(m)], axis=-1)
    while v.shape[-1] > 1:                             # neighbours in NESTED order first: a balanced tree
        v = v[..., 0::2] + v[..., 1::2]
    return v[..., 0] / dtype(m)
