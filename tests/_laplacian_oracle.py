"""numpy oracle of ``lssutil.laplacian`` (cora/signal/lssutil.py:188-222).  Test infrastructure only.

    out_i = S[-l (l + 1) a_i] / x_i^2 + diff2(maps, x)_i + 2 np.gradient(maps, x, axis=0)_i / x_i,
    a_i = map2alm(maps_i, iter=3) without weights (healpy's defaults), S the synthesis at the maps' nside,

written from the formula with ``oracle.sht`` for the transforms, ``np.gradient`` as it is and ``diff2`` written out
below as what its scheme is: the second derivative at x_i of the Lagrange cubic through four samples - rows
i - 2 .. i + 1 on rows 2 .. N - 2, the first four rows on rows 0 and 1, the last four on row N - 1.  Here the weights
are the second derivatives of the Lagrange basis polynomials, computed from their definition - not the closed-form
expressions in the spacings that the package evaluates - so the two are independent (they agree to 1e-16 of the
largest weight on uniform, non-uniform and descending x).

Tolerance per slice i (``tolerances``), every term derived:

  analysis   the iterated analysis is held to 1e-11 max|a_i| per coefficient (tests/test_gpu_displacement.py:273).
             Coefficient errors of that size, scaled by l (l + 1) / x_i^2, synthesise to a map of rms at most
             1e-11 max|a_i| sqrt(sum_l (2l + 1) l^2 (l + 1)^2 / 4 pi) / x_i^2 (Parseval).
  synthesis  one synthesis is held to 1e-11 of the rms of its map (tests/_grad_oracle.py): 1e-11 rms(S[l (l + 1) a_i]) /
             x_i^2, the rms from Parseval on the coefficients.
  radial     both sides evaluate sum_k (d_k + 2 g_k / x_i) w_k in floating point.  In units of u = eps / 2 relative to
             sum_k (|d_k| + |2 g_k / x_i|) |w_k|: a coefficient d_k costs at most 6 roundings from the spacings, g_k at
             most 4, the merge 2 / x, times g, plus d another 3, the four products and three sums of the stencil 5
             (gamma_5) - 18 u for the device; for numpy's separate sums no more (6 + 4 for the coefficients, 4 and 3 for
             the two stencils, 2 for 2 g / x, 2 for the additions: 21 u).  39 u together: RADIAL_EPS = 20 eps.
  sum        adding the radial to the angular part rounds twice on each side: 4 u (|angular| + radial terms) =
             2 eps |angular|, the radial share being inside the 20 eps.
"""
import numpy as np

from oracle import sht as osht

EPS = np.finfo(np.float64).eps
GATE = 1e-11
RADIAL_EPS = 20.0


def lagrange_d2_weights(xs, at):
    """Second derivative at ``at`` of the four Lagrange basis cubics on the nodes xs [4]: for basis j with the other
    nodes p, q, r: L_j(x) = (x - p)(x - q)(x - r) / ((x_j - p)(x_j - q)(x_j - r)), L_j'' = 2 (3 x - p - q - r) / (...)."""
    w = np.empty(4)
    for j in range(4):
        o = [xs[k] for k in range(4) if k != j]
        den = (xs[j] - o[0]) * (xs[j] - o[1]) * (xs[j] - o[2])
        w[j] = 2.0 * ((at - o[0]) + (at - o[1]) + (at - o[2])) / den
    return w


def first_rows(n):
    return np.clip(np.arange(n) - 2, 0, n - 4)


def diff2_weights(x):
    """[n, 4] weights of diff2 over the rows first_rows(n)[i] .. + 3"""
    x = np.asarray(x, dtype=np.float64)
    n = x.size
    first = first_rows(n)
    return np.stack([lagrange_d2_weights(x[first[i]:first[i] + 4], x[i]) for i in range(n)])


def diff2(f, x):
    """diff2(f, x, axis=0) for f [n, ncol]"""
    w, first = diff2_weights(x), first_rows(len(x))
    return np.stack([w[i] @ f[first[i]:first[i] + 4] for i in range(len(x))])


def gradient_weights(x):
    """[n, 4] weights of np.gradient(f, x, axis=0) (second order inside, first order at the ends) over the same rows"""
    x = np.asarray(x, dtype=np.float64)
    n = x.size
    first = first_rows(n)
    w = np.zeros((n, 4))
    eye = np.eye(n)
    g = np.gradient(eye, x, axis=0)                      # g[i, j] = weight of f[j] in row i
    for i in range(n):
        w[i] = g[i, first[i]:first[i] + 4]
        assert np.count_nonzero(g[i]) == np.count_nonzero(w[i])
    return w


def radial_weights(x):
    """Restatement of lssutil.laplacian_coefficients: d_k + 2 g_k / x_i, and the magnitudes |d_k| + |2 g_k / x_i|"""
    x = np.asarray(x, dtype=np.float64)
    d, g = diff2_weights(x), gradient_weights(x)
    return d + 2.0 * g / x[:, None], np.abs(d) + np.abs(2.0 * g / x[:, None])


def radial(maps, x):
    """diff2(maps, x) + 2 np.gradient(maps, x, axis=0) / x, the reference's two terms, and sum_k (|d_k| + |2 g_k / x|) |w_k|"""
    x = np.asarray(x, dtype=np.float64)
    _, mag = radial_weights(x)
    first = first_rows(len(x))
    terms = np.stack([mag[i] @ np.abs(maps[first[i]:first[i] + 4]) for i in range(len(x))])
    return diff2(maps, x) + 2.0 * np.gradient(maps, x, axis=0) / x[:, None], terms


def ell_factor(lmax):
    """l (l + 1) of every packed index"""
    l = np.concatenate([np.arange(mm, lmax + 1) for mm in range(lmax + 1)]).astype(np.float64)
    return l * (l + 1.0)


def analyse(maps, nside, lmax, niter=3):
    return np.stack([osht.map2alm(m, nside, lmax, use_weights=False, niter=niter) for m in maps])


def angular(alm, x, nside, lmax):
    """S[-l (l + 1) a_i] / x_i^2 for packed alm [n, nalm]"""
    fac = ell_factor(lmax)
    return np.stack([osht.alm2map(-fac * alm[i], nside, lmax) / x[i] ** 2 for i in range(len(x))])


def laplacian(maps, x, nside, lmax, niter=3):
    """(laplacian, angular part, radial part, radial magnitudes, alm) of maps [n, npix]"""
    maps = np.asarray(maps, dtype=np.float64)
    x = np.asarray(x, dtype=np.float64)
    alm = analyse(maps, nside, lmax, niter)
    ang = angular(alm, x, nside, lmax)
    rad, terms = radial(maps, x)
    return ang + rad, ang, rad, terms, alm


def map_rms(alm, lmax):
    """rms over the sphere of the real maps with packed coefficients alm [n, nalm] (Parseval)"""
    n0 = lmax + 1
    p = (alm[:, :n0].real ** 2).sum(axis=1) + 2.0 * (np.abs(alm[:, n0:]) ** 2).sum(axis=1)
    return np.sqrt(p / (4.0 * np.pi))


def angular_tolerance(alm, x, lmax):
    """[n]: the analysis and the synthesis gate propagated through l (l + 1) / x^2 (module docstring)"""
    l = np.arange(lmax + 1, dtype=np.float64)
    spread = np.sqrt(((2 * l + 1) * (l * (l + 1)) ** 2).sum() / (4.0 * np.pi))
    amax = np.abs(alm).max(axis=1)
    return GATE * (amax * spread + map_rms(ell_factor(lmax) * alm, lmax)) / np.asarray(x) ** 2


def tolerances(alm, x, lmax, ang, terms):
    """[n, npix] tolerance of a Laplacian against ``laplacian``: angular gates + radial rounding + the final sums"""
    return angular_tolerance(alm, x, lmax)[:, None] + RADIAL_EPS * EPS * terms + 2.0 * EPS * np.abs(ang)
