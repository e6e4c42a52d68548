"""Oracles and bounds of the constrained-galaxy kernels (csrc/galaxy.hip; test infrastructure only).

eps = 2^-52, u = eps / 2: one rounded operation errs by at most u relative.  The long-double evaluations below are taken
as exact (their own rounding, 2^-64, is covered by the factor SLACK = 1 + 2^-10 on every bound, which also takes the
terms of second order in u).

Reorder and alm_scale_l are exact: a permutation, and one IEEE product per component.  The permutations are those of
tests/_pointsource_oracle.py (ring2nest / nest2ring of the NESTED hierarchy), which the ud_grade kernel is pinned to.

Block variance.  n = 4^k children x_i with mean mu and variance V = sum (x_i - mu)^2 / n; L = log2 n.
    Pass 1.  A pairwise sum of n terms errs by at most L u sum |x_i| (Higham 2002, eq. 4.6) and the division by n (a
        power of two) is exact: |mu^ - mu| <= L u mean|x| =: dmu.
    Pass 2.  sum (x_i - mu^)^2 = n V + n (mu - mu^)^2 exactly (the two-pass identity of Chan, Golub & LeVeque 1983,
        section 2): the error of the mean enters squared.  Each term carries the rounding of the difference (twice,
        squared) and of the square, 3 u, the pairwise sum L u: a relative error (L + 3) u of a sum of non-negative
        terms.  So
            |V^ - V| <= (L + 3) u V + dmu^2 (1 + (L + 3) u),      dmu^2 <= L^2 u^2 mean|x|^2 <= L^2 u^2 V kappa^2,
        kappa^2 = 1 + mu^2 / V = mean(x^2) / V (mean|x|^2 <= mean(x^2)): the bound of Chan, Golub & LeVeque for the
        two-pass algorithm, with L in place of n for the pairwise sums.  It is used in its absolute form
            tol = (L + 3) u V + L^2 u^2 (V + mu^2),
        whose second term is the floor that the rounding of the mean leaves when V is small against mu^2.  The one-pass
        formula E[x^2] - E[x]^2 errs by about u kappa^2 V = u mean(x^2) instead, i.e. without the second factor u.
    A reference in float64 that sums in ANY order (numpy's var) obeys the same with n - 1 in place of L:
        tol_ref = (n + 2) u V + (n - 1)^2 u^2 (V + mu^2).

Combine.  From the float64 inputs h = haslam, s = sc, a = am, d-terms fg, fgs, r = lnr[c] = fl(log(efreq / 408)) and
    w = fl(1 / mv), exact values S = h exp(s r), x = (a / mv) (fg - fgs) / S, out = S (1 + tanh_lin(x)).
    S^:  e^ = fl(s r) = s r (1 + d), |d| <= u, moves exp by the factor exp(s r d): relative |s r| u.  The kernel's exp is
         glibc's (csrc/glibc_exp.h; glibc documents < 1 ulp, 0.511 measured): eps relative.  The product with h: u.
             rho_S = |s r| u + eps + u.
    t^:  w carries u against 1 / mv, a w one more u (the reference rounds a / mv once: u; 2 u covers both forms),
         fg - fgs is rounded once, u relative to |fg - fgs|, the product u:  rho_t = 4 u.
    x^ = fl(t^ / S^):  rho_x = rho_t + rho_S + u.  Its sign is that of fg - fgs, which a rounded difference keeps.
    x >= 0:  1 + x^ rounded: |fl(1 + x^) - (1 + x)| <= |x| rho_x + u (1 + x); the product with S^: rho_S + u of the
         result:   tol = S [ |x| rho_x + (1 + x) (rho_S + 2 u) ].
    x < 0:   |tanh x^ - tanh x| <= |x| rho_x sech^2(x*) <= |x| rho_x sech^2(x (1 - rho_x)) (sech^2 decreases in |x|); the
         device tanh is taken to meet the OpenCL C bound for double tanh, 5 ulp = 5 eps |tanh x| <= 5 eps - an
         ASSUMPTION: the ROCm device-library documents that state its bounds are not installed here; the device
         library is written to the OpenCL accuracy table.  1 + tanh x^ cancels: its rounding is u (1 + tanh x) <= u, and
         the errors above stay absolute, of order u S and not relative to the result:
             tol = S [ |x| rho_x sech^2(x (1 - rho_x)) + 5 eps |tanh x| + (1 + tanh x) (rho_S + 2 u) ].
    At x = +-0 both branches give 1 exactly, so out^ = S^; with s r = 0 (s = 0, or a channel at 408 MHz) exp gives 1
    and S^ = h exactly.
"""
import os

import numpy as np

import _pointsource_oracle as po

EPS = 2.0 ** -52
U = EPS / 2
LD = np.longdouble
SLACK = 1.0 + 2.0 ** -10
TANH_ULP = 5.0
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "galaxy_vectors.npz")


def load_golden():
    return np.load(GOLDEN)


# ---- reorder ----------------------------------------------------------------------------------------------------------

def reorder(maps, r2n):
    """healpy.reorder of [nmap, npix]: out[:, q] = maps[:, p(q)]."""
    maps = np.asarray(maps)
    npix = maps.shape[-1]
    nside = int(round((npix / 12) ** 0.5))
    perm = po.nest2ring(nside, np.arange(npix)) if r2n else po.ring2nest(nside, np.arange(npix))
    return maps[..., perm]


# ---- block variance ---------------------------------------------------------------------------------------------------

def _blocks(maps, nside_out):
    """[nmap, npix_out (NESTED), n] children of every output pixel, and the RING index of every NESTED output pixel."""
    maps = np.asarray(maps)
    nside_in = int(round((maps.shape[1] / 12) ** 0.5))
    n = (nside_in // nside_out) ** 2
    nest = maps[:, po.nest2ring(nside_in, np.arange(maps.shape[1]))]
    return nest.reshape(maps.shape[0], -1, n), po.nest2ring(nside_out, np.arange(12 * nside_out * nside_out)), n


def block_variance(maps, nside_out):
    """(var, tol, tol_ref) [nmap, npix_out] in RING order: the exact block variance (long double), the bound on the
    kernel's error and the bound on a float64 reference summing in any order (module docstring)."""
    blocks, ring_of, n = _blocks(np.asarray(maps, dtype=np.float64), nside_out)
    x = blocks.astype(LD)
    mu = x.mean(axis=2)
    V = ((x - mu[..., None]) ** 2).mean(axis=2)
    L = np.log2(n)
    tol = ((L + 3) * U * V + (L * U) ** 2 * (V + mu * mu)) * SLACK
    tol_ref = ((n + 2) * U * V + ((n - 1) * U) ** 2 * (V + mu * mu)) * SLACK
    out = [np.empty(V.shape, dtype=LD) for _ in range(3)]
    for o, v in zip(out, (V, tol, tol_ref)):
        o[:, ring_of] = v
    return out


def block_variance_onepass(maps, nside_out):
    """E[x^2] - E[x]^2 in float64, the formula the kernel must not use: RING order."""
    blocks, ring_of, _ = _blocks(np.asarray(maps, dtype=np.float64), nside_out)
    v = (blocks * blocks).mean(axis=2) - blocks.mean(axis=2) ** 2
    out = np.empty_like(v)
    out[:, ring_of] = v
    return out


# ---- combine ----------------------------------------------------------------------------------------------------------

def _combine_bound(S, x, th, rho_S, rho_t):
    rho_x = rho_t + rho_S + U
    with np.errstate(over="ignore"):
        sech2 = 1 / np.cosh(x * (1 - rho_x)) ** 2
    pos = np.abs(x) * rho_x + (1 + x) * (rho_S + 2 * U)
    neg = np.abs(x) * rho_x * sech2 + TANH_ULP * EPS * np.abs(th) + (1 + th) * (rho_S + 2 * U)
    return S * np.where(x < 0, neg, pos) * SLACK


def combine(fg, fgs, haslam, sc, am, mv, efreq, skip=2):
    """(out, tol, tol_ref) [nchan - skip, npix]: the exact value in long double from the float64 inputs (``lnr`` the
    float64 log(efreq / 408) handed to the kernel), the pointwise bound on the kernel of the module docstring, and the
    bound of the same shape on a float64 evaluation in the reference's order (galaxy.py:181-198): there
    S = h (efreq / 408)^sc carries the quotient and pow's ulp, and against exp(sc lnr) the rounding of lnr and log's ulp,
    rho_S = |s r| (u + eps) + u + eps + u; t = (a / mv) (fg - fgs): rho_t = 3 u; its tanh (glibc, < 1 ulp) is inside the
    5 ulp."""
    fg, fgs = np.asarray(fg, dtype=np.float64)[skip:], np.asarray(fgs, dtype=np.float64)[skip:]
    lnr = np.log(np.asarray(efreq, dtype=np.float64) / 408.0)[skip:]
    h, s, a = (np.asarray(v, dtype=np.float64).astype(LD)[None, :] for v in (haslam, sc, am))
    r = lnr.astype(LD)[:, None]
    S = h * np.exp(s * r)
    x = (a / LD(mv)) * (fg.astype(LD) - fgs.astype(LD)) / S
    th = np.tanh(x)
    out = S * (1 + np.where(x < 0, th, x))
    tol = _combine_bound(S, x, th, np.abs(s * r) * U + EPS + U, 4 * U)
    tol_ref = _combine_bound(S, x, th, np.abs(s * r) * (U + EPS) + 2 * U + EPS, 3 * U)
    return out, tol, tol_ref


def worst(err, tol):
    """max of err / tol with 0 / 0 = 0: the figure every test prints."""
    err, tol = np.asarray(err, dtype=LD), np.asarray(tol, dtype=LD)
    ratio = np.where(err == 0, 0.0, err / np.where(tol == 0, LD(1e-4000), tol))
    return float(ratio.max())
