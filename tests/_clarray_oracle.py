"""Host oracle for K1 (csrc/clarray.hip): numpy only, no GPU, no reference tree.

  * ``reference``           what corahip_clarray_table21cm is documented to compute, in np.longdouble and in the
                            CORNER form of bilinearmap.interp (four corners x three tables per multipole and sub-sample
                            pair - the form aps21_points_kernel implements literally), with its pointwise ``bound``;
  * ``reference_points``    the same for one sub-pair per point (corahip_aps_table21cm_points);
  * ``weighted_sum``        the Romberg double sum of romb_reduce_kernel / separable_kernel with a gamma_n bound;
  * ``kernel_restatement``  clarray21_kernel's arithmetic in float64 (profile per sub-pair, slot nkperp, 1-D
                            interpolation), with named mutants: the bound is checked on the host with it;
  * ``paths``               the kernel's branch predicates in float64, per channel pair and l launch;
  * ``pair_of_index``       the band / XCD-permuted pair enumeration;
  * ``make_case``           synthetic tables and channel data; ``make_points`` scattered points for the point form;
  * ``case`` / ``reference_of`` / ``expect``   the named cases of tests/test_gpu_clarray.py, their reference (computed
                            once per process) and the assertion that a case reaches the path it was written for.

The bound, per output element (channel pair, multipole), is the sum over the zint^2 sub-sample pairs of three parts:

  1. gamma_n * sum |weight * c_T * table corner| over the 12 products of the sub-pair, n = 2 zint + 21, counted from
     the kernel in units of u = 2^-53:
       9   W = w_a w_b pfd_a pfd_b / (xc^2 pi): three products, xc = (chi_a + chi_b) / 2 rounded once and squared (2),
           xc * xc (1), M_PI's own rounding (1), * M_PI (1), the division (1);
       3   c_dv = W (f_a b_b + f_b b_a): two products and a sum (relative to |f_a b_b| + |f_b b_a|, which is what the
           bound sums), times W; c_dd and c_vv take 2;
       2   1 - wy, and its product with c_T (wy = yy - y0 is exact);
       6   the 6-term profile: a product and at most five additions (fewer with fma contraction);
       1   fma(wx, s1 - s0, s0) (wx = fract(xx) is exact; the rounding of s1 - s0 is in part 2);
       2 zint   the additions of a term into s (over b) and of s into acc (over a).
  2. |dV/dx| * dx, dV/dx = the bracketing row difference of the sub-pair's combined profile, and
       dx = u (K_X (|log10l xscale| + |lxc| + 1) + K_ARG xscale),   K_X = 4 + 4 LOG10_ULP,  K_ARG = 2 / ln 10:
       xscale = (nkperp - 1) / log10(kperpmax / kperpmin) carries (2 + 2 LOG10_ULP) u (the quotient's rounding passes
       the logarithm with a factor 1 / ln(kperpmax / kperpmin) <= 1 - asserted -, the logarithm, the division), the
       product log10l * xscale 1 more, lxc = log10(xc kperpmin) * xscale 2 LOG10_ULP + 1 more, the subtraction 1 on each:
       3 + 2 LOG10_ULP and 3 + 4 LOG10_ULP, both <= K_X.  The two roundings of the logarithm's ARGUMENT (xc, xc *
       kperpmin) are an absolute 2u / ln 10 in the logarithm whatever its size - not relative to |lxc|, which vanishes at
       xc kperpmin = 1 - hence the K_ARG term.  The "+ 1" holds wx * u, the rounding of s1 - s0 in the fma form.
  3. |dV/dy| * dy, dy = K_Y u (y + 1), K_Y = 4: |chi_b - chi_a| (1), M_PI (1), kparmax / M_PI (1), the product (1).

Parts 2 and 3 are what make the bound hold when a float64 x or y falls on the other side of an integer from the
extended-precision one: the bilinear interpolant is CONTINUOUS there, so the two evaluations differ by at most the
larger of the two neighbouring slopes times the distance.  Where x (y) lies within 2 dx (2 dy) of an integer the slope
is therefore the larger of the slopes at x - 2 dx and x + 2 dx.  Past the clamps the interpolant is constant (slot
nkperp repeats the last row; column nkpar - 1 is its own neighbour), so the rounding of nk - 1e-5 does not enter.

LOG10_ULP is ASSUMED: nothing in the installed ROCm tree documents the accuracy of the device library's double
precision log10.  3 ulp is the OpenCL full-profile limit for log10, the specification OCML's functions are written to;
HIP's published figure is 1.  It was not tuned to any GPU result.

np.longdouble is the x87 80-bit format here (eps 1.08e-19), 2000 times finer than the float64 roundings it bounds.
"""
import numpy as np

LD = np.longdouble
U = 2.0 ** -53
LOG10_ULP = 3                    # assumed, see above
K_X = 4 + 4 * LOG10_ULP
K_Y = 4
K_ARG = 2.0 / np.log(10.0)
N_POINTS = 16                    # aps21_points_kernel, see reference_points
CL_BAND = 32
CL_LPT = 9
L_LAUNCH = 256 * CL_LPT          # multipoles of one launch of clarray21_kernel
PI_LD = LD(4) * np.arctan(LD(1))

MUTANTS = ("slot_prev_row", "wy_kept", "no_low_clamp_first", "w_reversed_a", "fb_partner", "drop_subpair")


def gamma(n):
    return LD(n) * LD(U) / (LD(1) - LD(n) * LD(U))


def n_terms(zint):
    return 2 * zint + 21


# ------------------------------------------------------------------ pair enumeration
def _band_count(n):
    return CL_BAND * (n - (CL_BAND - 1)) + (CL_BAND - 1) * CL_BAND // 2 if n >= CL_BAND else n * (n + 1) // 2


def pair_of_index(p, F):
    """Canonical pair p of (i, j >= i): bands of CL_BAND diagonals; inside a band's full rows p = 8 s + x is pair
    (row s // 4, separation 4 x + s % 4); then the tail rows, i-major."""
    B = 0
    while True:
        c = _band_count(F - CL_BAND * B)
        if p < c:
            break
        p -= c
        B += 1
    n = F - CL_BAND * B
    nfull = n - (CL_BAND - 1) if n >= CL_BAND else 0
    if p < nfull * CL_BAND:
        xq, sq = p & 7, p >> 3
        i, d = sq >> 2, 4 * xq + (sq & 3)
    else:
        p -= nfull * CL_BAND
        e = CL_BAND - 1 if n >= CL_BAND else n
        i = nfull
        while p >= e:
            p -= e
            e -= 1
            i += 1
        d = p
    return i, i + CL_BAND * B + d


def all_pairs(F):
    return np.array([pair_of_index(p, F) for p in range(F * (F + 1) // 2)], dtype=np.int64).reshape(-1, 2)


# ------------------------------------------------------------------ cases
def log10l_range(nl, first=0):
    """log10 of l = first .. first + nl - 1, with the l = 0 sentinel 1e-10 of the reference."""
    l = np.arange(first, first + nl, dtype=np.float64)
    return np.log10(np.where(l == 0, 1e-10, l))


def make_case(seed, F, zint, chan, half, log10l, nkperp=40, nkpar=64, kperpmin=1e-3, kperpmax=10.0, kparmax=5.0,
              smooth=False):
    """Tables [nkperp, nkpar] (random O(1) entries of both signs, or smooth ones), chi[i zint + a] = chan[i] + half *
    linspace(-1, 1, zint)[a], random pfd, f, b per sub-sample, and NON-UNIFORM weights with a negative entry that sum to
    1: neither a reversed nor a misattached weight leaves the sum unchanged."""
    rng = np.random.default_rng(seed)
    if smooth:
        xg, yg = np.meshgrid(np.arange(nkperp, dtype=np.float64), np.arange(nkpar, dtype=np.float64), indexing="ij")
        tabs = [np.exp(-0.03 * yg) * np.cos(0.31 * xg + 0.17 * yg + ph) * (1.0 + 0.02 * xg) for ph in (0.3, 1.7, 2.9)]
    else:
        tabs = list(rng.standard_normal((3, nkperp, nkpar)))
    chan = np.asarray(chan, dtype=np.float64)
    assert chan.shape == (F,)
    off = np.linspace(-1.0, 1.0, zint) if zint > 1 else np.zeros(1)
    chi = (chan[:, None] + half * off[None, :]).ravel()
    w = rng.uniform(0.5, 1.5, zint)
    if zint >= 3:
        w[zint // 2] *= -0.5
    w = w / w.sum()
    return dict(dd=np.ascontiguousarray(tabs[0]), dv=np.ascontiguousarray(tabs[1]), vv=np.ascontiguousarray(tabs[2]),
                nkperp=nkperp, nkpar=nkpar, kperpmin=float(kperpmin), kperpmax=float(kperpmax), kparmax=float(kparmax),
                chi=chi, pfd=rng.uniform(0.5, 1.5, F * zint), f=rng.uniform(0.3, 1.2, F * zint),
                b=rng.uniform(0.8, 2.0, F * zint), F=F, zint=zint, w=w, log10l=np.asarray(log10l, dtype=np.float64))


def _sub_indices(case, pairs):
    zint = case["zint"]
    a = np.repeat(np.arange(zint), zint)
    b = np.tile(np.arange(zint), zint)
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    return a, b, pairs[:, 0, None] * zint + a[None, :], pairs[:, 1, None] * zint + b[None, :]


# ------------------------------------------------------------------ extended-precision reference
def _bilinear(case, x, y, cs, cabs):
    """Corner-form lookup at (x, y) (clipped already, broadcastable longdouble arrays) combined with the coefficient
    triples cs (signed) and cabs (of absolute values) -> value, sum of |products|, dV/dx, dV/dy of the cell."""
    nkperp, nkpar = case["nkperp"], case["nkpar"]
    x0 = np.floor(x).astype(np.int64)
    y0 = np.floor(y).astype(np.int64)
    x1 = np.minimum(x0 + 1, nkperp - 1)
    y1 = np.minimum(y0 + 1, nkpar - 1)
    wx, wy = x - x0, y - y0
    V = A = SX = SY = LD(0)
    for T, c, ca in zip((case["dd"], case["dv"], case["vv"]), cs, cabs):
        t00, t01, t10, t11 = (T[x0, y0].astype(LD), T[x0, y1].astype(LD), T[x1, y0].astype(LD), T[x1, y1].astype(LD))
        r0 = (1 - wy) * t00 + wy * t01
        r1 = (1 - wy) * t10 + wy * t11
        V = V + c * ((1 - wx) * r0 + wx * r1)
        A = A + ca * ((1 - wx) * ((1 - wy) * np.abs(t00) + wy * np.abs(t01)) +
                      wx * ((1 - wy) * np.abs(t10) + wy * np.abs(t11)))
        SX = SX + c * (r1 - r0)
        SY = SY + c * ((1 - wx) * (t01 - t00) + wx * (t11 - t10))
    return V, A, SX, SY


def _scales_ld(case):
    ratio = LD(case["kperpmax"]) / LD(case["kperpmin"])
    assert np.log(ratio) >= 1, "the derivation of K_X needs ln(kperpmax / kperpmin) >= 1"
    return LD(case["nkperp"] - 1) / np.log10(ratio), LD(case["kparmax"]) / PI_LD


def _near_integer_slopes(case, x, y, dx, dy, cs, cabs, SX, SY):
    """|SX|, |SY| with the larger neighbouring slope where x (y) is within 2 dx (2 dy) of an integer."""
    ux, uy = LD(case["nkperp"]) - LD(1e-5), LD(case["nkpar"]) - LD(1e-5)
    SXa, SYa = np.abs(SX), np.abs(SY)
    shape = SXa.shape
    full = lambda v: np.broadcast_to(v, shape)
    fx = x - np.floor(x)
    m = full((fx < 2 * dx) | (1 - fx < 2 * dx))
    if m.any():
        xm, ym, dm = full(x)[m], full(y)[m], full(dx)[m]
        cm, cam = [full(c)[m] for c in cs], [full(c)[m] for c in cabs]
        lo = _bilinear(case, np.clip(xm - 2 * dm, 0, ux), ym, cm, cam)[2]
        hi = _bilinear(case, np.clip(xm + 2 * dm, 0, ux), ym, cm, cam)[2]
        SXa = SXa.copy()
        SXa[m] = np.maximum(SXa[m], np.maximum(np.abs(lo), np.abs(hi)))
    fy = y - np.floor(y)
    m = full((fy < 2 * dy) | (1 - fy < 2 * dy))
    if m.any():
        xm, ym, dm = full(x)[m], full(y)[m], full(dy)[m]
        cm, cam = [full(c)[m] for c in cs], [full(c)[m] for c in cabs]
        lo = _bilinear(case, xm, np.clip(ym - 2 * dm, 0, uy), cm, cam)[3]
        hi = _bilinear(case, xm, np.clip(ym + 2 * dm, 0, uy), cm, cam)[3]
        SYa = SYa.copy()
        SYa[m] = np.maximum(SYa[m], np.maximum(np.abs(lo), np.abs(hi)))
    return SXa, SYa


def reference(case, pairs=None, chunk=512):
    """(C, bound), longdouble [npairs, nl]: C[p, l] of channel pair pairs[p] (default: the canonical enumeration) and
    its pointwise tolerance (module docstring)."""
    F, zint = case["F"], case["zint"]
    pairs = all_pairs(F) if pairs is None else np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    xs, ys = _scales_ld(case)
    ux, uy = LD(case["nkperp"]) - LD(1e-5), LD(case["nkpar"]) - LD(1e-5)
    chi, pfd, f, b, w = (case[k].astype(LD) for k in ("chi", "pfd", "f", "b", "w"))
    lx = case["log10l"].astype(LD) * xs
    C = np.empty((len(pairs), lx.size), dtype=LD)
    B = np.empty_like(C)
    g = gamma(n_terms(zint))
    for p0 in range(0, len(pairs), chunk):
        a, bb, za, zb = _sub_indices(case, pairs[p0:p0 + chunk])
        xc = (chi[za] + chi[zb]) / 2
        lxc = np.log10(xc * LD(case["kperpmin"])) * xs
        y = np.clip(np.abs(chi[zb] - chi[za]) * ys, 0, uy)[:, :, None]
        W = w[a] * w[bb] * pfd[za] * pfd[zb] / (xc * xc * PI_LD)
        cs = [(W * b[za] * b[zb])[:, :, None], (W * (f[za] * b[zb] + f[zb] * b[za]))[:, :, None],
              (W * f[za] * f[zb])[:, :, None]]
        cabs = [np.abs(cs[0]), (np.abs(W) * (np.abs(f[za] * b[zb]) + np.abs(f[zb] * b[za])))[:, :, None], np.abs(cs[2])]
        x = np.clip(lx[None, None, :] - lxc[:, :, None], 0, ux)
        V, A, SX, SY = _bilinear(case, x, y, cs, cabs)
        dx = LD(U) * (K_X * (np.abs(lx)[None, None, :] + np.abs(lxc)[:, :, None] + 1) + LD(K_ARG) * xs)
        dy = K_Y * LD(U) * (y + 1)
        SXa, SYa = _near_integer_slopes(case, x, y, dx, dy, cs, cabs, SX, SY)
        C[p0:p0 + chunk] = V.sum(axis=1)
        B[p0:p0 + chunk] = g * A.sum(axis=1) + (SXa * dx).sum(axis=1) + (SYa * dy).sum(axis=1)
    return C, B


def reference_points(case, lx, chi1, chi2, cdd, cdv, cvv):
    """corahip_aps_table21cm_points: one sub-pair per point, coefficients given, the 1 / (xc^2 pi) applied at the end.
    n = N_POINTS = 16: the corner weight (1 - wx)(1 - wy) (3), its product with the table entry (1), the 4-term sum
    (3), c_T * v_T (1), the 3-term sum (2), and the divisor xc^2 pi (xc twice, xc * xc, M_PI, * M_PI: 5) with the
    division (1).  x is formed as (lx - log10(xc kperpmin)) * xscale: the same dx covers it (3 + 4 LOG10_ULP <= K_X)."""
    xs, ys = _scales_ld(case)
    ux, uy = LD(case["nkperp"]) - LD(1e-5), LD(case["nkpar"]) - LD(1e-5)
    lx, chi1, chi2 = (np.asarray(v, dtype=np.float64).astype(LD) for v in (lx, chi1, chi2))
    cs = [np.asarray(v, dtype=np.float64).astype(LD) for v in (cdd, cdv, cvv)]
    cabs = [np.abs(c) for c in cs]
    xc = (chi1 + chi2) / 2
    lxc = np.log10(xc * LD(case["kperpmin"])) * xs
    x = np.clip(lx * xs - lxc, 0, ux)
    y = np.clip(np.abs(chi2 - chi1) * ys, 0, uy)
    V, A, SX, SY = _bilinear(case, x, y, cs, cabs)
    dx = LD(U) * (K_X * (np.abs(lx * xs) + np.abs(lxc) + 1) + LD(K_ARG) * xs)
    dy = K_Y * LD(U) * (y + 1)
    SXa, SYa = _near_integer_slopes(case, x, y, dx, dy, cs, cabs, SX, SY)
    d = xc * xc * PI_LD
    return V / d, (gamma(N_POINTS) * A + SXa * dx + SYa * dy) / d


def weighted_sum(X, w, scale=None):
    """sum_ab w_a w_b X[..., a, ..., b] of romb_reduce_kernel (X = clt[l, i, a, j, b]) and, with ``scale`` = al[l],
    separable_kernel -> (value, bound), longdouble [nl, F, F].  n = 2 zint + 2: t += w_b x (a product, at most zint
    additions), s += w_a t (the same); one more for the product with al[l]."""
    X = np.asarray(X, dtype=np.float64).astype(LD)
    w = np.asarray(w, dtype=np.float64).astype(LD)
    zint = w.size
    ww = w[None, None, :, None, None] * w[None, None, None, None, :]
    val = (ww * X).sum(axis=(2, 4))
    mag = (np.abs(ww) * np.abs(X)).sum(axis=(2, 4))
    n = 2 * zint + 2
    if scale is not None:
        s = np.asarray(scale, dtype=np.float64).astype(LD)[:, None, None]
        val, mag, n = val * s, mag * np.abs(s), n + 1
    return val, gamma(n) * mag


# ------------------------------------------------------------------ the kernel, restated in float64
def _scales_f64(case):
    xs = np.float64(case["nkperp"] - 1) / np.log10(np.float64(case["kperpmax"]) / np.float64(case["kperpmin"]))
    return xs, np.float64(case["kparmax"]) / np.float64(np.pi)


def _sub_params_f64(case, pairs, mutant=None):
    """clarray21_kernel's per-sub-pair parameters, [npairs, zint^2] float64: lxc, y0, the six profile coefficients,
    and whether the sub-pair took the k_par edge."""
    nkpar, zint = case["nkpar"], case["zint"]
    xs, ys = _scales_f64(case)
    uy = np.float64(nkpar) - 1e-5
    a, b, za, zb = _sub_indices(case, pairs)
    chi, pfd, fz, bz, w = (case[k] for k in ("chi", "pfd", "f", "b", "w"))
    x1, x2 = chi[za], chi[zb]
    xc = 0.5 * (x1 + x2)
    lxc = np.log10(xc * np.float64(case["kperpmin"])) * xs
    yy = np.clip(np.abs(x2 - x1) * ys, 0.0, uy)
    y0 = yy.astype(np.int64)
    wy = yy - y0
    edge = y0 + 1 > nkpar - 1
    y0 = np.where(edge, nkpar - 2, y0)
    if mutant != "wy_kept":
        wy = np.where(edge, 1.0, wy)
    wa = w[zint - 1 - a] if mutant == "w_reversed_a" else w[a]
    W = wa * w[b] * pfd[za] * pfd[zb] / (xc * xc * np.float64(np.pi))
    if mutant == "drop_subpair":
        W = W.copy()
        W[:, -1] = 0.0
    cdd = W * bz[za] * bz[zb]
    cdv = W * (fz[za] * bz[za] + fz[zb] * bz[zb]) if mutant == "fb_partner" else W * (fz[za] * bz[zb] + fz[zb] * bz[za])
    cvv = W * fz[za] * fz[zb]
    coef = [cdd * (1.0 - wy), cdd * wy, cdv * (1.0 - wy), cdv * wy, cvv * (1.0 - wy), cvv * wy]
    return lxc, y0, coef, edge


def kernel_restatement(case, pairs=None, mutant=None):
    """clarray21_kernel in float64 -> [npairs, nl].  Per sub-pair the 1-D profile over the table rows, slot nkperp
    repeating row nkperp - 1, then s0 + wx (s1 - s0) at x = clamp(log10l xscale - lxc), summed over b then a.

    mutant: ``slot_prev_row`` slot nkperp from row nkperp - 2; ``wy_kept`` wy left at its clamped fraction with y0 =
    nkpar - 2; ``no_low_clamp_first`` the first entry unclamped below (the profile's first interval extrapolated);
    ``w_reversed_a`` w[zint - 1 - a] w[b] (a literal exchange of w[a] and w[b] is the same product); ``fb_partner``
    c_dv = W (f_a b_a + f_b b_b); ``drop_subpair`` the last (a, b) missing."""
    assert mutant is None or mutant in MUTANTS
    F, zint, nkperp = case["F"], case["zint"], case["nkperp"]
    pairs = all_pairs(F) if pairs is None else np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    xs, _ = _scales_f64(case)
    ux = np.float64(nkperp) - 1e-5
    lx = case["log10l"] * xs
    lxc, y0, coef, _ = _sub_params_f64(case, pairs, mutant)
    prof = np.empty(lxc.shape + (nkperp + 1,))
    body = 0.0
    for k, T in enumerate((case["dd"], case["dd"], case["dv"], case["dv"], case["vv"], case["vv"])):
        body = body + coef[k][:, :, None] * np.moveaxis(T[:, y0 + (k & 1)], 0, -1)
    prof[..., :nkperp] = body
    prof[..., nkperp] = prof[..., nkperp - 2 if mutant == "slot_prev_row" else nkperp - 1]
    xr = lx[None, None, :] - lxc[:, :, None]
    xx = np.clip(xr, 0.0, ux)
    x0 = xx.astype(np.int64)
    wx = xx - x0
    s0 = np.take_along_axis(prof, x0, axis=-1)
    s1 = np.take_along_axis(prof, x0 + 1, axis=-1)
    v = s0 + wx * (s1 - s0)
    if mutant == "no_low_clamp_first":
        v[:, :, 0] = np.where(xr[:, :, 0] < 0, prof[..., 0] + xr[:, :, 0] * (prof[..., 1] - prof[..., 0]), v[:, :, 0])
    v = v.reshape(len(pairs), zint, zint, lx.size)
    acc = np.zeros((len(pairs), lx.size))
    for a in range(zint):
        s = np.zeros_like(acc)
        for b in range(zint):
            s = s + v[:, a, b]
        acc = acc + s
    return acc


def make_points(case, n, seed):
    """n scattered points (lx, chi1, chi2, cdd, cdv, cvv) for corahip_aps_table21cm_points: chi over three decades, a
    fifth of the points at chi1 == chi2 (y = 0 exactly), separations past the k_par edge, lx from below the low clamp
    (the l = 0 sentinel included) to past the high one."""
    rng = np.random.default_rng(seed)
    chi1 = 10.0 ** rng.uniform(0.7, 3.7, n)
    sep = rng.uniform(-1.5, 1.5, n) * case["nkpar"] * np.pi / case["kparmax"]
    sep[::5] = 0.0
    chi2 = np.maximum(chi1 + sep, 1.0)
    lx = rng.uniform(-1.0, 3.5, n)
    lx[1::7] = -10.0
    return (lx, chi1, chi2) + tuple(rng.standard_normal((3, n)))


def points_restatement(case, lx, chi1, chi2, cdd, cdv, cvv):
    """aps21_points_kernel in float64."""
    nkperp, nkpar = case["nkperp"], case["nkpar"]
    xs, ys = _scales_f64(case)
    xc = 0.5 * (chi1 + chi2)
    xx = np.clip((lx - np.log10(xc * np.float64(case["kperpmin"]))) * xs, 0.0, np.float64(nkperp) - 1e-5)
    yy = np.clip(np.abs(chi2 - chi1) * ys, 0.0, np.float64(nkpar) - 1e-5)
    x0, y0 = xx.astype(np.int64), yy.astype(np.int64)
    wx, wy = xx - x0, yy - y0
    xb, yb = np.minimum(x0 + 1, nkperp - 1), np.minimum(y0 + 1, nkpar - 1)
    wa, wb, wc, wd = (1.0 - wx) * (1.0 - wy), (1.0 - wx) * wy, wx * (1.0 - wy), wx * wy
    v = [wa * T[x0, y0] + wb * T[x0, yb] + wc * T[xb, y0] + wd * T[xb, yb] for T in (case["dd"], case["dv"], case["vv"])]
    return (cdd * v[0] + cdv * v[1] + cvv * v[2]) / (xc * xc * np.float64(np.pi))


def points_clamps(case, lx, chi1, chi2):
    """Which points take the low / high x clamp, the k_par edge, and y = 0 (float64 predicates of the kernel)."""
    xs, ys = _scales_f64(case)
    xr = (lx - np.log10(0.5 * (chi1 + chi2) * case["kperpmin"])) * xs
    yr = np.abs(chi2 - chi1) * ys
    return dict(x_low=xr < 0, x_high=xr > case["nkperp"] - 1e-5, y_high=yr > case["nkpar"] - 1e-5, y_zero=yr == 0)


def paths(case, pairs=None):
    """clarray21_kernel's branch predicates in float64 -> one dict per l launch (l_base = 0, 2304, ...): scalars
    ``l_base``, ``n`` (entries), ``zint_inst`` (3, 5, 9 or 0), ``nsp`` (early entries, after the cap of 32 and min with
    n), ``every_individual`` (nsp >= n), and bool arrays [npairs]: ``all_fast``, ``fast_build`` (all_fast with a compiled
    ZINT: the row-major build), ``xhi_top`` (a profile's row range reaches nkperp: the slot is written), ``slot_read``
    (an entry has x >= nkperp - 1), ``kpar_edge``, ``clamp_low_first``, ``clamp_low_later`` (an entry other than the
    launch's first is clamped below), ``clamp_high``."""
    F, zint, nkperp = case["F"], case["zint"], case["nkperp"]
    pairs = all_pairs(F) if pairs is None else np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    xs, _ = _scales_f64(case)
    ux = np.float64(nkperp) - 1e-5
    ll = case["log10l"]
    nl = ll.size
    lxc, _, _, edge = _sub_params_f64(case, pairs)
    out = []
    for l_base in range(0, nl, L_LAUNCH):
        l_end = min(nl, l_base + L_LAUNCH)
        n = l_end - l_base
        lx = ll[l_base:l_end] * xs
        lx_hi = lx[-1]
        x2nd = (lx[1] if n > 1 else lx_hi) - lxc
        noclamp = (x2nd >= 0.0) & (lx_hi - lxc <= ux)
        all_fast = noclamp.all(axis=1)
        wide = (ll[l_base + 1:min(l_end, l_base + 65)] - ll[l_base:min(l_end, l_base + 65) - 1]) * xs >= 2.0
        lead = int(np.argmin(wide)) if (wide.size and not wide.all()) else wide.size
        nsp = min(min(32, lead), n)
        xhi = np.clip(lx_hi - lxc, 0.0, ux)
        xr = lx[None, None, :] - lxc[:, :, None]
        zi = zint if zint in (3, 5, 9) else 0
        out.append(dict(l_base=l_base, n=n, zint_inst=zi, nsp=nsp, every_individual=nsp >= n, all_fast=all_fast,
                        fast_build=all_fast & (zi > 0),
                        xhi_top=(np.minimum(xhi.astype(np.int64) + 2, nkperp) == nkperp).any(axis=1),
                        slot_read=(np.clip(xr, 0.0, ux) >= nkperp - 1).any(axis=(1, 2)),
                        kpar_edge=edge.any(axis=1), clamp_low_first=(xr[:, :, 0] < 0).any(axis=1),
                        clamp_low_later=(xr[:, :, 1:] < 0).any(axis=(1, 2)), clamp_high=(xr > ux).any(axis=(1, 2))))
    return out


# ------------------------------------------------------------------ the cases of tests/test_gpu_clarray.py
# name -> (make_case arguments, path the case is written for: a predicate on paths(case), see expect())
def _chan(c0, step, F):
    return c0 + step * np.arange(F)


def _specs():
    s = {}
    for z in (3, 5, 9, 1, 2, 4, 17):   # interior: 30 Mpc < chi < 1000 Mpc keeps 0 <= x <= nkperp - 1 for 1 <= l < 300
        s["interior_z%d" % z] = dict(seed=10 + z, F=5, zint=z, chan=_chan(300.0, 6.0, 5), half=2.5,
                                     log10l=log10l_range(300))
    s["top_clamped"] = dict(seed=31, F=5, zint=3, chan=_chan(5.0, 7.0, 5), half=2.0, log10l=log10l_range(300))
    # chi within a factor 10^(1 / xscale): every sub-pair's last multipole in the same one or two table intervals
    s["top_fast_slot"] = dict(seed=32, F=5, zint=3, chan=_chan(8.1, 0.2, 5), half=0.08, log10l=log10l_range(96))
    s["top_fast_slot_odd"] = dict(seed=33, F=5, zint=5, chan=_chan(8.1, 0.2, 5), half=0.08, log10l=log10l_range(96),
                                  nkperp=41, smooth=True)
    s["top_fast_below"] = dict(seed=34, F=5, zint=9, chan=_chan(10.1, 0.2, 5), half=0.08, log10l=log10l_range(96))
    s["low_clamp"] = dict(seed=35, F=5, zint=3, chan=_chan(3100.0, 6.0, 5), half=2.5, log10l=log10l_range(300))
    s["kpar_edge"] = dict(seed=36, F=6, zint=3, chan=_chan(300.0, 15.0, 6), half=4.0, log10l=log10l_range(60))
    s["nsp0"] = dict(seed=37, F=4, zint=3, chan=_chan(300.0, 6.0, 4), half=2.5, log10l=log10l_range(200, first=200))
    s["nsp32"] = dict(seed=38, F=3, zint=5, chan=_chan(500.0, 6.0, 3), half=2.5, log10l=log10l_range(300),
                      nkperp=511, nkpar=8, kperpmax=1.0, kparmax=1.0)
    for nl in (1, 2, 3):
        s["few_l0_nl%d" % nl] = dict(seed=40 + nl, F=3, zint=3, chan=_chan(300.0, 6.0, 3), half=2.5,
                                     log10l=log10l_range(nl))
        s["few_l5_nl%d" % nl] = dict(seed=50 + nl, F=3, zint=3, chan=_chan(300.0, 6.0, 3), half=2.5,
                                     log10l=np.log10(np.array([5.0, 50.0, 500.0])[:nl]))
    s["two_launches"] = dict(seed=61, F=3, zint=9, chan=_chan(500.0, 8.0, 3), half=3.0, log10l=log10l_range(2400))
    s["guard_2305"] = dict(seed=62, F=2, zint=3, chan=_chan(500.0, 8.0, 2), half=3.0, log10l=log10l_range(2305))
    s["guard_2049"] = dict(seed=63, F=2, zint=3, chan=_chan(500.0, 8.0, 2), half=3.0, log10l=log10l_range(2049))
    for F in LAYOUT_F:
        s["layout_F%d" % F] = dict(seed=70 + F, F=F, zint=3, chan=_chan(300.0, 0.5, F), half=0.2,
                                   log10l=log10l_range(40))
    return s


LAYOUT_F = (1, 2, 31, 33, 40, 65, 100)
_SPECS = _specs()
CASE_NAMES = tuple(_SPECS)
PATH_CASES = tuple(n for n in CASE_NAMES if not n.startswith("layout_"))
_cache = {}


def case(name):
    if ("case", name) not in _cache:
        _cache["case", name] = make_case(**_SPECS[name])
    return _cache["case", name]


def reference_of(name):
    """(C, bound) of a named case, computed once per process and shared (read-only) by the tests that need it."""
    if ("ref", name) not in _cache:
        C, B = reference(case(name))
        C.setflags(write=False)
        B.setflags(write=False)
        _cache["ref", name] = (C, B)
    return _cache["ref", name]


def expect(name):
    """Asserts that the named case reaches the path it was written for (from paths(): the kernel's own predicates)."""
    P = paths(case(name))
    p0 = P[0]
    every = lambda k, p=p0: bool(np.all(p[k]))
    some = lambda k, p=p0: bool(np.any(p[k]))
    if name.startswith("interior_z"):
        z = case(name)["zint"]
        assert every("all_fast") and not some("clamp_low_later") and not some("clamp_high") and every("clamp_low_first")
        assert p0["zint_inst"] == (z if z in (3, 5, 9) else 0) and 1 <= p0["nsp"] <= 31 and not some("kpar_edge")
    elif name == "top_clamped":
        assert some("clamp_high") and some("xhi_top") and some("slot_read") and p0["zint_inst"] == 3
        assert not every("all_fast")                    # not fast with a compiled ZINT
        assert bool(np.any(p0["clamp_high"] & ~p0["all_fast"]))
    elif name in ("top_fast_slot", "top_fast_slot_odd"):
        assert every("fast_build") and every("xhi_top") and every("slot_read") and not some("clamp_high")
    elif name == "top_fast_below":
        assert every("fast_build") and every("xhi_top") and not some("slot_read") and p0["zint_inst"] == 9
    elif name == "low_clamp":
        assert every("clamp_low_later") and not some("all_fast")
    elif name == "kpar_edge":
        assert some("kpar_edge") and not every("kpar_edge")
    elif name == "nsp0":
        assert p0["nsp"] == 0 and every("fast_build")
    elif name == "nsp32":
        assert p0["nsp"] == 32 and every("fast_build") and p0["zint_inst"] == 5
    elif name.startswith("few_l"):
        # nsp counts the wide gaps in front of the dense part: at most n - 1.  "Every entry built individually" (nsp >=
        # n) can therefore not happen; the nearest reachable state is a dense part of ONE entry.
        assert not p0["every_individual"] and p0["n"] == case(name)["log10l"].size
        if name.startswith("few_l5"):
            assert every("fast_build") and p0["nsp"] == p0["n"] - 1
        elif p0["n"] == 1:
            assert not some("all_fast") and p0["nsp"] == 0
        else:
            assert every("fast_build") and p0["nsp"] == min(p0["n"] - 1, 2)
    elif name == "two_launches":
        assert len(P) == 2 and P[1]["l_base"] == L_LAUNCH and P[1]["n"] == 96 and P[1]["nsp"] == 0
        assert every("fast_build") and every("fast_build", P[1]) and not some("clamp_low_first", P[1])
    elif name == "guard_2305":
        assert len(P) == 2 and P[1]["n"] == 1 and every("fast_build", P[1])
    elif name == "guard_2049":
        assert len(P) == 1 and p0["n"] == 2049 == 8 * 256 + 1 and every("fast_build")
    else:
        assert name.startswith("layout_F")
    return P
