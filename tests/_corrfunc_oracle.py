"""Host oracle of the xi(r) -> C_l kernels (cora_amd/csrc/corrfunc.hip): plain, slow restatements of
``corahip_xi_table_average`` and ``corahip_legendre_project`` in ``numpy.longdouble`` (64-bit mantissa, asserted
below), each returning the value AND a first-order bound on what the device may differ by.  CPU only.

Notation: eps = 2^-52 is the spacing of doubles at 1, so that ONE ROUNDING commits a relative error of at most eps / 2
(the unit roundoff u = 2^-53, which is what gamma_n = n u / (1 - n u) is made of); ulp(.) the spacing of doubles.  No
constant below was fitted to device output; tests/test_gpu_corrfunc.py prints and records the observed err / bound
next to them.  (A first version of this module charged u / 2 per rounding, half of what a rounding costs; the
Legendre matrix showed it at l = 1, where wt * mu is a single rounding and the device came out at 1.89 of that
bound.  Every count below was kept and the unit corrected.)

Separation.  r = sqrt(fma(d, d, ((2 x1) x2) (1 - mu))), d = x1 - x2, is restated in double bit for bit (the fma through
libm).  The oracle evaluates at that double; a device sqrt that rounds the other way moves r by one ulp, which the
bound carries as |dv/dr| ulp(r).  Where x1 x2 (1 - mu) = 0 the radicand is fl(d^2) and an IEEE sqrt returns |d|
itself: no such term (this is what makes xa[0] = 0 an exact handle on r).

Abscissa x(r), |x_dev - x| <= e_x:
  kind 0  x = r                      e_x = 0
  kind 1  x = log r  (fast_log01)    e_x = eps (0.75 + |x|)
          r = 2^e m, c = rint(64 m) / 64, t = fma(m, fl(1/c), -1) (|t| <= 0.0111: rounding <= 0.011 eps), table entry
          -ln fl(1/c) (|.| <= 0.35: half an ulp = eps / 4), degree-8 log1p (stated remainder 3e-17 |t| = 0.004 eps, Horner
          rounding < 0.02 eps), sum with the table entry (eps / 4), final fma e ln2 + (.) (eps / 2 |x|), the double ln2
          (relative error 0.3 eps on |e ln2| <= |x| + 0.35): 0.011 + 0.25 + 0.024 + 0.25 + 0.105 < 0.75, 0.5 + 0.3 < 1.
  kind 2  x = asinh(q), q = r / x_t  (fast_asinh_pos on the double r * fl(1 / x_t): relative error eps in q, which moves
          asinh by at most eps min(q, 1) <= eps |x| (small branch) or eps (big branch))
          q < 2^-6: odd series to q^9, remainder 0.0224 q^10 < 2^-65 relative; q^2, the Horner steps (each scaled by
                    q^2 <= 2^-12) and the final product: 1.5 eps relative             e_x = 2.5 eps |x|
          else    : w = q + sqrt(q^2 + 1): q^2 and + 1 (eps / 2 each, halved by the root), fast_sqrt_pos (rsq seed, two
                    Goldschmidt steps, one residual correction: one ulp <= 2 eps, scale-free, so for every normal
                    argument), the sum (eps / 2): 3 eps relative in w = 3 eps absolute in log w; fast_log01 as above
                    (0.75 + |x|) eps; the input eps                                      e_x = eps (5 + |x|)
          within 4 ulp of the switch the larger of the two.

Spline S at x (natural cubic, end-slope extrapolation, cubicspline.pyx:126-175), |S_dev(x) - S(x)| <= e_S:
  interior, a = (x_{k+1} - x) / h, b = (x - x_k) / h, H = h^2 / 6.  The device has a, b with relative error 2 eps
  (difference, fl(1 / fl(h)), product), H with 2 eps.  Linear part: 2.5 eps per product, eps for the sums.  Cubic part:
  delta(c^3 - c) <= |3 c^2 - 1| 2 eps c + eps c^3 + eps / 2 |c^3 - c|, then y2 (eps / 2), the sum (eps / 2), H (2.5 eps), the final
  sum (eps / 2):
      e_S = eps { 4 (|a y_k| + |b y_{k+1}|) + [g(a) |y2_k| + g(b) |y2_{k+1}|] H },  g(c) = 2 c |3 c^2 - 1| + c^3 + 5 |c^3 - c|
  This corrects the form e_S = c_S eps (... + |(c^3 - c) y2 H|) the work started from: that term vanishes at a knot
  (c = 1), where c^3 - c is a difference of two numbers of size 1 whose error 4 eps does not vanish.
  outside, S = (D -+ h y2 / 6)(x - x_end) + y_end with D = dy / h: 4 roundings on each slope term, 1.5 on the product,
  eps / 2 on the sum:   e_S = eps { 4 (|D| + |h y2 / 6|) |x - x_end| + |y_end| }
  x = -inf (kind 1 at r = 0): the double formula itself, 0 / inf / nan, compared for identity.
  |S'| in the bound is the slope at x and, where x lies within 2 (e_x + |dx/dr| ulp r) of a knot, also the one-sided
  slopes at that knot (equal for a C2 table; the tests also pass y'' tables that are not).

Value:  |v_dev - v| <= |dv/dy| (|S'| e_x + e_S) + d_out |v| + |dv/dr| ulp(r)
  kind 0  v = S                     d_out = 0
  kind 1  v = exp(y) (fast_exp)     d_out = 2.5 eps; a subnormal v instead to one smallest normal, absolutely
          t = |y| - k ln2: the hi product and difference are exact (ln2_hi has 21 trailing zero bits, k < 2^11),
          the lo term and the rounding of t 0.18 eps absolutely; degree-13 expm1 (stated remainder 4e-18 = 0.04 eps),
          Horner 0.07 eps, its last fma 0.2 eps: p = expm1(t) to 0.6 eps absolutely, (1 + p) >= 0.707: 0.85 eps relative in
          2^k (1 + p); fma eps / 2, + 1 eps / 2, the reciprocal for y < 0 eps / 2: 2.35 eps.  |y| >= 700: the library exp, one ulp.
  kind 2  v = f_t sinh(y) (fast_sinh)  d_out = 5 eps
          E = expm1|y| = 2^k p + (2^k - 1): 0.6 eps 2^k + eps / 2 |E| absolutely; for k >= 1 E >= 0.414 and 2^k / E <= 4.83:
          3.4 eps relative (k = 0: E = p to 0.7 eps).  (E + E / (E + 1)) / 2 has relative condition <= 1 in E; E + 1 and the
          quotient touch only the smaller term (eps / 4 each), the sum eps / 2, f_t eps / 2: 3.4 + 0.25 + 0.25 + 0.5 + 0.5 < 5.

Bin average (xint > 1): sum_ab |xw_a xw_b| bound_ab + gamma_{2 xint} sum_ab |xw_a xw_b v_ab| (two products and at most
2 xint - 2 inexact additions per term, in units of u).

Legendre matrix lm[l, m] = wt_m P_l(mu_m) by p_l = ((2l-1) x p_{l-1} - (l-1) p_{l-2}) / l in double.  Step k commits a
local error |rho_k| <= 2 eps (|(2k-1) x P_{k-1}| + |(k-1) P_{k-2}|) / k (two roundings on the first product, one on the
second, the difference, the quotient).  A perturbation at step k obeys the same recurrence from (0, 1) at (k-1, k),
so it reaches degree l as rho_k G(l, k), G(l, k) = k (Q_{k-1} P_l - P_{k-1} Q_l) with Q the second solution
(Q_0 = atanh x, Q_1 = x Q_0 - 1) and k (P_k Q_{k-1} - P_{k-1} Q_k) = 1 the Wronskian.  Hence, to first order,
      E_l(x) = |P_l| sum_{k<=l} rho_k k |Q_{k-1}| + |Q_l| sum_{k<=l} rho_k k |P_{k-1}|
At x = +-1 every operation of the recurrence is exact in double (the numerator is +-l): E_l = 0.
      |lm_dev - lm| <= |wt| (E_l + eps / 2 |P_l|)

Projection out[l, c] = sum_m lm[l, m] xi[m, c] on K padded to Kp = 16 ceil(nm / 16):
      gamma_{Kp+2} sum_m |lm[l, m] xi[m, c]| + sum_m |wt_m xi[m, c]| E_l(mu_m)   (+ sum_m |lm[l, m]| bound_xi[m, c])
"""
import ctypes
import ctypes.util

import numpy as np

LD = np.longdouble
assert np.finfo(LD).eps < 2e-19, "the oracle needs an extended-precision numpy.longdouble"

U = 2.0**-53                 # unit roundoff (gamma_n)
EPS = 2.0**-52               # spacing at 1: the unit of every derived constant of the docstring
TINY = float(np.finfo(np.float64).tiny)
LDS_PER_KNOT = 56            # bytes of LDS per knot in xi_table_kernel (5 doubles + 4 look-up cells)
LUT_PER_KNOT = 4
ASINH_SWITCH = 2.0**-6
GEMM_K = 16

_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.fma.restype = ctypes.c_double
_libm.fma.argtypes = [ctypes.c_double] * 3


def gamma(n):
    return n * U / (1.0 - n * U)


def fma(a, b, c):
    """Correctly rounded a * b + c on double arrays: in longdouble (two roundings at 2^-64) wherever that decides the
    rounding to double, through libm where the longdouble result lies within 2^-8 ulp of a tie."""
    a, b, c = np.broadcast_arrays(np.asarray(a, np.float64), np.asarray(b, np.float64), np.asarray(c, np.float64))
    with np.errstate(all="ignore"):
        z = a.astype(LD) * b.astype(LD) + c.astype(LD)
        out = np.asarray(z.astype(np.float64))
        sp = np.spacing(np.abs(out))
        need = ~(np.abs(np.abs(z - out) - 0.5 * sp) > sp * 2.0**-8) | ~(np.abs(out) > 1e-290)
        need &= np.isfinite(out) & (z != 0)
    if need.any():
        f = _libm.fma
        out[need] = [f(x, y, z) for x, y, z in zip(a[need].tolist(), b[need].tolist(), c[need].tolist())]
    return out


def radius(x1, x2, om):
    """The kernel's r in double, bit for bit, and whether it is free of the sqrt's rounding."""
    x1, x2, om = np.broadcast_arrays(np.asarray(x1, np.float64), np.asarray(x2, np.float64), np.asarray(om, np.float64))
    d = x1 - x2
    t = 2.0 * x1 * x2 * om
    return np.sqrt(fma(d, d, t)), t == 0.0


# ------------------------------------------------------------------ spline
def _knot_slopes(xs, ys, y2):
    """max of the one-sided |slopes| at every knot (extrapolation slopes at the two ends)."""
    h = np.diff(xs)
    D = np.diff(ys) / h
    right = D - h * (2 * y2[:-1] + y2[1:]) / 6          # at knot k from interval k
    left = D + h * (y2[:-1] + 2 * y2[1:]) / 6           # at knot k + 1 from interval k
    lo = D[0] - h[0] * y2[1] / 6
    hi = D[-1] + h[-1] * y2[-2] / 6
    r = np.concatenate([right, [hi]])
    l = np.concatenate([[lo], left])
    return np.maximum(np.abs(r), np.abs(l))


def spline(xs, ys, y2, x, tol=0.0):
    """S(x), the |S'| of the bound, e_S; x longdouble (finite, or -inf: handled by the caller)."""
    xs, ys, y2 = (np.asarray(v, np.float64).astype(LD) for v in (xs, ys, y2))
    n = xs.size
    x = np.asarray(x, LD)
    tol = np.broadcast_to(np.asarray(tol, np.float64), x.shape)
    S = np.empty(x.shape, LD)
    dS = np.empty(x.shape, LD)
    eS = np.empty(x.shape, LD)
    lo = x < xs[0]
    hi = x >= xs[n - 1]
    mid = ~(lo | hi)
    for sel, e, e1, sgn, j2 in ((lo, 0, 1, -1.0, 1), (hi, n - 1, n - 2, 1.0, n - 2)):
        if sel.any():
            h = abs(xs[e1] - xs[e])
            D = (ys[n - 1] - ys[n - 2]) / h if e else (ys[1] - ys[0]) / h
            c2 = h * y2[j2] / 6
            sl = D + sgn * c2
            dx = x[sel] - xs[e]
            S[sel] = sl * dx + ys[e]
            dS[sel] = abs(sl)
            eS[sel] = EPS * (4 * (abs(D) + abs(c2)) * np.abs(dx) + abs(ys[e]))
    k = np.clip(np.searchsorted(xs, x[mid], side="right") - 1, 0, n - 2)      # last knot with xs[k] <= x
    xm = x[mid]
    h = xs[k + 1] - xs[k]
    a = (xs[k + 1] - xm) / h
    b = (xm - xs[k]) / h
    H = h * h / 6
    S[mid] = a * ys[k] + b * ys[k + 1] + ((a * a * a - a) * y2[k] + (b * b * b - b) * y2[k + 1]) * H
    # (slopes and bounds need no extended precision)
    a, b, h, H = (v.astype(np.float64) for v in (a, b, h, H))
    yk, yk1, zk, zk1 = (v.astype(np.float64)[kk] for v in (ys, y2) for kk in (k, k + 1))
    dS[mid] = np.abs((yk1 - yk) / h + (-(3 * a * a - 1) * zk + (3 * b * b - 1) * zk1) * h / 6)

    def g(c):
        c3 = c * c * c
        return 2 * c * np.abs(3 * c * c - 1) + c3 + 5 * np.abs(c3 - c)

    eS[mid] = EPS * (4 * (np.abs(a * yk) + np.abs(b * yk1)) + (g(a) * np.abs(zk) + g(b) * np.abs(zk1)) * H)
    # one-sided slopes of a knot within tol
    ks = _knot_slopes(xs, ys, y2)
    j = np.clip(np.searchsorted(xs, x, side="right") - 1, 0, n - 1)
    j = np.where((j + 1 < n) & (np.abs(xs[np.minimum(j + 1, n - 1)] - x) < np.abs(x - xs[j])), j + 1, j)
    near = np.abs(x - xs[j]) <= tol
    dS = np.where(near, np.maximum(dS, ks[j]), dS)
    return S, dS, eS


def spline_double_formula(xs, ys, y2, x):
    """The reference formula in double (what a non-finite abscissa is compared with)."""
    xs, ys, y2 = (np.asarray(v, np.float64) for v in (xs, ys, y2))
    x = np.asarray(x, np.float64)
    with np.errstate(all="ignore"):
        h0 = xs[1] - xs[0]
        below = ((ys[1] - ys[0]) / h0 - h0 * y2[1] / 6.0) * (x - xs[0]) + ys[0]
        h1 = xs[-1] - xs[-2]
        above = ((ys[-1] - ys[-2]) / h1 + h1 * y2[-2] / 6.0) * (x - xs[-1]) + ys[-1]
    return np.where(x < xs[0], below, above)


# ------------------------------------------------------------------ xi(r)
def abscissa(kind, r, x_t):
    """x(r) in longdouble, e_x, |dx/dr| for double r >= 0."""
    r = np.asarray(r, np.float64)
    rl = r.astype(LD)
    with np.errstate(divide="ignore", invalid="ignore"):
        if kind == 0:
            return rl, np.zeros(r.shape), np.ones(r.shape, LD)
        if kind == 1:
            x = np.log(rl)
            return x, EPS * (0.75 + np.abs(x)).astype(np.float64), 1 / rl
        q = rl / LD(x_t)
        x = np.arcsinh(q)
        qd = r * (1.0 / x_t)
        small = EPS * 2.5 * np.abs(x)
        big = EPS * (5 + np.abs(x))
        near = np.abs(qd - ASINH_SWITCH) <= 4 * np.spacing(ASINH_SWITCH)
        ex = np.where(near, np.maximum(small, big), np.where(qd < ASINH_SWITCH, small, big))
        return x, ex.astype(np.float64), 1 / (abs(LD(x_t)) * np.sqrt(1 + q * q))


def xi_points(kind, xs, ys, y2, x_t, f_t, r, r_exact=False):
    """xi at the double separations r -> (value longdouble, bound float64).  A zero bound asks for identity
    (non-finite abscissa)."""
    r = np.asarray(r, np.float64)
    x, ex, dxdr = abscissa(kind, r, x_t)
    ur = np.where(np.broadcast_to(r_exact, r.shape), 0.0, np.spacing(r))
    fin = np.isfinite(x)
    xf = np.where(fin, x, LD(xs[0]))
    exf = np.where(fin, ex, 0.0)
    dxf = np.where(fin, dxdr, LD(0))
    S, dS, eS = spline(xs, ys, y2, xf, 2 * (exf + (dxf * ur).astype(np.float64)))
    with np.errstate(all="ignore"):
        if kind == 0:
            v, dvdy, dout = S, LD(1), 0.0
        elif kind == 1:
            v = np.exp(S)
            dvdy, dout = v, 2.5 * EPS
        else:
            v = LD(f_t) * np.sinh(S)
            dvdy, dout = abs(LD(f_t)) * np.cosh(S), 5 * EPS
        bound = dvdy * (dS * exf + eS) + dout * np.abs(v) + dvdy * dS * dxf * ur
        if kind == 1:
            bound = np.where(v < TINY, bound + TINY, bound)
        if not fin.all():
            yd = spline_double_formula(xs, ys, y2, np.where(fin, 0.0, x.astype(np.float64)))
            vd = np.exp(yd) if kind == 1 else (f_t * np.sinh(yd) if kind == 2 else yd)
            v = np.where(fin, v, vd.astype(LD))
            bound = np.where(fin, bound, 0.0)
    return v, np.asarray(bound, np.float64)


def xi_table_average(kind, xs, ys, y2, x_t, f_t, mu, xa, xw, F, xint):
    """corahip_xi_table_average -> (value [nm, F, F] longdouble, bound float64)."""
    mu, xa, xw = (np.asarray(v, np.float64) for v in (mu, xa, xw))
    om = 1.0 - mu
    nm, P = mu.size, xa.size
    iu, ju = np.triu_indices(P)                      # r is symmetric in (x1, x2) bit for bit
    v = np.empty((nm, P, P), LD)
    b = np.empty((nm, P, P))
    step = max(1, 200000 // iu.size)
    for m0 in range(0, nm, step):
        sl = slice(m0, m0 + step)
        r, exact = radius(xa[iu][None, :], xa[ju][None, :], om[sl, None])
        vc, bc = xi_points(kind, xs, ys, y2, x_t, f_t, r, exact)
        v[sl, iu, ju], b[sl, iu, ju] = vc, bc
        v[sl, ju, iu], b[sl, ju, iu] = vc, bc
    if xint == 1 and xw[0] == 1.0:
        return v, b
    w2 = np.abs(xw[:, None] * xw[None, :])
    v = v.reshape(nm, F, xint, F, xint)
    b = b.reshape(nm, F, xint, F, xint)
    with np.errstate(invalid="ignore"):
        val = np.einsum("miajb,a,b->mij", v, xw.astype(LD), xw.astype(LD))
        bound = np.einsum("miajb,ab->mij", b, w2) + gamma(2 * xint) * np.einsum("miajb,ab->mij", np.abs(v), w2.astype(LD))
    return val, np.asarray(bound, np.float64)


# ------------------------------------------------------------------ Legendre
def legendre(mu, lmax):
    """P_l(mu) [lmax+1, nm] in longdouble and E_l(mu), the first-order error of the double recurrence."""
    x = np.asarray(mu, np.float64).astype(LD)
    L = lmax + 1
    P = np.empty((L, x.size), LD)
    Q = np.zeros((L, x.size), LD)
    inner = np.abs(x) < 1
    P[0] = 1
    with np.errstate(divide="ignore"):
        Q[0] = np.where(inner, np.arctanh(np.where(inner, x, 0)), 0)
    if lmax >= 1:
        P[1] = x
        Q[1] = x * Q[0] - 1
    for l in range(2, L):
        P[l] = ((2 * l - 1) * x * P[l - 1] - (l - 1) * P[l - 2]) / l
        Q[l] = ((2 * l - 1) * x * Q[l - 1] - (l - 1) * Q[l - 2]) / l
    E = np.zeros((L, x.size), LD)
    if lmax >= 2:
        k = np.arange(2, L).astype(LD)[:, None]
        rho_k = 2 * EPS * (np.abs((2 * k - 1) * x * P[1:-1]) + np.abs((k - 1) * P[:-2]))     # rho_k * k
        E[2:] = np.abs(P[2:]) * np.cumsum(rho_k * np.abs(Q[1:-1]), axis=0) + np.abs(Q[2:]) * np.cumsum(rho_k * np.abs(P[1:-1]), axis=0)
        E[:, ~inner] = 0
    return P, E


def legendre_matrix(mu, wt, lmax):
    """lm[l, m] = wt_m P_l(mu_m) (longdouble) and the bound on the device's matrix."""
    P, E = legendre(mu, lmax)
    w = np.asarray(wt, np.float64).astype(LD)
    return w * P, np.asarray(np.abs(w) * (E + 0.5 * EPS * np.abs(P)), np.float64)


def legendre_project(mu, wt, lmax, xi, xi_bound=None):
    """corahip_legendre_project -> (out [lmax+1, ncol] longdouble, bound float64)."""
    P, E = legendre(mu, lmax)
    w = np.asarray(wt, np.float64).astype(LD)
    nm = w.size
    xi = np.asarray(xi, np.float64).reshape(nm, -1).astype(LD)
    lm = w * P
    Kp = (nm + GEMM_K - 1) // GEMM_K * GEMM_K
    axi = np.abs(xi).astype(np.float64)             # (the bounds themselves need no extended precision)
    alm = np.abs(lm).astype(np.float64)
    out = lm @ xi
    bound = gamma(Kp + 2) * (alm @ axi) + (np.abs(w) * E).astype(np.float64) @ axi
    if xi_bound is not None:
        bound = bound + alm @ np.asarray(xi_bound, np.float64).reshape(nm, -1)
    return out, bound


def worst_ratio(dev, val, bound):
    """max |dev - val| / bound; where the oracle value is not finite or the bound is zero the device must return the
    same thing (inf for a miss)."""
    dev = np.asarray(dev, np.float64)
    val = np.asarray(val, LD)
    bound = np.broadcast_to(np.asarray(bound, np.float64), dev.shape)
    with np.errstate(all="ignore"):
        vd = val.astype(np.float64)
        same = (dev == vd) | (np.isnan(dev) & np.isnan(vd))
        ident = ~np.isfinite(val) | ~(bound > 0) | ~np.isfinite(bound)
        ratio = np.abs(dev.astype(LD) - val) / np.where(ident, 1, bound)
        ratio = np.where(ident, np.where(same, 0.0, np.inf), np.where(np.isfinite(dev), ratio, np.inf))
    return float(np.max(ratio)) if ratio.size else 0.0


# ------------------------------------------------------------------ tables and point sets shared by the host and GPU tests
def xi_model(r):
    r = np.asarray(r, dtype=np.float64)
    return np.exp(-r / 60.0) * np.cos(r / 35.0) / (1.0 + (r / 15.0) ** 2)


X_T, F_T = 1.0, 1e-4          # the sinh interpolater's thresholds in every table below


def to_x(kind, r):
    r = np.asarray(r, np.float64)
    return r if kind == 0 else (np.log(r) if kind == 1 else np.arcsinh(r / X_T))


def to_r(kind, x):
    x = np.asarray(x, np.float64)
    with np.errstate(over="ignore"):
        return x if kind == 0 else (np.exp(x) if kind == 1 else X_T * np.sinh(x))


def natural_y2(xs, ys):
    from cora_amd.util import cubicspline as cs

    return cs.Interpolater(np.stack([xs, ys], axis=1))._y2.copy()


LAYOUTS = ("nk4", "uniform64", "log300", "mirror300", "close")


def table(kind, layout, nk=None):
    """(xs, ys, y2) in the spline's own space.  The knots are laid out in r for kind 0 and, with the same shapes, in x
    for kinds 1 and 2 (the kernel sees only x)."""
    lo, hi = ((0.0, 1.0e4), (np.log(0.05), np.log(2.0e4)), (0.0, np.arcsinh(2.0e4 / X_T)))[kind]
    span = hi - lo
    lg = np.concatenate([[0.0], np.logspace(-1, 3.7, 300)]) / 10.0**3.7
    if layout == "nk4":
        xs = lo + span * np.array([0.1, 0.3, 0.45, 0.9])
    elif layout == "uniform64":
        xs = lo + span * np.arange(64) / 63.0
    elif layout == "log300":
        xs = lo + span * lg
    elif layout == "mirror300":
        xs = lo + span * (1.0 - lg[::-1])
    elif layout == "close":
        xs = lo + span * np.arange(31) / 30.0
        xs[15] = xs[14] + 2.0**-40 * (1.0 if kind == 0 else span / 1e4 * 1024)
    elif layout == "max":
        xs = lo + span * np.arange(nk) / (nk - 1.0)
    else:
        raise ValueError(layout)
    assert np.all(np.diff(xs) > 0)
    r = to_r(kind, xs)
    f = xi_model(r) if kind != 1 else np.exp(-r / 80.0) + 1e-3
    ys = f if kind == 0 else (np.log(f) if kind == 1 else np.arcsinh(f / F_T))
    return xs, ys, natural_y2(xs, ys)


def kinked_table():
    """kind 0, 64 uniform knots, constant y and a y'' that is NOT the spline's: the right-hand slope at every knot
    k = 1 mod 3 is zero and the left-hand one h Y / 3, so that the interval chosen just right of a knot shows."""
    xs = 100.0 * np.arange(64)
    y2 = np.tile([0.0, 1.0, -2.0], 22)[:64] * 3.0e-2
    return xs, np.ones(64), y2


def neighbours(v, n=1):
    v = np.atleast_1d(np.asarray(v, np.float64))
    out = [v]
    up, dn = v, v
    for _ in range(n):
        up, dn = np.nextafter(up, np.inf), np.nextafter(dn, -np.inf)
        out += [up, dn]
    return np.concatenate(out)


Q_POINTS = (2.0**-30, 2.0**-7, 2.0**-5, 0.1, 1.0, 2.0**10, 1e8)       # u = r / x_t (2^-5 and 0.1: between the
#                                                                         switch and 2^-3, where a moved switch shows)


def spline_points(kind, xs, stride=1, ends=32):
    """Separations r >= 0 (r[0] = 0) that put x(r) on every knot and look-up-cell edge and one ulp (of r) either side,
    outside the table on both sides, and on the asinh switch; `stride` thins the knots and edges of a large table
    except the first and last `ends` of each."""
    n = xs.size
    nlut = LUT_PER_KNOT * n
    dx = (xs[-1] - xs[0]) / nlut
    edges = xs[0] + np.arange(nlut + 1) * dx

    def thin(v):
        keep = np.zeros(v.size, bool)
        keep[::stride] = True
        keep[:ends] = True
        keep[-ends:] = True
        return v[keep]

    pts = [neighbours(to_r(kind, thin(xs)), 1 if kind == 0 else 2), neighbours(to_r(kind, thin(edges)), 1 if kind == 0 else 2)]
    r0, r1 = to_r(kind, xs[0]), to_r(kind, xs[-1])
    pts.append(np.array([0.5 * r0, 0.9 * r0, r1 * 1.01, r1 * 1.5, r1 * 4.0]))
    pts.append(neighbours(X_T * ASINH_SWITCH))
    pts.append(X_T * np.array(Q_POINTS))
    r = np.unique(np.concatenate(pts))
    r = r[np.isfinite(r) & (r > 0)]
    return np.concatenate([[0.0], r])


Y_TARGETS = (1e-300, 2.0**-30, np.nextafter(0.5 * np.log(2.0), 0), 0.5 * np.log(2.0), np.nextafter(0.5 * np.log(2.0), 1),
             1.0, 40.0, 690.0, 699.9, 700.0, 705.0, 708.0)
Y_LOG_TAIL = (-700.5, -705.0, -708.39, -708.4, -710.0, -730.0, -744.0)


def plateau_table(kind):
    """Piecewise-linear table (y'' = 0) holding every target y on three consecutive knots, so that S = y exactly and
    S' = 0 around the middle one: (xs, ys, y2, r) with r[0] = 0 and r[1 + t] on the middle knot of target t."""
    ys = [s * y for y in Y_TARGETS for s in (1.0, -1.0)] + (list(Y_LOG_TAIL) if kind == 1 else [])
    lo, hi = ((1.0, 1.0e3), (np.log(0.5), np.log(2.0e3)), (np.arcsinh(1.0), np.arcsinh(2.0e3)))[kind]
    xs = lo + (hi - lo) * np.arange(3 * len(ys)) / (3 * len(ys) - 1.0)
    r = to_r(kind, xs[1::3])
    return xs, np.repeat(np.array(ys), 3), np.zeros(xs.size), np.concatenate([[0.0], r])


def interpolater(kind, xs, ys, y2):
    from cora_amd.util import cubicspline as cs

    cls = (cs.Interpolater, cs.LogInterpolater, cs.SinhInterpolater)[kind]
    obj = cls.__new__(cls)
    obj._data = np.stack([xs, ys], axis=1)
    obj._y2 = np.asarray(y2, np.float64).copy()
    obj.x_t, obj.f_t = X_T, F_T
    return obj


def spline_cases(kind, nk_max=2925):
    """(name, xs, ys, y2, r) of every table and its point set; nk_max: the largest table the device takes."""
    for layout in LAYOUTS:
        xs, ys, y2 = table(kind, layout)
        yield layout, xs, ys, y2, spline_points(kind, xs)
    xs, ys, y2 = table(kind, "max", nk_max)
    yield "max", xs, ys, y2, spline_points(kind, xs, stride=16)
    xs, ys, y2, r = plateau_table(kind)
    yield "plateau", xs, ys, y2, r
    if kind == 0:
        xs, ys, y2 = kinked_table()
        yield "kinked", xs, ys, y2, spline_points(kind, xs)
    if kind == 1:
        xs = np.log([1.0, 2.0, 3.0, 4.0])
        yield "zero_slope", xs, np.full(4, 0.25), np.zeros(4), np.array([0.0, 0.5, 1.0, 2.5, 4.0, 9.0])


def bin_average_case(kind, F, xint):
    """Distances, unnormalised asymmetric weights and two mu nodes for a radial-bin average over a uniform64 table."""
    rng = np.random.default_rng(100 * F + xint)
    xa = np.sort(rng.uniform(50.0, 3000.0, F * xint))
    xw = rng.uniform(0.2, 1.7, xint) * np.where(np.arange(xint) % 3 == 1, -1.0, 1.0)
    return np.array([1.0, 0.2, -0.7]), xa, xw


def projection_case(L, ncol, nm):
    """mu, wt and an xi of mixed signs whose columns span 1e-100 .. 1e100."""
    rng = np.random.default_rng(L * 1000003 + ncol * 1009 + nm)
    mu = np.sort(rng.uniform(-1.0, 1.0, nm))
    wt = rng.uniform(0.5, 2.0, nm)
    xi = rng.standard_normal((nm, ncol)) * 10.0 ** rng.uniform(-100, 100, ncol)
    return mu, wt, xi


_E2E = {}


def end_to_end_case(kind):
    """lmax 300, 20 distances, xromb 2 -> (lmax, xarray, C_l [lmax+1, F F] longdouble, bound, interpolater)."""
    if kind not in _E2E:
        import scipy.special as ss

        from oracle import corrfunc as ocf

        lmax = 300
        xa = 1400.0 + 12.5 * np.arange(20) + 3.0 * np.sin(np.arange(20))
        xs, ys, y2 = table(kind, "log300")
        mu, w, wsum = ss.roots_legendre(2 * lmax, mu=True)
        pts, xw, xint = ocf.radial_nodes(xa, 2)
        xi, xb = xi_table_average(kind, xs, ys, y2, X_T, F_T, mu, pts, xw, 20, xint)
        ref, bound = legendre_project(mu, w * 4.0 * np.pi / wsum, lmax, xi.reshape(mu.size, -1), xb.reshape(mu.size, -1))
        _E2E[kind] = (lmax, xa, ref, bound, interpolater(kind, xs, ys, y2))
    return _E2E[kind]
