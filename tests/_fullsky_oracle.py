"""Oracle of the exact curved-sky C_l (csrc/fullsky.hip), numpy only:

  jl_table_ld     j_l(x) for l = 0 .. lmax + 1 in np.longdouble: one downward recurrence over the whole l range, started
                  high enough that its truncation is below 1e-25, normalised to the larger of j_0 and j_1 (below order
                  8192 the recurrence recovers its own rounding errors);
  jl_d2_ld        j_l'' = (l (l - 1) / x^2 - 1) j_l + (2 / x) j_{l+1} from that table (-1/3, 2/15 at x = 0);
  jl_scheme_f64   the scheme the kernel is specified by, restated in float64 numpy from its description: upward while
                  l <= x, Miller from top + ceil(sqrt(160 top)) + 30 above, normalised next to floor(x);
  radial_cases / case_tables / radial_table_ld (table and bound), gram_ld / gram_bound / gram_table_bound, fullsky_grid,
  trapezoid_g.

The abscissa is always the float64 product k * chi, as the kernel forms it.

TOL_J, TOL_D2: the tolerance of the device table, in units of the envelope E(x) = 1 / max(x, 1).  They are 8 x the worst
err / E of jl_scheme_f64 against the longdouble table on the cases of radial_cases() (measure_scheme()); the factor is for
the device's sin / cos and fused multiply-adds, whose last bits differ and which a three-term recurrence adds up.
"""
import functools
import math

import numpy as np

LD = np.longdouble
assert np.finfo(LD).eps < 2e-19, "the oracle needs an extended-precision long double"
U = 2.0 ** -53

# measure_scheme() on this file's cases: worst err / E = 8.79e-13 for j_l (x = 3060.29 at l = 3060: three thousand upward
# steps end at the turning point) and 4.81e-14 for j_l'' (both in the lmax = 3071 case; 3.1e-14 and 4.8e-15 at lmax = 200)
TOL_J = 8 * 8.79e-13
TOL_D2 = 8 * 4.81e-14
assert TOL_J < 1e-11 and TOL_D2 < 1e-11


# jl_table_ld recovers the rounding errors of its recurrence below this order (three roundings a step, over the three
# thousand steps to a turning point at 3071, otherwise leave 0.5 - 1.5e-17 E: the random walk of the long double's own
# rounding).  Above it the plain step runs: an abscissa of 3.3e5 then keeps 3e-17 E, five orders below any tolerance here.
COMPENSATE_BELOW = 8192
_SPLIT = LD(2.0 ** 32 + 1.0)


def envelope(x):
    return 1.0 / np.maximum(np.asarray(x, dtype=np.float64), 1.0)


def jl_table_ld(lmax, x):
    """j_l(x), l = 0 .. lmax + 1, longdouble [lmax + 2, nx], for float64 abscissae x >= 0."""
    x = np.atleast_1d(np.asarray(x, dtype=np.float64)).astype(LD)
    top = lmax + 1
    nx = x.size
    T = np.zeros((top + 1, nx), dtype=LD)
    pos = x > 0
    T[0, ~pos] = 1.0
    if not pos.any():
        return T
    M = np.maximum(x, LD(top))
    start = np.where(pos, np.ceil(M + np.sqrt(400 * M) + 100), 0).astype(np.int64)
    order = np.argsort(-start, kind="stable")           # active abscissae are a prefix of this order
    xs, ss = x[order], start[order]
    npos = int(pos.sum())
    ix = np.zeros(nx, dtype=LD)
    ix[:npos] = 1 / xs[:npos]
    y0 = np.zeros(nx, dtype=LD)                          # order l
    y1 = np.zeros(nx, dtype=LD)                          # order l + 1
    d0 = np.zeros(nx, dtype=LD)                          # what the rounding so far has taken from y0, y1 (first order)
    d1 = np.zeros(nx, dtype=LD)
    xf = xs.astype(np.float64)
    gx = xf * (2.0 ** 27 + 1.0)
    xh = gx - (gx - xf)                                  # x = xh + xt, 27 + 26 bits: products with 32-bit halves are exact
    xt, xh = (xf - xh).astype(LD), xh.astype(LD)
    Ts = np.zeros((top + 1, nx), dtype=LD)
    big, small = LD("1e2000"), LD("1e-2000")
    na = 0
    for l in range(int(ss[0]), 0, -1):
        while na < npos and ss[na] >= l:
            y0[na] = 1.0
            na += 1
        a = slice(0, na)
        if l <= top:
            Ts[l, a] = y0[a] + d0[a]
        n = LD(2 * l + 1)
        if l > COMPENSATE_BELOW:
            t = n * y0[a] / xs[a] - y1[a]                # (a division: 1 / x rounded once would shift every abscissa)
            dn = d0[a]
        else:
            # the same step with its three rounding errors recovered (Dekker's splitting): ep of the product n y0,
            # eq of the quotient by x, es of the difference; they enter the recurrence of the correction d
            ya, yb, xa = y0[a], y1[a], xs[a]
            g = ya * _SPLIT
            h = g - (g - ya)
            A, B = n * h, n * (ya - h)
            pr = A + B
            ep = B - (pr - A)
            q = pr / xa
            g = q * _SPLIT
            qh = g - (g - q)
            qt = q - qh
            r = (((pr - qh * xh[a]) - qh * xt[a]) - qt * xh[a]) - qt * xt[a]
            eq = (r + ep) / xa
            t = q - yb
            bb = t - q
            es = (q - (t - bb)) + (-yb - bb)
            dn = n * d0[a] / xa - d1[a] + eq + es
        y1[a] = y0[a]
        y0[a] = t
        d1[a] = d0[a]
        d0[a] = dn
        over = np.abs(t) > big
        if over.any():
            idx = np.nonzero(over)[0]
            for v in (y0, y1, d0, d1):
                v[idx] *= small
            if l <= top:
                Ts[l:, idx] *= small
    Ts[0, :npos] = y0[:npos] + d0[:npos]
    s, c = np.sin(xs[:npos]), np.cos(xs[:npos])
    j0 = s * ix[:npos]
    j1 = (j0 - c) * ix[:npos]
    use0 = np.abs(j0) >= np.abs(j1)
    with np.errstate(divide="ignore", invalid="ignore"):
        scale = np.where(use0, j0 / Ts[0, :npos], j1 / Ts[1, :npos])
    T[:, order[:npos]] = Ts[:, :npos] * scale
    return T


def jl_d2_ld(T, x):
    """j_l'', l = 0 .. lmax, from the table of jl_table_ld (which holds lmax + 2 orders)."""
    x = np.atleast_1d(np.asarray(x, dtype=np.float64)).astype(LD)
    lmax = T.shape[0] - 2
    l = np.arange(lmax + 1, dtype=LD)[:, None]
    pos = x > 0
    ix = np.where(pos, 1 / np.where(pos, x, 1), 0)
    d2 = (l * (l - 1) * ix * T[:-1]) * ix - T[:-1] + 2 * ix * T[1:]
    z = ~pos
    if z.any():
        d2[:, z] = 0
        d2[0, z] = -LD(1) / 3
        if lmax >= 2:
            d2[2, z] = LD(2) / 15
    return d2


def miller_start(lmax):
    top = lmax + 1
    return top + int(math.ceil(math.sqrt(160.0 * top))) + 30


def jl_scheme_f64(lmax, x):
    """(j_l [lmax + 2, nx], j_l'' [lmax + 1, nx]) in float64 by the scheme of the kernel's specification, x > 0."""
    x = np.atleast_1d(np.asarray(x, dtype=np.float64))
    assert (x > 0).all()
    top = lmax + 1
    nx = x.size
    ix = 1.0 / x
    m = np.where(x < 1.0, 0, np.minimum(np.floor(x), top)).astype(np.int64)      # turning order (0 for x < 1)
    J = np.zeros((top + 2, nx))
    s, c = np.sin(x), np.cos(x)
    J[0] = s * ix
    J[1] = (J[0] - c) * ix
    for l in range(1, top + 1):                           # J[l + 1] by the step at order l, valid while l <= x
        J[l + 1] = np.where(l <= m, (2 * l + 1) * ix * J[l] - J[l - 1], 0.0)
    # the downward pass where the turning order is below top
    mil = np.nonzero(m < top)[0]
    if mil.size:
        xi = ix[mil]
        L = miller_start(lmax)
        Y = np.zeros((top + 2, mil.size))
        y0, y1 = np.ones(mil.size), np.zeros(mil.size)
        big, small = 2.0 ** 256, 2.0 ** -256
        for l in range(L, 0, -1):
            if l <= top:
                Y[l] = y0
            t = (2 * l + 1) * xi * y0 - y1
            y1, y0 = y0, t
            over = np.abs(y0) > big
            if over.any():
                y0 = np.where(over, y0 * small, y0)
                y1 = np.where(over, y1 * small, y1)
                if l <= top:
                    Y[l:, over] *= small
        Y[0] = y0
        mm = m[mil]
        cols = np.arange(mil.size)
        ja, jb = J[mm, mil], J[mm + 1, mil]
        p = np.where(np.abs(ja) >= np.abs(jb), mm, mm + 1)      # (x < 1: j_0, the larger of j_0 and j_1)
        scale = J[p, mil] / Y[p, cols]
        lo = np.arange(top + 2)[:, None]
        J[:, mil] = np.where(lo > mm[None, :], Y * scale, J[:, mil])
    J = J[: top + 1]
    l = np.arange(lmax + 1, dtype=np.float64)[:, None]
    d2 = (l * (l - 1) * ix * J[:-1]) * ix - J[:-1] + 2 * ix * J[1:]
    return J, d2


# ---- the cases of the device test ------------------------------------------------------------------------------------

def radial_cases():
    """name -> dict(lmax, k [nk], chi, cb, cf [F, nsub]); x = k * chi.  Unit coefficients where nsub = 1 (the test runs
    those twice: cb = 1, cf = 0 and cb = 0, cf = -1)."""
    rng = np.random.default_rng(20261021)
    cases = {}
    one = lambda F: np.ones((F, 1))
    cases["single"] = dict(lmax=0, k=np.array([0.37]), chi=np.array([[5.0]]), cb=one(1), cf=0 * one(1))
    cases["k0"] = dict(lmax=3, k=np.array([0.0, 0.01, 0.3, 1.1, 2.5]), chi=np.array([[1.0], [2.75]]), cb=one(2), cf=0 * one(2))
    x = np.concatenate([np.logspace(-3, np.log10(5e3), 127), [1.0, 100.0, 200.0]])
    cases["log"] = dict(lmax=200, k=x / 4.0, chi=np.array([[4.0], [4.0 * 1.37], [4.0 * 0.61]]), cb=one(3), cf=0 * one(3))
    xs = np.logspace(-2, np.log10(2e3), 70)
    chi = np.array([[3.0, 3.1, 3.2], [4.0, 4.3, 4.6], [0.9, 1.0, 1.1]])
    cases["sub"] = dict(lmax=200, k=xs / 3.0, chi=chi, cb=rng.uniform(-1, 1, (3, 3)), cf=rng.uniform(-1, 1, (3, 3)))
    xc = np.concatenate([3071.0 + np.linspace(-20, 20, 57), [3071.0, 3072.5, 3070.999, 3.1e3, 4.0e4, 4.1e4, 3.3e5]])
    cases["turn"] = dict(lmax=3071, k=xc / 1000.0, chi=np.array([[1000.0], [1000.5]]), cb=one(2), cf=0 * one(2))
    xt = np.array([0.0, 1e-300, 1e-80, 6e-52, 7e-52, 1e-20, 1e-8, 0.5])
    cases["tiny"] = dict(lmax=12, k=xt, chi=np.array([[1.0]]), cb=one(1), cf=0 * one(1))
    return cases


@functools.lru_cache(maxsize=None)
def case_tables(name):
    """The longdouble (j_l, j_l'') of every (channel, sub-sample) of a case of radial_cases(), computed once."""
    c = radial_cases()[name]
    out = []
    for i in range(c["chi"].shape[0]):
        for a in range(c["chi"].shape[1]):
            x = c["k"] * c["chi"][i, a]
            T = jl_table_ld(c["lmax"], x)
            out.append((T[:-1], jl_d2_ld(T, x), envelope(x)))
    return out


def radial_table_ld(case, cb=None, cf=None, tables=None):
    """(A [lmax + 1, F, nk] longdouble, bound [lmax + 1, F, nk] float64) of a case: the table and what the device may
    deviate from it by: sum_a (|cb_a| TOL_J + |cf_a| TOL_D2) E(x_a) + (nsub + 2) u sum_a (|cb_a j| + |cf_a j''|).
    tables: case_tables(name) of the case, if the caller has them."""
    cb = case["cb"] if cb is None else cb
    cf = case["cf"] if cf is None else cf
    k, chi, lmax = case["k"], case["chi"], case["lmax"]
    F, nsub = chi.shape
    A = np.zeros((lmax + 1, F, k.size), dtype=LD)
    B = np.zeros((lmax + 1, F, k.size))
    for i in range(F):
        mag = np.zeros((lmax + 1, k.size), dtype=LD)
        for a in range(nsub):
            if tables is not None:
                J, d2, E = tables[i * nsub + a]
            else:
                x = k * chi[i, a]
                T = jl_table_ld(lmax, x)
                J, d2, E = T[:-1], jl_d2_ld(T, x), envelope(x)
            A[:, i] += LD(cb[i, a]) * J - LD(cf[i, a]) * d2
            mag += abs(cb[i, a]) * np.abs(J) + abs(cf[i, a]) * np.abs(d2)
            B[:, i] += (abs(cb[i, a]) * TOL_J + abs(cf[i, a]) * TOL_D2) * E[None, :]
        B[:, i] += (nsub + 2) * U * mag.astype(np.float64)
    return A, B


def measure_scheme(verbose=False):
    """Worst err / E of the float64 restatement against the longdouble table over the abscissae of radial_cases()."""
    wj = wd = 0.0
    for name, c in radial_cases().items():
        x = np.unique((c["k"][None, None, :] * c["chi"][:, :, None]).ravel())
        x = x[x >= 2.0 ** -170]                           # (below: the kernel's closed forms, not the recurrences)
        T = jl_table_ld(c["lmax"], x)
        d2 = jl_d2_ld(T, x)
        J, D = jl_scheme_f64(c["lmax"], x)
        E = envelope(x)[None, :]
        ej = float(np.max(np.abs(J.astype(LD) - T).astype(np.float64) / E))
        ed = float(np.max(np.abs(D.astype(LD) - d2).astype(np.float64) / E))
        if verbose:
            print("%-8s lmax %4d  nx %3d   j_l %.3g   j_l'' %.3g" % (name, c["lmax"], x.size, ej, ed))
        wj, wd = max(wj, ej), max(wd, ed)
    return wj, wd


# ---- Gram sum ----------------------------------------------------------------------------------------------------------

def gram_ld(A, g, C0=None):
    """C[l, i, j] = C0 + sum_n g_n A[l, i, n] A[l, j, n] in longdouble, and sum_n |g_n A_i A_j| in float64."""
    A = np.asarray(A).astype(LD)
    g = np.asarray(g).astype(LD)
    C = np.einsum("n,lin,ljn->lij", g, A, A)
    S = np.einsum("n,lin,ljn->lij", np.abs(g), np.abs(A), np.abs(A)).astype(np.float64)
    if C0 is not None:
        C = C + np.asarray(C0).astype(LD)
        S = S + np.abs(np.asarray(C0, dtype=np.float64))
    return C, S


def gram_bound(S, nk):
    """(nk + 8) u sum_n |g_n A_i A_j|: nk fused multiply-adds in a row, the product g A rounded once, slack for the
    order inside an MFMA step."""
    return (nk + 8) * U * S


def gram_table_bound(A, B, g):
    """What table errors |dA| <= B add to the Gram sum: sum_n |g_n| (B_i |A_j| + |A_i| B_j + B_i B_j)."""
    A = np.abs(np.asarray(A).astype(np.float64))
    g = np.abs(np.asarray(g, dtype=np.float64))
    return (np.einsum("n,lin,ljn->lij", g, B, A) + np.einsum("n,lin,ljn->lij", g, A, B)
            + np.einsum("n,lin,ljn->lij", g, B, B))


# ---- quadrature grid ---------------------------------------------------------------------------------------------------

def fullsky_grid(chimax, kmax, oversample=4):
    """The uniform grid 0 .. kmax with the largest step that is <= pi / (oversample chimax), and its trapezoid weights."""
    n = max(int(math.ceil(kmax * oversample * chimax / math.pi)), 1)
    k = np.linspace(0.0, kmax, n + 1)
    w = np.full(n + 1, kmax / n)
    w[0] = w[-1] = 0.5 * kmax / n
    return k, w


def trapezoid_g(ps, k, w):
    """g_n = (2 / pi) w_n k_n^2 P(k_n); P is not evaluated at k = 0, where g = 0."""
    g = np.zeros_like(k)
    nz = k > 0
    g[nz] = (2.0 / math.pi) * w[nz] * k[nz] ** 2 * np.asarray(ps(k[nz]), dtype=np.float64)
    return g


def toy_ps(kstar):
    return lambda k: k ** 0.96 * np.exp(-0.5 * k ** 2 / kstar ** 2)
