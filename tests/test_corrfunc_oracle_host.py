"""The oracle of tests/_corrfunc_oracle.py held against the host code that exists (the interpolaters of
cora_amd/util/cubicspline.py, oracle/corrfunc.py, the golden Legendre vectors), and its bounds shown to bite: a numpy
restatement of the arithmetic of cora_amd/csrc/corrfunc.hip in double (fmas where the kernel writes fmas) stays
below them on the point sets of tests/test_gpu_corrfunc.py, and the same restatement with one deliberate defect
exceeds them at one point at least.  Runs without a GPU."""
import os

import numpy as np
import pytest

import _corrfunc_oracle as co

LD = co.LD
KINDS = (0, 1, 2)


# ------------------------------------------------------------------ the kernel's arithmetic, restated in double
def _log_tab():
    inv = 1.0 / (np.arange(45, 92) / 64.0)
    return inv, (-np.log(inv.astype(LD))).astype(np.float64)


_TAB = _log_tab()


def _horner(coef, r):
    p = np.full(r.shape, coef[0])
    for c in coef[1:]:
        p = co.fma(p, r, c)
    return p


def k_log(x):
    m, e = np.frexp(x)
    lo = m < 0.70710678118654752440
    m = np.where(lo, m + m, m)
    e = np.where(lo, e - 1, e)
    i = np.rint(m * 64.0).astype(int)
    r = co.fma(m, _TAB[0][i - 45], -1.0)
    p = _horner([-1 / 8.0, 1 / 7.0, -1 / 6.0, 1 / 5.0, -1 / 4.0, 1 / 3.0, -1 / 2.0], r)
    p = co.fma(p * r, r, r)
    return co.fma(e.astype(np.float64), 0.69314718055994530942, _TAB[1][i - 45] + p)


def k_asinh(u, switch=co.ASINH_SWITCH):
    u2 = u * u
    big = k_log(u + np.sqrt(u2 + 1.0))
    small = u * (1.0 + u2 * (-1.0 / 6.0 + u2 * (3.0 / 40.0 + u2 * (-15.0 / 336.0 + u2 * (105.0 / 3456.0)))))
    return np.where(u < switch, small, big)


_FACT = [6227020800.0, 479001600.0, 39916800.0, 3628800.0, 362880.0, 40320.0, 5040.0, 720.0, 120.0, 24.0, 6.0, 2.0]


def k_expm1(ay, drop_lo=False):
    kf = np.rint(ay * 1.44269504088896340736)
    r = co.fma(-kf, 6.93147180369123816490e-01, ay)
    if not drop_lo:
        r = co.fma(-kf, 1.90821492927058770002e-10, r)
    p = _horner([1.0 / f for f in _FACT], r)
    p = co.fma(p * r, r, r)
    two_k = np.ldexp(1.0, kf.astype(int))
    return co.fma(two_k, p, two_k - 1.0)


def k_sinh(y, **kw):
    E = k_expm1(np.abs(y), **kw)
    s = 0.5 * (E + E / (E + 1.0))
    return np.where(y < 0.0, -s, s)


def k_exp(y, **kw):
    ay = np.abs(y)
    short = ay < 700.0
    E1 = k_expm1(np.where(short, ay, 0.0), **kw) + 1.0
    return np.where(short, np.where(y < 0.0, 1.0 / E1, E1), np.exp(y))


def k_spline(xs, ys, y2, x, defect=None):
    n = xs.size
    out = np.empty(x.shape)
    lo = x < xs[0]
    hi = x >= xs[n - 1]
    mid = ~(lo | hi)
    h = xs[1] - xs[0]
    out[lo] = ((ys[1] - ys[0]) / h - h * y2[1] / 6.0) * (x[lo] - xs[0]) + ys[0]
    h = xs[n - 1] - xs[n - 2]
    j2 = n - 1 if defect == "y2_last" else n - 2
    out[hi] = ((ys[n - 1] - ys[n - 2]) / h + h * y2[j2] / 6.0) * (x[hi] - xs[n - 1]) + ys[n - 1]
    xm = x[mid]
    kl = np.clip(np.searchsorted(xs, xm, side="right") - 1, 0, n - 2)
    if defect == "k_minus_1":
        kl = np.where((kl > 0) & (xm - xs[kl] <= np.spacing(xs[kl])), kl - 1, kl)
    hh = xs[kl + 1] - xs[kl]
    ih = 1.0 / hh
    a, b = (xs[kl + 1] - xm) * ih, (xm - xs[kl]) * ih
    out[mid] = a * ys[kl] + b * ys[kl + 1] + ((a * a * a - a) * y2[kl] + (b * b * b - b) * y2[kl + 1]) * ((hh * hh) / 6.0)
    return out


def k_xi(kind, xs, ys, y2, x_t, f_t, r, defect=None):
    with np.errstate(all="ignore"):
        if kind == 1:
            x = np.where(r > 0.0, k_log(np.where(r > 0.0, r, 1.0)), -np.inf)
            return k_exp(k_spline(xs, ys, y2, x, defect), drop_lo=defect == "ln2_lo")
        if kind == 2:
            x = k_asinh(r * (1.0 / x_t), 2.0**-3 if defect == "switch" else co.ASINH_SWITCH)
            return f_t * k_sinh(k_spline(xs, ys, y2, x, defect), drop_lo=defect == "ln2_lo")
        return k_spline(xs, ys, y2, r, defect)


def k_table_average(kind, xs, ys, y2, x_t, f_t, mu, xa, xw, F, xint, defect=None):
    r, _ = co.radius(xa[None, :, None], xa[None, None, :], (1.0 - mu)[:, None, None])
    v = k_xi(kind, xs, ys, y2, x_t, f_t, r.ravel(), defect).reshape(mu.size, F, xint, F, xint)
    acc = np.zeros((mu.size, F, F))
    with np.errstate(invalid="ignore"):
        for a in range(xint):
            row = np.zeros((mu.size, F, F))
            for b in range(xint):
                row += xw[b] * v[:, :, a, :, b]
            acc += row if defect == "outer_weight" else xw[a] * row
    return acc


def k_project(mu, wt, lmax, xi, defect=None):
    nm, L = mu.size, lmax + 1
    Kp = (nm + 15) // 16 * 16
    lm = np.full((L, Kp), np.nan)                      # the scratch slot: whatever an earlier call left there
    m = np.arange(Kp if defect != "pad_column" else nm)
    x = np.where(m < nm, mu[np.minimum(m, nm - 1)], 0.0)
    w = np.where(m < nm, wt[np.minimum(m, nm - 1)], 0.0)
    p0, p1 = np.ones(m.size), x
    lm[0, m] = w
    if lmax >= 1:
        lm[1, m] = w * x
    for l in range(2, L):
        p0, p1 = p1, ((2.0 * l - 1.0) * x * p1 - (l - 1.0) * p0) / l
        lm[l, m] = w * p1
    B = np.zeros((Kp, xi.shape[1]))
    B[:nm] = xi
    out = np.zeros((L, xi.shape[1]))
    with np.errstate(invalid="ignore"):
        for c in range(Kp // 16 - (1 if defect == "k_chunk" else 0)):
            out += lm[:, 16 * c:16 * c + 16] @ B[16 * c:16 * c + 16]
    return out


# ------------------------------------------------------------------ oracle against the host code that exists
@pytest.mark.parametrize("kind", KINDS)
def test_interpolaters_within_oracle_bounds(kind):
    """Interpolater / LogInterpolater / SinhInterpolater at the point sets of the GPU test."""
    for layout, xs, ys, y2, r in co.spline_cases(kind):
        with np.errstate(all="ignore"):
            got = co.interpolater(kind, xs, ys, y2).value(r)
        val, bound = co.xi_points(kind, xs, ys, y2, co.X_T, co.F_T, r, True)
        ratio = co.worst_ratio(got, val, bound)
        print("interpolater kind %d %-10s %5d points  err/bound %.3f" % (kind, layout, r.size, ratio))
        assert ratio <= 1.0, (kind, layout, ratio)


def test_legendre_matches_golden_and_host():
    from oracle import corrfunc as ocf

    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "corrfunc_vectors.npz"))
    mu = g["legendre_l12_mu"]
    lm, bound = co.legendre_matrix(mu, np.ones(mu.size), 12)
    assert np.abs(g["legendre_l12"] - lm).max() < 1e-14        # (not the double recurrence: the existing tolerance)
    mu = np.concatenate([[1.0, -1.0, 0.0, 1 - 2.0**-52, -(1 - 2.0**-52)], np.polynomial.legendre.leggauss(43)[0]])
    lm, bound = co.legendre_matrix(mu, np.ones(mu.size), 2048)
    ratio = co.worst_ratio(ocf.legendre_array(2048, mu), lm, bound + 1e-300)
    print("legendre_array lmax 2048 err/bound %.3f" % ratio)
    assert ratio <= 1.0
    assert np.all(bound[:, :2] == 0.5 * co.EPS) and np.all(lm[:, 0] == 1)


@pytest.mark.parametrize("kind", KINDS)
def test_corr_to_clarray_within_composed_bound(kind):
    """oracle/corrfunc.py through a host interpolater, per (l, i, j), at the GPU test's end-to-end case."""
    from oracle import corrfunc as ocf

    lmax, xa, ref, bound, interp = co.end_to_end_case(kind)
    with np.errstate(all="ignore"):
        got = ocf.corr_to_clarray(lambda rr: interp.value(np.ravel(rr)).reshape(np.shape(rr)), lmax, xa, xromb=2, q=2)
    ratio = co.worst_ratio(got.reshape(lmax + 1, -1), ref, bound)
    print("corr_to_clarray host kind %d err/bound %.3f" % (kind, ratio))
    assert ratio <= 1.0


# ------------------------------------------------------------------ the bounds can fail
@pytest.mark.parametrize("kind", KINDS)
def test_restatement_within_bounds_and_spline_defects_caught(kind):
    defects = {"k_minus_1": (0,), "y2_last": KINDS, "ln2_lo": (1, 2), "switch": (2,)}
    worst = {d: 0.0 for d in defects if kind in defects[d]}
    for layout, xs, ys, y2, r in co.spline_cases(kind):
        val, bound = co.xi_points(kind, xs, ys, y2, co.X_T, co.F_T, r, True)
        ratio = co.worst_ratio(k_xi(kind, xs, ys, y2, co.X_T, co.F_T, r), val, bound)
        print("restatement kind %d %-10s err/bound %.3f" % (kind, layout, ratio))
        assert ratio <= 1.0, (kind, layout, ratio)
        for d in worst:
            worst[d] = max(worst[d], co.worst_ratio(k_xi(kind, xs, ys, y2, co.X_T, co.F_T, r, d), val, bound))
    print("defects kind %d" % kind, worst)
    assert all(v > 1.0 for v in worst.values()), worst


@pytest.mark.parametrize("kind", KINDS)
def test_bin_average_defect_caught(kind):
    xs, ys, y2 = co.table(kind, "uniform64")
    for F, xint in ((3, 2), (2, 9)):
        mu, xa, xw = co.bin_average_case(kind, F, xint)
        val, bound = co.xi_table_average(kind, xs, ys, y2, co.X_T, co.F_T, mu, xa, xw, F, xint)
        good = k_table_average(kind, xs, ys, y2, co.X_T, co.F_T, mu, xa, xw, F, xint)
        bad = k_table_average(kind, xs, ys, y2, co.X_T, co.F_T, mu, xa, xw, F, xint, "outer_weight")
        rg, rb = co.worst_ratio(good, val, bound), co.worst_ratio(bad, val, bound)
        print("bin average kind %d F %d xint %d err/bound %.3f, without xw[a] %.3g" % (kind, F, xint, rg, rb))
        assert rg <= 1.0 < rb


def test_projection_defects_caught():
    for L, ncol, nm in ((129, 5, 17), (3, 129, 33), (40, 7, 16)):
        mu, wt, xi = co.projection_case(L, ncol, nm)
        val, bound = co.legendre_project(mu, wt, L - 1, xi)
        r0 = co.worst_ratio(k_project(mu, wt, L - 1, xi), val, bound)
        print("projection L %d ncol %d nm %d err/bound %.3f" % (L, ncol, nm, r0))
        assert r0 <= 1.0
        if nm > 16:
            assert co.worst_ratio(k_project(mu, wt, L - 1, xi, "k_chunk"), val, bound) > 1.0
        if nm % 16:
            assert co.worst_ratio(k_project(mu, wt, L - 1, xi, "pad_column"), val, bound) > 1.0
