"""Host oracle of the redshift-space correlation kernels - ``corahip_jl_romb`` (cora_amd/csrc/pk2xi.hip), ``corahip_xi_rsd``
(cora_amd/csrc/rsdcorr.hip) - and of the multipole route ``corrfunc.ps_to_multipoles``: numpy restatements that return the
value AND a first-order bound on what the device may differ by, in the manner of tests/_pk2xi_oracle.py.  CPU only.

eps = 2^-52; one rounding costs eps / 2.  No constant below was fitted to device output.

j_l, one evaluation (``jl_error_constant``).  x is the double product ka r on both sides.  l = 0 is sinc_romb's sinc: 4 eps
(_pk2xi_oracle).  l = 2, 4 on the device:
  closed form, |x| >= X_l (X_2 = 2, X_4 = 4), y = fl(1 / x), y2 = fl(y y):
      j_2 = ((3 y2 - 1) s - 3 y c) y                j_4 = ((105 y2^2 - 45 y2 + 1) s - (105 y2 - 10) y c) y
    A monomial term c_n y^n (s or c) carries: the sine or cosine 2 eps (the documented 2 ulp of the device's functions),
    y eps / 2 and y2 1.5 eps, i.e. at most n / 2 + 1 / 2 eps for y^n, and at most 5 roundings (eps / 2 each) on its way
    through the fmas, the product with s or c, the difference and the final product: 2 + 1.5 + 2 <= 6 eps for the terms of j_2
    (n <= 3) and 2 + 2.5 + 2.5 = 7 eps for those of j_4 (n <= 5).  The terms do not cancel in the bound:
      E_2(x) = 6 (3 y^3 + 3 y^2 + y) eps            E_4(x) = 7 (105 y^5 + 105 y^4 + 45 y^3 + 10 y^2 + y) eps
    both falling in x: 9.75 eps at x = 2, 14.63 eps at x = 4.  This is the cancellation of the closed forms: the result is
    x^l / (2l+1)!! while the terms are 3 / x^2 (l = 2) and 105 / x^4 (l = 4), a loss of 945 x 105 / x^8 relatively for
    j_4 - at x = 0.5 E_4 would be 3e4 eps (``defect="switch"``).
  series, |x| < X_l: j_l = x^l / (2l+1)!! A_1, A_m = 1 - t_m A_{m+1}, t_m = x^2 / (2 m (2 m + 2 l + 1)), A_{NT+1} = 1,
    NT = 11 (l = 2), 13 (l = 4).  t_m < 1 and 0 < A_m <= 1 throughout, so nothing cancels.  fl(t_m) carries 1.5 eps (x^2, the
    rounded constant, the product), the fma eps / 2: e_m <= t_m (e_{m+1} + 1.5 eps) + eps / 2 absolutely, e_{NT+1} = 0.  The
    factor x^l / (2l+1)!!: 2 eps (l = 2: x^2, the constant, two products), 3.5 eps (l = 4).  The first term left out,
    x^l / (2l+1)!! prod_{m <= NT+1} t_m, is 1.2e-18 (l = 2, x = 2) and 1.6e-18 (l = 4, x = 4):
      E_l(x) = x^l / (2l+1)!! (e_1 + 2 or 3.5 eps) + truncation,   rising in x: 0.78 eps at x = 2, 1.5 eps at x = 4.
  C_l = max of the two at the switch: C_0 = 4, C_2 = 9.75, C_4 = 14.63.

Romberg (``jl_romb``).  Structure, order and table are sinc_romb's, so its bound holds with the evaluation constant
replaced (|j_l| <= 1 like |sinc|):  bound = dlk eps [ (C_l + 1/2 + D / 2) sum_i Wabs_i |g_i| + 4 k Tmax ].

Multipole route (``multipoles``): the direct part is ``jl_romb``; a level of the FFTLog part is _pk2xi_oracle's with
mu = l + 1/2 (the convolution bound, the error of U, 4 eps for f and the factor), the Richardson table as there.

xi_rsd.  r = fl(sqrt(fl(fl(pi^2) + fl(sigma^2)))) and mu = fl(pi / fl(r + 1e-100)) are formed without contraction by the
device and by numpy alike, so the oracle evaluates the splines at the device's r bit for bit: the spline error is e_S of
_corrfunc_oracle (``spline``), no abscissa term.  mu^2 carries 2.5 eps relatively; P_2 = (3 mu^2 - 1) / 2: (3 x 3 + 1) / 2 = 5 eps
absolutely; P_4 = (35 mu^4 - 30 mu^2 + 3) / 8: (35 x 6.5 + 30 x 3.5 + 2 x 3) / 8 < 43 eps.  A term T = q c_j S P (q = 1, 2/3,
1/5, 4/3, 4/7, 8/35 rounded) has at most 4 roundings of its own (q, two or three products), the five additions of the
expression commit eps / 2 of a partial sum each, the last product with c3 eps / 2:
    bound = |c3| { sum_T |q c_j| (e_S |P| + |S| e_P) + 6 eps sum_T |T| }
The reference (numpy temporaries, scipy's lpn recurrence, the Cython spline) commits roundings of the same count in
another order: the goldens are compared at twice this bound.
"""
import os

import numpy as np

import _corrfunc_oracle as co
import _pk2xi_oracle as po

LD = np.longdouble
EPS = 2.0**-52
PI_LD = po.PI_LD
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rsdcorr_vectors.npz")

SWITCH = {2: 2.0, 4: 4.0}           # JL_SWITCH2, JL_SWITCH4 of pk2xi.hip
TERMS = {2: 11, 4: 13}              # JL_TERMS2, JL_TERMS4
DFACT = {0: 1.0, 2: 15.0, 4: 945.0}
ORDERS = (0, 2, 4)
DIRECT_K = 16
MAX_LINE = 4096


def load_golden():
    return np.load(GOLDEN)


# the spectra of the powerspectrum goldens (tests/golden/make_golden_rsdcorr.py hands these to the reference)
def ps_vv(k):
    return k * np.exp(-8.0 * k)


def ps_dd(k):
    return 3.0 * k * np.exp(-6.0 * k)


def ps_dv(k):
    return 2.0 * k * np.exp(-7.0 * k)


def ps_vv2d(k, mu):
    return k * np.exp(-8.0 * k) * (1.0 + 0.5 * mu**2)


# ---------------------------------------------------------------------------------------------------------------------
# j_l
# ---------------------------------------------------------------------------------------------------------------------
def _closed(l, x, s, c):
    y = 1 / x
    y2 = y * y
    if l == 2:
        return ((3 * y2 - 1) * s - 3 * y * c) * y
    return (((105 * y2 - 45) * y2 + 1) * s - (105 * y2 - 10) * y * c) * y


def jl_all(x):
    """(j_0, j_2, j_4)(x) to the longdouble working precision, one sine and cosine for the three: the ascending series
    (40 terms) below x = 3 (l = 2) and 6 (l = 4), where the closed form has lost 3 / x^2 = 0.33 (105 / x^4 = 0.08) of 2^-64
    at the most."""
    x = np.asarray(x, dtype=LD)
    safe = np.where(x == 0, LD(1), x)
    s, c = np.sin(safe), np.cos(safe)
    out = [np.where(x == 0, LD(1), s / safe)]
    for l in (2, 4):
        with np.errstate(all="ignore"):
            j = _closed(l, safe, s, c)
        ax = np.abs(x)
        # (below x = 1 the terms fall by 1 / (2 m (2 m + 2 l + 1)) at least: the 13th is below 1e-27)
        for small, nt in ((ax < 1, 12), ((ax >= 1) & (ax < (3 if l == 2 else 6)), 40)):
            x2 = x[small] * x[small]
            term = np.ones_like(x2)
            tot = np.ones_like(x2)
            for m in range(1, nt + 1):
                term = term * (-x2 / LD(2 * m * (2 * m + 2 * l + 1)))
                tot = tot + term
            j[small] = x2 ** (l // 2) / LD(DFACT[l]) * tot
        out.append(j)
    return out


def jl(l, x):
    """j_l(x), l in (0, 2, 4), exact to the longdouble working precision."""
    return jl_all(np.atleast_1d(np.asarray(x, dtype=LD)))[l // 2].reshape(np.shape(x))


def jl_device(l, x, defect=None):
    """The device's arithmetic in double (numpy's sin / cos; the fma of a series step as a product and a difference).
    defect: "switch" - the closed forms from x = 2^-4 on, where they cancel; "term" - the x^4 term of the series missing."""
    x = np.asarray(x, dtype=np.float64)
    safe = np.where(x == 0, 1.0, x)
    s, c = np.sin(safe), np.cos(safe)
    if l == 0:
        return np.where(x == 0, 1.0, s / safe)
    x2 = x * x
    if defect == "term":
        term, tot = np.ones_like(x), np.ones_like(x)
        for m in range(1, TERMS[l] + 1):
            term = term * (-x2 * (1.0 / (2.0 * m * (2.0 * m + 2 * l + 1))))
            if m != 2:
                tot = tot + term
        acc = tot
    else:
        acc = np.ones_like(x)
        for m in range(TERMS[l], 0, -1):
            acc = 1.0 - (x2 * (1.0 / (2.0 * m * (2.0 * m + 2 * l + 1)))) * acc
    ser = (x2 * (1.0 / 15.0) * acc) if l == 2 else ((x2 * x2) * (1.0 / 945.0) * acc)
    with np.errstate(all="ignore"):
        closed = _closed(l, safe, s, c)
    switch = 2.0**-4 if defect == "switch" else SWITCH[l]
    return np.where(np.abs(x) < switch, ser, closed)


def jl_closed_error(l, x):
    """E_l(x) / eps of the closed form."""
    y = 1.0 / np.asarray(x, dtype=np.float64)
    if l == 2:
        return 6.0 * (3 * y**3 + 3 * y**2 + y)
    return 7.0 * (105 * y**5 + 105 * y**4 + 45 * y**3 + 10 * y**2 + y)


def jl_series_error(l, x):
    """E_l(x) / eps of the series with TERMS[l] terms, the truncation included."""
    x2 = float(x) ** 2
    t = [x2 / (2.0 * m * (2.0 * m + 2 * l + 1)) for m in range(1, TERMS[l] + 2)]
    assert max(t) < 1.0
    e = 0.0
    for m in range(TERMS[l], 0, -1):
        e = t[m - 1] * (e + 1.5) + 0.5
    lead = float(x) ** l / DFACT[l]
    return lead * (e + (2.0 if l == 2 else 3.5)) + lead * float(np.prod(t)) / EPS


def jl_error_constant(l):
    """C_l: the absolute error of one device evaluation of j_l in units of eps, over every x."""
    if l == 0:
        return 4.0
    return max(float(jl_closed_error(l, SWITCH[l])), jl_series_error(l, SWITCH[l]))


def jl_romb(g, ka, dlk, r, lmask=None, defect=None, chunk=32):
    """corahip_jl_romb -> (value [nspec, 3, nr] longdouble, bound [nspec, 3, nr] float64).  With ``defect`` the value is
    what a device with that defect in j_l would return (``jl_device``), summed in longdouble."""
    g = np.atleast_2d(np.asarray(g, dtype=np.float64))
    ka = np.asarray(ka, dtype=np.float64)
    r = np.atleast_1d(np.asarray(r, dtype=np.float64))
    nspec, K = g.shape[0], g.shape[1] - 1
    k = K.bit_length() - 1
    assert K == 1 << k and k >= 1 and ka.size == K + 1 and 1 <= nspec <= 3
    lmask = [7] * nspec if lmask is None else list(lmask)
    W, Wabs = po.romb_weights(k)
    Wg = W[None, :] * g.astype(LD)
    val = np.zeros((nspec, 3, r.size), dtype=LD)
    for a in range(0, r.size, chunk):
        x = ka[None, :] * r[a:a + chunk, None]                          # the double product, as the device forms it
        exact = None if defect else jl_all(x.astype(LD))
        for i, l in enumerate(ORDERS):
            if not any((m >> i) & 1 for m in lmask):
                continue
            j = jl_device(l, x, defect).astype(LD) if defect else exact[i]
            val[:, i, a:a + chunk] = (Wg[:, None, :] * j[None, :, :]).sum(axis=2) * LD(dlk)
    bound = np.zeros((nspec, 3, r.size))
    cls = po.sample_classes(k)
    D = max(K // 256, 1) + 7 + k
    for s in range(nspec):
        ag = np.abs(g[s])
        absS = np.array([ag[cls == t].sum() for t in range(k)] + [0.0])
        tail = np.cumsum(absS[::-1])[::-1]
        Tmax = max(2.0**t * (0.5 * (ag[0] + ag[K]) + tail[t]) for t in range(k + 1))
        wsum = float((Wabs * ag).sum())
        for i, l in enumerate(ORDERS):
            bound[s, i] = abs(dlk) * EPS * ((jl_error_constant(l) + 0.5 + D / 2.0) * wsum + 4.0 * k * Tmax)
    for s in range(nspec):
        for i in range(3):
            if not (lmask[s] >> i) & 1:
                val[s, i], bound[s, i] = 0, 0.0
    zero = r == 0.0
    val[:, 1:, zero], bound[:, 1:, zero] = 0, 0.0
    return val, bound


# ---------------------------------------------------------------------------------------------------------------------
# the multipole route
# ---------------------------------------------------------------------------------------------------------------------
def splits(N):
    """Whether corahip_logconv_split takes N: one line up to 4096, else two factors of at most 4096 each."""
    return N <= MAX_LINE or any(N % a == 0 and N // a <= MAX_LINE for a in range(2, MAX_LINE + 1))


def multipole_grids(ra, rswitch=10.0, richardson_n=6, pad_decades=4.0):
    """(nlow, npad_low, N0, kfine) of ``corrfunc.ps_to_multipoles``.  ra must be a log grid.  Level 0 of the FFTLog part
    works on k = 1 / ra reversed, continued by whole steps d = ln(ra[1] / ra[0]): npad = ceil(pad_decades ln 10 / d) steps
    below, at least as many above, the total N0 the smallest from rnum + 2 npad on for which every level length
    N0 2^ii splits; kfine is the finest level's grid, exp(ln k_first + j d / umax), with the points of level 0 that fall
    on 1 / ra set to those values."""
    ra = np.asarray(ra, dtype=np.float64)
    d = float(np.log(ra[1] / ra[0]))
    npad = int(np.ceil(pad_decades * np.log(10.0) / d))
    umax = 2 ** (richardson_n - 1)
    n0 = ra.size + 2 * npad
    N0 = next((n for n in range(n0, 2 * n0 + 1) if all(splits(n * 2**ii) for ii in range(richardson_n))), None)
    if N0 is None:
        raise ValueError("no FFTLog length between %d and %d splits at every Richardson level" % (n0, 2 * n0))
    j = np.arange(N0 * umax, dtype=np.float64)
    kfine = np.exp(np.log(1.0 / ra[-1]) + (j - npad * umax) * (d / umax))
    kfine[npad * umax:(npad + ra.size) * umax:umax] = 1.0 / ra[::-1]
    return int(np.count_nonzero(ra < rswitch)), npad, N0, kfine


def direct_grid():
    ka = np.logspace(-5, 3, (1 << DIRECT_K) + 1)
    return ka, float(np.log(ka[1] / ka[0]))


def multipoles(psfunc, ls, ra, rswitch=10.0, richardson_n=6, pad_decades=4.0, rows=None):
    """xi_l on ``ra`` for every l of ``ls`` -> (value [len(ls), rnum] float64, bound).  rows: the indices of the direct
    part to evaluate (default all below rswitch); the others are NaN."""
    ra = np.asarray(ra, dtype=np.float64)
    nlow, npad, N0, kfine = multipole_grids(ra, rswitch, richardson_n, pad_decades)
    umax = 2 ** (richardson_n - 1)
    val = np.full((len(ls), ra.size), np.nan)
    bnd = np.full((len(ls), ra.size), np.nan)
    rows = np.arange(nlow) if rows is None else np.asarray([i for i in rows if i < nlow], dtype=int)
    if rows.size:
        ka, dlk = direct_grid()
        g = np.reshape(psfunc(ka[np.newaxis, :]), -1) * ka**3 / (2 * np.pi**2)
        mask = sum(1 << (l // 2) for l in ls)
        v, b = jl_romb(g, ka, dlk, ra[rows], [mask])
        for n, l in enumerate(ls):
            val[n, rows] = v[0, l // 2].astype(np.float64)
            bnd[n, rows] = b[0, l // 2] + EPS * np.abs(val[n, rows])
    if nlow < ra.size:
        Pfine = np.reshape(psfunc(kfine), -1)
        ffine = Pfine * kfine**1.5
        fac = (2 * np.pi) ** -1.5 * ra**-1.5
        w = np.abs(po.richardson_weights(richardson_n)).astype(np.float64)
        for n, l in enumerate(ls):
            est, eb = [], []
            for ii in range(richardson_n):
                u = 2**ii
                step = umax >> ii
                k, f = kfine[::step], ffine[::step]
                N = k.size
                U, bU = po.fftlog_phase(l + 0.5, N * float(np.log(kfine[step] / kfine[0])), N)
                gt, bc = po.logconv(f, U)
                lev = bc + 2.0 / N * float((np.abs(np.fft.rfft(f)) * bU).sum())
                gt = gt[::-1][(u - 1)::u][N0 - npad - ra.size:N0 - npad]
                est.append(gt * fac)
                eb.append(lev * fac + 4 * EPS * np.abs(est[-1]))
            hi = po.richardson(est, 2.0)
            bh = sum(w[i] * eb[i] for i in range(richardson_n))
            bh = bh + 3 * EPS * richardson_n * sum(w[i] * np.abs(est[i]) for i in range(richardson_n))
            val[n, nlow:], bnd[n, nlow:] = hi[nlow:], bh[nlow:]
    return val, bnd


# the analytic pair P = k exp(-a^2 k^2)
A_GAUSS = 1.0


def pk_gauss(k, a=A_GAUSS):
    return k * np.exp(-(a * k) ** 2)


def xi_gauss(l, r, a=A_GAUSS, envelope=False):
    """xi_l(r) = (1 / 2 pi^2) int k^3 exp(-a^2 k^2) j_l(k r) dk (G&R 6.631.1), mpmath at 30 digits -> float64.
      = (2 pi^2)^-1 sqrt(pi / 2r) Gamma(s) (r / 2a)^nu / (2 a^(7/2) Gamma(nu + 1)) 1F1(s; nu + 1; -r^2 / 4 a^2),
    nu = l + 1/2, s = (l + 4) / 2.  It falls as a power law at large r (xi_0 after one change of sign).  envelope: the
    scale the errors are judged against, the running maximum of |xi_l| from the right: |xi_l| itself where it falls,
    bridged across the zero of xi_0 by the lobe that follows it."""
    import mpmath

    mpmath.mp.dps = 30
    nu, s = l + mpmath.mpf(1) / 2, mpmath.mpf(l + 4) / 2
    out = []
    for x in np.atleast_1d(np.asarray(r, dtype=np.float64)):
        x = mpmath.mpf(float(x))
        v = (mpmath.sqrt(mpmath.pi / (2 * x)) * mpmath.gamma(s) * (x / (2 * a)) ** nu
             / (2 * mpmath.mpf(a) ** 3.5 * mpmath.gamma(nu + 1)) * mpmath.hyp1f1(s, nu + 1, -x * x / (4 * a * a)))
        out.append(float(v / (2 * mpmath.pi**2)))
    out = np.array(out)
    if envelope:
        return np.maximum.accumulate(np.abs(out)[::-1])[::-1]
    return out


# ---------------------------------------------------------------------------------------------------------------------
# xi(pi, sigma)
# ---------------------------------------------------------------------------------------------------------------------
Q_TERMS = (1.0, 2.0 / 3.0, 1.0 / 5.0, 4.0 / 3.0, 4.0 / 7.0, 8.0 / 35.0)


def coef_rows(b1, b2, f1, f2, D1, D2, pf1, pf2):
    """The coefficient rows the front end hands to the device, in its arithmetic."""
    b1, b2, f1, f2, D1, D2, pf1, pf2 = np.broadcast_arrays(*(np.asarray(v, np.float64) for v in (b1, b2, f1, f2, D1, D2, pf1, pf2)))
    return np.stack([b1 * b2, 0.5 * (b1 * f2 + b2 * f1), f1 * f2, D1 * D2 * pf1 * pf2], axis=-1).reshape(-1, 4)


def xi_rsd(kx, ky, ky2, pi, sigma, coef, defect=None):
    """corahip_xi_rsd -> (value [n] longdouble, bound [n] float64).  ky, ky2 [nfun, nk] in the order vv0 vv2 vv4 (dd0 dv0
    dv2).  defect: "p4" (the constant of P_4 3 -> 2), "47" (4/7 -> 4/5), "clamp" (r clamped to the knots, no extrapolation)."""
    kx = np.asarray(kx, np.float64)
    ky, ky2 = np.atleast_2d(np.asarray(ky, np.float64)), np.atleast_2d(np.asarray(ky2, np.float64))
    pi, sigma = np.asarray(pi, np.float64).ravel(), np.asarray(sigma, np.float64).ravel()
    coef = np.asarray(coef, np.float64).reshape(-1, 4)
    nfun = ky.shape[0]
    assert nfun in (3, 6) and pi.shape == sigma.shape
    r = np.sqrt(pi * pi + sigma * sigma)                 # numpy rounds every operation: the device's bits
    mu = (pi / (r + 1e-100)).astype(LD)
    rr = np.clip(r, kx[0], kx[-1]) if defect == "clamp" else r
    S, eS = [], []
    for f in range(nfun):
        v, _, e = co.spline(kx, ky[f], ky2[f], rr.astype(LD))
        S.append(v)
        eS.append(np.asarray(e, dtype=np.float64))
    c = coef[np.arange(pi.size) % coef.shape[0]]
    c0, c1, c2, c3 = (c[:, i].astype(LD) for i in range(4))
    mu2 = mu * mu
    P2 = (3 * mu2 - 1) / 2
    P4 = (35 * mu2 * mu2 - 30 * mu2 + (2 if defect == "p4" else 3)) / 8
    one = np.ones_like(mu)
    q47 = LD(4) / (5 if defect == "47" else 7)
    sel = (3, 4, 0, 5, 1, 2) if nfun == 6 else (0, 0, 0, 1, 1, 2)             # dd0 dv0 vv0 dv2 vv2 vv4
    terms = ((LD(1), c0, one, 0.0), (LD(2) / 3, c1, one, 0.0), (LD(1) / 5, c2, one, 0.0),
             (-LD(4) / 3, c1, P2, 5.0), (-q47, c2, P2, 5.0), (LD(8) / 35, c2, P4, 43.0))
    val = np.zeros(pi.size, dtype=LD)
    prop = np.zeros(pi.size)
    mag = np.zeros(pi.size)
    for (q, cj, P, eP), t in zip(terms, sel):
        T = q * cj * S[t] * P
        val = val + T
        qc = np.abs((q * cj).astype(np.float64))
        prop += qc * (eS[t] * np.abs(P.astype(np.float64)) + np.abs(S[t].astype(np.float64)) * eP * EPS)
        mag += np.abs(T.astype(np.float64))
    ac3 = np.abs(c3.astype(np.float64))
    return val * c3, ac3 * (prop + 6.0 * EPS * mag)


def synthetic_tables(nk, nfun, seed=0):
    """A log grid of nk knots on 1e-2 .. 1e3 and nfun smooth tables with natural second derivatives."""
    kx = np.logspace(-2, 3, nk)
    lr = np.log10(kx)
    rng = np.random.default_rng(seed)
    ky = np.stack([(1.0 + 0.3 * f) * np.cos(0.7 * (f + 1) * lr + f) / (1.0 + (kx / (5.0 + f)) ** 1.5) + 0.01 * rng.standard_normal()
                   for f in range(nfun)])
    ky2 = np.stack([co.natural_y2(kx, y) for y in ky])
    return kx, ky, ky2
