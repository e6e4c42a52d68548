"""Oracle of the LOFAR synchrotron model (cora_amd.foreground.lofar, csrc/lofar.hip): the model restated in numpy on
``np.longdouble`` (64-bit mantissa here), and the error bounds the device is held to.  No GPU and no reference tree:
the reference's own outputs are in tests/golden/lofar_vectors.npz (tests/golden/make_golden_lofar.py).

Bounds, with u = 2^-53:

  los          |out - exact| <= (nz + 2 max_z|x_i b_z| + 2 E + 4) u sum_z |a_z| exp(x_i b_z) per (channel, pixel):
               nz for the ordered sum of nz terms, each added by an fma (nz - 1 roundings; the product a e is not
               rounded); 2 |x b| because b = fma(sb, beta, b0) and the product t = x b are rounded once each and exp
               turns an absolute error of its argument into a relative one of its value (the rounding of x = ln(nu / nu_0)
               on the host is the same kind of term: the oracle takes x as given, the class tests get it through
               ``propagate``); E for exp itself, E = 1 ulp = 2 u being the bound csrc/lofar.hip states for glibc's exp;
               4 u for a = fma(sa, A, a0) (one rounding, u) and the second-order remainder.
  moments      relative (n + 3) u, n the number of summands of the longer pass: the classical bound of the two-pass
               variance (Chan, Golub & LeVeque 1983: n u + n^2 kappa^2 u^2, kappa^2 = 1 + mean^2 / var), halved by the
               root, with one rounding each for the mean's division, the variance's division and the root.  Two things
               are assumed of the input, and ``moments_condition`` checks them for every field the tests use:
               (i)  n kappa^2 u << 1, so that the second-order term is out of sight;
               (ii) for the column sums, whose inputs s_p are themselves rounded sums of depth d (a lane adds
                    ceil(nz / 64) terms, then six tree levels, of which only those with a partner among the first
                    min(nz, 64) lanes round): |ds_p| <= d u sum_z |f|, and a perturbation ds moves a standard deviation
                    by at most rms(ds), so the relative error from this source is <= d u rms_p(sum_z |f|) / std(s); this
                    must fit into n u with n = ncol nz, i.e.  d rms_p(sum_z |f|) / std(s) <= ncol nz.
               For a field of unit variance and mean m the ratio in (ii) is ~ sqrt(nz) max(|m|, 0.8): at (70, 1000)
               d = 22 and (ii) allows |m| up to ~100 standard deviations.  The offset case of the tests uses 64, where a
               one-pass E[f^2] - E[f]^2 already loses kappa^2 = 4097 times the bound.
  propagate    first-order effect on Tb of perturbations of the raw fields (|dA| <= eps_a, |dbeta| <= eps_b, absolute), of
               relative errors of the two scale factors beyond those (rel_sa, rel_sb) and of x (rel_x), through
                 sa = A_std / std_p(sum_z A),  a = a0 + sa A:   |da_z| <= sa eps_a + |sa A_z| (nz eps_a / std_s + rel_sa)
                 sb = beta_std / std(beta),    b = b0 + sb beta: |db_z| <= sb eps_b + |sb beta_z| (eps_b / std_b + rel_sb)
                 Tb = sum_z a_z exp(x b_z):     |dTb| <= sum_z (|da_z| + |a_z| |x| (|db_z| + rel_x |b_z|)) exp(x b_z)
               (a standard deviation moves by at most the rms of the perturbation of its input: nz eps_a for the column
               sums, eps_b for the elements).
"""
import os

import numpy as np

LD = np.longdouble
U = LD(2.0) ** -53
EXP_ULP = 1                      # E: the ulp bound of the device exp (csrc/lofar.hip, include/corahip.h)
FIELD_TOL = 1e-13                # the project's tolerance of a device field against numpy's, relative to max|field|
ATTRS = ("nu_0", "correlated", "A_amp", "A_std", "beta_mean", "beta_std", "alpha", "delta")
CASES = ("c5_12_9", "c5_12_9_corr", "c3_8_7", "c4_6_6")


def load_golden():
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lofar_vectors.npz"))


def golden_attrs(g):
    return dict(zip(ATTRS, (float(v) for v in g["attrs"])))


def golden_case(g, tag):
    """(params dict, A, beta (A itself when correlated), Tb) of a golden case."""
    p = g[tag + "__params"]
    par = dict(nu_num=int(p[0]), x_num=int(p[1]), y_num=int(p[2]), x_width=float(p[3]), y_width=float(p[4]),
               nu_lower=float(p[5]), nu_upper=float(p[6]), correlated=bool(p[7]))
    A = g[tag + "__A"]
    beta = A if par["correlated"] else g[tag + "__beta"]
    return par, A, beta, g[tag + "__Tb"]


def worst(err, tol):
    """max err / tol, with 0 / 0 = 0."""
    err, tol = np.asarray(err, dtype=LD), np.asarray(tol, dtype=LD)
    r = np.where(err > 0, err / np.where(tol > 0, tol, LD(1e-4000)), LD(0))
    return float(r.max())


def _terms(A, beta, x, a0, sa, b0, sb):
    A = np.asarray(A, dtype=LD).reshape(-1, np.shape(A)[-1])
    beta = np.asarray(beta, dtype=LD).reshape(A.shape)
    x = np.asarray(x, dtype=LD).reshape(-1)
    a = LD(a0) + LD(sa) * A                                     # [ncol, nz]
    b = LD(b0) + LD(sb) * beta
    e = np.exp(x[:, None, None] * b[None])                      # [nfreq, ncol, nz]
    return a, b, x, e


def los(A, beta, x, a0=0.0, sa=1.0, b0=0.0, sb=1.0):
    """``(ref, bound)``, both longdouble [nfreq, ncol]: the line-of-sight sum and the bound `los` of the module docstring."""
    a, b, x, e = _terms(A, beta, x, a0, sa, b0, sb)
    nz = a.shape[1]
    ref = (a[None] * e).sum(axis=2)
    xb = np.abs(x[:, None, None] * b[None]).max(axis=2)
    bound = (nz + 2 * xb + 2 * EXP_ULP + 4) * U * (np.abs(a)[None] * e).sum(axis=2)
    return ref, bound


def moments(f):
    """``(values, rel_bound)``: values = longdouble (std of the column sums, std of the elements, max |f|), ddof 0;
    rel_bound = (n + 3) u, n = the number of elements (the summands of the longer pass, for the column sums too: every
    element goes into them)."""
    f = np.asarray(f, dtype=LD).reshape(-1, np.shape(f)[-1])
    s = f.sum(axis=1)
    sd_s = np.sqrt(((s - s.mean()) ** 2).mean())
    sd = np.sqrt(((f - f.mean()) ** 2).mean())
    return (sd_s, sd, np.abs(f).max()), (f.size + 3) * U


def moments_condition(f):
    """The two assumptions of the moments bound (module docstring) as numbers that must be <= 1: (n kappa^2 u) 1e3 for
    the elements and for the column sums, and d rms(sum |f|) / (std(s) ncol nz)."""
    f = np.asarray(f, dtype=LD).reshape(-1, np.shape(f)[-1])
    ncol, nz = f.shape
    s = f.sum(axis=1)
    var_s, var = ((s - s.mean()) ** 2).mean(), ((f - f.mean()) ** 2).mean()
    k2, k2s = 1 + f.mean() ** 2 / var, 1 + s.mean() ** 2 / var_s
    lanes = min(nz, 64)
    d = (nz + 63) // 64 - 1 + int(np.ceil(np.log2(lanes))) if lanes > 1 else 0
    sabs = np.sqrt((np.abs(f).sum(axis=1) ** 2).mean())
    return float(f.size * k2 * U * 1e3), float(ncol * k2s * U * 1e3), float(d * sabs / (np.sqrt(var_s) * ncol * nz))


def scales(A, beta, attrs, numz):
    """(a0, sa, b0, sb) of lofar.py:63-64 in longdouble, from the raw fields."""
    (sd_s, _, _), _ = moments(A)
    (_, sd_b, _), _ = moments(beta)
    return LD(attrs["A_amp"]) / numz, LD(attrs["A_std"]) / sd_s, LD(attrs["beta_mean"]), LD(attrs["beta_std"]) / sd_b


def channels(par):
    """Channel centres of Map3d (maps.py: nu_lower + (i + 1/2) (nu_upper - nu_lower) / nu_num)."""
    return par["nu_lower"] + (np.arange(par["nu_num"]) + 0.5) * ((par["nu_upper"] - par["nu_lower"]) / par["nu_num"])


def model(A, beta, par, attrs):
    """``LofarGDSE.getfield`` (lofar.py:52-73) behind its two draws, in longdouble: ``(Tb [nu_num, x_num, y_num], x, scales)``."""
    numz = (par["x_num"] + par["y_num"]) // 2
    sc = scales(A, beta, attrs, numz)
    x = np.log(np.asarray(channels(par), dtype=LD) / LD(attrs["nu_0"]))
    ref, _ = los(A, beta, x, *sc)
    return ref.reshape(par["nu_num"], par["x_num"], par["y_num"]), x, sc


def propagate(A, beta, x, sc, eps_a=0.0, eps_b=0.0, rel_sa=0.0, rel_sb=0.0, rel_x=0.0):
    """The bound `propagate` of the module docstring, longdouble [nfreq, ncol]; ``sc`` = (a0, sa, b0, sb)."""
    a0, sa, b0, sb = sc
    a, b, x, e = _terms(A, beta, x, a0, sa, b0, sb)
    A2 = np.asarray(A, dtype=LD).reshape(a.shape)
    B2 = np.asarray(beta, dtype=LD).reshape(a.shape)
    nz = a.shape[1]
    (sd_s, _, _), _ = moments(A2)
    (_, sd_b, _), _ = moments(B2)
    da = abs(sa) * eps_a + np.abs(sa * A2) * (nz * eps_a / sd_s + rel_sa)
    db = abs(sb) * eps_b + np.abs(sb * B2) * (eps_b / sd_b + rel_sb)
    return ((da[None] + np.abs(a)[None] * np.abs(x)[:, None, None] * (db + rel_x * np.abs(b))[None]) * e).sum(axis=2)
