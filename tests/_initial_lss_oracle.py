"""Helpers of the initial-LSS tests (tests/test_initial_lss_host.py, tests/test_gpu_initial_lss.py): the joint
xi(r) -> C_l route held to the derived bounds of tests/_corrfunc_oracle.py function by function, the extended covariance
placed by four numpy assignments, the restated CPU pipeline (P(k) -> xi -> C_l -> draw) and the statistics of a draw.
CPU only; nothing here is fitted to device output."""
import numpy as np

import _corrfunc_oracle as co
import _pk2xi_oracle as po

KSMOOTH = 0.02


def ps(k):
    """The test spectrum: 2e4 x / (1 + x^2)^2, x = k / 0.02."""
    x = np.asarray(k, dtype=np.float64) / 0.02
    return 2e4 * x / (1.0 + x * x) ** 2


class StandInCosmology:
    """``comoving_distance`` returns the distances it was made with, whatever the redshifts."""

    def __init__(self, chi):
        self.chi = np.asarray(chi, dtype=np.float64)

    def comoving_distance(self, z):
        assert len(z) == self.chi.size
        return self.chi.copy()


def triu(F):
    return np.triu_indices(F)


def pack(a):
    """[..., F, F] -> [..., F (F + 1) / 2]: the upper triangle, row-major."""
    iu, ju = triu(a.shape[-1])
    return a[..., iu, ju]


def multi_tables(kind, xs, ys, y2, f_t2):
    """The three slots of the point-set test: the table, its negative (kind 1: ys - 1; a log table has no negative) and
    the table again with another f_t -> (ky [3, nk], ky2 [3, nk], f_t [3])."""
    y1, z1 = (ys - 1.0, y2) if kind == 1 else (-ys, -y2)
    return np.stack([ys, y1, ys]), np.stack([y2, z1, y2]), np.array([co.F_T, co.F_T, f_t2])


def xi_multi_reference(kind, xs, ky, ky2, x_t, f_t, mu, xa, xw, F, xint):
    """co.xi_table_average per function with that function's f_t -> (value [nm, nfun, F, F] longdouble, bound)."""
    vals, bounds = [], []
    for f in range(ky.shape[0]):
        v, b = co.xi_table_average(kind, xs, ky[f], ky2[f], x_t, f_t[f], mu, xa, xw, F, xint)
        vals.append(v)
        bounds.append(b)
    return np.stack(vals, axis=1), np.stack(bounds, axis=1)


def quadrature(lmax, chi, xromb, q):
    """Nodes, projection weights, radial points, their weights and count per bin of corr_to_clarray."""
    import scipy.special as ss

    from oracle import corrfunc as ocf

    mu, w, wsum = ss.roots_legendre(q * lmax, mu=True)
    pts, xw, xint = ocf.radial_nodes(chi, xromb)
    return mu, w * 4.0 * np.pi / wsum, pts, xw, xint


def aps_reference(corrs, lmax, chi, xromb, q):
    """The oracle's C_l of every interpolater on the knots it holds -> (value [nfun, L, F, F] longdouble, bound)."""
    mu, wt, pts, xw, xint = quadrature(lmax, chi, xromb, q)
    F = len(chi)
    vals, bounds = [], []
    for c in corrs:
        kind, kx, ky, ky2, x_t, f_t = c._device_spline()
        xi, xb = co.xi_table_average(kind, kx, ky, ky2, x_t, f_t, mu, pts, xw, F, xint)
        v, b = co.legendre_project(mu, wt, lmax, xi.reshape(mu.size, -1), xb.reshape(mu.size, -1))
        vals.append(v.reshape(lmax + 1, F, F))
        bounds.append(b.reshape(lmax + 1, F, F))
    return np.stack(vals), np.stack(bounds)


def extended(cdd, cpd, cpp):
    """The reference's placement (lss.py:441-445)."""
    L, nz = cdd.shape[0], cdd.shape[1]
    cla = np.zeros((L, 2 * nz, 2 * nz), dtype=cdd.dtype)
    cla[:, nz:, nz:] = cdd
    cla[:, :nz, nz:] = cpd
    cla[:, nz:, :nz] = cpd
    cla[:, :nz, :nz] = cpp
    return cla


def jittered(ext):
    """The blocks as mkfullsky factors them (skysim.py:115-117)."""
    n = ext.shape[1]
    return np.stack([c + np.identity(n) * (c.diagonal().max() * 1e-14) for c in ext])


def is_positive_definite(ext):
    try:
        for c in jittered(ext):
            np.linalg.cholesky(c)
    except np.linalg.LinAlgError:
        return False
    return True


def draw_z_scores(phi, delta, ext):
    """Per slice the pixel mean of delta^2 and of phi delta against their expectations sum_l (2l+1) C_l / 4 pi, in units
    of sigma: sigma^2 = sum (2l+1) 2 C_dd^2 / (4 pi)^2 and sum (2l+1) (C_pp C_dd + C_pd^2) / (4 pi)^2 -> [2, nz]."""
    nz = phi.shape[0]
    wl = (2.0 * np.arange(ext.shape[0]) + 1.0)
    i = np.arange(nz)
    cpp, cdd, cpd = ext[:, i, i], ext[:, nz + i, nz + i], ext[:, i, nz + i]
    e_dd = (wl[:, None] * cdd).sum(0) / (4 * np.pi)
    e_pd = (wl[:, None] * cpd).sum(0) / (4 * np.pi)
    s_dd = np.sqrt((wl[:, None] * 2 * cdd**2).sum(0)) / (4 * np.pi)
    s_pd = np.sqrt((wl[:, None] * (cpp * cdd + cpd**2)).sum(0)) / (4 * np.pi)
    z_dd = ((delta**2).mean(axis=1) - e_dd) / s_dd
    z_pd = ((phi * delta).mean(axis=1) - e_pd) / s_pd
    return np.stack([z_dd, z_pd]), e_pd / s_pd


# ------------------------------------------------------------------ the restated pipeline on the CPU
CHI_DRAW = 1500.0 + 150.0 * np.arange(4)
CHI_INDEFINITE = 2300.0 + 8.0 * np.arange(4)
NSIDE = 16

_HOST = {}


def host_correlations(samples_per_decade=100, richardson_n=9):
    """``lss.calculate_correlations(ps, samples_per_decade=..., ksmooth=0.02)`` restated: ``_pk2xi_oracle.ps_to_corr`` on
    the regularised spectrum times k^-n, into SinhInterpolaters."""
    key = (samples_per_decade, richardson_n)
    if key not in _HOST:
        from cora_amd.signal import lssutil
        from cora_amd.util import cubicspline

        out = {}
        for n, f_t in ((0, 1e-3), (2, 1e-6), (4, 1e2)):
            def psn(k, n=n):
                k = np.asarray(k, dtype=np.float64)
                return (lssutil.cutoff(k, -4, 1, 0.5, 6) * lssutil.cutoff(k, 4, -1, 0.5, 4)
                        * np.exp(-0.5 * (k / KSMOOTH) ** 2) * ps(k) * k**-float(n))

            r, c, _ = po.ps_to_corr(psn, minlogr=-1, maxlogr=5, switchlogr=1, samples_per_decade=samples_per_decade,
                                    richardson_n=richardson_n, pad_low=4, pad_high=6)
            out["corr%d" % n] = cubicspline.SinhInterpolater(np.column_stack([r, c]), x_t=r[1], f_t=f_t)
        _HOST[key] = out
    return _HOST[key]


def host_extended(corrs, chi, nside=NSIDE, xromb=2, q=4):
    """numpy quadrature and projection of the three functions, placed -> [L, 2 nz, 2 nz]."""
    from oracle import corrfunc as ocf

    lmax = 3 * nside - 1
    c0, c2, c4 = (ocf.corr_to_clarray(corrs[k], lmax, chi, xromb=xromb, q=q) for k in ("corr0", "corr2", "corr4"))
    return extended(c0, c2, c4)
