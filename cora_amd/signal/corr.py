"""Counterpart of the hot-path part of cora/signal/corr.py: the flat-sky FFT table model
of C_l(z, z') (``RedshiftCorrelation.angular_powerspectrum_fft``, corr.py:891-982).

Setup (host, one-off per instance, exactly the reference's recipe corr.py:909-942):
P(k) on a [500 log k_perp] x [32768 linear k_par] grid, times {1, mu^2, mu^4}, DCT-I along
k_par -> three [500, 32768] tables, uploaded once to HBM (393 MB) and cached.
Evaluation (device): K1 in csrc/clarray.hip, either fused with the Romberg channel
average (through ``skysim.clarray``) or at arbitrary broadcast points (calling
``angular_powerspectrum`` directly).

The flat-sky redshift-space cube (``_realisation_dv`` / ``realisation``, corr.py:562-770) runs on
the GPU through csrc/flatsky.hip: Gaussian field draw, the mu^2 velocity field by rfftn / irfftn,
per-slice growth factors and the ray-traced trilinear resampling.

The redshift-space correlation function xi(pi, sigma; z1, z2) (corr.py:242-446) runs through
csrc/rsdcorr.hip (``corahip_xi_rsd``: the six multipole splines and the Legendre combination fused, one pass over the
points) on tables that ``gen_cache`` makes on the device (``corrfunc.ps_to_multipoles``: ``corahip_jl_romb`` and FFTLog) or
``_load_cache`` reads from a file.  ``powerspectrum`` / ``powerspectrum_1D`` call Python spectra and stay host numpy.

The exact curved-sky C_l(z, z') (``angular_powerspectrum_full``, corr.py:777-868: dead code in the reference, which
imports a module that does not exist) runs through csrc/fullsky.hip: on one uniform wavenumber grid the integral is a
Gram product over k of a table of radial functions, ``C_l[i, j] = sum_n g_n A_l[i, n] A_l[j, n]`` with ``A_l[i, n] =
cb_i j_l(k_n chi_i) - cf_i j_l''(k_n chi_i)``; the channel average of ``skysim.clarray`` is taken inside the table.  The
reference's piecewise adaptive integrator is not reproduced.
"""
import math
from os.path import exists

import numpy as np

from .. import _lib
from ..core import gaussianfield
from ..util import constants, fftutil
from ..util import cubicspline as cs
from ..util.cosmology import Cosmology


class RedshiftCorrelation(object):
    r"""Redshift-space correlations in the linear regime: the C_l(z, z') table model.

    Parameters
    ----------
    ps_vv : function
        Velocity power spectrum P(k) [k in h/Mpc] at ``redshift``.
    ps_dd, ps_dv : function, optional
        Accepted for interface compatibility; the table model uses ``ps_vv`` with ``bias``.
    redshift : scalar, optional
        Redshift at which the power spectra are calculated.
    bias : scalar, optional
        Bias between the observable and the velocities.
    """

    ps_vv = None
    ps_dd = None
    ps_dv = None
    ps_2d = False
    ps_redshift = 0.0
    bias = 1.0
    _vv_only = False

    _cached = False

    kperpmin = 1e-4
    kperpmax = 40.0
    nkperp = 500
    kparmax = 20.0
    nkpar = 32768
    _freq_window = 0.0
    _aps_cache = False

    def __init__(self, ps_vv=None, ps_dd=None, ps_dv=None, redshift=0.0, bias=1.0):
        self.ps_vv = ps_vv
        self.ps_dd = ps_dd
        self.ps_dv = ps_dv
        self.ps_redshift = redshift
        self.bias = bias
        self._vv_only = False if ps_dd and ps_dv else True
        self.cosmology = Cosmology()
        self._dev_tables = {}

    @classmethod
    def from_file_matterps(cls, fname, redshift=0.0, bias=1.0):
        """Initialise from a cached 4-column multipole file of a single power spectrum (corr.py:114-132)."""
        rc = cls(redshift=redshift, bias=bias)
        rc._vv_only = True
        rc._load_cache(fname)
        return rc

    @classmethod
    def from_file_fullps(cls, fname, redshift=0.0):
        """Initialise from a cached 7-column multipole file of the three power spectra (corr.py:134-150)."""
        rc = cls(redshift=redshift)
        rc._vv_only = False
        rc._load_cache(fname)
        return rc

    # ---- power spectra (corr.py:152-240): Python spectra, host numpy --------------------------
    def powerspectrum(self, kpar, kperp, z1=None, z2=None):
        """The redshift-space power spectrum at (kpar, kperp) (corr.py:152-201): ``ps_vv (b1 + mu^2 f1)(b2 + mu^2 f2)``
        (``ps_vv(k, mu)`` with ``ps_2d``), or the three-spectrum form, times D1 D2 pf1 pf2.  A redshift left ``None`` is
        ``ps_redshift``."""
        if z1 is None:
            z1 = self.ps_redshift
        if z2 is None:
            z2 = self.ps_redshift
        b1, b2 = self.bias_z(z1), self.bias_z(z2)
        f1, f2 = self.growth_rate(z1), self.growth_rate(z2)
        D1 = self.growth_factor(z1) / self.growth_factor(self.ps_redshift)
        D2 = self.growth_factor(z2) / self.growth_factor(self.ps_redshift)
        pf1, pf2 = self.prefactor(z1), self.prefactor(z2)
        k2 = kpar**2 + kperp**2
        k = k2**0.5
        mu = kpar / k
        mu2 = kpar**2 / k2
        if self._vv_only:
            if self.ps_2d:
                ps = self.ps_vv(k, mu) * (b1 + mu2 * f1) * (b2 + mu2 * f2)
            else:
                ps = self.ps_vv(k) * (b1 + mu2 * f1) * (b2 + mu2 * f2)
        else:
            ps = b1 * b2 * self.ps_dd(k) + mu2 * self.ps_dv(k) * (f1 * b2 + f2 * b1) + mu2**2 * f1 * f2 * self.ps_vv(k)
        return D1 * D2 * pf1 * pf2 * ps

    def powerspectrum_1D(self, k_vec, z1, z2, numz):
        """The real-space power spectrum ``ps_vv(k)`` times the square of the mean of D(z) pf(z) b(z) over ``numz + 1``
        slices equally spaced in comoving distance between ``z1`` and ``z2`` (corr.py:203-240)."""
        c1 = self.cosmology.comoving_distance(z1)
        c2 = self.cosmology.comoving_distance(z2)
        comoving_inv = inverse_approx(self.cosmology.comoving_distance, z1, z2)
        za = comoving_inv(np.linspace(c1, c2, numz + 1, endpoint=True))
        Dz = self.growth_factor(za) / self.growth_factor(self.ps_redshift)
        dfactor = np.mean(Dz * self.prefactor(za) * self.bias_z(za))
        return self.ps_vv(k_vec) * dfactor * dfactor

    # ---- xi(pi, sigma; z1, z2) (corr.py:242-446) ------------------------------------------------
    _MULTIPOLES = ("_vv0i", "_vv2i", "_vv4i", "_dd0i", "_dv0i", "_dv2i")

    def _set_multipoles(self, ra, cols):
        """``cols``: vv0 vv2 vv4 (dd0 dv0 dv2) on ``ra`` -> the interpolaters of the reference and the knot arrays
        (knots, y [nfun, nk], y'' [nfun, nk]) the device evaluator takes."""
        ra = np.ascontiguousarray(ra, dtype=np.float64)
        for name, col in zip(self._MULTIPOLES, cols):
            setattr(self, name, cs.Interpolater(ra, np.asarray(col, dtype=np.float64)))
        sp = [getattr(self, name) for name in self._MULTIPOLES[: len(cols)]]
        self._xi_knots = (ra, np.stack([i._data[:, 1] for i in sp]), np.stack([i._y2 for i in sp]))
        self.__dict__.pop("_xi_knots_dev", None)
        self._cached = True

    def _load_cache(self, fname):
        """Load a multipole table ``r vv0 vv2 vv4 [dd0 dv0 dv2]`` written by :meth:`gen_cache` or by the reference
        (corr.py:372-397)."""
        if not exists(fname):
            raise Exception("Cache file does not exist.")
        a = np.loadtxt(fname)
        if not self._vv_only and a.shape[1] != 7:
            raise Exception("Cache file has wrong number of columns.")
        self._set_multipoles(a[:, 0], [a[:, i] for i in range(1, 4 if self._vv_only else 7)])

    def gen_cache(self, fname=None, rmin=1e-3, rmax=1e4, rnum=1000):
        """Tabulate the multipoles xi_0, xi_2, xi_4 of ``ps_vv`` - and xi_0 of ``ps_dd``, xi_0, xi_2 of ``ps_dv`` when the
        three spectra are given - on ``logspace(log10 rmin, log10 rmax, rnum)`` and keep them as the interpolaters the
        correlation function reads (corr.py:399-446).  With ``fname`` the 4- or 7-column text file of the reference is
        written, unless it exists.

        The integrals run on the device (``corrfunc.ps_to_multipoles``) and are the clean ones over k in (0, inf).  The
        reference's ``_integrate`` (corr.py:994-1050, dead there: it imports a module that does not exist) integrated
        between 1e-4 pi / r and 1e3 pi / r with a smoothed upper edge, and so did the table the reference ships for the 21cm
        model: that table differs from the clean integral below r ~ 0.05 and above r ~ 30.  ``_load_cache`` of that file
        reproduces the reference's numbers."""
        from . import corrfunc

        ra = np.logspace(np.log10(rmin), np.log10(rmax), rnum)
        ps, ls = [self.ps_vv], [(0, 2, 4)]
        if not self._vv_only:
            ps, ls = ps + [self.ps_dd, self.ps_dv], ls + [(0,), (0, 2)]
        xi = corrfunc.ps_to_multipoles(ps, ls, ra)
        cols = [xi[0][0], xi[0][2], xi[0][4]]
        if not self._vv_only:
            cols += [xi[1][0], xi[2][0], xi[2][2]]
        if fname and not exists(fname):
            np.savetxt(fname, np.dstack([ra] + cols)[0])
        self._set_multipoles(ra, cols)

    def _z_coefficients(self, z1, z2):
        """The coefficient rows (b1 b2, (b1 f2 + b2 f1) / 2, f1 f2, D1 D2 pf1 pf2) of the model hooks on the broadcast
        redshifts -> (rows [nz, 4], the shape the redshifts broadcast to)."""
        z1, z2 = np.broadcast_arrays(np.asarray(z1, dtype=np.float64), np.asarray(z2, dtype=np.float64))
        b1, b2 = self.bias_z(z1), self.bias_z(z2)
        f1, f2 = self.growth_rate(z1), self.growth_rate(z2)
        D1 = self.growth_factor(z1) / self.growth_factor(self.ps_redshift)
        D2 = self.growth_factor(z2) / self.growth_factor(self.ps_redshift)
        pf1, pf2 = self.prefactor(z1), self.prefactor(z2)
        one = np.ones(z1.shape)
        rows = np.stack([one * (b1 * b2), one * (0.5 * (b1 * f2 + b2 * f1)), one * (f1 * f2), one * (D1 * D2 * pf1 * pf2)], axis=-1)
        return np.ascontiguousarray(rows.reshape(-1, 4), dtype=np.float64), z1.shape

    def redshiftspace_correlation_device(self, pi, sigma, z1=None, z2=None):
        """:meth:`redshiftspace_correlation` on float64 device tensors ``pi``, ``sigma`` (broadcast against each other and
        against the redshifts) -> device tensor.  The redshifts are host scalars or arrays."""
        import torch

        ctx = _lib.get_context()
        if z1 is None and z2 is None:
            z1 = z2 = self.ps_redshift
        elif z2 is None:
            z2 = z1
        elif z1 is None:
            z1 = self.ps_redshift
        if not self._cached:
            self.gen_cache()
        rows, zshape = self._z_coefficients(z1, z2)
        pi, sigma = torch.broadcast_tensors(torch.as_tensor(pi, dtype=torch.float64, device=ctx.device),
                                            torch.as_tensor(sigma, dtype=torch.float64, device=ctx.device))
        shape = tuple(np.broadcast_shapes(tuple(pi.shape), zshape))
        if len(rows) > 1:
            # point i reads row i % ncoef: true as it is when the redshifts lie on the trailing axes of the result
            full = np.broadcast_to(np.arange(len(rows)).reshape(zshape), shape).reshape(-1)
            if not np.array_equal(full, np.arange(full.size) % len(rows)):
                rows = rows[full]
        pi, sigma = (t.expand(shape).contiguous().reshape(-1) for t in (pi, sigma))
        dev = self.__dict__.get("_xi_knots_dev")
        if dev is None or dev[0] != ctx.device.index:
            dev = self._xi_knots_dev = (ctx.device.index,) + tuple(ctx.to_device(a) for a in self._xi_knots)
        out = ctx.xi_rsd(dev[1], dev[2], dev[3], pi, sigma, ctx.to_device(rows))
        return out.reshape(shape)

    def redshiftspace_correlation(self, pi, sigma, z1=None, z2=None):
        """The correlation function in the flat-sky approximation at radial separation ``pi`` and transverse separation
        ``sigma`` (h^-1 Mpc), numpy in and out (corr.py:242-348); ``pi`` and ``sigma`` broadcast to a common shape.

        With neither redshift given both points are at ``ps_redshift``; with only ``z1`` the second point is at ``z1``.
        The model hooks ``bias_z``, ``growth_rate``, ``growth_factor`` and ``prefactor`` are evaluated on the host on the
        redshifts only; the multipole splines and the Legendre combination run on the device (``corahip_xi_rsd``).

        With only ``ps_vv`` known, dd0 = dv0 = vv0 and dv2 = vv2 enter the formula of the reference's docstring.  (The
        reference itself does that for scalar arguments only: for arrays it scales the three names in place although they
        are one array, so each ends up times b1 b2 (b1 f2 + b2 f1) / 2 f1 f2.  That is not reproduced.)

        Extension: the redshifts may be arrays that broadcast against the points (the reference tests ``z == None``, which
        fails for arrays of more than one element).  Without a cache the call runs :meth:`gen_cache` with its defaults
        first, where the reference would enter its dead ``_integrate`` at every r."""
        out = self.redshiftspace_correlation_device(np.asarray(pi, dtype=np.float64), np.asarray(sigma, dtype=np.float64),
                                                    z1, z2).cpu().numpy()
        return out if out.ndim else float(out)

    def angular_correlation(self, theta, z1, z2):
        """Angular correlation function in the flat-sky approximation: ``theta`` in radians between points at ``z1``
        and ``z2`` (corr.py:350-370)."""
        za = (z1 + z2) / 2.0
        sigma = theta * self.cosmology.proper_distance(za)
        pi = self.cosmology.comoving_distance(z2) - self.cosmology.comoving_distance(z1)
        return self.redshiftspace_correlation(pi, sigma, z1, z2)

    # ---- model hooks (corr.py:448-530) --------------------------------------------------
    def bias_z(self, z):
        return self.bias * np.ones_like(z)

    def growth_factor(self, z):
        return 1.0 / (1.0 + z)

    def growth_rate(self, z):
        return 1.0 * np.ones_like(z)

    def prefactor(self, z):
        return 1.0 * np.ones_like(z)

    def mean(self, z):
        return np.ones_like(z) * 0.0

    # ---- flat-sky redshift-space cube (corr.py:547-770) ----------------------------------
    _sigma_v = 0.0

    def sigma_v(self, z):
        """Pairwise velocity dispersion, ``_sigma_v`` km/s -> h^-1 Mpc (corr.py:549-556)."""
        return np.ones_like(z) * (self._sigma_v / 100.0)

    def velocity_damping(self, kpar):
        """Lorentzian damping of the line-of-sight modes (corr.py:558-560)."""
        return (1.0 + (kpar * self.sigma_v(self.ps_redshift)) ** 2.0) ** -1.0

    def _cube_generator(self, d, n):
        # field generator + mu^2 array of one cube geometry, resident on the device and reused between calls
        key = (tuple(float(x) for x in d), tuple(int(x) for x in n))
        cache = self.__dict__.setdefault("_cube_cache", {})
        if key not in cache:
            rfv = gaussianfield.RandomField(npix=np.array(n), wsize=np.array(d))
            rfv.powerspectrum = lambda karray: (self.ps_vv((karray**2).sum(axis=3) ** 0.5)
                                                * self.velocity_damping(karray[..., 0]))
            rfv.generate_kweight()
            kvec = fftutil.rfftfreqn(rfv._n, (rfv._w / rfv._n) / (2 * math.pi))
            with np.errstate(invalid="ignore", divide="ignore"):
                mu2 = kvec[..., 0] ** 2 / (kvec**2).sum(axis=3)
            mu2.flat[0] = 0.0
            cache.clear()
            cache[key] = (rfv, _lib.get_context().to_device(mu2))
        return cache[key]

    def _realisation_dv_device(self, d, n, seed=None):
        """Density and line-of-sight velocity cubes as device tensors (corr.py:562-603).

        ``seed=None`` uses numpy's global state exactly as the reference; an integer draws on the GPU.
        """
        if not self._vv_only:
            raise Exception("Doesn't work for independent fields, I need to think a bit more first.")
        ctx = _lib.get_context()
        rfv, mu2 = self._cube_generator(d, n)
        df = rfv.getfield_device(seed=seed)
        spec = ctx.spec_mul_real(ctx.rfftn(df), mu2)
        vf = ctx.irfftn(spec)
        return df, vf

    def _realisation_dv(self, d, n):
        df, vf = self._realisation_dv_device(d, n)
        return df.cpu().numpy(), vf.cpu().numpy()

    def realisation(self, z1, z2, thetax, thetay, numz, numx, numy, zspace=True, refinement=1,
                    report_physical=False, density_only=False, no_mean=False, no_evolution=False, pad=5,
                    seed=None, device=False):
        """Simulate a redshift-space volume ``[numz, numx, numy]`` in the flat-sky approximation.

        Same arguments and geometry as corr.py:605-770: a padded comoving box between ``z1`` and ``z2`` is
        filled with a Gaussian density field and its mu^2 velocity field, scaled slice by slice with
        D(z), b(z), f(z), the prefactor and the mean, and resampled along the lines of sight onto regular
        angle / redshift (``zspace``) or angle / scale-factor bins by trilinear interpolation.  ``seed`` and
        ``device`` are extensions: device-side normals, and device tensors instead of numpy arrays.
        """
        cosmo = self.cosmology
        d1, d2 = cosmo.proper_distance(z1), cosmo.proper_distance(z2)
        c1, c2 = cosmo.comoving_distance(z1), cosmo.comoving_distance(z2)
        c_center = (c1 + c2) / 2.0
        d = np.array([c2 - c1, thetax * d2 * constants.degree, thetay * d2 * constants.degree])
        n = np.array([numz, int(d2 / d1 * numx), int(d2 / d1 * numy)])
        if (n[-1] + pad) % 2 != 0:
            pad += 1
        d = d * (n + pad).astype(float) / n.astype(float)
        c1 = c_center - (c_center - c1) * (n[0] + pad) / float(n[0])
        c2 = c_center + (c2 - c_center) * (n[0] + pad) / float(n[0])
        n = refinement * (n + pad)

        ctx = _lib.get_context()
        df, vf = self._realisation_dv_device(d, n, seed=seed)
        n = tuple(df.shape)

        # redshift of every slice of the box, then the slice factors
        comoving_inv = inverse_approx(cosmo.comoving_distance, z1, z2)
        za = comoving_inv(np.linspace(c1, c2, n[0], endpoint=True))
        mz = self.mean(za)
        Dz = self.growth_factor(za) / self.growth_factor(self.ps_redshift)
        dfac = Dz * self.prefactor(za) * self.bias_z(za)
        vfac = Dz * self.prefactor(za) * self.growth_rate(za)
        if no_evolution:
            dfac = np.full(n[0], np.mean(dfac))
            vfac = np.full(n[0], np.mean(vfac))
        mean = np.zeros(n[0]) if no_mean else mz * np.ones(n[0])
        rsf = ctx.cube_affine(df, None if density_only else vf, ctx.to_device(dfac), ctx.to_device(vfac),
                              ctx.to_device(mean))

        # lines of sight: regular in redshift or in scale factor
        if zspace:
            za = np.linspace(z1, z2, numz, endpoint=False)
        else:
            za = 1.0 / np.linspace(1.0 / (1 + z2), 1.0 / (1 + z1), numz, endpoint=False)[::-1] - 1.0
        da = cosmo.proper_distance(za)
        xa = cosmo.comoving_distance(za)
        tx = np.linspace(-thetax / 2.0, thetax / 2.0, numx) * constants.degree
        ty = np.linspace(-thetay / 2.0, thetay / 2.0, numy) * constants.degree
        zc = (xa - c1) / (c2 - c1) * (n[0] - 1.0)
        acube = ctx.raytrace_slices(rsf, ctx.to_device(zc), ctx.to_device(da), ctx.to_device(tx), ctx.to_device(ty),
                                    d[1], d[2])
        if not device:
            acube, rsf = acube.cpu().numpy(), (rsf.cpu().numpy() if report_physical else rsf)
        if report_physical:
            return acube, rsf, (c1, c2, d[1], d[2])
        return acube

    # ---- table build / cache (corr.py:870-887, 909-942) ---------------------------------
    # K0: the tables are BUILT ON THE DEVICE (csrc/tables21.hip): P(k) on the 500 x 32768 grid - by the device spline
    # evaluator when ps_vv is the library's own spline form (Corr21cm: exp(-k^2 / 2 k*^2) LogInterpolater), by one
    # vectorised host call of the user's callable otherwise (it IS a Python callback) - then mu^2 / mu^4 and the
    # DCT-I along k_par on the GPU.  They stay in HBM; the host copies (`_aps_dd` ...) are made only when asked for.
    def _ps_spline_plan(self):
        """(interpolater, kstar) when ``ps_vv`` is still the spline-form callable a subclass registered."""
        plan = getattr(self, "_ps_plan", None)
        if plan is None or self.ps_2d or self.ps_vv is not plan["callable"]:
            return None
        return plan["spline"], float(plan["kstar"]())

    def _build_tables(self, ctx=None):
        ctx = ctx if ctx is not None else _lib.get_context()
        kperp = np.logspace(np.log10(self.kperpmin), np.log10(self.kperpmax), self.nkperp)
        kpar = np.linspace(0, self.kparmax, self.nkpar)
        kt_d, kp_d = ctx.to_device(kperp), ctx.to_device(kpar)
        sp = self._ps_spline_plan()
        kind = sp[0]._device_spline()[0] if sp is not None else None
        if sp is not None and kind in (0, 1):
            _, x, y, y2, _, _ = sp[0]._device_spline()
            dd, dv, vv = ctx.ps_table21cm(kt_d, kp_d, spline=(kind == 1, ctx.to_device(x), ctx.to_device(y), ctx.to_device(y2)),
                                          kstar=sp[1], freq_window=self._freq_window)
        else:
            kpar2, kperp2 = kpar[np.newaxis, :], kperp[:, np.newaxis]
            k = (kpar2**2 + kperp2**2) ** 0.5
            window = np.sinc(kpar2 * self._freq_window / (2 * np.pi)) ** 2
            dd_h = (self.ps_vv(k, kpar2 / k) if self.ps_2d else self.ps_vv(k)) * window
            dd, dv, vv = ctx.ps_table21cm(kt_d, kp_d, dd=ctx.to_device(np.ascontiguousarray(dd_h, dtype=np.float64)))
        norm = self.kparmax / (2 * self.nkpar)
        for t in (dd, dv, vv):
            ctx.dct1_rows(t, norm)
        # (the other devices' copies stay: a second context must not evict the first one's tables)
        if getattr(self, "_dev_tables", None) is None:
            self._dev_tables = {}
        pins = self.__dict__.get("_pins")
        if pins and ctx.device.index in pins:              # the set being replaced is pinned: not any more
            self._unpin({ctx.device.index: pins.pop(ctx.device.index)})
        self._dev_tables[ctx.device.index] = (dd, dv, vv)
        self._host_tables = None
        self._aps_cache = True

    def _host_copy(self, i):
        if not self._aps_cache:
            self._build_tables()
        if getattr(self, "_host_tables", None) is None:
            dev = next(iter(self._dev_tables.values()))
            self._host_tables = tuple(t.cpu().numpy() for t in dev)
        return self._host_tables[i]

    def _set_host_table(self, i, value):
        """Assigning a table (what the reference's load_fft_cache does, corr.py:879-887, and user subclasses may):
        it becomes the host copy; the device copies are dropped and re-uploaded on next use."""
        cur = list(self._host_tables) if getattr(self, "_host_tables", None) is not None else (
            [self._host_copy(k) if k != i else None for k in range(3)] if self._aps_cache else [None, None, None])
        cur[i] = np.ascontiguousarray(value, dtype=np.float64)
        self._host_tables = tuple(cur)
        self._drop_dev_tables()
        if all(t is not None for t in cur):
            self.nkperp, self.nkpar = cur[0].shape
            self._aps_cache = True

    _aps_dd = property(lambda self: self._host_copy(0), lambda self, v: self._set_host_table(0, v))
    _aps_dv = property(lambda self: self._host_copy(1), lambda self, v: self._set_host_table(1, v))
    _aps_vv = property(lambda self: self._host_copy(2), lambda self, v: self._set_host_table(2, v))

    def save_fft_cache(self, fname):
        """Save the three lookup tables (corr.py:870-877)."""
        np.savez(fname, dd=self._aps_dd, dv=self._aps_dv, vv=self._aps_vv)

    def load_fft_cache(self, fname):
        """Load lookup tables saved by :meth:`save_fft_cache` (corr.py:879-887)."""
        a = np.load(fname)
        self._host_tables = (a["dd"], a["dv"], a["vv"])
        self.nkperp, self.nkpar = self._host_tables[0].shape
        self._aps_cache = True
        self._drop_dev_tables()

    _table_generation = [0]      # process-wide counter: every (re)built / uploaded table set gets its own number

    @staticmethod
    def _unpin(pins):
        """Withdraws the K1 pins listed in ``pins`` ({device index: (ctx, generation)}): called when the device tables they
        vouch for are dropped - by the setters, ``load_fft_cache``, a rebuild - and by the finaliser of the model (the
        caching allocator hands a freed block to the next same-size request: a stale pin would vouch for foreign data)."""
        for ctx, gen in list(pins.values()):
            try:
                ctx.unpin_tables(gen)
            except Exception:       # (interpreter shutdown: the context may be gone already)
                pass
        pins.clear()

    def _drop_dev_tables(self):
        pins = self.__dict__.get("_pins")
        if pins:
            self._unpin(pins)
        self.__dict__.pop("_dev_table_gen", None)
        self._dev_tables = {}

    def _tables_on(self, ctx):
        dd_dv_vv = self._tables_on_unpinned(ctx)
        # K1 may keep its transposed copy of these tables between calls: they are this instance's cache and change only
        # through _build_tables / load_fft_cache / the _aps_* setters, each of which makes a new entry with a new number
        gens = self.__dict__.setdefault("_dev_table_gen", {})
        key = ctx.device.index
        if gens.get(key, (None, None))[0] is not dd_dv_vv:
            RedshiftCorrelation._table_generation[0] += 1
            gens[key] = (dd_dv_vv, RedshiftCorrelation._table_generation[0])
        ctx.pin_tables(*dd_dv_vv, gens[key][1])
        pins = self.__dict__.get("_pins")
        if pins is None:
            import weakref

            pins = self._pins = {}
            weakref.finalize(self, RedshiftCorrelation._unpin, pins)     # (holds the dict, not the model)
        pins[key] = (ctx, gens[key][1])
        return dd_dv_vv

    def _tables_on_unpinned(self, ctx):
        key = ctx.device.index
        if key not in self._dev_tables:
            ht = getattr(self, "_host_tables", None)
            if self._aps_cache and ht is not None and all(t is not None for t in ht):
                self._dev_tables[key] = tuple(ctx.to_device(t) for t in ht)   # loaded cache
            elif self._aps_cache and self._dev_tables:
                src = next(iter(self._dev_tables.values()))                   # another GPU holds them: device-to-device
                self._dev_tables[key] = tuple(t.to(ctx.device) for t in src)
            else:
                self._build_tables(ctx)
        return self._dev_tables[key]

    # ---- per-redshift quantities (corr.py:944-951) --------------------------------------
    def _z_quantities(self, za):
        za = np.asarray(za, dtype=np.float64)
        chi = self.cosmology.comoving_distance(za)
        pfd = self.prefactor(za) * self.growth_factor(za) / self.growth_factor(self.ps_redshift)
        return chi, pfd, self.growth_rate(za) * np.ones_like(za), self.bias_z(za) * np.ones_like(za)

    def _table_plan(self, za_to_z):
        def prepare(ctx, za):
            dd, dv, vv = self._tables_on(ctx)
            chi, pfd, f, b = self._z_quantities(za_to_z(za))
            return dict(dd=dd, dv=dv, vv=vv, kperpmin=self.kperpmin, kperpmax=self.kperpmax,
                        kparmax=self.kparmax, chi=chi, pfd=pfd, f=f, b=b)

        return dict(kind="table21cm", prepare=prepare)

    def _clarray_plan(self, aps):
        """Protocol used by ``skysim.clarray`` to recognise the models that run on the device: the un-overridden flat-sky
        method (``angular_powerspectrum`` is an alias of it) is the table model, the un-overridden
        ``angular_powerspectrum_full`` the exact curved-sky one; any other bound method - a subclass override, ... - goes
        down the generic host-callable path."""
        fn = getattr(aps, "__func__", None)
        if fn is RedshiftCorrelation.angular_powerspectrum_full:
            return self._fullsky_plan(lambda z: z)
        if fn is not RedshiftCorrelation.angular_powerspectrum_fft:
            return None
        return self._table_plan(lambda z: z)

    # ---- exact curved-sky C_l (corr.py:777-868) ------------------------------------------------
    fullsky_oversample = 4
    fullsky_kmax = None            # the upper limit of the k integral; None: the default of _fullsky_grid

    def _fullsky_check(self):
        if not self._vv_only:
            raise Exception("Only works for vv_only at the moment.")
        if self.ps_2d:
            raise ValueError("angular_powerspectrum_full takes an isotropic ps_vv(k), not ps_2d")
        if self._freq_window != 0:
            raise ValueError("angular_powerspectrum_full: _freq_window must be 0 (the exact channel average of "
                             "skysim.clarray replaces that window)")

    def _fullsky_grid(self, chimax, kmax=None, oversample=None):
        """The wavenumber grid of the exact C_l and its weights ``g_n = (2 / pi) w_n k_n^2 P(k_n)`` (host arrays).

        Uniform from 0 to ``kmax`` with the largest step that is not above ``pi / (oversample chimax)`` - ``oversample``
        samples per period of the fastest component ``cos(k (x1 + x2))``, default ``fullsky_oversample`` = 4 - and the
        trapezoid weights ``w``: the integrand vanishes at both ends, so the rule converges fast.  ``kmax`` defaults to the
        attribute ``fullsky_kmax`` and, where that is None, to ``6 _kstar`` for the library's own spline spectrum (``exp(-18)`` at the cut) and to ``kperpmax`` otherwise.
        ``ps_vv`` is evaluated once, on the grid without k = 0 (where g = 0)."""
        if kmax is None:
            kmax = self.fullsky_kmax
        if kmax is None:
            sp = self._ps_spline_plan()
            kmax = 6.0 * sp[1] if sp is not None else self.kperpmax
        kmax = float(kmax)
        oversample = self.fullsky_oversample if oversample is None else oversample
        if not (kmax > 0 and np.isfinite(kmax)) or not (oversample > 0 and np.isfinite(oversample)):
            raise ValueError("kmax and oversample must be positive (got %r, %r)" % (kmax, oversample))
        if not (chimax > 0 and np.isfinite(chimax)):
            raise ValueError("the largest comoving distance must be positive (got %r)" % (chimax,))
        n = max(int(math.ceil(kmax * oversample * chimax / math.pi)), 1)
        k = np.linspace(0.0, kmax, n + 1)
        w = np.full(n + 1, kmax / n)
        w[0] = w[-1] = 0.5 * kmax / n
        g = np.zeros(n + 1)
        g[1:] = (2.0 / math.pi) * w[1:] * k[1:] ** 2 * np.asarray(self.ps_vv(k[1:]), dtype=np.float64)
        return k, g

    def _fullsky_plan(self, za_to_z, kmax=None, oversample=None):
        """The plan ``skysim.clarray`` runs the exact model by: ``prepare(za, zint, w)`` -> the arguments of
        ``Context.clarray_fullsky`` for the ``F zint`` sub-samples ``za`` with Romberg weights ``w`` [zint]."""
        self._fullsky_check()

        def prepare(za, zint, w):
            chi, pfd, f, b = self._z_quantities(za_to_z(np.asarray(za, dtype=np.float64)))
            k, g = self._fullsky_grid(float(np.max(chi)), kmax, oversample)
            wa = np.asarray(w, dtype=np.float64)[np.newaxis, :]
            shape = (-1, zint)
            return dict(k=k, g=g, chi=chi.reshape(shape), cb=wa * (pfd * b).reshape(shape), cf=wa * (pfd * f).reshape(shape))

        return dict(kind="fullsky", prepare=prepare)

    def angular_powerspectrum_full(self, la, za1, za2, kmax=None, oversample=None):
        r"""The angular power spectrum C_l(z1, z2) on the curved sky, calculated explicitly (corr.py:777-868), at broadcast
        points; a scalar in gives a float out.

        .. math:: C_l(z_1, z_2) = \frac{2}{\pi} D_1 D_2 p_1 p_2 \int_0^{k_{max}} k^2 P(k)
                  [b_1 j_l(k x_1) - f_1 j_l''(k x_1)] [b_2 j_l(k x_2) - f_2 j_l''(k x_2)] dk

        for a model with ``ps_vv`` only (an Exception with the reference's message otherwise); ``ps_2d`` and a non-zero
        ``_freq_window`` raise ValueError, and so does an ``l`` that is negative or not an integer.  The integral is the
        trapezoid rule on the grid of :meth:`_fullsky_grid` for the largest distance among the redshifts (``kmax``,
        ``oversample``: see there); the reference's piecewise adaptive scheme is not reproduced.  The per-redshift work is
        done on the unique redshifts; the table of radial functions is built once for them, all C_l[i, j] up to the
        largest l come from one Gram product per l on the device, and the requested (l, i, j) are gathered."""
        self._fullsky_check()
        la = np.asarray(la, dtype=np.float64)
        za1, za2 = np.asarray(za1, dtype=np.float64), np.asarray(za2, dtype=np.float64)
        if la.size and (not np.all(np.isfinite(la)) or np.any(la < 0) or np.any(la != np.round(la))):
            raise ValueError("angular_powerspectrum_full: l must be a non-negative integer")
        shape = np.broadcast(la, za1, za2).shape
        if la.size == 0 or za1.size == 0 or za2.size == 0:
            return np.zeros(shape)
        zu, inv = np.unique(np.concatenate([za1.ravel(), za2.ravel()]), return_inverse=True)
        chi, pfd, f, b = self._z_quantities(zu)
        k, g = self._fullsky_grid(float(np.max(chi)), kmax, oversample)
        i1 = inv[: za1.size].reshape(za1.shape)
        i2 = inv[za1.size :].reshape(za2.shape)
        import torch

        ctx = _lib.get_context()
        C = ctx.clarray_fullsky(k, g, chi, pfd * b, pfd * f, int(la.max()))

        def index(a):
            return torch.from_numpy(np.ascontiguousarray(np.broadcast_to(a, shape)).astype(np.int64).ravel()).to(ctx.device)

        res = C[index(la), index(i1), index(i2)].cpu().numpy().reshape(shape)
        return res if res.ndim else float(res)

    # ---- the aps callable ------------------------------------------------------------------
    def angular_powerspectrum_fft(self, la, za1, za2):
        """C_l(z1, z2) in the flat-sky limit, at broadcast points (corr.py:891-982)."""
        import torch

        ctx = _lib.get_context()
        dd, dv, vv = self._tables_on(ctx)
        la, za1, za2 = (np.asarray(v, dtype=np.float64) for v in (la, za1, za2))
        shape = np.broadcast(la, za1, za2).shape
        # per-redshift work on the unique redshifts only (chi is an ODE solve)
        zu, inv = np.unique(np.concatenate([za1.ravel(), za2.ravel()]), return_inverse=True)
        chi, pfd, f, b = self._z_quantities(zu)
        i1 = inv[: za1.size].reshape(za1.shape)
        i2 = inv[za1.size :].reshape(za2.shape)
        la = np.where(la == 0.0, 1e-10, la)

        def full(a):
            return np.array(np.broadcast_to(a, shape), dtype=np.float64, order="C").ravel()

        P = pfd[i1] * pfd[i2]
        args = [np.log10(la), chi[i1], chi[i2], b[i1] * b[i2] * P, (f[i1] * b[i2] + f[i2] * b[i1]) * P,
                f[i1] * f[i2] * P]
        dev = [torch.from_numpy(full(a)).to(ctx.device) for a in args]
        out = ctx.aps_table21cm_points(dd, dv, vv, self.kperpmin, self.kperpmax, self.kparmax, *dev)
        res = out.cpu().numpy().reshape(shape)
        return res if res.ndim else float(res)

    angular_powerspectrum = angular_powerspectrum_fft


def inverse_approx(f, x1, x2):
    """Spline of the inverse of a monotonic ``f`` sampled at 1000 points of [x1, x2] (corr.py:1053-1076)."""
    xa = np.linspace(x1, x2, 1000)
    return cs.Interpolater(f(xa), xa)
