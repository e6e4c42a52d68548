"""Counterpart of cora/signal/lssmodels.py: the redshift models a tracer simulation takes its per-slice numbers from.

Host code, O(nchi) work.  Three sets of polynomial models in ``(z - z0)`` - the Lagrangian bias ``bias``, the HI
density parameter ``omega_HI`` and the Finger-of-God velocity scale ``sigma_P`` - plus the mean 21 cm brightness
temperature and the effective number density of correlated shot noise.  The call surface is the reference's
(``bias["HI"](z)``, ``omega_HI.evaluate(z, model=...)``, ...), so that code written against it runs unchanged; the
coefficient tables are the published fits the reference cites, named below.  Every value is
``sum_i c_i (z - z0) ** p_i`` summed in table order, which is also the order the reference adds in
(tests/test_shotnoise_host.py compares with vectors made by the reference, tests/golden/make_golden_shotnoise.py).
"""
import numpy as np

from ..util import constants


class PolyModelSet:
    """A family of named models ``f(x) = sum_i coeff_i (x - x0) ** power_i``.

    A subclass provides ``_models``: name -> ``(x0, coeffs)`` (powers 0, 1, 2, ...) or ``(x0, coeffs, powers)``, and
    may name a ``default_model`` used when none is asked for.
    """

    _models = {}
    default_model = None

    @classmethod
    def _name(cls, model):
        if model is None:
            model = cls.default_model
            if model is None:
                raise ValueError("No model provided and no default specified.")
        if model not in cls._models:
            raise ValueError(f'Model "{model}" not known.')
        return model

    @classmethod
    def get(cls, model=None):
        """The model as a function of ``x`` (scalar or array)."""
        name = cls._name(model)
        return lambda x: cls.evaluate(x, model=name)

    def __class_getitem__(cls, model):
        return cls.get(model)

    @classmethod
    def evaluate(cls, x, model=None):
        """The values of ``model`` (None: the default) at ``x``."""
        return cls.evaluate_poly(x, *cls._models[cls._name(model)])

    @staticmethod
    def evaluate_poly(x, x0, coeffs, powers=None):
        """``sum_i coeffs[i] (x - x0) ** powers[i]``; ``powers`` None: 0, 1, 2, ...  The terms are stacked and summed
        along the new axis, in order."""
        if powers is None:
            powers = range(len(coeffs))
        return np.sum([c * (x - x0) ** p for p, c in zip(powers, coeffs)], axis=0)

    @classmethod
    def models(cls):
        """The names of the models, in table order."""
        return list(cls._models)


class bias(PolyModelSet):
    """LAGRANGIAN linear bias b_L(z) = b_E(z) - 1 of four tracers.

    ``eboss_qso``  quadratic fit to the eBOSS quasar subsamples, Laurent et al. 2017 (arXiv:1705.04718, eqs 5.2-5.3)
    ``eboss_lrg``  quadratic through the BOSS + eBOSS HOD model of Zhai et al. 2017 (arXiv:1607.05383, figure 12)
    ``eboss_elg``  b_E = 1.5 at z = 0.85 (de Mattia et al. 2020, arXiv:2007.09008) with the slope db/dz ~ 0.7 of the
                   simulations of Merson et al. 2019 (arXiv:1903.02030)
    ``HI``         quintic fit to the table of Castorina & Villaescusa-Navarro (arXiv:1609.05157, arXiv:1804.09180) as
                   published with the PUMA noise calculator

    >>> bias["HI"](1.0)
    0.489
    """

    _models = {
        "eboss_qso": (1.55, [1.38, 1.42, 0.278]),
        "eboss_lrg": (0.40, [1.03, 0.862, 0.131]),
        "eboss_elg": (0.85, [0.5, 0.7]),
        "HI": (1.0, [0.489, 0.460, -0.118, 0.0678, -0.0128, 0.0009]),
    }


class omega_HI(PolyModelSet):
    """Omega_HI(z).

    ``Crighton2015``  4e-4 (1 + z)^0.6 (arXiv:1506.02037); the default
    ``SKA``           the quadratic of the SKA cosmology red book (arXiv:1811.02743)
    ``uniform``       6e-4 at every redshift (Switzer et al. 2013, arXiv:1304.3712, with b_HI = 1)
    """

    _models = {
        "Crighton2015": (-1.0, [4e-4], [0.6]),
        "SKA": (0.0, [4.8e-4, 3.9e-4, -6.5e-5]),
        "uniform": (0.0, [0.6e-3]),
    }
    default_model = "Crighton2015"


class sigma_P(PolyModelSet):
    """Finger-of-God velocity dispersion scale in Mpc/h (for the squared-Lorentzian damping of ``fingers_of_god``).

    ``LRG``, ``ELG``, ``QSO``: normalised to the eBOSS measurements (arXiv:2007.08994, arXiv:2007.09008,
    arXiv:1801.03062), with the redshift dependence of a satellite-weighted halo velocity dispersion under the HODs
    of Alam et al. 2020 (arXiv:1910.05095); the ``...alt`` forms use the HODs of arXiv:1607.05383, arXiv:2007.09012 and
    arXiv:1812.05760 instead.  ``HI``: the Lorentzian-profile model of Sarkar & Bharadwaj 2019 (arXiv:1906.07032)
    times sqrt(2).
    """

    _models = {
        "HI": (1.0, [1.930, -1.479, 0.814]),
        "LRG": (0.70, [3.642, 0.019, -0.194]),
        "ELG": (0.85, [2.787, -0.774, 0.083]),
        "QSO": (1.48, [1.119, -0.138, -0.058]),
        "LRGalt": (0.70, [3.642, -0.469, -0.183]),
        "ELGalt": (0.85, [2.787, -0.780, 0.078]),
        "QSOalt": (1.48, [1.119, -0.007, -0.117]),
    }


def mean_21cm_temperature(c, z, omega_HI):
    """Mean 21 cm brightness temperature in K at redshift ``z`` for the HI density parameter ``omega_HI`` (values, not
    a model name) in cosmology ``c``: ``T0 (H(0) / H(z)) (1 + z)^2 h omega_HI``, with T0 = 191.06 mK from fundamental
    constants and the A_10 of Gould 1994 (ApJ 423, 522)."""
    T0 = 191.06e-3
    h = c.H0 / 100.0
    return T0 * (c.H(0) / c.H(z)) * (1 + z) ** 2 * h * omega_HI


def log_M_HI_g_to_n_eff(log_M_HI_g, c, z, model=None):
    """Effective number density in (Mpc/h)^-3 of the correlated shot noise of tracers that carry ``10**log_M_HI_g``
    solar masses of HI each: ``rho_HI(z) / M_HI`` with ``rho_HI = omega_HI(z) 3 H0^2 / (8 pi G)``; ``model`` names the
    ``omega_HI`` model (None: its default)."""
    h = c.H0 / 100
    H0_SI = c.H(0)
    omHI = omega_HI.evaluate(z, model=model)
    M_HI_g = (10**log_M_HI_g) * constants.solar_mass
    n_eff = (3.0 * omHI * H0_SI**2) / (8 * np.pi * constants.G * M_HI_g)     # 1 / m^3
    n_eff *= constants.mega_parsec**3 / h**3
    return n_eff
