"""Poisson processes on the host (counterpart of cora/foreground/poisson.py).

Setup-stage code in numpy on the package's cubic spline.  Every function draws from numpy's legacy global state in the
order the reference does, so that under ``np.random.seed(k)`` it consumes the same stream; the device population of
:mod:`cora_amd.foreground.pointsource` takes only the expected count and the inverse-CDF spline from here
(:func:`inverse_cdf`).
"""
import numpy as np
import numpy.random as rnd
from scipy.integrate import cumulative_trapezoid, quad
from scipy.optimize import fminbound

from ..util import cubicspline as cs

CDF_SAMPLES = 10000     # samples of the rate behind the inverse CDF (poisson.py:196)


def homogeneous_process(t, rate):
    """Event times in [0, t] of a Poisson process of constant ``rate`` (poisson.py:10-41): cumulative sums of
    exponential intervals, drawn in blocks until they pass ``t``."""
    iv = rnd.exponential(1.0 / rate, int(1.2 * rate * t + 1))
    n = int(0.4 * rate * t + 1)
    while iv.sum() < t:
        iv = np.concatenate((iv, rnd.exponential(1.0 / rate, n)))
    ts = np.cumsum(iv)
    return ts[:int(np.searchsorted(ts, [t])[0])]


def inhomogeneous_process(t, rate):
    """Event times in [0, t] of a Poisson process of variable ``rate(time)`` (poisson.py:76-132): 500 equal blocks, in
    each a homogeneous process at the block's highest rate thinned by ``rate / max``."""

    def block(dt, brate):
        rmax = brate(fminbound(lambda x: -brate(x), 0.0, dt))
        ut = homogeneous_process(dt, rmax)
        if ut.shape[0] == 0:
            return ut
        da = rnd.rand(ut.shape[0])
        ra = np.vectorize(brate)(ut)
        return ut[np.where(da < ra / rmax)]

    nbin = 500
    dt = t / (1.0 * nbin)
    iv = np.array([], dtype=np.float64)
    for i in range(nbin):
        tmin = i * t / (1.0 * nbin)
        iv = np.concatenate((iv, tmin + block(dt, lambda tr, tmin=tmin: rate(tr + tmin))))
    return iv


def expected_events(t, rate):
    """The mean number of events in [0, t]: the quadrature of ``rate`` (poisson.py:191)."""
    return quad(rate, 0.0, t)[0]


def inverse_cdf(t, rate):
    """Spline of the inverse of the normalised cumulative rate on [0, t] (poisson.py:196-204): its argument is a
    uniform deviate in [0, 1), its value an event time."""
    ts = np.linspace(0.0, t, CDF_SAMPLES)
    cumr = cumulative_trapezoid(rate(ts), ts, initial=0)
    cumr /= cumr[-1]
    return cs.Interpolater(cumr, ts)


def inhomogeneous_process_approx(t, rate):
    """Approximate, fast realisation of a variable-rate Poisson process (poisson.py:166-206): the number of events from
    a Poisson distribution about the integrated rate, each event the inverse CDF of a uniform deviate.  Not ordered in
    time."""
    total = np.random.poisson(expected_events(t, rate))
    return inverse_cdf(t, rate)(np.random.rand(total))
