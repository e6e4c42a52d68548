r"""LOFAR foreground model on the GPU.

API counterpart of cora/foreground/lofar.py: the Galactic diffuse synchrotron emission of Jelic et al. [1]_, the one
``Map3d`` foreground whose frequency structure comes from a spectral index per voxel and not from a covariance.  Two 3-d
Gaussian fields on an ``[x_num, y_num, numz]`` box - an amplitude ``A`` and a spectral index ``beta`` - are rescaled to
the model's standard deviations and summed along the line of sight,

    Tb[i, x, y] = sum_z A[x, y, z] (nu_i / nu_0) ** beta[x, y, z].

The fields come from :class:`~cora_amd.core.gaussianfield.RandomField` (device line FFTs), the standard deviations from
``Context.field_moments`` and the sum from ``Context.powerlaw_los`` (csrc/lofar.hip), which folds the two rescalings
in: nothing of the size of a field is written besides the fields themselves.

References
----------
.. [1] http://arxiv.org/abs/0804.1130
"""
import numpy as np

from .. import _lib
from ..core import gaussianfield, maps

# integer seeds: the second field (beta) is drawn with seed + this, modulo 2^64 (the 64-bit golden ratio: s and s + 1
# share no field, as they would with an increment of 1)
BETA_SEED_OFFSET = 0x9E3779B97F4A7C15


def beta_seed(seed):
    """Seed of the ``beta`` field of ``LofarGDSE.getfield(seed=int)``: ``(seed + BETA_SEED_OFFSET) mod 2^64``."""
    return (int(seed) + BETA_SEED_OFFSET) & (2**64 - 1)


class _LofarGDSE_3D(gaussianfield.RandomField):
    delta = -4.0

    def powerspectrum(self, karray):
        r"""Power law power spectrum ``|k|^delta``, zero at k = 0 (lofar.py:19-25)."""
        with np.errstate(divide="ignore"):
            ps = (karray**2).sum(axis=3) ** (self.delta / 2.0)
        ps[0, 0, 0] = 0.0
        return ps


class LofarGDSE(maps.Map3d):
    r"""LOFAR synchrotron model (lofar.py:28-73).

    A 3-d section of the galaxy with an independent power law emission at each point (separate amplitude and spectral
    index), integrated over the third axis into an angle-angle-frequency map.  ``correlated``: the spectral index field
    is the amplitude field (one draw) instead of a draw of its own.
    """

    nu_0 = 325.0

    correlated = False

    A_amp = 20
    A_std = A_amp * 0.02

    beta_mean = -2.55
    beta_std = 0.1

    alpha = -2.7

    _lf = None      # (geometry key, the 3-d field generator with its k-space weights)

    def _fields_device(self, seed=None):
        """The two raw fields (device, ``[x_num, y_num, numz rounded down to even]``) and ``numz``; ``beta is A`` when
        ``correlated``.  ``A`` is drawn first."""
        numz = int((self.x_num + self.y_num) // 2)
        npix = [self.x_num, self.y_num, numz]
        wsize = [5.0 / self.x_width, 5.0 / self.y_width, 1.0]
        # the k-space weights of the box are made on the host: kept while geometry and slope stay as they are
        key = (tuple(npix), tuple(wsize), float(self.alpha))
        if self._lf is None or self._lf[0] != key:
            lf = _LofarGDSE_3D(npix=npix, wsize=wsize)
            lf.delta = self.alpha
            self._lf = (key, lf)
        lf = self._lf[1]
        A = lf.getfield_device(seed=seed)
        if self.correlated:
            beta = A
        else:
            beta = lf.getfield_device(seed=None if seed is None else beta_seed(seed))
        return A, beta, numz

    def _los_device(self, A, beta, numz):
        """lofar.py:63-71 for raw device fields: ``[nu_num, x_num, y_num]`` on the device."""
        ctx = _lib.get_context()
        a_colstd, a_std, a_max = ctx.field_moments(A)
        b_std, b_max = (a_std, a_max) if beta is A else ctx.field_moments(beta)[1:]
        x = np.log(np.asarray(self.nu_pixels, dtype=np.float64) / self.nu_0)
        out = ctx.powerlaw_los(A, beta, x, a0=(1.0 * self.A_amp) / numz, sa=self.A_std / a_colstd, b0=self.beta_mean,
                               sb=self.beta_std / b_std, beta_absmax=b_max)
        return out.reshape(len(x), int(A.shape[0]), int(A.shape[1]))

    def getfield_device(self, seed=None):
        """One realisation as a device tensor ``[nu_num, x_num, y_num]``.

        ``seed=None`` follows the reference: the normals of both fields come from numpy's global state, ``A`` before
        ``beta`` (one draw when ``correlated``).  An integer ``seed`` (extension) draws both fields on the device from the
        Philox stream: ``A`` with ``seed``, ``beta`` with :func:`beta_seed` ``(seed)``."""
        A, beta, numz = self._fields_device(seed)
        return self._los_device(A, beta, numz)

    def getfield(self, seed=None):
        r"""Lofar synchrotron, numpy ``[nu_num, x_num, y_num]``."""
        return self.getfield_device(seed=seed).cpu().numpy()
