"""Host side of the polarised spectra and of ``lssutil.laplacian`` (no GPU): call surfaces, the field-major index rule,
the errors that are decided before any device work, the new symbol, and the merged radial stencil of the Laplacian
against a numpy restatement (tests/_laplacian_oracle.py)."""
import inspect
import os
import re

import numpy as np
import pytest

import _laplacian_oracle as lo
from cora_amd import _lib
from cora_amd.core import skysim
from cora_amd.signal import lssutil
from cora_amd.util import hputil

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = np.finfo(np.float64).eps


def _params(f):
    return [(p.name, p.default) for p in inspect.signature(f).parameters.values()]


def test_signatures():
    E = inspect.Parameter.empty
    assert hputil.SKY_CHUNK == 16
    assert _params(hputil.map2alm_sky_device) == [("maps", E), ("lmax", None), ("use_weights", None), ("niter", None),
                                                  ("chunk", hputil.SKY_CHUNK)]
    assert _params(hputil.map2alm_sky_bytes) == [("nside", E), ("lmax", E), ("npol", E), ("chunk", hputil.SKY_CHUNK)]
    assert _params(hputil.cross_spectra_pol_device) == [("maps", E), ("maps2", None), ("lmax", None), ("use_weights", None),
                                                        ("niter", None)]
    assert _params(hputil.anafast_pol) == [("map1", E), ("map2", None), ("lmax", None), ("iter", 3), ("use_weights", False)]
    assert _params(skysim.clarray_from_maps) == [("maps", E), ("lmax", None), ("niter", None), ("use_weights", None)]
    assert _params(lssutil.laplacian) == [("maps", E), ("x", E), ("lmax", None), ("niter", 3)]
    assert _params(lssutil.laplacian_device) == [("maps", E), ("x", E), ("out", None), ("lmax", None), ("niter", 3),
                                                 ("chunk", lssutil.SLICE_CHUNK)]
    assert _params(lssutil.laplacian_bytes) == [("nside", E), ("lmax", E), ("chunk", lssutil.SLICE_CHUNK)]
    assert _params(_lib.Context.alm_gather_channels)[1:] == [("src", E), ("nsrc", E), ("idx", E), ("dst", E), ("ndst", E),
                                                             ("dst_first", 0)]
    assert _params(_lib.Context.slice_diff2)[1:] == [("f", E), ("x", E), ("g", None), ("h", None), ("s", None), ("t", None),
                                                     ("out", None), ("coef", None)]
    assert "anafast_pol" in hputil.anafast.__doc__


def test_gather_symbol_is_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "corahip.h")).read()
    assert re.search(r"\bint corahip_alm_gather_channels\(corahip_ctx \*ctx, const double \*src, int nsrc, const int32_t \*idx,"
                     r" int n, int lmax,\s+double \*dst, int ndst, int dst_first\);", header)
    assert "alm_gather_channels" in header.split("#define CORAHIP_ABI_MINOR")[1].split("\n")[0]
    res, args = _lib.SIGNATURES["corahip_alm_gather_channels"]
    assert res is _lib.c_int and len(args) == 9
    assert hasattr(_lib.load(), "corahip_alm_gather_channels")


def test_field_major_index_rule():
    F = 5
    assert hputil.sky_channel(0, 0, F) == 0 and hputil.sky_channel(1, 0, F) == F and hputil.sky_channel(2, 4, F) == 14
    p, f = np.meshgrid(np.arange(4), np.arange(F), indexing="ij")
    assert np.array_equal(hputil.sky_channel(p, f, F).ravel(), np.arange(4 * F))          # = reshape(P, F) of the channel axis


def test_anafast_still_refuses_pol_and_names_anafast_pol():
    with pytest.raises(NotImplementedError) as e:
        hputil.anafast(np.zeros((3, 48)), pol=True)
    assert "anafast_pol" in str(e.value)


@pytest.mark.parametrize("shape", [(48,), (2, 2, 3, 48)])
def test_wrong_rank(shape):
    import torch

    with pytest.raises(ValueError):
        skysim.clarray_from_maps(np.zeros(shape))
    with pytest.raises(ValueError):
        skysim.clarray_from_maps(torch.zeros(shape, dtype=torch.float64))
    with pytest.raises(ValueError):
        hputil.map2alm_sky_device(torch.zeros(shape, dtype=torch.float64))
    with pytest.raises(ValueError):
        hputil.cross_spectra_pol_device(torch.zeros(shape, dtype=torch.float64))


@pytest.mark.parametrize("npol", [2, 5])
def test_wrong_number_of_polarisation_components(npol):
    import torch

    host = np.zeros((2, npol, 48))
    dev = torch.zeros((2, npol, 48), dtype=torch.float64)
    for call in (lambda: skysim.clarray_from_maps(host), lambda: skysim.clarray_from_maps(dev),
                 lambda: hputil.map2alm_sky_device(dev), lambda: hputil.cross_spectra_pol_device(dev),
                 lambda: hputil.cross_spectra_pol_device(torch.zeros((2, 3, 48), dtype=torch.float64), dev)):
        with pytest.raises(Exception) as e:
            call()
        assert type(e.value) is Exception and str(e.value) == "Wrong number of polarisation components."


def test_bad_pixel_counts_and_anafast_pol_shapes():
    import torch

    with pytest.raises(ValueError):
        skysim.clarray_from_maps(np.zeros((2, 3, 50)))                      # not 12 nside^2
    with pytest.raises(ValueError):
        hputil.map2alm_sky_device(torch.zeros((2, 3, 50), dtype=torch.float64))
    for bad in (np.zeros((2, 48)), np.zeros(48), np.zeros((1, 3, 48)), np.zeros((4, 48)), np.zeros((3, 50))):
        with pytest.raises(ValueError):
            hputil.anafast_pol(bad)
    with pytest.raises(ValueError):
        hputil.anafast_pol(np.zeros((3, 48)), np.zeros((3, 192)))


def test_laplacian_errors_before_device_work():
    with pytest.raises(ValueError) as e:
        lssutil.laplacian(np.zeros((3, 48)), np.arange(3.0) + 1)
    assert "at least 4" in str(e.value)
    with pytest.raises(ValueError):
        lssutil.laplacian(np.zeros((5, 48)), np.arange(4.0) + 1)             # x of the wrong length
    with pytest.raises(ValueError):
        lssutil.laplacian(np.zeros((5, 50)), np.arange(5.0) + 1)             # not a HEALPix map
    with pytest.raises(ValueError):
        lssutil.laplacian(np.zeros((5, 2, 48)), np.arange(5.0) + 1)
    with pytest.raises(ValueError):
        lssutil.laplacian_coefficients(np.arange(3.0) + 1)


def _coords(kind, n):
    rng = np.random.default_rng(n)
    if kind == "uniform":
        return 150.0 + 3.0 * np.arange(n)
    steps = np.cumsum(rng.uniform(2.0, 6.0, n))
    return 200.0 + steps if kind == "nonuniform" else 400.0 - steps


@pytest.mark.parametrize("kind", ["uniform", "nonuniform", "descending"])
@pytest.mark.parametrize("n", [4, 5, 9])
def test_merged_laplacian_coefficients(n, kind):
    """coef[i, k] = d_k + (2 / x_i) g_k over the rows first[i] .. first[i] + 3 against the restatement from Lagrange weights
    and np.gradient.  Tolerance 4 eps (|d_k| + |2 g_k / x_i|): each side forms d_k (a few roundings from the spacings),
    g_k, 2 g_k / x and one sum; the largest ratio measured over these nine cases is 1.4."""
    x = _coords(kind, n)
    coef = lssutil.laplacian_coefficients(x)
    ref, mag = lo.radial_weights(x)
    assert coef.shape == (n, 4) and np.array_equal(lo.first_rows(n), _lib.Context.diff2_coefficients(x)[1])
    assert np.array_equal(coef[mag == 0], ref[mag == 0])                     # an entry without terms is an exact zero
    r = (np.abs(coef - ref)[mag > 0] / (EPS * mag[mag > 0])).max()
    print("merged coefficients n %d %s: worst err / (eps magnitude) %.3g" % (n, kind, r))
    assert r <= 4.0
    # the table is a second-derivative-plus-(2/x)-first-derivative stencil: exact on 1, x, x^2 up to rounding of the sum
    first = lo.first_rows(n)
    for p, want in ((0, np.zeros(n)), (1, 2.0 / x), (2, 6.0 * np.ones(n))):
        f = x ** p
        got = np.array([coef[i] @ f[first[i]:first[i] + 4] for i in range(n)])
        if p == 2:                       # np.gradient is first order on the end rows: exact for x^2 inside only
            got, want = got[1:-1], want[1:-1]
        scale = np.array([mag[i] @ np.abs(f[first[i]:first[i] + 4]) for i in range(n)])
        scale = scale[1:-1] if p == 2 else scale
        assert (np.abs(got - want) <= 16 * EPS * scale).all(), (p, kind, n)
