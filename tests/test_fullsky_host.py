"""Host checks of the exact curved-sky C_l (csrc/fullsky.hip, RedshiftCorrelation.angular_powerspectrum_full): the oracle
of tests/_fullsky_oracle.py pinned to a 40-digit recurrence, the quadrature grid against an adaptive integrator, the new
symbols and the argument rules.  The GPU is then held to the oracle in tests/test_gpu_fullsky.py."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import _fullsky_oracle as fo

LD = fo.LD

# (l, x): small and large arguments, both sides of the turning point, l = floor(x) and its neighbours
PIN_POINTS = [(0, 0.5), (1, 1e-3), (5, 0.1), (2, 1.0), (9, 10.0), (10, 10.0), (11, 10.0), (100, 200.0), (200, 100.0),
              (199, 200.5), (200, 200.5), (201, 200.5), (3070, 3071.0), (3071, 3071.0), (3072, 3071.0), (3071, 3072.5),
              (3072, 3072.5), (3073, 3072.5), (50, 5e3), (3000, 4.5e3)]


def _mp_jl(mp, lmax, x):
    """j_0 .. j_{lmax+1} at the float64 x by a downward recurrence at 40 digits (mpmath.besselj does not converge at
    these arguments), normalised to the larger of j_0 and j_1."""
    x = mp.mpf(float(x))
    M = max(float(x), lmax + 1)
    L = int(M + math.sqrt(400 * M) + 100)
    y1, y0 = mp.mpf(0), mp.mpf(1)
    out = [None] * (lmax + 2)
    for l in range(L, 0, -1):
        if l <= lmax + 1:
            out[l] = y0
        y0, y1 = (2 * l + 1) / x * y0 - y1, y0
    out[0] = y0
    j0 = mp.sin(x) / x
    j1 = mp.sin(x) / x ** 2 - mp.cos(x) / x
    s = j0 / out[0] if abs(j0) >= abs(j1) else j1 / out[1]
    return [v * s for v in out]


def test_oracle_pinned_to_mpmath():
    mp = pytest.importorskip("mpmath")
    with mp.workdps(40):
        worst = 0.0
        for l, x in PIN_POINTS:
            T = fo.jl_table_ld(l, [x])
            d2 = fo.jl_d2_ld(T, [x])
            m = _mp_jl(mp, l, x)
            xm = mp.mpf(float(x))
            md2 = (mp.mpf(l) * (l - 1) / xm ** 2 - 1) * m[l] + 2 / xm * m[l + 1]
            E = 1.0 / max(x, 1.0)
            ej = float(abs(mp.mpf(np.format_float_scientific(T[l, 0], precision=24)) - m[l])) / E
            ed = float(abs(mp.mpf(np.format_float_scientific(d2[l, 0], precision=24)) - md2)) / E
            print("l = %4d  x = %-8g  j_l: %.2e E   j_l'': %.2e E" % (l, x, ej, ed))
            worst = max(worst, ej, ed)
            assert ej <= 1e-17 and ed <= 1e-17, (l, x, ej, ed)
    print("worst %.3g of the envelope" % worst)


def test_oracle_zero_argument():
    T = fo.jl_table_ld(4, [0.0, 2.0])
    d2 = fo.jl_d2_ld(T, [0.0, 2.0])
    assert np.array_equal(T[:, 0], np.array([1, 0, 0, 0, 0, 0], dtype=LD))
    assert d2[0, 0] == -LD(1) / 3 and d2[2, 0] == LD(2) / 15 and not d2[[1, 3, 4], 0].any()
    # j_0''(x) = -j_0 + (2 / x) j_1 at x = 2, from the closed forms
    x = LD(2)
    j0, j1 = np.sin(x) / x, np.sin(x) / x ** 2 - np.cos(x) / x
    assert abs(T[0, 1] - j0) < 1e-18 and abs(d2[0, 1] - (2 / x * j1 - j0)) < 1e-18


def test_scheme_restated_in_float64_is_inside_its_tolerance():
    """The constants of the oracle module are what measure_scheme() gives (x 8), and below the cap of 1e-11."""
    wj, wd = fo.measure_scheme()
    print("float64 scheme, worst err / E: j_l %.3g, j_l'' %.3g" % (wj, wd))
    assert 0.9 * fo.TOL_J <= 8 * wj <= 1.1 * fo.TOL_J and 0.9 * fo.TOL_D2 <= 8 * wd <= 1.1 * fo.TOL_D2
    assert fo.TOL_J < 1e-11 and fo.TOL_D2 < 1e-11


# ---- the grid ----------------------------------------------------------------------------------------------------------

KSTAR = 0.5
CHI = np.array([40.0, 47.5, 61.0])
BIAS = np.array([1.0, 1.2, 0.9])
GROWTH = np.array([0.8, 0.75, 0.7])
GRID_L = (0, 1, 2, 5, 17, 40)


def _toy_trapezoid(lmax, oversample):
    k, w = fo.fullsky_grid(CHI.max(), 7 * KSTAR, oversample)
    g = fo.trapezoid_g(fo.toy_ps(KSTAR), k, w)
    case = dict(lmax=lmax, k=k, chi=CHI[:, None], cb=BIAS[:, None], cf=GROWTH[:, None])
    A, _ = fo.radial_table_ld(case)
    C, _ = fo.gram_ld(A, g)
    return C.astype(np.float64)


@pytest.fixture(scope="module")
def toy_quad():
    """C_l[i, j] of the toy model by scipy's adaptive integrator, l in GRID_L."""
    si = pytest.importorskip("scipy.integrate")
    sp = pytest.importorskip("scipy.special")
    ps = fo.toy_ps(KSTAR)

    def radial(l, i, k):
        x = k * CHI[i]
        jl, jl1 = sp.spherical_jn(l, x), sp.spherical_jn(l + 1, x)
        if x == 0.0:
            d2 = {0: -1.0 / 3.0, 2: 2.0 / 15.0}.get(l, 0.0)
        else:
            d2 = (l * (l - 1) / x ** 2 - 1.0) * jl + 2.0 / x * jl1
        return BIAS[i] * jl - GROWTH[i] * d2

    out = {}
    for l in GRID_L:
        C = np.zeros((3, 3))
        for i in range(3):
            for j in range(i, 3):
                f = lambda k: k * k * ps(k) * radial(l, i, k) * radial(l, j, k)
                v, _ = si.quad(f, 0.0, 7 * KSTAR, epsrel=1e-11, epsabs=0.0, limit=4000)
                C[i, j] = C[j, i] = 2.0 / math.pi * v
        out[l] = C
    return out


def test_grid_against_adaptive_quadrature(toy_quad):
    """The trapezoid rule with oversample = 4 on the toy model: at most 1e-5 (l = 0) and 1e-6 (l > 0) of max sqrt(C_ii C_jj)
    from the adaptive integral, and oversample = 8 is no further away."""
    C4, C8 = _toy_trapezoid(max(GRID_L), 4), _toy_trapezoid(max(GRID_L), 8)
    for l in GRID_L:
        q = toy_quad[l]
        scale = np.sqrt(np.outer(np.diag(q), np.diag(q))).max()
        d4, d8 = np.abs(C4[l] - q).max() / scale, np.abs(C8[l] - q).max() / scale
        print("l = %2d: oversample 4 -> %.3g, 8 -> %.3g" % (l, d4, d8))
        assert d4 <= (1e-5 if l == 0 else 1e-6), (l, d4)
        assert d8 <= d4, (l, d4, d8)


def test_model_grid_is_the_oracles():
    """RedshiftCorrelation._fullsky_grid: the same k and g as the oracle's grid, the defaults for kmax, P not called at 0."""
    from cora_amd.signal import corr, corr21cm

    seen = []

    def ps(k):
        seen.append(np.asarray(k).copy())
        return fo.toy_ps(0.02)(k)

    rc = corr.RedshiftCorrelation(ps_vv=ps, redshift=0.0)
    k, g = rc._fullsky_grid(2345.6, kmax=0.14)
    ko, wo = fo.fullsky_grid(2345.6, 0.14, 4)
    assert np.array_equal(k, ko) and np.allclose(g, fo.trapezoid_g(fo.toy_ps(0.02), ko, wo), rtol=1e-15, atol=0)
    assert len(seen) == 1 and seen[0].min() > 0 and g[0] == 0.0
    assert k[1] - k[0] <= math.pi / (4 * 2345.6) and k[-1] == 0.14
    k8, _ = rc._fullsky_grid(2345.6, kmax=0.14, oversample=8)
    assert np.array_equal(k8, fo.fullsky_grid(2345.6, 0.14, 8)[0]) and k8.size > 1.9 * k.size
    assert rc._fullsky_grid(10.0)[0][-1] == rc.kperpmax                 # a foreign spectrum: kperpmax
    cr = corr21cm.Corr21cm()
    assert cr._fullsky_grid(10.0)[0][-1] == 6 * cr._kstar               # the library's spline form: exp(-18) at the cut


# ---- symbols and arguments ---------------------------------------------------------------------------------------------

NAMES = ["corahip_sphbessel_radial", "corahip_cl_gram", "corahip_clarray_fullsky_workspace_bytes", "corahip_clarray_fullsky"]


def test_abi_symbols_present():
    from cora_amd import _lib

    lib = ctypes.CDLL(_lib.LIB_PATH)
    header = open(os.path.join(os.path.dirname(_lib._HERE), "include", "corahip.h")).read()
    minor = [line for line in header.splitlines() if line.startswith("#define CORAHIP_ABI_MINOR")]
    assert len(minor) == 1 and re.match(r"#define CORAHIP_ABI_MINOR 12\s", minor[0]) and lib.corahip_abi_minor() == 12
    for n in NAMES:
        assert n in _lib.SIGNATURES and hasattr(lib, n) and ("int %s(" % n) in header
        assert n[len("corahip_"):] in minor[0]
    assert [len(_lib.SIGNATURES[n][1]) for n in NAMES] == [11, 9, 4, 13]
    for m in ("sphbessel_radial", "cl_gram", "clarray_fullsky", "clarray_fullsky_chunk"):
        assert callable(getattr(_lib.Context, m))


def test_c_argument_checks_need_no_device():
    from cora_amd import _lib

    lib = ctypes.CDLL(_lib.LIB_PATH)
    for n in NAMES:
        getattr(lib, n).restype = ctypes.c_int
    L = ctypes.c_long
    assert lib.corahip_sphbessel_radial(None, None, 1, None, None, None, 1, 1, 0, L(1), None) == -1
    assert lib.corahip_cl_gram(None, None, None, 0, 1, 1, L(1), None, 0) == -1
    assert lib.corahip_clarray_fullsky(None, None, None, 1, None, None, None, 1, 1, 0, 16, None, None) == -1
    b = ctypes.c_size_t(0)
    ws = lib.corahip_clarray_fullsky_workspace_bytes
    assert ws(3, 5, 17, ctypes.byref(b)) == 0 and b.value == 4 * 5 * 32 * 8          # chunks are padded to 16 columns
    assert ws(2048, 256, 4096, ctypes.byref(b)) == 0 and b.value == 2049 * 256 * 4096 * 8 > 2 ** 32
    for bad in ((-1, 5, 16), (3, 0, 16), (3, 5, 0), (3, 70000, 16)):
        assert ws(*bad, ctypes.byref(b)) == -1, bad
    assert ws(3, 5, 16, None) == -1


def test_model_argument_errors():
    """Every rule is checked before a device is touched."""
    from cora_amd.signal import corr, corr21cm

    toy = fo.toy_ps(0.02)
    rc = corr.RedshiftCorrelation(ps_vv=toy, redshift=0.0)
    for bad in (-1, 2.5, [0, 1, -3], float("nan")):
        with pytest.raises(ValueError, match="non-negative integer"):
            rc.angular_powerspectrum_full(bad, 1.0, 1.0, kmax=0.14)
    full = corr.RedshiftCorrelation(ps_vv=toy, ps_dd=toy, ps_dv=toy)
    with pytest.raises(Exception, match="Only works for vv_only at the moment."):
        full.angular_powerspectrum_full(2, 1.0, 1.0)
    with pytest.raises(Exception, match="Only works for vv_only at the moment."):
        full._clarray_plan(full.angular_powerspectrum_full)
    rc2 = corr.RedshiftCorrelation(ps_vv=lambda k, mu: toy(k), redshift=0.0)
    rc2.ps_2d = True
    with pytest.raises(ValueError, match="ps_2d"):
        rc2.angular_powerspectrum_full(2, 1.0, 1.0)
    rc3 = corr.RedshiftCorrelation(ps_vv=toy, redshift=0.0)
    rc3._freq_window = 0.5
    with pytest.raises(ValueError, match="_freq_window"):
        rc3.angular_powerspectrum_full(2, 1.0, 1.0)
    with pytest.raises(ValueError, match="_freq_window"):
        rc3._clarray_plan(rc3.angular_powerspectrum_full)
    for kw in (dict(kmax=0.0), dict(kmax=-1.0), dict(kmax=0.14, oversample=0)):
        with pytest.raises(ValueError, match="must be positive"):
            rc._fullsky_grid(100.0, **kw)
    # the plans
    assert rc._clarray_plan(rc.angular_powerspectrum_full)["kind"] == "fullsky"
    assert rc._clarray_plan(rc.angular_powerspectrum)["kind"] == "table21cm"
    cr = corr21cm.Corr21cm(ps=toy, redshift=0.0)
    assert cr._clarray_plan(cr.angular_powerspectrum_full)["kind"] == "fullsky"
    assert cr._clarray_plan(cr.angular_powerspectrum)["kind"] == "table21cm"

    class Sub(corr.RedshiftCorrelation):
        def angular_powerspectrum_full(self, la, za1, za2):
            return 0.0

    sub = Sub(ps_vv=toy)
    assert sub._clarray_plan(sub.angular_powerspectrum_full) is None       # an override goes down the generic path


def test_plan_prepares_the_channel_average():
    """prepare(): chi, cb = w pf D b, cf = w pf D f on the [F, zint] sub-samples, the grid for the largest distance; in
    frequency for Corr21cm."""
    from cora_amd.core import skysim
    from cora_amd.signal import corr21cm
    from cora_amd.util import constants

    cr = corr21cm.Corr21cm(ps=fo.toy_ps(0.02), redshift=0.0)
    nu = np.array([[700.0, 701.0, 702.0], [710.0, 711.0, 712.0]]).ravel()
    w = skysim.romberg_weights(1)
    p = cr._clarray_plan(cr.angular_powerspectrum_full)["prepare"](nu, 3, w)
    z = constants.nu21 / nu - 1.0
    chi, pfd, f, b = cr._z_quantities(z)
    assert p["chi"].shape == p["cb"].shape == p["cf"].shape == (2, 3)
    assert np.array_equal(p["chi"], chi.reshape(2, 3))
    assert np.allclose(p["cb"], (np.tile(w, 2) * pfd * b).reshape(2, 3), rtol=1e-15, atol=0)
    assert np.allclose(p["cf"], (np.tile(w, 2) * pfd * f).reshape(2, 3), rtol=1e-15, atol=0)
    assert np.array_equal(p["k"], cr._fullsky_grid(chi.max())[0])
