"""Host side of the redshift-space correlation work: the oracle of tests/_rsdcorr_oracle.py against independent
evaluations (scipy, mpmath, a closed form, the reference's goldens), its bounds against five deliberate defects, and the
parts of the package that need no GPU (the ABI, argument checks, the loaders, the power spectra).

Measured on the CPU (the figures the assertions at 4 x rest on):

  multipole route against the closed form of P = k exp(-k^2), rnum 141 on 1e-1 .. 1e4, rswitch 10, six levels, four
  decades of padding, errors over the envelope, no point left out:
      direct part (r < 10)      l = 0, 2, 4     6.36e-13  6.36e-13  6.36e-13
      FFTLog part               l = 0, 2, 4     5.53e-5   2.47e-7   4.33e-8
    (l = 0: FFTLog at q = 0 is periodic in ln r; xi_0(r) carries the image of xi_0 thirteen decades below, about
    xi_0(0) 10^-19.5, against a tail of 1e-17 at r = 1e4.  With two decades of padding the figure was 54.6.)
  the oracle's table of the 21cm model against the table the reference ships, every row of 0.1 <= r <= 10 (285), largest
  difference relative to the column's largest magnitude there:
      xi_0, xi_2, xi_4          8.78e-7  8.14e-6  4.58e-6
    (outside: 0.4 % to 0.8 % at r = 30 .. 36, unrelated above r = 400 - printed, not asserted; the direct rows below
    r = 0.1 are not evaluated here.)
"""
import ctypes
import functools
import os

import numpy as np
import pytest

import _rsdcorr_oracle as ro

EPS = ro.EPS


def _f64(a):
    return np.asarray(a, dtype=np.float64)


# ---- j_l --------------------------------------------------------------------------------------------------------------
def test_jl_against_scipy_and_mpmath():
    """The oracle's j_l at 1e-6 .. 1e7 against scipy (whose own error is of the order of eps times the envelope
    1 / max(x, 1): 8 eps allowed) and, at 60 arguments around the switches, against mpmath at 30 digits (2^-60)."""
    import mpmath
    import scipy.special as ss

    x = np.logspace(-6, 7, 1301)
    mpmath.mp.dps = 30
    xs = np.concatenate([np.logspace(-3, 3, 40), [1.9, 2.0, 2.1, 2.9, 3.0, 3.1, 3.9, 4.0, 4.1, 5.9, 6.0, 6.1, 1e5, 1e6 + 0.5]])
    for l in ro.ORDERS:
        j = ro.jl(l, x)
        assert np.abs(_f64(j) - ss.spherical_jn(l, x)).max() <= 8 * EPS
        exact = np.array([float(mpmath.besselj(l + 0.5, mpmath.mpf(float(v))) * mpmath.sqrt(mpmath.pi / (2 * mpmath.mpf(float(v)))) - mpmath.mpf(float(ro.jl(l, np.array([v]))[0].astype(np.float64)))) for v in xs])
        # (the longdouble value is compared after rounding to double: half an ulp of |j_l| <= 1, plus 2^-60)
        assert np.abs(exact).max() <= 0.5 * EPS + 2.0**-60
    assert ro.jl(0, np.zeros(1))[0] == 1 and ro.jl(2, np.zeros(1))[0] == 0 and ro.jl(4, np.zeros(1))[0] == 0


def test_device_arithmetic_is_inside_the_evaluation_constant():
    """The device's formulas restated in double stay within C_l eps of the exact j_l on both sides of the switches, and
    the constants are the documented ones."""
    assert ro.jl_error_constant(0) == 4.0 and ro.jl_error_constant(2) == 9.75
    assert abs(ro.jl_error_constant(4) - 14.636) < 1e-3
    assert ro.jl_series_error(2, 2.0) < 1.0 and ro.jl_series_error(4, 4.0) < 2.0
    x = np.concatenate([np.logspace(-8, 6, 20001), np.nextafter([2.0, 2.0, 4.0, 4.0], [0, 9, 0, 9]), [0.0]])
    for l in ro.ORDERS:
        err = np.abs(_f64(ro.jl_device(l, x).astype(ro.LD) - ro.jl(l, x)))
        print("j_%d in double: worst error %.3g eps of %.4g allowed" % (l, err.max() / EPS, ro.jl_error_constant(l)))
        assert err.max() <= ro.jl_error_constant(l) * EPS


@functools.lru_cache(maxsize=None)
def _romb_case(k=8):
    rng = np.random.default_rng(77)
    ka = np.logspace(-5, 3, (1 << k) + 1)
    g = rng.standard_normal((2, ka.size))
    r = np.array([0.0, 1e-3, 0.05, 0.3, 1.0, 2.5, 30.0, 1e3])
    return g, ka, float(np.log(ka[1] / ka[0])), r


def test_jl_romb_oracle():
    """Masks, r = 0, the l = 0 slot against _pk2xi_oracle.sinc_romb, and the double restatement inside the bound."""
    import _pk2xi_oracle as po

    g, ka, dlk, r = _romb_case()
    val, bound = ro.jl_romb(g, ka, dlk, r, [0b111, 0b001])
    assert val.shape == bound.shape == (2, 3, r.size)
    assert np.all(val[1, 1:] == 0) and np.all(bound[1, 1:] == 0) and np.all(val[:, 1:, 0] == 0)
    for s in range(2):
        v0, b0 = po.sinc_romb(g[s], ka, dlk, r)
        assert np.all(val[s, 0] == v0) and np.allclose(bound[s, 0], b0, rtol=1e-15)
    dev, _ = ro.jl_romb(g, ka, dlk, r, [0b111, 0b001], defect="none")
    assert np.all(np.abs(_f64(dev - val)) <= bound)


@pytest.mark.parametrize("defect", ["switch", "term"])
def test_jl_bound_rejects(defect):
    """A series switch moved down to 2^-4, where the closed forms cancel, and a series without its x^4 term."""
    g, ka, dlk, r = _romb_case()
    val, bound = ro.jl_romb(g, ka, dlk, r)
    bad, _ = ro.jl_romb(g, ka, dlk, r, defect=defect)
    ratio = np.abs(_f64(bad - val))[:, 1:, 1:] / bound[:, 1:, 1:]
    print("defect %s: worst err / bound %.3g" % (defect, ratio.max()))
    assert ratio.max() > 1.0
    assert np.all(bad[:, 0] == ro.jl_romb(g, ka, dlk, r, defect="none")[0][:, 0])       # (l = 0 has no such defect)


# ---- xi(pi, sigma) ------------------------------------------------------------------------------------------------------
def _models():
    """The three objects of the goldens on the host: (tables, coefficient rows per redshift form)."""
    from cora_amd.signal import corr, corr21cm

    g = ro.load_golden()
    c21 = corr21cm.Corr21cm()
    mps = corr.RedshiftCorrelation(redshift=1.5, bias=2.0)
    fps = corr.RedshiftCorrelation(redshift=1.5)
    out = {}
    for name, obj, tab in (("c21", c21, g["table"]), ("mps", mps, g["table"]), ("fps", fps, g["table7"])):
        obj._vv_only = tab.shape[1] == 4
        obj._set_multipoles(tab[:, 0], [tab[:, i] for i in range(1, tab.shape[1])])
        out[name] = obj
    return g, out


ZFORMS = (("none", None, None), ("z1", 0.8, None), ("z12", 0.8, 1.1))


def _rows(obj, z1, z2):
    if z1 is None:
        z1 = obj.ps_redshift
    if z2 is None:
        z2 = z1
    return obj._z_coefficients(z1, z2)[0]


def test_xi_rsd_oracle_against_the_reference():
    """The oracle on the reference's tables at the 200 golden points (the origin, either component zero, negative pi,
    r outside the knots, r on a knot and one ulp to either side) for the three objects and three redshift forms: within
    twice the bound of the reference's results."""
    g, models = _models()
    worst = 0.0
    for name, obj in models.items():
        kx, ky, ky2 = obj._xi_knots
        for tag, z1, z2 in ZFORMS:
            val, bound = ro.xi_rsd(kx, ky, ky2, g["pi"], g["sigma"], _rows(obj, z1, z2))
            err = np.abs(_f64(val - g["xi_%s_%s" % (name, tag)].astype(ro.LD)))
            assert np.all(np.isfinite(_f64(val))) and np.all(err <= 2 * bound), (name, tag, (err / bound).max())
            worst = max(worst, (err / bound).max())
    print("oracle xi_rsd against the reference: worst err / bound %.3g" % worst)


@pytest.mark.parametrize("defect", ["p4", "47", "clamp"])
def test_xi_rsd_bound_rejects(defect):
    """P_4 with the constant 2 for 3, 4/7 replaced by 4/5, extrapolation replaced by clamping: each is outside twice the
    bound of the reference's results somewhere."""
    g, models = _models()
    obj = models["fps"]
    kx, ky, ky2 = obj._xi_knots
    val, bound = ro.xi_rsd(kx, ky, ky2, g["pi"], g["sigma"], _rows(obj, 0.8, 1.1), defect=defect)
    err = np.abs(_f64(val - g["xi_fps_z12"].astype(ro.LD)))
    print("defect %s: worst err / bound %.3g, %d points outside" % (defect, (err / bound).max(), np.count_nonzero(err > 2 * bound)))
    assert np.any(err > 2 * bound)


# ---- the multipole route ------------------------------------------------------------------------------------------------
RA_PAIR = np.logspace(-1, 4, 141)


@functools.lru_cache(maxsize=None)
def pair_multipoles():
    return ro.multipoles(ro.pk_gauss, (0, 2, 4), RA_PAIR)


def test_multipole_route_against_the_closed_form():
    """P = k exp(-k^2): xi_l in closed form (1F1, mpmath at 30 digits).  Errors over the envelope, no point left out,
    asserted at 4 x the figures of the module docstring."""
    val, bound = pair_multipoles()
    nlow = ro.multipole_grids(RA_PAIR)[0]
    assert nlow == 56 and np.all(np.isfinite(val)) and np.all(bound > 0)
    measured = {0: (6.36e-13, 5.53e-5), 2: (6.36e-13, 2.47e-7), 4: (6.36e-13, 4.33e-8)}
    for n, l in enumerate((0, 2, 4)):
        rel = np.abs(val[n] - ro.xi_gauss(l, RA_PAIR)) / ro.xi_gauss(l, RA_PAIR, envelope=True)
        print("l = %d of the envelope: direct %.3g, FFTLog %.3g, below 1e3 %.3g"
              % (l, rel[:nlow].max(), rel[nlow:].max(), rel[nlow:][RA_PAIR[nlow:] < 1e3].max()))
        assert rel[:nlow].max() <= 4 * measured[l][0]
        assert rel[nlow:].max() <= 4 * measured[l][1]


def test_oracle_table_against_the_shipped_one():
    """The multipoles of the 21cm model's spectrum by the oracle's route on the reference's grid against the table the
    reference ships, for 0.1 <= r <= 10 (its integrals ran to epsrel 1e-7 between 1e-4 pi / r and 1e3 pi / r): at 4 x the
    figures of the module docstring, per column relative to the column's largest magnitude there."""
    from cora_amd.signal import corr21cm

    tab = ro.load_golden()["table"]
    ra = np.logspace(-3, 4, 1000)
    assert np.allclose(tab[:, 0], ra, rtol=1e-15)
    sel = np.flatnonzero((ra >= 0.1) & (ra <= 10))
    rows = sel                                   # every row of the range
    val, _ = ro.multipoles(corr21cm.Corr21cm().ps_vv, (0, 2, 4), ra, rows=rows)
    far = np.flatnonzero(ra >= 10)
    for n, m in enumerate((8.78e-7, 8.14e-6, 4.58e-6)):
        col = tab[:, n + 1]
        scale = np.abs(col[sel]).max()
        d = np.abs(val[n] - col)
        print("xi_%d: 0.1 <= r <= 10 worst %.3g of the column's %.3g; relative at r = 30, 36, 100, 400, 1e3, 1e4: %s"
              % (2 * n, d[rows].max() / scale, scale,
                 " ".join("%.2g" % (d[i] / abs(col[i])) for i in (np.argmin(np.abs(ra - x)) for x in (30, 36, 100, 400, 1e3, 1e4)))))
        assert np.all(np.isfinite(val[n][rows])) and np.all(np.isfinite(val[n][far]))
        assert d[rows].max() / scale <= 4 * m


def test_multipole_grids():
    """Level 0 is 1 / ra reversed, continued by whole steps; every level length splits; a length that cannot: ValueError
    before anything else happens."""
    from cora_amd.signal import corrfunc

    for ra, kw in ((RA_PAIR, {}), (np.logspace(-3, 4, 1000), {}), (np.logspace(0, 2, 30), dict(richardson_n=3, pad_decades=0.5))):
        nlow, npad, N0, kfine = ro.multipole_grids(ra, **kw)
        plan = corrfunc._MultipolePlan(ra, **kw)
        umax = 2 ** (kw.get("richardson_n", 6) - 1)
        assert (plan.nlow, plan.npad, plan.n) == (nlow, npad, N0) and np.array_equal(plan.kfine, kfine)
        k0 = kfine[::umax]
        assert np.array_equal(k0[npad:npad + ra.size], 1.0 / ra[::-1]) and N0 - ra.size - npad >= npad
        assert np.allclose(np.diff(np.log(kfine)), np.log(ra[1] / ra[0]) / umax, rtol=1e-6)
        assert all(ro.splits(N0 * 2**ii) for ii in range(len(plan.splits)))
    assert np.array_equal(corrfunc._MultipolePlan(np.logspace(-3, 4, 1000)).kdirect, ro.direct_grid()[0])
    assert not ro.splits(3 * 4099) and ro.splits(2142 * 32)
    with pytest.raises(ValueError, match="Richardson levels"):
        corrfunc._MultipolePlan(np.logspace(-3, 4, 1000), richardson_n=16)
    with pytest.raises(ValueError, match="logarithmically"):
        corrfunc._MultipolePlan(np.linspace(1, 2, 10))
    with pytest.raises(ValueError, match="orders are 0, 2 and 4"):
        corrfunc.ps_to_multipoles([ro.pk_gauss], [(1,)], RA_PAIR)


# ---- the package --------------------------------------------------------------------------------------------------------
def test_abi_symbols_present():
    from cora_amd import _lib

    lib = ctypes.CDLL(_lib.LIB_PATH)
    header = open(os.path.join(os.path.dirname(_lib._HERE), "include", "corahip.h")).read()
    minor_line = header.split("#define CORAHIP_ABI_MINOR")[1].split("\n")[0]
    assert minor_line.startswith(" 12 ") and "and (redshift-space correlation) jl_romb, xi_rsd" in minor_line
    assert lib.corahip_abi_minor() == 12
    for n in ("corahip_jl_romb", "corahip_xi_rsd"):
        assert n in _lib.SIGNATURES and hasattr(lib, n) and ("int %s(" % n) in header
    for m in ("jl_romb", "xi_rsd"):
        assert callable(getattr(_lib.Context, m))


def test_argument_checks_return_einval():
    """The range checks come before anything is dereferenced: with stand-in pointers the calls return CORAHIP_EINVAL and
    name the argument; with every argument in range the same stand-ins pass the range checks (jl_romb with nr = 0 and
    xi_rsd with n = 0 return 0 without touching anything)."""
    from cora_amd import _lib

    lib = _lib.load()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, _lib.PTR)
    ctx = ctypes.cast(buf, ctypes.c_void_p)
    masks = (ctypes.c_int * 3)(7, 7, 7)

    def err():
        return lib.corahip_last_error().decode()

    assert lib.corahip_jl_romb(ctx, p, 1, masks, p, 4, 0.1, p, 0, p) == 0
    for nspec, k in ((0, 4), (4, 4), (1, 0), (1, 25)):
        assert lib.corahip_jl_romb(ctx, p, nspec, masks, p, k, 0.1, p, 0, p) == -1 and "nspec" in err()
    bad = (ctypes.c_int * 3)(8, 7, 7)
    assert lib.corahip_jl_romb(ctx, p, 1, bad, p, 4, 0.1, p, 0, p) == -1
    assert lib.corahip_xi_rsd(ctx, p, p, p, 4, 3, p, p, 0, p, 1, p) == 0
    for nfun in (0, 1, 2, 4, 5, 7):
        assert lib.corahip_xi_rsd(ctx, p, p, p, 4, nfun, p, p, 0, p, 1, p) == -1 and "nfun" in err()
    assert lib.corahip_xi_rsd(ctx, p, p, p, 3, 3, p, p, 0, p, 1, p) == -1 and "nk = 3" in err()
    assert lib.corahip_xi_rsd(ctx, p, p, p, (1 << 24) + 1, 6, p, p, 0, p, 1, p) == -1 and "nk" in err()
    for ncoef in (0, -1):
        assert lib.corahip_xi_rsd(ctx, p, p, p, 4, 6, p, p, 0, p, ncoef, p) == -1 and "ncoef" in err()
    assert lib.corahip_xi_rsd(None, p, p, p, 4, 6, p, p, 0, p, 1, p) == -1 and "ctx" in err()


def test_loaders(tmp_path):
    """Signatures, attributes and exception strings of the reference's loaders."""
    from cora_amd.signal import corr
    from cora_amd.util import cubicspline

    g = ro.load_golden()
    with pytest.raises(Exception, match="^Cache file does not exist.$"):
        corr.RedshiftCorrelation.from_file_matterps(str(tmp_path / "absent.dat"))
    f4, f7 = str(tmp_path / "t4.dat"), str(tmp_path / "t7.dat")
    np.savetxt(f4, g["table"])
    np.savetxt(f7, g["table7"])
    with pytest.raises(Exception, match="^Cache file has wrong number of columns.$"):
        corr.RedshiftCorrelation.from_file_fullps(f4)
    assert corr.RedshiftCorrelation()._cached is False
    a = corr.RedshiftCorrelation.from_file_matterps(f4, redshift=1.5, bias=2.0)
    b = corr.RedshiftCorrelation.from_file_fullps(f7, redshift=1.5)
    c = corr.RedshiftCorrelation.from_file_matterps(f7)                   # (the reference reads the first four columns)
    assert a._cached and b._cached and a._vv_only and not b._vv_only and a.bias == 2.0 and a.ps_redshift == 1.5
    for obj, names, tab in ((a, corr.RedshiftCorrelation._MULTIPOLES[:3], g["table"]), (b, corr.RedshiftCorrelation._MULTIPOLES, g["table7"]),
                            (c, corr.RedshiftCorrelation._MULTIPOLES[:3], g["table"])):
        for i, name in enumerate(names):
            sp = getattr(obj, name)
            assert isinstance(sp, cubicspline.Interpolater) and np.array_equal(sp._data, tab[:, [0, i + 1]])
        kx, ky, ky2 = obj._xi_knots
        assert ky.shape == ky2.shape == (len(names), 1000) and np.array_equal(kx, tab[:, 0])
        assert np.array_equal(ky[2], tab[:, 3]) and np.array_equal(ky2[0], obj._vv0i._y2)
    assert not hasattr(a, "_dd0i")
    assert b._dd0i(1.0) == pytest.approx(float(np.interp(1.0, g["table7"][:, 0], g["table7"][:, 4])), abs=1e-3)


def test_corr21cm_builds_no_cache_at_construction():
    from cora_amd.signal import corr21cm

    c = corr21cm.Corr21cm()
    assert c._cached is False and not hasattr(c, "_vv0i")
    for name in ("get_pwrspec", "get_kiyo_field_physical", "redshiftspace_correlation", "angular_correlation", "gen_cache"):
        assert callable(getattr(c, name))


def test_powerspectrum_against_the_reference():
    """The three branches of ``powerspectrum`` and ``powerspectrum_1D`` against the reference: 4 ulp of the largest term."""
    from cora_amd.signal import corr, corr21cm

    g = ro.load_golden()
    vv = corr.RedshiftCorrelation(ps_vv=ro.ps_vv, redshift=1.5, bias=2.0)
    full = corr.RedshiftCorrelation(ps_vv=ro.ps_vv, ps_dd=ro.ps_dd, ps_dv=ro.ps_dv, redshift=1.5)
    two = corr.RedshiftCorrelation(ps_vv=ro.ps_vv2d, redshift=1.5, bias=2.0)
    two.ps_2d = True
    kpar, kperp = g["kpar"], g["kperp"]
    k = (kpar**2 + kperp**2) ** 0.5
    mu2 = kpar**2 / k**2

    def largest_term(o, z1, z2):
        z1 = o.ps_redshift if z1 is None else z1
        z2 = o.ps_redshift if z2 is None else z2
        b1, b2, f1, f2 = o.bias_z(z1), o.bias_z(z2), o.growth_rate(z1), o.growth_rate(z2)
        pre = (o.growth_factor(z1) * o.growth_factor(z2) / o.growth_factor(o.ps_redshift) ** 2 * o.prefactor(z1) * o.prefactor(z2))
        if o._vv_only:
            pvv = o.ps_vv(k, kpar / k) if o.ps_2d else o.ps_vv(k)
            terms = [pvv * b1 * b2, pvv * mu2 * f1 * b2, pvv * mu2 * f2 * b1, pvv * mu2**2 * f1 * f2]
        else:
            terms = [b1 * b2 * o.ps_dd(k), mu2 * o.ps_dv(k) * (f1 * b2 + f2 * b1), mu2**2 * f1 * f2 * o.ps_vv(k)]
        return pre * np.max(np.abs(terms), axis=0)

    for name, o in (("vv", vv), ("full", full), ("2d", two)):
        for tag, z1, z2 in (("none", None, None), ("z12", 0.8, 1.1)):
            got = o.powerspectrum(kpar, kperp, z1, z2)
            ref = g["ps_%s_%s" % (name, tag)]
            assert got.shape == ref.shape == (7, 5) and np.all(ref != 0)
            assert np.all(np.abs(got - ref) <= 4 * EPS * largest_term(o, z1, z2)), (name, tag)
    c21 = corr21cm.Corr21cm()
    got = c21.powerspectrum_1D(g["k1d"], 0.8, 1.1, 16)
    assert np.all(np.abs(got - g["ps1d"]) <= 4 * EPS * np.abs(g["ps1d"])) and np.all(g["ps1d"] > 0)
    assert np.array_equal(vv.powerspectrum(kpar, kperp, np.array(0.8), np.array(1.1)), vv.powerspectrum(kpar, kperp, 0.8, 1.1))
