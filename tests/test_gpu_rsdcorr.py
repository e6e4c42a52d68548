"""The redshift-space correlation kernels called directly - ctx.jl_romb (cora_amd/csrc/pk2xi.hip), ctx.xi_rsd
(cora_amd/csrc/rsdcorr.hip) - the multipole route ``corrfunc.ps_to_multipoles`` end to end and the public calls of
``RedshiftCorrelation`` / ``Corr21cm``, held to the derived bounds of tests/_rsdcorr_oracle.py.  Every output is filled
with a NaN byte pattern first; each test prints its worst err / bound.  tests/test_rsdcorr_host.py shows that the same bounds
reject five deliberate defects.  Run with -m gpu.

Observed on the MI355X (worst err / bound; the constants are derived in the oracle, none was fitted):

  jl_romb, k = 1 / 2 / 5 / 8 / 16, nr = 257, three integrands   l = 0: 0.076 / 0.043 / 0.017 / 0.0043 / 0.00011
                                                                l = 2: 0.022 / 0.0040 / 0.0013 / 0.00030 / 0.0000086
                                                                l = 4: 0.011 / 0.0019 / 0.00053 / 0.00015 / 0.0000039
  jl_romb, nr = 1 (r = 1e3: k r up to 1e6), three integrands    l = 0: 0.0069 / 0.036 / 0.0021 / 0.00077 / 0.000040
                                                                l = 2, 4: below 0.00031
    (every l = 0 slot has the bits of sinc_romb, every cleared slot and the l = 2, 4 slots at r = 0 are +0.0)
  fftlog_phase, mu = 4.5, eta to 3.5e5 / fine steps / N = 700   0.23 / 0.18 / 0.16
  ps_to_multipoles, l = 0 / 2 / 4, levels 255 .. 8160           direct part 0.0016 / 0.00076 / 0.00019, FFTLog part
                                                                0.00033 / 0.00022 / 0.00028; against the closed form, of
                                                                the envelope: direct 6.4e-13 each, FFTLog 55 / 7.7e-7 / 9.1e-8
  xi_rsd, golden points, 21cm model / matter file / full file   0.21 / 0.17 / 0.21; against the reference 0.26 / 0.29 / 0.16
  xi_rsd, synthetic, n = 100 003, nk 4 / 4097                   0.26 / 0.19 (n = 1: below 0.04)
  redshiftspace_correlation against the reference               0.29 at the most; angular_correlation 0.11
  Corr21cm table against the shipped one, 0.1 <= r <= 10        xi_0 / xi_2 / xi_4: 4.3e-7 / 2.0e-6 / 3.3e-6 of the column's largest on
                                                                the rows of the host figures (all rows: 8.8e-7 / 8.1e-6 / 4.6e-6)

The Romberg bounds are worst-case sums over 2^k samples, which random roundings stay far below; the spline bound is
dominated by the 4 eps of each linear term.
"""
import functools

import numpy as np
import pytest

import _pk2xi_oracle as po
import _rsdcorr_oracle as ro

pytestmark = pytest.mark.gpu


def _poisoned(ctx, shape, dtype=None):
    import torch

    t = ctx.empty(shape, dtype=dtype)
    t.view(torch.uint8).fill_(0xFF)            # every double a NaN: an element the kernel does not write shows
    return t


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _same_bits(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _romb_case(k, nr, nspec):
    """_romb_case of test_gpu_pk2xi.py for nspec integrands; the separations of nr = 257 include 0, pairs that put
    ka r on both sides of each order's switch (2 and 4) within one separation, and 1e3 (arguments to 1e6)."""
    rng = np.random.default_rng(100 * k + nr)
    ka = np.logspace(-5, 3, (1 << k) + 1)
    g = rng.standard_normal((nspec, ka.size))
    if nr == 1:
        r = np.array([1e3])
    else:
        r = np.concatenate([[0.0, 2.0 / ka[ka.size // 2], 4.0 / ka[ka.size // 2], 2e-3, 4e-3, 3.0, 1e3], np.logspace(-1, 3, nr - 7)])
    return g, ka, float(np.log(ka[1] / ka[0])), r


@functools.lru_cache(maxsize=None)
def _romb_reference(k, nr):
    """The oracle for three integrands and every order, once per (k, nr): the case with one integrand has the first of the
    three (the same random stream), a cleared slot is zero with a zero bound.  (k = 16, nr = 257 is 5e7 extended-precision
    sines and cosines: the one slow reference of this file, shared by its two cases.)"""
    g, ka, dlk, r = _romb_case(k, nr, 3)
    return ro.jl_romb(g, ka, dlk, r)


@pytest.mark.parametrize("nspec,lmask", [(1, (0b111,)), (3, (0b111, 0b001, 0b011))])
@pytest.mark.parametrize("nr", [1, 257])
@pytest.mark.parametrize("k", [1, 2, 5, 8, 16])
def test_jl_romb(ctx, k, nr, nspec, lmask):
    """Random g: every slot against the longdouble Romberg sum over the exact j_l; cleared slots and the l = 2, 4 slots at
    r = 0 are +0.0; the l = 0 slot has the bits of ctx.sinc_romb; a second call returns the same bits."""
    import torch

    g, ka, dlk, r = _romb_case(k, nr, nspec)
    d = ctx.to_device
    out = _poisoned(ctx, (nspec, 3, r.size))
    ctx.jl_romb(d(g), d(ka), dlk, d(r), lmask, out=out)
    again = ctx.jl_romb(d(g), d(ka), dlk, d(r), lmask)
    sinc = [ctx.sinc_romb(d(g[s]), d(ka), dlk, d(r)).cpu().numpy() for s in range(nspec)]
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert np.array_equal(g, _romb_case(k, nr, 3)[0][:nspec])
    val, bound = (v[:nspec].copy() for v in _romb_reference(k, nr))
    for s in range(nspec):
        for i in range(3):
            if not (lmask[s] >> i) & 1:
                val[s, i], bound[s, i] = 0, 0.0
    err = np.abs((got.astype(ro.LD) - val).astype(np.float64))
    on = bound > 0
    ratio = [float((err[:, i][on[:, i]] / bound[:, i][on[:, i]]).max()) if on[:, i].any() else 0.0 for i in range(3)]
    print("jl_romb k %d nr %d nspec %d: worst err / bound l = 0, 2, 4: %.3g %.3g %.3g" % (k, nr, nspec, *ratio))
    assert np.all(np.isfinite(got)) and np.all(err <= bound)
    assert np.all(_bits(got[~on]) == 0)                               # +0.0, not -0.0 and not left alone
    for s in range(nspec):
        assert not (lmask[s] & 1) or _same_bits(got[s, 0], sinc[s])
    assert _same_bits(got, again.cpu().numpy())


def test_jl_romb_zero_lag(ctx):
    """r = 0: dlk romb(g) for l = 0 - no sine enters - and +0.0 for l = 2, 4."""
    g, ka, dlk, _ = _romb_case(10, 1, 2)
    out = _poisoned(ctx, (2, 3, 3))
    ctx.jl_romb(ctx.to_device(g), ctx.to_device(ka), dlk, ctx.to_device(np.zeros(3)), out=out)
    got = out.cpu().numpy()
    W, _ = po.romb_weights(10)
    val, bound = ro.jl_romb(g, ka, dlk, np.zeros(3))
    for s in range(2):
        assert np.all(val[s, 0] == (W * g[s]).sum() * ro.LD(dlk))
    assert np.all(np.abs((got - val).astype(np.float64)) <= bound) and np.all(_bits(got[:, 1:]) == 0)


@pytest.mark.parametrize("mu,L,N", [(4.5, 2 * np.pi * 4096 / 3.5e5, 8192), (4.5, 20.0, 2001), (4.5, 3.0, 700)])
def test_fftlog_phase_order_four(ctx, mu, L, N):
    """mu = l + 1/2 for l = 4 at the three (L, N) of test_gpu_pk2xi.py::test_fftlog_phase."""
    import torch

    out = _poisoned(ctx, (N // 2 + 1,), torch.complex128)
    ctx.fftlog_phase(mu, L, N, out=out)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    U, bound = po.fftlog_phase(mu, L, N)
    err = np.abs((got.astype(np.clongdouble) - U)).astype(np.float64)
    print("fftlog_phase mu %.1f eta to %.3g: worst err / bound %.3g" % (mu, 2 * np.pi * (N // 2) / L, (err / bound).max()))
    assert got[0] == 1.0 and np.all(err <= bound) and np.all(np.abs(np.abs(got) - 1.0) <= 4 * po.EPS)


def test_multipole_route_end_to_end(ctx):
    """P = k exp(-k^2), rnum 141 on 1e-1 .. 1e4, six levels: the grids are the oracle's, every value is inside its bound;
    the distance to the closed form is printed (tests/test_rsdcorr_host.py holds the oracle to it)."""
    from cora_amd.signal import corrfunc

    ra = np.logspace(-1, 4, 141)
    plan = corrfunc._MultipolePlan(ra)
    nlow, npad, N0, kfine = ro.multipole_grids(ra)
    assert (plan.nlow, plan.npad, plan.n) == (nlow, npad, N0) and np.array_equal(plan.kfine, kfine)
    assert np.array_equal(plan.kdirect, ro.direct_grid()[0]) and plan.dlk == ro.direct_grid()[1]
    got = corrfunc.ps_to_multipoles([ro.pk_gauss], [(0, 2, 4)], ra)[0]
    val, bound = ro.multipoles(ro.pk_gauss, (0, 2, 4), ra)
    for n, l in enumerate((0, 2, 4)):
        err = np.abs(got[l] - val[n])
        env = np.abs(got[l] - ro.xi_gauss(l, ra)) / ro.xi_gauss(l, ra, envelope=True)
        print("ps_to_multipoles l = %d: worst err / bound, direct part %.3g, FFTLog part %.3g; against the closed form, of "
              "the envelope: direct %.3g, FFTLog %.3g" % (l, (err / bound[n])[:nlow].max(), (err / bound[n])[nlow:].max(),
                                                         env[:nlow].max(), env[nlow:].max()))
        assert got[l].shape == ra.shape and np.all(np.isfinite(got[l])) and np.all(err <= bound[n])
    dev = corrfunc.ps_to_multipoles_device([ro.pk_gauss, ro.pk_gauss], [(0,), (2, 4)], ra)
    assert sorted(dev[0]) == [0] and sorted(dev[1]) == [2, 4] and dev[1][4].is_cuda
    for n, l in enumerate((0, 2, 4)):            # (other integrand counts are other kernel instances: the bound, not the bits)
        assert np.all(np.abs(dev[0 if l == 0 else 1][l].cpu().numpy() - val[n]) <= bound[n])


# ---- xi_rsd -----------------------------------------------------------------------------------------------------------
def _xi_rsd(ctx, kx, ky, ky2, pi, sg, coef):
    import torch

    d = ctx.to_device
    args = (d(kx), d(ky), d(ky2), d(pi), d(sg), d(coef))
    out = _poisoned(ctx, (pi.size,))
    ctx.xi_rsd(*args, out=out)
    again = ctx.xi_rsd(*args)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert _same_bits(got, again.cpu().numpy())
    return got


def _golden_models():
    import test_rsdcorr_host as th

    return th._models()


@pytest.mark.parametrize("name", ["c21", "mps", "fps"])
def test_xi_rsd_golden_points(ctx, name):
    """The 200 golden points on the reference's tables (nfun 3: the 21cm model and the single-spectrum file; nfun 6: the
    7-column file), ncoef 1, the three redshift forms: inside the oracle's bound and within twice the bound of the reference."""
    import test_rsdcorr_host as th

    g, models = _golden_models()
    obj = models[name]
    kx, ky, ky2 = obj._xi_knots
    assert ky.shape[0] == (6 if name == "fps" else 3)
    for tag, z1, z2 in th.ZFORMS:
        coef = th._rows(obj, z1, z2)
        got = _xi_rsd(ctx, kx, ky, ky2, g["pi"], g["sigma"], coef)
        val, bound = ro.xi_rsd(kx, ky, ky2, g["pi"], g["sigma"], coef)
        err = np.abs((got.astype(ro.LD) - val).astype(np.float64))
        ref = np.abs(got - g["xi_%s_%s" % (name, tag)])
        print("xi_rsd %s %s: worst err / bound %.3g, against the reference %.3g" % (name, tag, (err / bound).max(), (ref / bound).max()))
        assert np.all(np.isfinite(got)) and np.all(err <= bound) and np.all(ref <= 2 * bound)


def _points(n, kx, seed):
    """n points whose r covers the knots, both extrapolation ranges, the origin and the knots themselves."""
    rng = np.random.default_rng(seed)
    r = 10.0 ** rng.uniform(np.log10(kx[0]) - 1, np.log10(kx[-1]) + 0.5, n)
    ang = rng.uniform(0, np.pi, n)
    pi, sg = r * np.cos(ang), r * np.sin(ang)
    m = min(n, kx.size)
    pi[:m], sg[:m] = kx[:m], 0.0
    if n > 3:
        pi[-1], sg[-1] = 0.0, 0.0
        pi[-2], sg[-2] = 0.0, np.nextafter(kx[-1], 0)
    return pi, sg


@pytest.mark.parametrize("ncoef", [1, 7, "n"])
@pytest.mark.parametrize("n", [1, 100003])
@pytest.mark.parametrize("nk,nfun", [(4, 3), (4, 6), (4097, 3), (4097, 6)])
def test_xi_rsd_synthetic(ctx, nk, nfun, n, ncoef):
    """nk = 4 (the minimum) and 4097, one point and 100 003 (no multiple of a block), one coefficient row, seven and one per
    point: inside the oracle's bound; the same bits on a second call."""
    ncoef = n if ncoef == "n" else ncoef
    kx, ky, ky2 = ro.synthetic_tables(nk, nfun, seed=nk + nfun)
    pi, sg = _points(n, kx, n + ncoef)
    rng = np.random.default_rng(ncoef)
    coef = rng.uniform(0.5, 2.0, (ncoef, 4)) * np.where(rng.uniform(size=(ncoef, 4)) < 0.2, -1.0, 1.0)
    got = _xi_rsd(ctx, kx, ky, ky2, pi, sg, coef)
    val, bound = ro.xi_rsd(kx, ky, ky2, pi, sg, coef)
    err = np.abs((got.astype(ro.LD) - val).astype(np.float64))
    print("xi_rsd nk %d nfun %d n %d ncoef %d: worst err / bound %.3g" % (nk, nfun, n, ncoef, (err / bound).max()))
    assert np.all(np.isfinite(got)) and np.all(err <= bound)


@pytest.mark.parametrize("nfun", [3, 6])
def test_xi_rsd_on_poisoned_scratch(ctx, nfun):
    """The interval records and the look-up grid live in context scratch (slot 12): the result must not depend on what
    the slot held before the call (0x00, 0xFF, 0x7E)."""
    from _poison import poisoned_runs

    kx, ky, ky2 = ro.synthetic_tables(301, nfun, seed=5)
    pi, sg = _points(20011, kx, 3)
    d = ctx.to_device
    args = (d(kx), d(ky), d(ky2), d(pi), d(sg), d(np.array([[1.0, 0.9, 0.8, 0.5], [2.0, 1.1, 0.7, 0.25]])))
    ref, _ = poisoned_runs(ctx, lambda: ctx.xi_rsd(*args), slots=(12,), label="xi_rsd nfun %d" % nfun)
    val, bound = ro.xi_rsd(kx, ky, ky2, pi, sg, args[5].cpu().numpy())
    assert np.all(np.abs((ref[0].cpu().numpy().astype(ro.LD) - val).astype(np.float64)) <= bound)


def test_jl_romb_on_poisoned_allocations(ctx):
    from _poison import poisoned_runs

    g, ka, dlk, r = _romb_case(8, 257, 3)
    d = ctx.to_device
    args = (d(g), d(ka), dlk, d(r), (7, 1, 3))
    poisoned_runs(ctx, lambda: ctx.jl_romb(*args), scratch=False, label="jl_romb")


def test_wrappers_reject_bad_arguments(ctx):
    d = ctx.to_device
    kx, ky, ky2 = ro.synthetic_tables(8, 3)
    p = d(np.ones(5))
    with pytest.raises(ValueError, match="3 tables"):
        ctx.xi_rsd(d(kx), d(ky[:2]), d(ky2[:2]), p, p, d(np.ones((1, 4))))
    with pytest.raises(ValueError, match="ncoef >= 1"):
        ctx.xi_rsd(d(kx), d(ky), d(ky2), p, p, d(np.ones((0, 4))))
    with pytest.raises(ValueError, match="at least 4 knots"):
        ctx.xi_rsd(d(kx[:3]), d(ky[:, :3]), d(ky2[:, :3]), p, p, d(np.ones((1, 4))))
    with pytest.raises(ValueError, match="1 to 3 integrands"):
        ctx.jl_romb(d(np.ones((4, 5))), d(np.ones(5)), 0.1, p)
    with pytest.raises(ValueError, match="2\\^k \\+ 1"):
        ctx.jl_romb(d(np.ones((1, 6))), d(np.ones(6)), 0.1, p)
    with pytest.raises(ValueError, match="lmask"):
        ctx.jl_romb(d(np.ones((1, 5))), d(np.ones(5)), 0.1, p, lmask=[8])


# ---- the public calls -----------------------------------------------------------------------------------------------------
def _worst(obj, g, got, name, tag, z1, z2):
    import test_rsdcorr_host as th

    kx, ky, ky2 = obj._xi_knots
    _, bound = ro.xi_rsd(kx, ky, ky2, g["pi"], g["sigma"], th._rows(obj, z1, z2))
    ref = np.abs(got - g["xi_%s_%s" % (name, tag)])
    assert np.all(ref <= 2 * bound), (name, tag, (ref / bound).max())
    return float((ref / bound).max())


def test_redshiftspace_correlation_against_the_reference(ctx, tmp_path):
    """Through ``_load_cache(table)`` on the 21cm model and through ``from_file_matterps`` / ``from_file_fullps``: the
    reference's results at the golden points, the three redshift forms."""
    import test_rsdcorr_host as th
    from cora_amd.signal import corr, corr21cm

    g = ro.load_golden()
    f4, f7 = str(tmp_path / "t4.dat"), str(tmp_path / "t7.dat")
    np.savetxt(f4, g["table"])
    np.savetxt(f7, g["table7"])
    c21 = corr21cm.Corr21cm()
    c21._load_cache(f4)
    objs = {"c21": c21, "mps": corr.RedshiftCorrelation.from_file_matterps(f4, redshift=1.5, bias=2.0),
            "fps": corr.RedshiftCorrelation.from_file_fullps(f7, redshift=1.5)}
    for name, obj in objs.items():
        for tag, z1, z2 in th.ZFORMS:
            got = obj.redshiftspace_correlation(g["pi"], g["sigma"], z1, z2)
            assert got.shape == (200,)
            print("redshiftspace_correlation %s %s: worst |got - reference| / bound %.3g" % (name, tag, _worst(obj, g, got, name, tag, z1, z2)))
    one = objs["fps"].redshiftspace_correlation(float(g["pi"][40]), float(g["sigma"][40]), 0.8, 1.1)
    assert isinstance(one, float) and one == objs["fps"].redshiftspace_correlation(g["pi"], g["sigma"], 0.8, 1.1)[40]
    dev = objs["fps"].redshiftspace_correlation_device(ctx.to_device(g["pi"]), ctx.to_device(g["sigma"]), 0.8, 1.1)
    assert dev.is_cuda and np.array_equal(dev.cpu().numpy(), objs["fps"].redshiftspace_correlation(g["pi"], g["sigma"], 0.8, 1.1))
    for name in ("c21", "fps"):
        got = objs[name].angular_correlation(g["theta"], 0.8, 1.1)
        ref = g["ang_" + name]
        # (the reference's result at the same points: the bound of xi_rsd at those separations)
        cos = objs[name].cosmology
        sg = g["theta"] * cos.proper_distance(0.95)
        pi = np.full(16, cos.comoving_distance(1.1) - cos.comoving_distance(0.8))
        kx, ky, ky2 = objs[name]._xi_knots
        _, bound = ro.xi_rsd(kx, ky, ky2, pi, sg, th._rows(objs[name], 0.8, 1.1))
        print("angular_correlation %s: worst |got - reference| / bound %.3g" % (name, (np.abs(got - ref) / bound).max()))
        assert got.shape == (16,) and np.all(np.abs(got - ref) <= 2 * bound)


def test_array_redshifts_broadcast(ctx):
    """z1 [3, 1], z2 [1, 4] with pi [5, 1, 1] (an extension: the reference takes scalar redshifts) against a loop of
    scalar calls; and redshifts on a leading axis, where the rows cannot be read cyclically."""
    import test_rsdcorr_host as th

    g, models = th._models()
    obj = models["fps"]
    z1 = np.array([0.5, 0.8, 1.2])[:, None]
    z2 = np.array([0.6, 0.9, 1.1, 1.5])[None, :]
    pi = np.array([-30.0, -2.5, 0.0, 1.0, 80.0])[:, None, None]
    sigma = 3.0
    got = obj.redshiftspace_correlation(pi, sigma, z1, z2)
    assert got.shape == (5, 3, 4) and np.all(np.isfinite(got))
    # the model hooks see arrays here and scalars there: an ulp in a coefficient row is allowed, no more
    tol = 16 * ro.EPS * np.abs(got).max()
    for i in range(5):
        for a in range(3):
            for b in range(4):
                one = obj.redshiftspace_correlation(float(pi[i, 0, 0]), sigma, float(z1[a, 0]), float(z2[0, b]))
                assert abs(got[i, a, b] - one) <= tol
    lead = obj.redshiftspace_correlation(np.array([1.0, 2.0, 3.0, 4.0]), sigma, np.array([0.5, 0.8])[:, None], 1.0)
    assert lead.shape == (2, 4) and abs(lead[1, 2] - obj.redshiftspace_correlation(3.0, sigma, 0.8, 1.0)) <= tol


def test_gen_cache_round_trip_and_lazy_build(ctx, tmp_path, monkeypatch):
    """``gen_cache(fname)`` writes a file that ``_load_cache`` reads back to the same interpolaters (three spectra: seven
    columns); ``Corr21cm().redshiftspace_correlation`` builds its cache once - two calls, one ``gen_cache``."""
    from cora_amd.signal import corr, corr21cm, corrfunc

    full = corr.RedshiftCorrelation(ps_vv=ro.pk_gauss, ps_dd=lambda k: 2.0 * ro.pk_gauss(k), ps_dv=lambda k: ro.pk_gauss(k, 1.5), redshift=1.0)
    fname = str(tmp_path / "cache.dat")
    full.gen_cache(fname, rmin=1e-1, rmax=1e4, rnum=141)
    assert full._cached and np.loadtxt(fname).shape == (141, 7)
    back = corr.RedshiftCorrelation.from_file_fullps(fname, redshift=1.0)
    for name in corr.RedshiftCorrelation._MULTIPOLES:
        a, b = getattr(full, name), getattr(back, name)
        assert np.array_equal(a._data, b._data) and np.array_equal(a._y2, b._y2)
    assert np.array_equal(full._dd0i._data[:, 1], 2.0 * full._vv0i._data[:, 1])
    # (the values themselves: test_multipole_route_end_to_end, the same grid and spectrum)
    got = corrfunc.ps_to_multipoles([ro.pk_gauss], [(0, 2, 4)], np.logspace(-1, 4, 141))[0]
    for l, name in ((0, "_vv0i"), (2, "_vv2i"), (4, "_vv4i")):
        col = getattr(full, name)._data[:, 1]
        assert np.all(np.isfinite(col)) and np.allclose(col, got[l], rtol=1e-9, atol=1e-12 * np.abs(got[l]).max())
    vv = corr.RedshiftCorrelation(ps_vv=ro.pk_gauss)
    vv.gen_cache(rmin=1e-1, rmax=1e4, rnum=141)
    assert np.allclose(vv._vv2i._data, full._vv2i._data, rtol=1e-9, atol=1e-12 * np.abs(full._vv2i._data[:, 1]).max())
    assert not hasattr(vv, "_dd0i")

    calls = []
    orig = corr21cm.Corr21cm.gen_cache
    monkeypatch.setattr(corr21cm.Corr21cm, "gen_cache", lambda self, *a, **k: (calls.append(1), orig(self, *a, **k))[1])
    c = corr21cm.Corr21cm()
    assert not c._cached and calls == []
    v1 = c.redshiftspace_correlation(10.0, 5.0)
    v2 = c.redshiftspace_correlation(10.0, 5.0)
    assert calls == [1] and v1 == v2 and np.isfinite(v1) and c._vv0i._data.shape == (1000, 2)
    # the clean integral against the table the reference ships where the two agree: every row of 0.1 <= r <= 10 at 4 x
    # the figures the oracle measures on those rows (tests/test_rsdcorr_host.py).  The ends are printed.
    tab = ro.load_golden()["table"]
    ra = tab[:, 0]
    sel = np.flatnonzero((ra >= 0.1) & (ra <= 10))
    for n, (name, m) in enumerate((("_vv0i", 8.78e-7), ("_vv2i", 8.14e-6), ("_vv4i", 4.58e-6))):
        col = tab[:, n + 1]
        diff = np.abs(getattr(c, name)._data[:, 1] - col)
        scale = np.abs(col[sel]).max()
        ends = " ".join("%.2g" % (diff[i] / abs(col[i])) for i in (int(np.argmin(np.abs(ra - x))) for x in (1e-3, 1e-2, 0.05, 30, 36, 100, 400)))
        print("Corr21cm table xi_%d against the shipped one, 0.1 <= r <= 10, of the column's largest: %.3g; relative at "
              "r = 1e-3, 1e-2, 0.05, 30, 36, 100, 400: %s" % (2 * n, diff[sel].max() / scale, ends))
        assert diff[sel].max() / scale <= 4 * m


def test_pwrspec_and_physical_field(ctx):
    """``get_pwrspec`` is ``powerspectrum_1D`` over the band; ``get_kiyo_field_physical`` returns what ``realisation`` does."""
    from cora_amd.signal import corr21cm

    c = corr21cm.Corr21cm()
    c.x_num, c.y_num, c.nu_num = 8, 10, 6
    c.x_width, c.y_width, c.nu_lower, c.nu_upper = 3.0, 5.0, 500.0, 560.0
    k = np.array([0.01, 0.1, 1.0])
    z1, z2 = c._band_redshifts()
    assert np.array_equal(c.get_pwrspec(k), c.powerspectrum_1D(k, z1, z2, 256)) and c.get_pwrspec(k).shape == (3,)
    cube, rsf, dims = c.get_kiyo_field_physical(seed=7)
    ref = c.realisation(z1, z2, 3.0, 5.0, 6, 8, 10, zspace=False, report_physical=True, seed=7)
    assert cube.shape == ref[0].shape == (6, 8, 10) and np.array_equal(cube, ref[0])
    assert rsf.shape == ref[1].shape and len(dims) == 4 and dims == ref[2]
    assert not c._cached                    # (neither call needs the multipole table)
