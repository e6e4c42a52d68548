"""Host checks of the P(k) -> xi(r) route (csrc/pk2xi.hip, corrfunc.ps_to_corr, lssutil.cutoff, lss.calculate_correlations):
the oracle of tests/_pk2xi_oracle.py against the reference's own numbers (tests/golden/pk2xi_vectors.npz, written by
tests/golden/make_golden_pk2xi.py) and against an analytic transform pair, its bounds against seven deliberate defects,
the new symbols and the argument checks.  The GPU is then held to the oracle in tests/test_gpu_pk2xi.py."""
import ctypes
import os

import numpy as np
import pytest
import scipy.integrate as si
import scipy.special as ss

import _pk2xi_oracle as po

GOLDEN_PS_TO_CORR = dict(minlogr=-1, maxlogr=3, switchlogr=1, samples_per_decade=10, richardson_n=3, pad_low=2, pad_high=2)


@pytest.fixture(scope="module")
def gold():
    return po.load_golden()


def _f64(x):
    return np.asarray(x).astype(np.float64)


# ---- Richardson and Romberg ------------------------------------------------------------------------------------------
def test_richardson_matches_the_reference(gold):
    """The package's and the oracle's table are the reference's statement for statement: the same bits, base_pow 1 and 2,
    t = 2 and 3, the last entry and the whole table."""
    from cora_amd.signal import corrfunc

    est = list(gold["rich_est"])
    for rich in (corrfunc.richardson, po.richardson):
        for bp in (1, 2):
            assert np.array_equal(rich(est, 2.0, base_pow=bp), gold["rich_t2_bp%d" % bp])
            table = rich(est, 2.0, base_pow=bp, return_table=True)
            ref = gold["rich_t2_bp%d_table" % bp].reshape(4, 4, 3)
            assert [len(row) for row in table] == [1, 2, 3, 4]
            for i in range(4):
                for j in range(i + 1):
                    assert np.array_equal(table[i][j], ref[i, j])
        assert np.array_equal(rich(est[:3], 3.0), gold["rich_t3"])


def test_richardson_weight_norms():
    """||w||_1 of the linear map the t = 2 table is: what the end-to-end bound multiplies the level bounds with."""
    for n, norm in ((3, 5.0), (6, 7.76), (9, 8.19)):
        w = po.richardson_weights(n)
        assert abs(float(w.sum()) - 1.0) < 1e-15 and abs(float(np.abs(w).sum()) - norm) < 0.005


@pytest.mark.parametrize("k", [1, 2, 5, 8, 16])
def test_class_sum_form_is_scipy_romb(k):
    """Trapezoid estimates from class sums, then the 4^j table: scipy.integrate.romb to rounding, with weights >= 0."""
    y = np.random.default_rng(k).standard_normal((1 << k) + 1)
    W, Wabs = po.romb_weights(k)
    assert np.all(W > 0) and np.all(Wabs >= W) and abs(float(W.sum()) - (1 << k)) < 1e-12 * (1 << k)
    assert abs(float((W * y).sum()) - si.romb(y)) <= 64 * po.EPS * np.abs(y).sum()


def test_oracle_matches_reference_corr_direct(gold):
    """_corr_direct of the reference for P = k e^(-8 k) at k = 4, 8, 16, r = 0 included.  The reference forms
    sin(pi y) / (pi y) with y = ka r / pi in double: three more roundings in the argument than the device's one, each worth
    the same 2 x (relative argument error) in sinc, and no deeper sums - inside twice the device's bound."""
    r = gold["direct_r"]
    assert r[0] == 0.0
    for k in (4, 8, 16):
        val, bound = po.corr_direct(po.pk_pair, -5, 3, r, k=k)
        err = np.abs(_f64(val - gold["direct_k%d" % k]))
        print("k = %d: reference against the oracle, worst err / bound %.3g" % (k, (err / bound).max()))
        assert np.all(err <= 2 * bound)
    # k = 4 and 16 differ by far more than any bound: the golden pins the order, not just the integrand
    assert np.abs(gold["direct_k4"] - gold["direct_k16"]).max() > 1e6 * bound.max()


def test_cutoff_matches_the_reference(gold):
    from cora_amd.signal import lssutil

    x = gold["cutoff_x"]
    for name, args in (("cutoff_low", (-4, 1, 0.5, 6)), ("cutoff_high", (4, -1, 0.5, 4)), ("cutoff_other", (0.3, -3, 0.25, 2.5))):
        got = lssutil.cutoff(x, *args)
        assert np.array_equal(got, gold[name])
        exact = _f64(po.cutoff(x, *args))
        # log10, the quotient, tanh, 1 +, 0.5 *, the power: the argument of tanh is good to 2 eps (|arg| + 1), tanh' <= 1,
        # and the power multiplies the relative error by the index
        arg = np.abs((np.log10(x) - args[0]) / args[2])
        tol = args[3] * po.EPS * (2 * (arg + 1) / np.maximum(0.5 * (1 + np.tanh(np.sign(args[1]) * (np.log10(x) - args[0]) / args[2])), 1e-300) + 4) * exact
        assert np.all(np.abs(got - exact) <= tol + 1e-300)
    assert lssutil.cutoff(1e-9, -4, 1, 0.5, 6) < 1e-50 and 1 - 1e-6 < lssutil.cutoff(1.0, -4, 1, 0.5, 6) < 1.0


# ---- the FFTLog kernel and the convolution -------------------------------------------------------------------------
def test_oracle_phase_against_scipy_loggamma():
    """theta = eta ln 2 + 2 Im lnGamma((mu + 1 + i eta) / 2) with scipy's loggamma in double, inside the device's bound."""
    for mu, L, N in ((0.5, 40.0, 4000), (2.5, 3.0, 700), (0.5, 2 * np.pi * 4096 / 3.5e5, 8192)):
        theta, bound = po.fftlog_theta(mu, L, N)
        eta = 2 * np.pi * np.arange(N // 2 + 1) / L
        ref = eta * np.log(2.0) + 2 * ss.loggamma((mu + 1 + 1j * eta) / 2).imag
        assert theta[0] == 0 and np.all(np.abs(_f64(theta - ref)) <= bound)
        U, bU = po.fftlog_phase(mu, L, N)
        assert np.all(np.abs(np.abs(U) - 1) < 1e-18) and np.all(bU >= bound)
    # the two shifts of the oracle (40 with eight terms for the value, 16 with seven as the device) agree to the stated
    # truncation
    x, y = po.LD(0.75), np.linspace(0, 50, 501).astype(po.LD)
    a, _, _ = po._im_lngamma_terms(x, y, 40, 8)
    b, mag, _ = po._im_lngamma_terms(x, y, 16, 7)
    assert np.all(np.abs(a - b) <= po.TRUNC + 16 * np.finfo(po.LD).eps * mag)       # (the longdouble roundings of both)


SPLITS = [(2, 4096), (41, 100), (105, 1), (3, 35), (125, 112), (4, 3500)]


def _signal(N, seed):
    rng = np.random.default_rng(seed)
    U = np.exp(1j * rng.uniform(0, 2 * np.pi, N // 2 + 1))
    U[0] = 1.0
    return rng.standard_normal(N), U


@pytest.mark.parametrize("N1,N2", SPLITS)
def test_four_step_scheme_is_the_circular_convolution(N1, N2):
    """Forward along axis 0, twiddle, forward along axis 1, U_m at m = k1 + N1 k2, and back: irfft(rfft(f) U), natural
    order, no transpose; the imaginary part of the result is rounding."""
    f, U = _signal(N1 * N2, N1)
    val, bound = po.logconv(f, U)
    got = po.logconv_four_step(f, U, N1, N2)
    assert np.abs(got.real - val).max() <= 16 * po.EPS * np.abs(val).max() and np.abs(got - val).max() <= bound


# ---- deliberate defects ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("defect", ["class", "half", "pow4", "r0"])
def test_romberg_bound_rejects(defect):
    """A class taken one too high, the end samples at full weight, 2^j for 4^j in the table, sinc(0) = 0."""
    k = 8
    ka = np.logspace(-5, 3, (1 << k) + 1)
    g = ka**3 * po.pk_pair(ka) / (2 * np.pi**2) + 1e-3 * ka       # the second term keeps the end sample k = 1e3 alive
    r = np.array([0.0, 0.3, 4.0])
    dlk = np.log(ka[1] / ka[0])
    val, bound = po.sinc_romb(g, ka, dlk, r)
    bad, _ = po.sinc_romb(g, ka, dlk, r, defect=defect)
    miss = np.abs(_f64(bad - val)) / bound
    print("%s: err / bound %s" % (defect, miss))
    assert miss[0] > 1e3 and (defect == "r0" or np.all(miss > 1e3))


@pytest.mark.parametrize("defect", ["unconj", "nyquist", "twiddle"])
@pytest.mark.parametrize("N1,N2", [(41, 100), (2, 4096)])
def test_convolution_bound_rejects(defect, N1, N2):
    """U_{N-m} unconjugated above N / 2, the Nyquist product kept complex (it shows in the imaginary part, which the GPU
    test holds to the same bound), the four-step twiddle left out."""
    f, U = _signal(N1 * N2, 5)
    val, bound = po.logconv(f, U)
    bad = po.logconv_four_step(f, U, N1, N2, defect=defect)
    miss = np.abs(bad - val).max() / bound
    print("%s %d x %d: err / bound %.3g" % (defect, N1, N2, miss))
    assert miss > 1e3


# ---- ps_to_corr --------------------------------------------------------------------------------------------------------
def test_oracle_matches_reference_ps_to_corr(gold):
    """The reference's ps_to_corr with the oracle's P2xi standing in for hankl: the same r bit for bit (grids, padding,
    decimation, trimming, zero lag, concatenation); the direct part as above; the FFTLog part - UNPINNED in its values, the
    stand-in being ours - differs only in where P is evaluated (each level's own logspace there, a strided subset of the
    finest here, wavenumbers a few ulp apart)."""
    r, val, bound = po.ps_to_corr(po.pk_pair, **GOLDEN_PS_TO_CORR)
    assert np.array_equal(r, gold["ps_to_corr_r"]) and r[0] == 0.0 and r.size == 42
    err = np.abs(val - gold["ps_to_corr_xi"])
    print("reference ps_to_corr against the oracle, worst err / bound: direct %.3g, FFTLog %.3g"
          % ((err / bound)[:21].max(), (err / bound)[21:].max()))
    assert np.all(err[:21] <= 2 * bound[:21]) and np.all(err[21:] <= bound[21:])


def test_oracle_against_the_analytic_pair():
    """P = k e^(-a k), a = 8, has xi(r) = 2 sin(3 atan(r / a)) / (2 pi^2 r (a^2 + r^2)^1.5) and xi(0) = 6 / (2 pi^2 a^4).
    Errors over the envelope 2 / (2 pi^2 r (a^2 + r^2)^1.5), no point left out, asserted at 4 x what the oracle measures on
    the CPU:

      direct part (2^16 + 1 wavenumbers, r = 0 and 0.1 .. 10)                                  6.36e-13
      FFTLog part, samples_per_decade 20, richardson_n 6, pads 4 / 6, maxlogr 4                2.50e-7
      the same below r = 1e3                                                                   4.93e-11

    (At the defaults of calculate_correlations - 1000 samples per decade, nine levels to 3 584 000 points - the oracle is at
    3.03e-9 of the envelope for r < 1e3; it takes 48 s there, so that size is not part of the suite.)"""
    kw = dict(minlogr=-1, maxlogr=4, switchlogr=1, samples_per_decade=20, richardson_n=6, pad_low=4, pad_high=6)
    r, val, bound = po.ps_to_corr(po.pk_pair, **kw)
    rel = np.abs(_f64(val - po.xi_pair(r))) / po.xi_envelope(r)
    lo = r < 10
    print("of the envelope: direct %.3g, FFTLog %.3g, below 1e3 %.3g" % (rel[lo].max(), rel[~lo].max(), rel[~lo & (r < 1e3)].max()))
    assert rel[lo].max() <= 4 * 6.36e-13
    assert rel[~lo].max() <= 4 * 2.50e-7
    assert rel[~lo & (r < 1e3)].max() <= 4 * 4.93e-11
    assert val[0] == pytest.approx(6 / (2 * np.pi**2 * 8.0**4), rel=1e-11)


# ---- the package -------------------------------------------------------------------------------------------------------
def test_abi_symbols_present():
    from cora_amd import _lib
    from cora_amd.signal import corrfunc, lss, lssutil

    names = ["corahip_sinc_romb", "corahip_fftlog_phase", "corahip_logconv", "corahip_logconv_split"]
    lib = ctypes.CDLL(_lib.LIB_PATH)
    header = open(os.path.join(os.path.dirname(_lib._HERE), "include", "corahip.h")).read()
    assert "#define CORAHIP_ABI_MINOR 12 " in header
    minor_line = header.split("#define CORAHIP_ABI_MINOR")[1].split("\n")[0]
    assert "and (pk2xi) sinc_romb, fftlog_phase, logconv, logconv_split" in minor_line
    for n in names:
        assert n in _lib.SIGNATURES and hasattr(lib, n) and ("int %s(" % n) in header
    for m in ("sinc_romb", "fftlog_phase", "logconv", "logconv_split"):
        assert callable(getattr(_lib.Context, m))
    for mod, fs in ((corrfunc, ("richardson", "ps_to_corr", "ps_to_corr_device")), (lssutil, ("cutoff",)), (lss, ("calculate_correlations",))):
        for f in fs:
            assert callable(getattr(mod, f))


def test_logconv_split_rule():
    """(N, 1) up to 4096 points; beyond, two divisors of at most 4096 each; none: ValueError naming the rule.  Host only."""
    from cora_amd import _lib

    split = _lib.Context.logconv_split
    assert split(1) == (1, 1) and split(700) == (700, 1) and split(4096) == (4096, 1)
    for N in (4100, 8192, 12285, 22400, 14000 * 256, 4096 * 4096):
        n1, n2 = split(N)
        assert n1 * n2 == N and 1 < n1 <= 4096 and 1 < n2 <= 4096
    assert split(8192) == (2, 4096) and split(22400) == (175, 128)
    for N in (3 * 4099, 4099, 4096 * 4096 + 1, 4096 * 4097):
        with pytest.raises(ValueError, match="both factors <= 4096"):
            split(N)
    with pytest.raises(ValueError):
        split(0)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    a, b = ctypes.c_int(0), ctypes.c_int(0)
    assert lib.corahip_logconv_split(ctypes.c_int64(3 * 4099), ctypes.byref(a), ctypes.byref(b)) == -1      # CORAHIP_EINVAL


class _Untouchable:
    def __getattr__(self, name):
        raise AssertionError("the library was touched (%s) before the arguments were checked" % name)


def test_argument_errors_before_the_library(monkeypatch):
    import torch

    from cora_amd import _lib
    from cora_amd.signal import corrfunc

    ctx = _lib.Context.__new__(_lib.Context)
    ctx.lib, ctx.h, ctx.device = _Untouchable(), None, torch.device("cpu")
    z = lambda n, dt=torch.float64: torch.zeros(n, dtype=dt)  # noqa: E731
    for g, ka, r in ((z(16), z(16), z(3)), (z(2), z(2), z(3)), (z(17), z(16), z(3)), (z(17).float(), z(17), z(3)),
                     (z(17).numpy(), z(17), z(3)), (z(34)[::2], z(17), z(3)), (z(17), z(17), z((3, 1))), (z(17), z(17), z(3).float())):
        with pytest.raises(ValueError):
            ctx.sinc_romb(g, ka, 0.1, r)
    with pytest.raises(ValueError, match="out must be"):
        ctx.sinc_romb(z(17), z(17), 0.1, z(3), out=z(4))
    big = z(40)
    with pytest.raises(ValueError, match="overlaps"):
        ctx.sinc_romb(big[:17], big[20:37], 0.1, z(3), out=big[16:19])
    for mu, L, N in ((-1.0, 1.0, 8), (0.5, 0.0, 8), (0.5, 1.0, 0), (0.5, float("nan"), 8)):
        with pytest.raises(ValueError, match="fftlog_phase needs"):
            ctx.fftlog_phase(mu, L, N)
    with pytest.raises(ValueError, match="out"):
        ctx.fftlog_phase(0.5, 1.0, 8, out=z(4, torch.complex128))
    c = torch.complex128
    for data, u, split in ((z(8), z(5, c), None), (z(8, c), z(4, c), None), (z(8, c), z(5), None), (z(0, c), z(1, c), None),
                           (z(8, c), z(5, c), (2, 3)), (z(8, c), z(5, c), (0, 8)), (z(8192, c), z(4097, c), (8192, 1)),
                           (z(16, c)[::2], z(5, c), None), (z(3 * 4099, c), z(3 * 4099 // 2 + 1, c), None)):
        with pytest.raises(ValueError):
            ctx.logconv(data, u, split)
    both = z(16, c)
    with pytest.raises(ValueError, match="overlaps"):
        ctx.logconv(both[:8], both[6:11])

    # corrfunc: refused before a context is asked for
    monkeypatch.setattr(_lib, "get_context", lambda *a, **k: (_ for _ in ()).throw(AssertionError("context asked for")))
    with pytest.raises(NotImplementedError, match="hankel"):
        corrfunc.ps_to_corr(po.pk_pair, fftlog=False)
    with pytest.raises(ValueError, match="both factors <= 4096"):
        corrfunc.ps_to_corr(po.pk_pair, maxlogr=5, switchlogr=1, samples_per_decade=4099, richardson_n=2)
    with pytest.raises(ValueError, match="richardson_n"):
        corrfunc.ps_to_corr(po.pk_pair, richardson_n=0)
    with pytest.raises(TypeError):
        corrfunc.ps_to_corr(po.pk_pair, upsample=10)


def test_plan_grids_are_the_reference_grids(gold):
    """The host side of ps_to_corr - the r and k grids, the trim mask, the zero lag, the concatenation - against the
    reference's own r; one evaluation grid per route, the coarser levels being strided subsets of the finest."""
    from cora_amd.signal import corrfunc

    plan = corrfunc._CorrPlan(**GOLDEN_PS_TO_CORR)
    assert np.array_equal(plan.r, gold["ps_to_corr_r"])
    assert plan.kdirect.size == 65537 and plan.kfine.size == 60 * 4 and plan.n == 60 and plan.splits == [(60, 1), (120, 1), (240, 1)]
    assert np.allclose(plan.kfine[::4], np.logspace(-5, 1, 60, endpoint=False), rtol=64 * po.EPS, atol=0)
    d = corrfunc._CorrPlan(minlogr=-1, maxlogr=5, switchlogr=1, samples_per_decade=1000, pad_low=4, pad_high=6, richardson_n=9)
    assert d.n == 14000 and d.kfine.size == 3584000 and d.r.size == 6002 and d.splits[-1][0] * d.splits[-1][1] == 3584000


def test_calculate_correlations_composition(monkeypatch):
    """P is evaluated once per grid, regularised by the two cut-offs and the Gaussian, and handed on as P, P / k^2 and
    P / k^4; the three tables come back as sinh interpolaters with x_t = r[1] and f_t = 1e-3, 1e-6, 1e2."""
    import torch

    from cora_amd.signal import corrfunc, lss, lssutil
    from cora_amd.util import cubicspline

    seen, calls = [], []

    def fake_run(self, pd, pf):
        seen.append((np.array(pd), np.array(pf)))
        return torch.from_numpy(np.exp(-self.r / 40.0) * np.cos(self.r / 25.0) * pd[30000])

    def ps(k):
        calls.append(np.shape(k))
        return 3.0 * k / (1.0 + (k / 0.02) ** 2.5)

    monkeypatch.setattr(corrfunc._CorrPlan, "run", fake_run)
    out = lss.calculate_correlations(ps, samples_per_decade=10, ksmooth=5.0)
    plan = corrfunc._CorrPlan(-1, 5, 1, 10, pad_low=4, pad_high=6, richardson_n=9)
    assert calls == [(65537,), (140 * 256,)] and len(seen) == 3 and sorted(out) == ["corr0", "corr2", "corr4"]
    for (pd, pf), n, f_t in zip(seen, (0, 2, 4), (1e-3, 1e-6, 1e2)):
        for got, k in ((pd, plan.kdirect), (pf, plan.kfine)):
            # (cutoff itself is held to the reference above; deep in the cut its 1 + tanh cancels, so it is used as it is)
            want = (lssutil.cutoff(k, -4, 1, 0.5, 6) * lssutil.cutoff(k, 4, -1, 0.5, 4) * np.exp(-0.5 * (k / 5.0) ** 2)
                    * 3.0 * k / (1.0 + (k / 0.02) ** 2.5) * k ** float(-n))
            assert np.all(np.abs(got - want) <= 16 * po.EPS * np.abs(want))
        c = out["corr%d" % n]
        assert isinstance(c, cubicspline.SinhInterpolater) and c.f_t == f_t and c.x_t == plan.r[1]
        knots = np.exp(-plan.r / 40.0) * np.cos(plan.r / 25.0) * pd[30000]
        assert np.allclose(c(plan.r[1:]), knots[1:], rtol=1e-9, atol=1e-12 * f_t)
