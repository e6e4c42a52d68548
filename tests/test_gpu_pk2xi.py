"""The P(k) -> xi(r) kernels (cora_amd/csrc/pk2xi.hip) called directly - ctx.sinc_romb, ctx.fftlog_phase, ctx.logconv -
and ``corrfunc.ps_to_corr`` / ``lss.calculate_correlations`` end to end, held to the derived bounds of
tests/_pk2xi_oracle.py.  Every output is filled with a NaN byte pattern first; each test prints its worst err / bound.
tests/test_pk2xi_host.py shows that the same bounds reject seven deliberate defects.  Run with -m gpu.

Observed on the MI355X (worst err / bound; the constants are derived in the oracle, none was fitted):

  sinc_romb, k = 1 / 2 / 5 / 8 / 10 / 16, nr = 257       0.055 / 0.033 / 0.012 / 0.0022 / 0.0011 / 0.00010
  sinc_romb, nr = 1 (r = 1e3: k r up to 1e6)             0.0028 / 0.00063 / 0.00013 / 0.000017 / 0.000059 / 0.000029
  fftlog_phase, eta to 3.5e5 / fine steps / mu = 2.5     0.24 / 0.18 / 0.16
  logconv, N = 105 .. 22400 (one pass and four-step)     0.00028 .. 0.0021, imaginary residue 0.00016 .. 0.0022
  logconv, N = 3 584 000 (875 x 4096) against numpy.fft  0.000038
  ps_to_corr, levels 700 .. 22400                        direct part 0.0024, FFTLog part 0.00016; against the analytic
                                                         pair 6.4e-13 (direct) and 3.4e-10 (r < 1e3) of the envelope

The Romberg and convolution bounds are worst-case sums over 2^k samples and log2 N stages, which random roundings stay
far below; the phase bound is dominated by the rounding of eta at theta ~ 4e6.
"""
import numpy as np
import pytest

import _pk2xi_oracle as po

pytestmark = pytest.mark.gpu


def _poisoned(ctx, shape, dtype=None):
    import torch

    t = ctx.empty(shape, dtype=dtype)
    t.view(torch.uint8).fill_(0xFF)            # every double a NaN: an element the kernel does not write shows
    return t


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


def _romb_case(k, nr):
    rng = np.random.default_rng(100 * k + nr)
    ka = np.logspace(-5, 3, (1 << k) + 1)
    g = rng.standard_normal(ka.size)            # every sample matters, also those at k r ~ 1e6
    r = np.array([1e3]) if nr == 1 else np.concatenate([[0.0], np.logspace(-1, 3, nr - 1)])
    return g, ka, float(np.log(ka[1] / ka[0])), r


@pytest.mark.parametrize("nr", [1, 257])
@pytest.mark.parametrize("k", [1, 2, 5, 8, 10, 16])
def test_sinc_romb(ctx, k, nr):
    """Random g on 2^k + 1 log-spaced wavenumbers up to 1e3, r = 0 and r up to 1e3 (k r to 1e6): every separation
    against the longdouble Romberg sum; a second call returns the same bits."""
    import torch

    g, ka, dlk, r = _romb_case(k, nr)
    d = ctx.to_device
    out = _poisoned(ctx, (r.size,))
    ctx.sinc_romb(d(g), d(ka), dlk, d(r), out=out)
    again = ctx.sinc_romb(d(g), d(ka), dlk, d(r))
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    val, bound = po.sinc_romb(g, ka, dlk, r)
    err = np.abs((got.astype(po.LD) - val).astype(np.float64))
    print("sinc_romb k %d nr %d: worst err / bound %.3g (|value| up to %.3g, bound %.3g)"
          % (k, nr, (err / bound).max(), float(np.abs(val).max()), bound.max()))
    assert np.all(np.isfinite(got)) and np.all(err <= bound)
    assert _same_bits(got, again.cpu().numpy())


def test_sinc_romb_zero_lag_is_the_plain_integral(ctx):
    """r = 0: sinc = 1 for every sample, so the result is dlk romb(g) - no sine enters."""
    g, ka, dlk, _ = _romb_case(10, 1)
    got = ctx.sinc_romb(ctx.to_device(g), ctx.to_device(ka), dlk, ctx.to_device(np.zeros(3))).cpu().numpy()
    W, _ = po.romb_weights(10)
    val, bound = po.sinc_romb(g, ka, dlk, np.zeros(3))
    assert np.all(val == (W * g).sum() * po.LD(dlk))
    assert np.all(np.abs((got - val).astype(np.float64)) <= bound) and got[0] == got[1] == got[2]


@pytest.mark.parametrize("mu,L,N", [(0.5, 2 * np.pi * 4096 / 3.5e5, 8192), (0.5, 20.0, 2001), (2.5, 3.0, 700)])
def test_fftlog_phase(ctx, mu, L, N):
    """eta = 2 pi m / L from 0 to 3.5e5 (the top of the 3 584 000-point level of the default pipeline) in coarse steps, a
    fine grid at small eta, and another order: against the longdouble phase; unit modulus; U_0 = 1 exactly."""
    import torch

    out = _poisoned(ctx, (N // 2 + 1,), torch.complex128)
    ctx.fftlog_phase(mu, L, N, out=out)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    U, bound = po.fftlog_phase(mu, L, N)
    err = np.abs((got.astype(np.clongdouble) - U)).astype(np.float64)
    print("fftlog_phase mu %.1f eta to %.3g: worst err / bound %.3g (bound up to %.3g)"
          % (mu, 2 * np.pi * (N // 2) / L, (err / bound).max(), bound.max()))
    assert got.shape == (N // 2 + 1,) and got[0] == 1.0
    assert np.all(err <= bound)
    assert np.all(np.abs(np.abs(got) - 1.0) <= 4 * po.EPS)


def _signal(N, seed):
    rng = np.random.default_rng(seed)
    f = rng.standard_normal(N)
    U = np.exp(1j * rng.uniform(0, 2 * np.pi, N // 2 + 1))
    U[0] = 1.0
    return f, U


def _logconv(ctx, f, U, split):
    import torch

    data = _poisoned(ctx, (f.size,), torch.complex128)
    data.copy_(torch.from_numpy(f.astype(np.complex128)))
    ctx.logconv(data, torch.from_numpy(np.ascontiguousarray(U, dtype=np.complex128)).to(ctx.device), split)
    torch.cuda.synchronize()
    return data.cpu().numpy()


@pytest.mark.parametrize("N,split", [(105, None), (105, (3, 35)), (700, None), (4096, None), (4096, (64, 64)),
                                     (4100, (41, 100)), (8192, None), (12285, None), (22400, None), (22400, (175, 128))])
def test_logconv(ctx, N, split):
    """Random real signal, random unit-modulus kernel (every mode matters, Nyquist included): one pass up to 4096 points,
    the four-step split above and where a split is given; odd and even N, Bluestein and power-of-two factors."""
    f, U = _signal(N, N + (split or (0,))[0])
    used = ctx.logconv_split(N) if split is None else split
    assert used[0] * used[1] == N and max(used) <= 4096 and (N <= 4096 or min(used) > 1)
    got = _logconv(ctx, f, U, split)
    val, bound = po.logconv(f, U)
    err = np.abs(got.real - val).max()
    print("logconv N %d as %d x %d: worst err / bound %.3g, imaginary residue / bound %.3g (bound %.3g)"
          % (N, used[0], used[1], err / bound, np.abs(got.imag).max() / bound, bound))
    assert np.all(np.isfinite(got.view(np.float64)))
    assert err <= bound and np.abs(got.imag).max() <= bound


def test_logconv_longest_level(ctx):
    """N = 3 584 000 = 14000 x 2^8, the finest level of the default pipeline, against numpy.fft."""
    N = 3584000
    f, U = _signal(N, 7)
    n1, n2 = ctx.logconv_split(N)
    assert n1 * n2 == N and max(n1, n2) <= 4096
    got = _logconv(ctx, f, U, None)
    val, bound = po.logconv(f, U)
    err = np.abs(got.real - val).max()
    print("logconv N %d as %d x %d: worst err / bound %.3g (bound %.3g)" % (N, n1, n2, err / bound, bound))
    assert err <= bound and np.abs(got.imag).max() <= bound


def test_logconv_rejects_a_length_without_a_split(ctx):
    """4099 is prime: 3 x 4099 has no pair of factors below 4097.  The message names the rule."""
    import torch

    with pytest.raises(ValueError, match="both factors <= 4096"):
        ctx.logconv_split(3 * 4099)
    data = torch.zeros(3 * 4099, dtype=torch.complex128, device=ctx.device)
    with pytest.raises(ValueError, match="both factors <= 4096"):
        ctx.logconv(data, ctx.fftlog_phase(0.5, 10.0, 3 * 4099))
    with pytest.raises(ValueError, match="does not factor"):
        ctx.logconv(data, ctx.fftlog_phase(0.5, 10.0, 3 * 4099), (3, 4099))


E2E = dict(minlogr=-1, maxlogr=5, switchlogr=1, samples_per_decade=50, pad_low=4, pad_high=6, richardson_n=6)


def test_ps_to_corr_end_to_end(ctx):
    """P = k e^(-8 k), 50 samples per decade, pads 4 / 6, six Richardson levels of 700 .. 22400 points (one pass and
    four-step): grids identical to the oracle's and every value inside its bound (the distance to the analytic xi is
    printed; tests/test_pk2xi_host.py holds the oracle to it)."""
    from cora_amd.signal import corrfunc

    plan = corrfunc._CorrPlan(**E2E)
    assert [plan.n * 2**ii for ii in range(6)] == [700, 1400, 2800, 5600, 11200, 22400]
    assert [min(s) == 1 for s in plan.splits] == [True, True, True, False, False, False]
    r, xi = corrfunc.ps_to_corr(po.pk_pair, **E2E)
    ro, val, bound = po.ps_to_corr(po.pk_pair, **E2E)
    assert r.shape == ro.shape == xi.shape and r[0] == 0.0
    assert np.array_equal(r, ro)
    err = np.abs(xi - val)
    lo = r < 10
    print("ps_to_corr: worst err / bound, direct part %.3g, FFTLog part %.3g" % ((err / bound)[lo].max(), (err / bound)[~lo].max()))
    assert np.all(np.isfinite(xi)) and np.all(err <= bound)
    env = np.abs(xi - po.xi_pair(r).astype(np.float64)) / po.xi_envelope(r)
    mid = ~lo & (r < 1e3)
    print("ps_to_corr against the analytic pair, of the envelope: direct %.3g, FFTLog below 1e3 %.3g, all %.3g"
          % (env[lo].max(), env[mid].max(), env[~lo].max()))

    rd, xid = corrfunc.ps_to_corr_device(po.pk_pair, **E2E)
    assert rd.is_cuda and xid.is_cuda and np.array_equal(xid.cpu().numpy(), xi)
    with pytest.raises(NotImplementedError, match="hankel"):
        corrfunc.ps_to_corr(po.pk_pair, fftlog=False)


def test_calculate_correlations_feeds_corr_to_clarray(ctx):
    """The three correlation functions of a regularised spectrum, as interpolaters, into corr_to_clarray at lmax 24."""
    from cora_amd.signal import corrfunc, lss
    from cora_amd.util import cubicspline

    calls = []

    def ps(k):
        calls.append(np.size(k))
        return 2e4 * k / (1.0 + (k / 0.02) ** 2.6)

    out = lss.calculate_correlations(ps, samples_per_decade=50)
    assert sorted(out) == ["corr0", "corr2", "corr4"] and calls == [65537, 700 * 256]
    chi = np.array([1500.0, 1520.0, 1545.0, 1575.0])
    for name, f_t in (("corr0", 1e-3), ("corr2", 1e-6), ("corr4", 1e2)):
        c = out[name]
        assert isinstance(c, cubicspline.SinhInterpolater) and c.f_t == f_t and abs(c.x_t - 0.1) < 1e-16
        cl = corrfunc.corr_to_clarray(c, 24, chi, xromb=1)
        assert cl.shape == (25, 4, 4) and np.all(np.isfinite(cl))
        assert np.array_equal(cl, cl.transpose(0, 2, 1))
