"""Host checks of the polarised-galaxy path (csrc/faraday.hip, cora_amd.foreground.galaxy): the numpy oracle
(tests/_faraday_oracle.py) and the package's host functions against the outputs of the reference's own ``getpolsky``
(tests/golden/faraday_vectors.npz, written by tests/golden/make_golden_faraday.py), and argument checking."""
import numpy as np
import pytest

import _faraday_oracle as fo

EPS = fo.EPS


@pytest.fixture(scope="module")
def cases():
    return fo.load_golden()


def _worst(err, tol):
    return float(np.max(err / np.maximum(tol, np.finfo(np.float64).tiny)))


@pytest.mark.parametrize("name", ["a", "b"])
def test_oracle_reproduces_golden_maps(cases, name):
    """The oracle's map2 / map4 / map5 against the reference's.  Bounds, a few eps times the sum of the magnitudes of
    the terms of each sum (S2 for the inverse FFT and the two scalings, its product with |pta| for the dot):

        S2[p, k]  = sum_j |base taper|[p, j] / nphi * w[p, k] / (2 sqrt(var))
        tol_map2  = (8 + 2 log2 nphi) eps S2                  (FFT of <= 2 log2 nphi stages, variance, two products)
        tol_map4  = (8 + 2 log2 nphi + nphi + 8) eps S2 |pta| (the dot in any order, tanh / abs / divide; 1-Lipschitz)
        tol_map5  = tol_map4 T + 2 eps |map5|"""
    c = cases[name]
    sigma = np.abs(c["faraday"])
    assert np.array_equal(sigma, c["sigma_phi"])
    map2, map4, w, pta, map5 = fo.mix_reference(c["base"], sigma, c["freq"], c["T"], c["dphi"], c["maxphi"])
    phifreq, pcfreq = fo.depth_grid(c["dphi"], c["maxphi"])
    nphi = len(phifreq)
    assert map2.shape == c["map2"].shape == (12 * c["nside"] ** 2, nphi)
    var = fo.chunk_var(np.fft.ifft(c["base"] * fo.taper(pcfreq), axis=1))
    S2 = (np.abs(c["base"] * fo.taper(pcfreq)).sum(axis=1) / nphi)[:, None] * c["w"] / (2 * var**0.5)
    k2 = 8 + 2 * np.log2(nphi)
    tol2 = k2 * EPS * S2
    tol4 = (k2 + nphi + 8) * EPS * (S2 @ np.abs(c["pta"]))
    tol5 = np.zeros_like(c["map5"])
    tol5[:, 1] = tol5[:, 2] = tol4.T * c["T"]
    tol5 += 2 * EPS * np.abs(c["map5"])
    r2, r4, r5 = (_worst(np.abs(map2 - c["map2"]), tol2), _worst(np.abs(map4 - c["map4"]), tol4),
                  _worst(np.abs(map5 - c["map5"]), tol5))
    print("case %s: worst err / tol  map2 %.3g  map4 %.3g  map5 %.3g" % (name, r2, r4, r5))
    assert r2 <= 1 and r4 <= 1 and r5 <= 1
    assert np.array_equal(map5[:, 0], c["T"]) and not map5[:, 3].any()
    # w and pta to 4 eps relative
    rw = _worst(np.abs(w - c["w"]), 4 * EPS * np.abs(c["w"]))
    rp = _worst(np.abs(pta - c["pta"]), 4 * EPS * np.abs(c["pta"]))
    print("case %s: worst err / (4 eps |.|)  w %.3g  pta %.3g" % (name, rw, rp))
    assert rw <= 1 and rp <= 1


@pytest.mark.parametrize("name", ["a", "b"])
def test_package_grid_and_transfer_match_golden(cases, name):
    from cora_amd.foreground import galaxy

    c = cases[name]
    phifreq, pcfreq = galaxy.faraday_depth_grid(c["dphi"], c["maxphi"])
    ophi, opc = fo.depth_grid(c["dphi"], c["maxphi"])
    assert np.array_equal(phifreq, ophi) and np.array_equal(pcfreq, opc) and len(phifreq) == c["pta"].shape[0]
    df = np.median(np.diff(c["freq"]))
    pta = galaxy.faraday_transfer(phifreq[:, None], c["freq"][None, :], df) / c["dphi"]
    r = _worst(np.abs(pta - c["pta"]), 4 * EPS * np.abs(c["pta"]))
    print("case %s: faraday_transfer worst err / (4 eps |pta|) %.3g" % (name, r))
    assert r <= 1
    with pytest.raises(ValueError):
        galaxy.faraday_depth_grid(1.0, 0.5)
    # the default spectrum is the reference's (galaxy.py:244-246) and leaves its argument alone
    l = np.arange(5.0)
    cl = galaxy.polarisation_angular_ps(l)
    assert l[0] == 0 and cl[0] == (1e16 / 100.0) ** -2.8 and np.array_equal(cl[1:], (l[1:] / 100.0) ** -2.8)


@pytest.mark.parametrize("nphi", [2, 6, 18, 32, 34, 1000])
def test_longdouble_idft_against_numpy(nphi):
    """The dense long-double inverse DFT against np.fft.ifft, row by row: ||diff||_2 <= 8 log2(nphi) eps ||row||_2
    (pocketfft's own error is O(log2 n) eps normwise; the long-double product contributes a rounding to double)."""
    rng = np.random.default_rng(nphi)
    x = rng.normal(size=(7, nphi)) + 1j * rng.normal(size=(7, nphi))
    a, b = fo.idft_exact(x), np.fft.ifft(x, axis=1)
    r = np.linalg.norm(a - b, axis=1) / (8 * np.log2(nphi) * EPS * np.linalg.norm(b, axis=1))
    print("nphi %d: worst err / tol %.3g" % (nphi, r.max()))
    assert r.max() <= 1


def test_chunk_var_restated():
    rng = np.random.default_rng(3)
    for n in (1, 63, 12 * 1000):
        a = (rng.normal(size=n) + 1j * rng.normal(size=n)).reshape(-1, 1 if n < 100 else 1000)
        v, m = fo.variance_exact(a)
        assert abs(fo.chunk_var(a) - v) <= 64 * EPS * v + (n == 1) * 1e-300 and abs(m - a.mean()) <= 64 * EPS * abs(m)


class _Untouchable:
    def __getattr__(self, name):
        raise AssertionError("the library was touched (%s) before the arguments were checked" % name)


def _fake_ctx():
    import torch

    from cora_amd._lib import Context

    ctx = Context.__new__(Context)
    ctx.lib = _Untouchable()
    ctx.h = None
    ctx.device = torch.device("cpu")
    return ctx


def test_python_layer_checks_arguments_before_the_library():
    import torch

    ctx = _fake_ctx()
    y = torch.zeros((5, 6), dtype=torch.complex128)
    phi, sigma, A = np.zeros(6), np.ones(5), np.zeros((3, 6), dtype=np.complex128)
    bad = [
        dict(y=torch.zeros((5, 6), dtype=torch.float64)),              # dtype
        dict(y=torch.zeros((5, 7), dtype=torch.complex128), phi=np.zeros(7), A=np.zeros((3, 7), dtype=np.complex128)),  # odd
        dict(y=torch.zeros((5, 6, 1), dtype=torch.complex128)),        # rank
        dict(y=torch.zeros((6, 5), dtype=torch.complex128).T),         # not contiguous
        dict(y=np.zeros((5, 6), dtype=np.complex128)),                 # not a device tensor
        dict(phi=np.zeros(5)), dict(sigma=np.ones(6)), dict(sigma=np.ones((5, 1))),
        dict(A=np.zeros((3, 5), dtype=np.complex128)), dict(A=np.zeros(6, dtype=np.complex128)),
        dict(A=np.zeros((0, 6), dtype=np.complex128)),
        dict(intensity=torch.zeros((3, 4), dtype=torch.float64)),
        dict(intensity=torch.zeros((3, 5), dtype=torch.float32)),
        dict(intensity=np.zeros((3, 5))),
        dict(out=torch.zeros((3, 4), dtype=torch.complex128)),
        dict(out=torch.zeros((3, 5), dtype=torch.float64)),
        dict(intensity=torch.zeros((3, 5), dtype=torch.float64), out=torch.zeros((3, 5), dtype=torch.complex128)),
    ]
    for kw in bad:
        args = dict(y=y, phi=phi, sigma=sigma, A=A, scale=1.0)
        args.update(kw)
        with pytest.raises(ValueError):
            ctx.faraday_mix(**args)
    for t in (torch.zeros(4, dtype=torch.float64), np.zeros(4, dtype=np.complex128), torch.zeros(0, dtype=torch.complex128),
              torch.zeros((4, 4), dtype=torch.complex128)[:, 1]):
        with pytest.raises(ValueError):
            ctx.complex_variance(t)
    ycube = torch.zeros((12, 8), dtype=torch.complex128)
    for maps, k0 in ((torch.zeros((3, 12)), 0), (torch.zeros((4, 12), dtype=torch.float64), 7),
                     (torch.zeros((4, 11), dtype=torch.float64), 0), (torch.zeros((4, 12), dtype=torch.float64), -1),
                     (torch.zeros((4, 12), dtype=torch.float32), 0), (np.zeros((4, 12)), 0)):
        with pytest.raises(ValueError):
            ctx.faraday_pack(maps, ycube, k0)
    with pytest.raises(ValueError):
        ctx.faraday_pack(torch.zeros((4, 12), dtype=torch.float64), torch.zeros((12, 8), dtype=torch.float64), 0)


def test_pipeline_checks_its_inputs_before_the_device(monkeypatch):
    from cora_amd import _lib
    from cora_amd.foreground import galaxy

    def no_context(*a, **k):
        raise AssertionError("the device was touched before the arguments were checked")

    monkeypatch.setattr(_lib, "get_context", no_context)
    freq = 400.0 + 2.0 * np.arange(3)
    good = np.ones(48)
    for sigma in (np.zeros(48), -good, np.where(np.arange(48) == 5, np.nan, 1.0), np.where(np.arange(48) == 5, np.inf, 1.0),
                  np.ones(47)):
        with pytest.raises(ValueError):
            galaxy.polarised_fraction_device(sigma, freq, 2, maxphi=3.0)
    with pytest.raises(ValueError):
        galaxy.polarised_fraction_device(good, freq, 2, maxphi=3.0, base=np.zeros((48, 8), dtype=np.complex128))
    with pytest.raises(ValueError):
        galaxy.polarised_fraction_device(good, freq.reshape(3, 1), 2, maxphi=3.0)
    with pytest.raises(ValueError):
        galaxy.polarised_fraction_device(good, freq, 2, maxphi=0.5)


def test_flat_spectrum_variance_check_passes_on_the_oracle():
    """The statistical check of the drawn path in tests/test_gpu_faraday.py, on the CPU: the oracle's mkfullsky with the
    same numpy seed (the package continues numpy's stream on the device) gives maps whose per-channel mean square is
    within the test's 5 sigma bound, so the seed chosen there is not an unlucky one."""
    from oracle import skysim as osk

    nside, maxphi, seed = fo.DRAWN["nside"], fo.DRAWN["maxphi"], fo.DRAWN["seed"]
    lmax = 3 * nside - 1
    phifreq, pcfreq = fo.depth_grid(1.0, maxphi)
    nphi = len(pcfreq)
    t2 = fo.taper(pcfreq)[0] ** 2
    corr = np.zeros((lmax + 1, 2 * nphi, 2 * nphi))
    i = np.arange(2 * nphi)
    corr[:, i, i] = 0.5 * np.repeat(t2, 2)[None, :]
    maps = osk.mkfullsky(corr, nside, rng=np.random.default_rng(seed))
    power = (maps[0::2] ** 2 + maps[1::2] ** 2).mean(axis=1)
    mean, sigma = fo.flat_power_bound(nside)
    dev = np.abs(power / t2 - mean) / sigma
    print("oracle: worst deviation %.2f sigma (bound 5); exact-covariance sigma / chi2 sigma = %.4f"
          % (dev.max(), fo.pixel_power_sigma(nside, np.full(lmax + 1, 0.5))[1] * 2**0.5 / sigma))
    assert dev.max() <= 5
