"""The polarised-galaxy path on the device (csrc/faraday.hip through cora_amd._lib.Context and
cora_amd.foreground.galaxy) against the numpy oracle of tests/_faraday_oracle.py and the outputs of the reference's own
getpolsky (tests/golden/faraday_vectors.npz).

Tolerances are derived, not tuned (eps = 2^-52, u = eps / 2):

  faraday_mix      per element of z = scale sum_phi A w y, with t = 0.25 (phi / sigma)^2:
                       tol_z = eps scale sum_phi (2 nphi + 16 + 3 t) |A| w |y|.
                   The kernel computes z = (scale / W) sum_phi A (e y), e = exp(-t), W = sum_phi e.  The complex inner
                   product is two real sums of 2 nphi products each, FMA-accumulated: each part is within nphi eps of
                   sum |A| |e y| in any order, the modulus of the error within sqrt(2) nphi eps.  W is a sum of nphi
                   positive terms: nphi u in any order.  Together < 2 nphi eps.  The exponent's argument is formed as
                   q = phi (1 / sigma), t = 0.25 q q: three roundings that count twice, twice and once, 2.5 eps t in
                   e, under 3 t eps.  What is left - exp (1 ulp), the product e y, the errors of e inside W (a
                   w-weighted mean of (2.5 t + 1) eps, about 2.25 eps for Gaussian weights), scale / W and the final
                   product - stays under 8 eps, inside the constant 16.
                   The reference is the oracle in long double on the same y and scale (its error is 2^-11 eps).
                   z -> z tanh|z| / |z| is 1-Lipschitz: tol_P = tol_z + 8 eps |P| (hypot, tanh, quotient, product).
                   Polarised planes: tol_P |T| + eps |P T|.  Plane 0 is T bit for bit, plane 3 exactly 0.
  complex_variance _faraday_oracle.variance_bound: (D + 5) u relative, D the number of additions an element goes
                   through in the kernel's own order, plus the square of the error of the mean.
  pack             exact equality.
  inverse FFT      16 log2(4 nphi) eps ||row||_2 per element (row of the exact result; by Parseval the norm of the input
                   row / sqrt(nphi)): three radix-2 transforms of padded length <= 4 nphi plus the chirp products of
                   Bluestein, each within 4 log2 eps normwise.
Every test prints its worst error over tolerance.  Run with -m gpu."""
import ctypes

import numpy as np
import pytest

import _faraday_oracle as fo

pytestmark = pytest.mark.gpu

EPS = fo.EPS


def _ratio(err, tol):
    """worst err / tol; a non-zero error where the tolerance is zero counts as inf"""
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(tol > 0, err / np.where(tol > 0, tol, 1.0), np.where(err > 0, np.inf, 0.0))
    return float(np.max(r)) if r.size else 0.0


def _cdev(ctx, a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.complex128)).to(ctx.device)


def _host(t):
    return t.cpu().numpy()


def _grid(nphi):
    return np.fft.fftfreq(nphi, d=1.0 / nphi)          # the reference's depth grid with dphi = 1


def _mix_inputs(ncol, nphi, nfreq, seed):
    rng = np.random.default_rng(seed)
    y = rng.standard_normal((ncol, nphi)) + 1j * rng.standard_normal((ncol, nphi))
    sigma = np.exp(rng.uniform(np.log(0.3), np.log(2.0 * nphi + 1.0), ncol))
    # edge columns: all weight in the phi = 0 bin (the other exponentials underflow to exact zeros), uniform weights,
    # an all-zero column, a column that saturates
    idx = rng.permutation(ncol)
    edges = {}
    for name, i in zip(("narrow", "wide", "zero", "big"), idx):
        edges[name] = int(i)
    if "narrow" in edges:
        sigma[edges["narrow"]] = 0.05
    if "wide" in edges:
        sigma[edges["wide"]] = 1e6
    if "zero" in edges:
        y[edges["zero"]] = 0.0
    if "big" in edges:
        y[edges["big"]] *= 1e6
    freq = 400.0 + 2.0 * np.arange(nfreq)
    A = fo.ptrans(_grid(nphi)[:, None], freq[None, :], 2.0).T.copy() * (1.0 + 0.25 * rng.standard_normal((nfreq, nphi)))
    T = rng.uniform(2.0, 30.0, (nfreq, ncol))
    return y, _grid(nphi), sigma, A, 0.7, T, edges


SHAPES = [(1, 18, 130), (15, 6, 3), (17, 2, 16), (127, 32, 17), (129, 1000, 130), (768, 32, 16), (3073, 34, 17),
          (17, 34, 1), (130, 18, 3)]


@pytest.mark.parametrize("ncol,nphi,nfreq", SHAPES)
def test_faraday_mix_matches_oracle(ctx, ncol, nphi, nfreq):
    """Both output forms against the long-double oracle on the same y and scale, under the bounds of the module
    docstring; out pre-filled with NaN, inputs unchanged, a second call bit-identical."""
    import torch

    y, phi, sigma, A, scale, T, edges = _mix_inputs(ncol, nphi, nfreq, 100000 * ncol + 100 * nphi + nfreq)
    z, P = fo.mix_exact(y, scale, phi, sigma, A.T)
    tol_z = fo.z_bound(y, scale, phi, sigma, A.T)
    tol_P = tol_z + 8 * EPS * np.abs(P)
    # the float64 statement-order oracle is itself inside the bound
    _, P64, _ = fo.mix(y, scale, phi, sigma, A.T)
    assert _ratio(np.abs(P64 - P), tol_P) <= 1.0

    yd, Ad, Td = _cdev(ctx, y), _cdev(ctx, A), ctx.to_device(T)
    phid, sigd = ctx.to_device(phi), ctx.to_device(sigma)
    keep = [t.clone() for t in (yd, Ad, Td, phid, sigd)]
    out = torch.empty((nfreq, ncol), dtype=torch.complex128, device=ctx.device)
    torch.view_as_real(out).fill_(float("nan"))
    ctx.faraday_mix(yd, phid, sigd, Ad, scale, out=out)
    got = _host(out).T
    assert np.isfinite(got.real).all() and np.isfinite(got.imag).all()
    worst = _ratio(np.abs(got - P), tol_P)
    out5 = torch.full((nfreq, 4, ncol), float("nan"), dtype=torch.float64, device=ctx.device)
    ctx.faraday_mix(yd, phid, sigd, Ad, scale, intensity=Td, out=out5)
    got5 = _host(out5)
    assert np.isfinite(got5).all()
    assert np.array_equal(got5[:, 0], T) and not got5[:, 3].any() and not np.signbit(got5[:, 3]).any()
    PT = P.T * T
    tol5 = tol_P.T * np.abs(T) + EPS * np.abs(PT)
    worst5 = max(_ratio(np.abs(got5[:, 1] - PT.real), tol5), _ratio(np.abs(got5[:, 2] - PT.imag), tol5))
    print("faraday_mix ncol %d nphi %d nfreq %d: worst err / tol  P %.3g  planes %.3g" % (ncol, nphi, nfreq, worst, worst5))
    assert worst <= 1.0 and worst5 <= 1.0
    for a, b in zip(keep, (yd, Ad, Td, phid, sigd)):
        assert torch.equal(a, b)
    if "zero" in edges:
        assert not got[edges["zero"]].any() and not got5[:, 1:3, edges["zero"]].any()
    if "big" in edges and nphi > 2:
        assert np.all(np.abs(got[edges["big"]]) > 1 - 1e-9) and np.all(np.abs(got) <= 1.0 + 4 * EPS)
    if "narrow" in edges:
        # the only non-zero weight is the phi = 0 bin: z = scale A[:, 0] y[p, 0]
        p = edges["narrow"]
        z0 = scale * A[:, 0] * y[p, 0]
        assert np.all(np.abs(got[p] - fo.saturate(z0)) <= 8 * EPS * np.abs(z0) + tol_P[p])
    assert torch.equal(ctx.faraday_mix(yd, phid, sigd, Ad, scale), out)
    assert torch.equal(ctx.faraday_mix(yd, phid, sigd, Ad, scale, intensity=Td), out5)
    # host arrays for phi, sigma and A give the same bits
    assert torch.equal(ctx.faraday_mix(yd, phi, sigma, A, scale), out)


def test_faraday_mix_refuses_overlap(ctx):
    import torch

    from cora_amd import _lib

    ncol, nphi, nfreq = 17, 6, 3
    buf = torch.zeros(ncol * nphi + nfreq * ncol, dtype=torch.complex128, device=ctx.device)
    y = buf[:ncol * nphi].view(ncol, nphi)
    A = torch.zeros((nfreq, nphi), dtype=torch.complex128, device=ctx.device)
    phi, sigma = ctx.to_device(_grid(nphi)), ctx.to_device(np.ones(ncol))
    T = torch.ones((nfreq, ncol), dtype=torch.float64, device=ctx.device)
    over = buf[ncol * nphi - 1:ncol * nphi - 1 + nfreq * ncol].view(nfreq, ncol)
    with pytest.raises(ValueError):
        ctx.faraday_mix(y, phi, sigma, A, 1.0, out=over)
    over5 = torch.view_as_real(buf).view(-1)[:nfreq * 4 * ncol].view(nfreq, 4, ncol)      # lies over y
    with pytest.raises(ValueError):
        ctx.faraday_mix(y, phi, sigma, A, 1.0, intensity=T, out=over5)
    # the library itself refuses too, before any launch: CORAHIP_EINVAL
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    for out, inten in ((over, None), (T, T), (A, None)):
        rc = ctx.lib.corahip_faraday_mix(ctx.h, p(y), ncol, nphi, p(phi), p(sigma), p(A), nfreq, 1.0,
                                         None if inten is None else p(inten), p(out))
        assert rc == -1, rc
        with pytest.raises(_lib.CoraHipError):
            _lib._check(rc)
    # odd nphi, empty shapes
    assert ctx.lib.corahip_faraday_mix(ctx.h, p(y), ncol, 5, p(phi), p(sigma), p(A), nfreq, 1.0, None, p(T)) == -1
    assert ctx.lib.corahip_faraday_mix(ctx.h, p(y), 0, nphi, p(phi), p(sigma), p(A), nfreq, 1.0, None, p(T)) == -1
    ctx.sync()


@pytest.mark.parametrize("count", [1, 63, 65, 12 * 1000, 3073 * 34])
def test_complex_variance(ctx, count):
    """Against the long-double variance and numpy's chunk_var restated.  Device bound: variance_bound (module
    docstring).  numpy's chunk_var: pairwise sums in blocks of 128 with 8 accumulators (depth <= 16 + log2 count), 30
    chunk sums in sequence, |x|^2 of a complex difference (4 u), the mean likewise: (16 + log2 count + 30 + 8) u."""
    rng = np.random.default_rng(count)
    a = (rng.standard_normal(count) + 1j * rng.standard_normal(count)) * 3.0 + (1.5 - 0.5j)
    a = a.reshape(-1, 34) if count % 34 == 0 else a
    var_x, mean_x = fo.variance_exact(a)
    D, k = fo.variance_bound(count)
    assert D <= count
    d = _cdev(ctx, a)
    var, mean = ctx.complex_variance(d)
    tol_m = (D + 1) * 0.5 * EPS * max(np.abs(a.real).sum(), np.abs(a.imag).sum()) / count
    tol = k * EPS * var_x + 2 * tol_m**2
    tol_np = (16 + np.log2(count) + 30 + 8) * 0.5 * EPS * var_x
    r = _ratio(np.array([abs(var - var_x)]), np.array([tol]))
    rm = max(abs(mean.real - mean_x.real), abs(mean.imag - mean_x.imag)) / tol_m
    rn = _ratio(np.array([abs(var - fo.chunk_var(a))]), np.array([tol + tol_np]))
    print("complex_variance count %d (D = %d): worst err / tol  var %.3g  mean %.3g  against chunk_var %.3g" % (count, D, r, rm, rn))
    assert r <= 1.0 and rm <= 1.0 and rn <= 1.0
    assert ctx.complex_variance(d) == (var, mean)
    assert np.array_equal(_host(d), a.reshape(_host(d).shape))


@pytest.mark.parametrize("npix", [12, 48, 3072])
def test_pack_is_transpose_and_interleave(ctx, npix):
    import torch

    nphi = 40
    rng = np.random.default_rng(npix)
    y = torch.empty((npix, nphi), dtype=torch.complex128, device=ctx.device)
    torch.view_as_real(y).fill_(float("nan"))
    want = np.full((npix, nphi), np.nan + 1j * np.nan)
    for k0, nc in ((3, 1), (5, 3), (21, 16)):
        maps = rng.standard_normal((2 * nc, npix))
        ctx.faraday_pack(ctx.to_device(maps), y, k0)
        want[:, k0:k0 + nc] = (maps[0::2] + 1j * maps[1::2]).T
    got = _host(y)
    assert np.array_equal(got.real, want.real, equal_nan=True) and np.array_equal(got.imag, want.imag, equal_nan=True)
    assert np.isnan(got[:, :3]).all() and np.isnan(got[:, 37:]).all() and np.isfinite(got[:, 21:37].real).all()


@pytest.fixture(scope="module")
def cases():
    return fo.load_golden()


@pytest.mark.parametrize("name", ["a", "b"])
def test_deterministic_pipeline_against_golden(ctx, cases, name):
    """polarised_galaxy_device(base=...) stage by stage (case a: nphi 32, the direct FFT; case b: nphi 6, Bluestein).

    y (debug) against the long-double inverse DFT of base taper under the FFT bound by_el[p] of the module docstring;
    the variance against the long-double variance of the device's own y; the mix against the long-double oracle fed
    the device's y and scale.  map5 against the golden under the sum of the bounds: the golden's y (pocketfft) and the
    device's y are each within by_el of the exact one, so dy = 2 by_el; the two variances differ by their own bounds
    (device: variance_bound; numpy: as in test_complex_variance) plus 2 rms(dy) / sqrt(var) from dy, and scale =
    1 / (2 sqrt(var)) moves by half of that, relatively; the two sums over depth are each within tol_z:
        tol_z5 = 2 tol_z + scale (dy w) |pta| + |z| rel_scale,   tol_P5 = tol_z5 + 16 eps |P|,
        map5:  tol_P5 T + 2 eps |map5|."""
    from cora_amd.foreground import galaxy
    from cora_amd.util import hputil

    c = cases[name]
    sigma = c["sigma_phi"]
    phifreq, pcfreq = fo.depth_grid(c["dphi"], c["maxphi"])
    nphi = len(phifreq)
    npix = 12 * c["nside"] ** 2
    kw = dict(maxphi=c["maxphi"], dphi=c["dphi"], base=c["base"])
    map5, yd, var, A = galaxy.polarised_galaxy_device(c["T"], sigma, c["freq"], c["nside"], celestial=False, debug=True, **kw)
    y, got5 = _host(yd), _host(map5)
    assert got5.shape == (len(c["freq"]), 4, npix) and np.array_equal(A.T, c["pta"])

    y_x = fo.idft_exact(c["base"] * fo.taper(pcfreq))
    by_el = 16 * np.log2(4 * nphi) * EPS * np.linalg.norm(y_x, axis=1)
    r_fft = _ratio(np.abs(y - y_x), np.broadcast_to(by_el[:, None], y.shape))

    var_x, _ = fo.variance_exact(y)
    D, k = fo.variance_bound(y.size)
    tol_m = (D + 1) * 0.5 * EPS * max(np.abs(y.real).sum(), np.abs(y.imag).sum()) / y.size
    rel_var = k * EPS + 2 * tol_m**2 / var_x
    r_var = abs(var - var_x) / (rel_var * var_x)

    scale = 1.0 / (2.0 * var**0.5)
    z, P = fo.mix_exact(y, scale, phifreq, sigma, c["pta"])
    tol_z = fo.z_bound(y, scale, phifreq, sigma, c["pta"])
    tol_P = tol_z + 8 * EPS * np.abs(P)
    PT = P.T * c["T"]
    tol5 = tol_P.T * c["T"] + EPS * np.abs(PT)
    r_mix = max(_ratio(np.abs(got5[:, 1] - PT.real), tol5), _ratio(np.abs(got5[:, 2] - PT.imag), tol5))
    assert np.array_equal(got5[:, 0], c["T"]) and not got5[:, 3].any()

    dy = 2 * by_el
    rel_np = (16 + np.log2(y.size) + 30 + 8) * 0.5 * EPS
    rel_scale = 0.5 * (rel_var + rel_np + 2 * np.sqrt(np.mean(dy**2)) / np.sqrt(var_x))
    tol_z5 = 2 * tol_z + scale * ((dy[:, None] * c["w"]) @ np.abs(c["pta"])) + np.abs(z) * rel_scale
    tol_P5 = tol_z5 + 16 * EPS * np.abs(P)
    tolg = np.zeros_like(c["map5"])
    tolg[:, 1] = tolg[:, 2] = tol_P5.T * c["T"]
    tolg += 2 * EPS * np.abs(c["map5"])
    r_gold = _ratio(np.abs(got5 - c["map5"]), tolg)
    print("case %s (nphi %d): worst err / tol  fft %.3g  variance %.3g  mix %.3g  map5 against golden %.3g"
          % (name, nphi, r_fft, r_var, r_mix, r_gold))
    assert r_fft <= 1.0 and r_var <= 1.0 and r_mix <= 1.0 and r_gold <= 1.0

    # the fraction alone is the same P, and the celestial form is the existing rotation of the galactic one
    Pd = galaxy.polarised_fraction_device(sigma, c["freq"], c["nside"], **kw)
    assert np.array_equal(_host(Pd).real * c["T"], got5[:, 1]) and np.array_equal(_host(Pd).imag * c["T"], got5[:, 2])
    cel = galaxy.polarised_galaxy(c["T"], sigma, c["freq"], c["nside"], celestial=True, **kw)
    rot = hputil.rotate_map_device(map5.reshape(-1, npix), hputil.coord_matrix("C", "G"))
    assert cel.shape == got5.shape and np.array_equal(cel.reshape(-1, npix), _host(rot))


def test_drawn_path(ctx):
    """nside 8, maxphi 8 (nphi 16), 4 channels.  The same DeviceRNG seed twice gives identical bits; |Q + iU| < T for
    positive T; the variance of y scale is 1/4 within the variance bound (+ 4 eps for the square root, the quotient
    and the square)."""
    import torch

    from cora_amd.foreground import galaxy
    from cora_amd.util.nputil import DeviceRNG

    nside, maxphi, nfreq = fo.DRAWN["nside"], fo.DRAWN["maxphi"], fo.DRAWN["nfreq"]
    npix = 12 * nside * nside
    rng = np.random.default_rng(5)
    sigma = np.exp(rng.uniform(np.log(0.3), np.log(20.0), npix))
    T = rng.uniform(2.0, 30.0, (nfreq, npix))
    freq = 400.0 + 2.0 * np.arange(nfreq)
    a, y, var, A = galaxy.polarised_galaxy_device(T, sigma, freq, nside, rng=DeviceRNG(77), celestial=False, maxphi=maxphi,
                                                  debug=True)
    b = galaxy.polarised_galaxy_device(T, sigma, freq, nside, rng=DeviceRNG(77), celestial=False, maxphi=maxphi)
    other = galaxy.polarised_galaxy_device(T, sigma, freq, nside, rng=DeviceRNG(78), celestial=False, maxphi=maxphi)
    assert torch.equal(a, b) and not torch.equal(a, other)
    m = _host(a)
    assert m.shape == (nfreq, 4, npix) and np.isfinite(m).all()
    pol = np.hypot(m[:, 1], m[:, 2])
    assert np.all(pol < m[:, 0]) and np.array_equal(m[:, 0], T) and pol.max() > 0.05 * T.min()

    yh = _host(y)
    assert yh.shape == (npix, 16)
    var_x, _ = fo.variance_exact(yh)
    D, k = fo.variance_bound(yh.size)
    tol_m = (D + 1) * 0.5 * EPS * max(np.abs(yh.real).sum(), np.abs(yh.imag).sum()) / yh.size
    scale = 1.0 / (2.0 * var**0.5)
    tol = 0.25 * (k * EPS + 2 * tol_m**2 / var_x + 4 * EPS)
    r = abs(scale * scale * var_x - 0.25) / tol
    print("drawn path: |var(y scale) - 1/4| / tol %.3g" % r)
    assert r <= 1.0


def test_drawn_maps_have_the_flat_spectrum_variance(ctx):
    """With angular(l) = 1 the mean square of conj-depth map k is taper_k^2 sum_l (2l+1) / (4 pi) in expectation: its
    real and imaginary parts are independent fields with C_l = taper_k^2 / 2, and the mean square over the pixels of a
    band-limited field with a_lm of variance C_l is C chi^2_N / (4 pi) with N = sum_l (2l+1) = (lmax + 1)^2 degrees of
    freedom (mean N, variance 2 N).  For the two parts together: mean taper^2 N / (4 pi), sigma taper^2 sqrt(N) /
    (4 pi); the check is 5 sigma.  (The pixel sum is not an exact quadrature at lmax = 3 nside - 1; the expectation is
    exact all the same and sigma from the exact pixel covariance is 1 % larger, tests/test_faraday_host.py.)  The maps
    continue numpy's stream of the given seed, so the CPU oracle draws the same fields:
    test_flat_spectrum_variance_check_passes_on_the_oracle shows that the seed passes there."""
    from cora_amd.foreground import galaxy

    nside, maxphi, seed = fo.DRAWN["nside"], fo.DRAWN["maxphi"], fo.DRAWN["seed"]
    phifreq, pcfreq = fo.depth_grid(1.0, maxphi)
    nphi = len(pcfreq)
    base = galaxy.faraday_base_maps_device(nside, pcfreq, rng=np.random.default_rng(seed), angular=lambda l: 1.0, chunk=nphi)
    m = _host(base)
    assert m.shape == (12 * nside * nside, nphi)
    power = (np.abs(m) ** 2).mean(axis=0)
    mean, sigma = fo.flat_power_bound(nside)
    dev = np.abs(power / fo.taper(pcfreq)[0] ** 2 - mean) / sigma
    print("flat spectrum: worst deviation %.2f sigma (bound 5)" % dev.max())
    assert dev.max() <= 5
    # drawn in chunks the maps are other numbers of the same distribution
    m2 = _host(galaxy.faraday_base_maps_device(nside, pcfreq, rng=np.random.default_rng(seed), angular=lambda l: 1.0, chunk=3))
    dev2 = np.abs((np.abs(m2) ** 2).mean(axis=0) / fo.taper(pcfreq)[0] ** 2 - mean) / sigma
    print("flat spectrum, chunks of 3: worst deviation %.2f sigma" % dev2.max())
    assert np.isfinite(m2).all() and dev2.max() <= 5


def test_cube_that_does_not_fit_is_refused_before_allocation(ctx):
    import torch

    from cora_amd.foreground import galaxy

    before = torch.cuda.memory_allocated()
    with pytest.raises(MemoryError):
        galaxy.polarised_fraction_device(np.ones(12 * 512**2), 400.0 + np.arange(2.0), 512, maxphi=5000.0)    # 503 GB
    assert torch.cuda.memory_allocated() == before
