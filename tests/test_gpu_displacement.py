"""The displacement-field step on the device (csrc/sht_der1.hip through Context.alm2map_der1 / radial_gradient,
cora_amd.signal.lssutil and cora_amd.signal.lss) against the numpy oracle of tests/_grad_oracle.py.

Every comparison of a derivative map with the ladder oracle uses the DERIVED per-ring tolerance
(_grad_oracle.tolerances): the project's gate for one scalar synthesis, 1e-11 rms of the map, propagated through
(x S[a1] - S[a2]) / sin theta and S[a3] / sin theta.  Each test prints the device's worst error / tolerance per ring
group.  Run with -m gpu."""
import numpy as np
import pytest

import _grad_oracle as go
import _za_oracle as zo

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps


def _to_dev_alm(ctx, alm, lmax):
    import torch

    return ctx.alm_packed_to_dev(torch.from_numpy(np.ascontiguousarray(alm, dtype=np.complex128)).to(ctx.device), lmax)


def _ring_groups(nside):
    """name -> ring indices (0-based): the three rings next to each pole, the rest of the caps, the belt."""
    nring = 4 * nside - 1
    r = np.arange(nring)
    polar = (r < 3) | (r >= nring - 3)
    belt = (r >= nside - 1) & (r <= 3 * nside - 1)
    return {"polar": r[polar], "cap": r[~polar & ~belt], "belt": r[belt]}


def _check_maps(label, got, ref, tol_ring, nside):
    """got, ref [npix]; tol_ring [nring]: every pixel within its ring's tolerance; prints worst err / tol per group."""
    from oracle import healpix

    ri = healpix.ring_info(nside)
    err = np.abs(got - ref)
    worst = np.maximum.reduceat(err, ri["start"])
    ok = True
    parts = []
    for name, rings in _ring_groups(nside).items():
        if rings.size == 0:
            continue
        t = tol_ring[rings]
        ratio = np.where(t > 0, worst[rings] / np.where(t > 0, t, 1.0), np.where(worst[rings] > 0, np.inf, 0.0))
        parts.append("%s %.2e" % (name, ratio.max()))
        ok &= bool((worst[rings] <= t).all())
    print("%s: worst err / tol  %s" % (label, "  ".join(parts)))
    return ok


@pytest.mark.parametrize("nside,lmax,nnu", [(8, 23, 3), (32, 95, 8), (64, 191, 5), (64, 128, 12), (16, 47, 1)])
def test_alm2map_der1_matches_ladder(ctx, nside, lmax, nnu):
    rng = np.random.default_rng(1000 * nside + nnu)
    alm = go.random_alm(rng, lmax, nnu)
    if nnu > 1:
        alm[1] = go.random_alm(rng, lmax, 1, 3.0)[0]
    if nnu > 2:
        alm[-1] = 0.0
    dev = _to_dev_alm(ctx, alm, lmax)
    keep = dev.clone()
    dth, dph = ctx.alm2map_der1(dev, nside, lmax, nnu)
    assert bool((dev == keep).all())                                   # inputs unchanged
    dth_h, dph_h = dth.cpu().numpy(), dph.cpu().numpy()
    rth, rph = go.der1_ladder(alm, nside, lmax)
    tt, tp = go.tolerances(alm, nside, lmax)
    ok = True
    for k in range(nnu):
        ok &= _check_maps("nside %d lmax %d ch %d theta" % (nside, lmax, k), dth_h[k], rth[k], tt[k], nside)
        ok &= _check_maps("nside %d lmax %d ch %d phi" % (nside, lmax, k), dph_h[k], rph[k], tp[k], nside)
    assert ok
    if nnu > 2:
        assert not dth_h[-1].any() and not dph_h[-1].any()             # the zero channel is exactly zero
    # the chunked path (a budget that holds one group of four fields) equals the unchunked one
    small = ctx.alm2map_der1_bytes(nside, lmax, 4)
    cth, cph = ctx.alm2map_der1(dev, nside, lmax, nnu, max_bytes=small)
    for a, b in ((cth, dth), (cph, dph)):
        assert float((a - b).abs().max()) <= 1e-13 * float(b.abs().max())
    # per-field factors and the second 1 / sin theta are applied by the combining kernel
    from oracle import healpix

    st = ctx.to_device(rng.uniform(0.5, 2.0, nnu))
    sp = ctx.to_device(rng.uniform(0.5, 2.0, nnu))
    sth_pix = ctx.to_device(go.per_pixel(nside, healpix.ring_info(nside)["sth"]))
    fth, fph = ctx.alm2map_der1(dev, nside, lmax, nnu, scale_theta=st, scale_phi=sp, phi_extra=1)
    assert float((fth - dth * st[:, None]).abs().max()) <= 1e-13 * float(fth.abs().max())
    assert float((fph - dph * sp[:, None] / sth_pix[None, :]).abs().max()) <= 1e-13 * float(fph.abs().max())


def test_hputil_alm2map_der1_api(ctx):
    from cora_amd.util import hputil
    from oracle import sht as osht

    nside, lmax = 16, 40
    alm = go.random_alm(np.random.default_rng(4), lmax, 1, 3.0)[0]
    got = hputil.alm2map_der1(alm, nside)
    assert got.shape == (3, 12 * nside * nside)
    ref = osht.alm2map(alm, nside, lmax)
    assert np.abs(got[0] - ref).max() <= 1e-11 * ref.std()
    rth, rph = go.der1_ladder(alm, nside, lmax)
    tt, tp = go.tolerances(alm, nside, lmax)
    assert _check_maps("hputil.alm2map_der1 theta", got[1], rth, tt, nside)
    assert _check_maps("hputil.alm2map_der1 phi", got[2], rph, tp, nside)


def test_single_modes_nside1024_all_pixels(ctx):
    """a_10, a_11, a_20, a_22 alone and summed on the (1024, 2048) plan against the elementary derivatives of
    Y_10, Y_11, Y_20, Y_22: every ring, every ring-FFT class, both hemispheres at full size."""
    from oracle import healpix
    from oracle import sht as osht

    nside, lmax = 1024, 2048
    nalm = (lmax + 1) * (lmax + 2) // 2
    modes = [((1, 0), 1.3 + 0j), ((1, 1), 0.7 - 0.4j), ((2, 0), -0.9 + 0j), ((2, 2), 0.5 + 0.8j)]
    alm = np.zeros((5, nalm), dtype=np.complex128)
    for k, ((l, m), a) in enumerate(modes):
        alm[k, osht.alm_index(l, m, lmax)] = a
        alm[4, osht.alm_index(l, m, lmax)] = a
    ri = healpix.ring_info(nside)
    z, s = go.per_pixel(nside, ri["z"]), go.per_pixel(nside, ri["sth"])
    npix = 12 * nside * nside
    j = np.arange(npix) - np.repeat(ri["start"], ri["nphi"])
    phi = np.repeat(ri["phi0"], ri["nphi"]) + 2.0 * np.pi * j / np.repeat(ri["nphi"], ri["nphi"])
    e1, e2 = np.exp(1j * phi), np.exp(2j * phi)
    k10, k11, k20, k22 = np.sqrt(3 / (4 * np.pi)), -np.sqrt(3 / (8 * np.pi)), np.sqrt(5 / (16 * np.pi)), \
        0.25 * np.sqrt(15 / (2 * np.pi))
    a10, a11, a20, a22 = (a for _, a in modes)
    ref_t = np.zeros((5, npix))
    ref_p = np.zeros((5, npix))
    ref_t[0] = -a10.real * k10 * s                                     # Y_10 = k cos
    ref_t[1] = 2.0 * (a11 * k11 * z * e1).real                         # Y_11 = k sin e^{i phi}
    ref_p[1] = 2.0 * (a11 * 1j * k11 * e1).real
    ref_t[2] = a20.real * k20 * (-6.0 * z * s)                         # Y_20 = k (3 cos^2 - 1)
    ref_t[3] = 2.0 * (a22 * k22 * 2.0 * s * z * e2).real               # Y_22 = k sin^2 e^{2 i phi}
    ref_p[3] = 2.0 * (a22 * 2j * k22 * s * e2).real
    ref_t[4], ref_p[4] = ref_t[:4].sum(axis=0), ref_p[:4].sum(axis=0)
    dth, dph = ctx.alm2map_der1(_to_dev_alm(ctx, alm, lmax), nside, lmax, 5)
    dth, dph = dth.cpu().numpy(), dph.cpu().numpy()
    tt, tp = go.tolerances(alm, nside, lmax)
    ok = True
    for k in range(5):
        ok &= _check_maps("single modes ch %d theta" % k, dth[k], ref_t[k], tt[k], nside)
        ok &= _check_maps("single modes ch %d phi" % k, dph[k], ref_p[k], tp[k], nside)
    assert ok


def test_fullsize_selected_rings(ctx):
    """nside 1024, lmax 2048, 8 fields with l^-3 spectra on polar rings, a non-power-of-two cap ring, both belt edges,
    the equator and their southern mirrors, against the ladder oracle; the CPU restatement of the closed form must
    itself stay within a tenth of the tolerance, so the yardstick cannot hide a failure."""
    from oracle import healpix

    nside, lmax, nf = 1024, 2048, 8
    rings1 = [1, 2, 3, 683, 1023, 1024, 2048, 3072, 3413, 4093, 4094, 4095]
    rings = [r - 1 for r in rings1]
    alm = go.random_alm(np.random.default_rng(77), lmax, nf, 3.0)
    dth, dph = ctx.alm2map_der1(_to_dev_alm(ctx, alm, lmax), nside, lmax, nf)
    ri = healpix.ring_info(nside)
    tt, tp = go.tolerances(alm, nside, lmax)
    lad = go.der1_ladder(alm, nside, lmax, rings=rings)
    com = go.der1_composed(alm, nside, lmax, rings=rings)
    ok = True
    for k, r in enumerate(rings):
        s, n = int(ri["start"][r]), int(ri["nphi"][r])
        gt, gp = dth[:, s:s + n].cpu().numpy(), dph[:, s:s + n].cpu().numpy()
        et, ep = np.abs(gt - lad[k][0]).max(axis=1), np.abs(gp - lad[k][1]).max(axis=1)
        ct, cp = np.abs(com[k][0] - lad[k][0]).max(axis=1), np.abs(com[k][1] - lad[k][1]).max(axis=1)
        std = lad[k][0].std(axis=1)
        print("ring %4d: device err/tol theta %.2e phi %.2e | err/ring std theta %.2e | cpu closed form err/tol theta %.2e "
              "phi %.2e" % (rings1[k], (et / tt[:, r]).max(), (ep / tp[:, r]).max(), (et / std).max(),
                            (ct / tt[:, r]).max(), (cp / tp[:, r]).max()))
        assert (ct <= 0.1 * tt[:, r]).all() and (cp <= 0.1 * tp[:, r]).all(), rings1[k]
        ok &= bool((et <= tt[:, r]).all() and (ep <= tp[:, r]).all())
    assert ok


def _np_gradient_terms(f, x):
    """numpy's own coefficients: sum of |a f[i-1]| + |b f[i]| + |c f[i+1]| per element (one-sided pair at the ends)."""
    d = np.diff(x)
    hs, hd = d[:-1, None], d[1:, None]
    a, b, c = -hd / (hs * (hd + hs)), (hd - hs) / (hd * hs), hs / (hd * (hd + hs))
    t = np.empty_like(f)
    t[1:-1] = np.abs(a * f[:-2]) + np.abs(b * f[1:-1]) + np.abs(c * f[2:])
    t[0] = (np.abs(f[0]) + np.abs(f[1])) / abs(d[0])
    t[-1] = (np.abs(f[-1]) + np.abs(f[-2])) / abs(d[-1])
    return t


@pytest.mark.parametrize("n", [2, 3, 7, 33])
@pytest.mark.parametrize("npix", [12 * 16 ** 2, 1000003])
def test_radial_gradient_matches_numpy(ctx, n, npix):
    rng = np.random.default_rng(n * 7 + npix % 11)
    worst = 0.0
    for case, (sign, scaled, offset) in enumerate([(1.0, False, 0.0), (-1.0, True, 0.0), (1.0, True, 1e6)]):
        x = sign * (50.0 + np.cumsum(rng.uniform(0.5, 3.0, n)))
        f = rng.normal(size=(n, npix)) + offset
        s_r = rng.uniform(-2.0, 2.0, n) if scaled else None
        fd = ctx.to_device(f)
        keep = fd.clone()
        got = ctx.radial_gradient(fd, x, scale=s_r).cpu().numpy()
        assert bool((fd == keep).all())
        sr = np.ones(n) if s_r is None else s_r
        ref = np.gradient(f, x, axis=0) * sr[:, None]
        bound = 4.0 * EPS * np.abs(sr)[:, None] * _np_gradient_terms(f, x)
        ratio = (np.abs(got - ref) / bound).max()
        worst = max(worst, ratio)
        assert ratio <= 1.0, (n, npix, case, ratio)
    print("radial_gradient n %d npix %d: worst err / bound %.3f" % (n, npix, worst))


def test_radial_gradient_rejects_overlap_and_bad_shapes(ctx):
    from cora_amd import _lib

    n, npix = 4, 768
    buf = ctx.empty((2 * n, npix))
    buf.zero_()
    x = np.arange(n, dtype=np.float64)
    with pytest.raises(ValueError):
        ctx.radial_gradient(buf[:n], x, out=buf[:n])
    with pytest.raises(ValueError):
        ctx.radial_gradient(buf[:n], x, out=buf[2:n + 2])
    ctx.radial_gradient(buf[:n], x, out=buf[n:])                       # adjacent, not overlapping: fine
    with pytest.raises(ValueError):
        ctx.radial_gradient(buf[:n], x[:-1])
    with pytest.raises(ValueError):
        ctx.radial_gradient(buf[:1], x[:1])
    # the C ABI refuses what it cannot take instead of faulting
    coef = ctx.to_device(np.zeros((n, 3)))
    with pytest.raises(_lib.CoraHipError):
        _lib._check(ctx.lib.corahip_radial_gradient(ctx.h, ctx._f64(buf), ctx._f64(coef), None, 1, npix, ctx._f64(buf[n:])))
    with pytest.raises(_lib.CoraHipError):
        _lib._check(ctx.lib.corahip_der1_alm_prep(ctx.h, ctx.sht_plan(8, 23), ctx._f64(buf), 2, 1, 2, ctx._f64(buf)))
    with pytest.raises(_lib.CoraHipError):
        _lib._check(ctx.lib.corahip_der1_combine(ctx.h, ctx.sht_plan(8, 23), ctx._f64(buf), 1, 5, None, None, 0,
                                                 ctx._f64(buf), ctx._f64(buf)))
    with pytest.raises(_lib.CoraHipError):
        _lib._check(ctx.lib.corahip_der1_combine(ctx.h, ctx.sht_plan(8, 23), ctx._f64(buf), 1, 4, None, None, 2,
                                                 ctx._f64(buf), ctx._f64(buf)))


def _smooth_maps(ctx, nside, lmax_in, n, seed, amp=1.0):
    alm = amp * go.random_alm(np.random.default_rng(seed), lmax_in, n, 3.0)
    return ctx.alm2map(_to_dev_alm(ctx, alm, lmax_in), nside, lmax_in, n), alm


@pytest.mark.parametrize("lmax", [None, 48])
def test_gradient_device_matches_oracle(ctx, lmax):
    import torch
    from cora_amd.signal import lssutil
    from cora_amd.util import hputil
    from oracle import sht as osht

    nside, n = 32, 6
    npix = 12 * nside * nside
    lm = 3 * nside - 1 if lmax is None else lmax
    rng = np.random.default_rng(21)
    maps, _ = _smooth_maps(ctx, nside, 95, n, 20)
    maps = maps + ctx.to_device(1e-3 * rng.normal(size=(n, npix)))     # not band-limited: the iterations matter
    x = 900.0 + np.cumsum(rng.uniform(2.0, 9.0, n))
    out = torch.full((3, n, npix), 7.0, dtype=torch.float64, device=ctx.device)
    grad = lssutil.gradient_device(maps, x, out=out, lmax=lmax)
    assert grad is out
    g = grad.cpu().numpy()
    mh = maps.cpu().numpy()
    # the coefficients the device's own analysis produced: isolates the new code
    adev = hputil.map2alm_device(maps, nside, lm, use_weights=True, niter=3)
    sq = ctx.alm_dev_to_square(adev, lm, n).cpu().numpy()[:, 0]
    packed = np.stack([hputil.pack_alm(sq[i], lm) for i in range(n)])
    for i in range(n):
        ref = osht.map2alm(mh[i], nside, lm, True, 3)
        assert np.abs(packed[i] - ref).max() <= 1e-11 * np.abs(ref).max()
    ref = go.gradient(mh, x, lambda i: packed[i], nside, lm)
    tt, tp = go.tolerances(packed, nside, lm)
    ok = True
    for i in range(n):
        ok &= _check_maps("gradient lmax %d map %d theta" % (lm, i), g[1, i], ref[1, i], tt[i] / x[i], nside)
        ok &= _check_maps("gradient lmax %d map %d phi" % (lm, i), g[2, i], ref[2, i], tp[i] / x[i], nside)
    assert ok
    assert (np.abs(g[0] - ref[0]) <= 4.0 * EPS * _np_gradient_terms(mh, x)).all()
    # grad0=False leaves the radial component zero
    out.fill_(7.0)
    g0 = lssutil.gradient_device(maps, x, grad0=False, out=out, lmax=lmax).cpu().numpy()
    assert not g0[0].any()
    assert np.abs(g0[1:] - g[1:]).max() <= 1e-13 * np.abs(g[1:]).max()
    # numpy in, numpy out
    gh = lssutil.gradient(mh, x, lmax=lmax)
    assert gh.shape == (3, n, npix)
    for c in range(3):
        assert np.abs(gh[c] - g[c]).max() <= 1e-12 * np.abs(g[c]).max()


def _scaled(g, D, f, sth):
    """lss.py:815-828 applied in numpy to the plain gradient."""
    fac = D if f is None else D * (1.0 + f)
    return np.stack([g[0] * fac[:, None], g[1] * D[:, None], g[2] * D[:, None] / sth[None, :]])


def test_zeldovich_displacement_fuses_the_scalings(ctx):
    from cora_amd.signal import lss, lssutil
    from oracle import healpix

    nside, nchi, lmax = 64, 9, 128
    rng = np.random.default_rng(31)
    phi, _ = _smooth_maps(ctx, nside, 64, nchi, 30)
    chi = 1500.0 + np.cumsum(rng.uniform(3.0, 8.0, nchi))
    D = rng.uniform(0.4, 0.9, nchi)
    f = rng.uniform(0.7, 1.0, nchi)
    g = lssutil.gradient_device(phi, chi, lmax=lmax).cpu().numpy()
    sth = go.per_pixel(nside, healpix.ring_info(nside)["sth"])
    for ff in (f, None):
        psi = lss.zeldovich_displacement_device(phi, ctx.to_device(chi), D, ff, lmax=lmax).cpu().numpy()
        assert psi.shape == (3, nchi, 12 * nside * nside)
        ref = _scaled(g, D, ff, sth)
        assert np.isfinite(psi[2]).all()
        for c in range(3):
            err = np.abs(psi[c] - ref[c]).max() / np.abs(ref[c]).max()
            print("zeldovich_displacement component %d (f %s): %.2e" % (c, "given" if ff is not None else "None", err))
            assert err <= 1e-13, (c, err)
    # numpy in, numpy out
    ph = lss.zeldovich_displacement(phi.cpu().numpy(), chi, D, f, lmax=lmax)
    ref = _scaled(g, D, f, sth)
    for c in range(3):
        assert np.abs(ph[c] - ref[c]).max() <= 1e-12 * np.abs(ref[c]).max()


def test_zeldovich_density_matches_oracle(ctx):
    from cora_amd.signal import lss

    nside, nchi, lmax = 32, 8, 64
    npix = 12 * nside * nside
    rng = np.random.default_rng(41)
    phi, _ = _smooth_maps(ctx, nside, 32, nchi, 40, amp=10.0)
    chi = 800.0 + 8.0 * np.arange(nchi) + rng.uniform(-1.0, 1.0, nchi)
    D = rng.uniform(0.5, 0.9, nchi)
    f = rng.uniform(0.7, 1.0, nchi)
    delta = ctx.to_device(rng.normal(0, 0.8, (nchi, npix)))
    db = ctx.to_device(rng.normal(0, 0.4, (nchi, npix)))
    got = lss.zeldovich_density_device(phi, delta, db, chi, D, f, lmax=lmax).cpu().numpy()
    psi = lss.zeldovich_displacement_device(phi, chi, D, f, lmax=lmax).cpu().numpy()
    dbh, dmh = db.cpu().numpy(), delta.cpu().numpy() * D[:, None]
    ref = zo.za_density_sph(psi, dbh, dmh, chi, np.zeros((nchi, npix)))
    err = np.abs(got - ref).max() / np.abs(ref + 1).max()
    print("zeldovich_density vs oracle: %.2e; |psi| max r %.2f, theta %.3f rad (pixel %.3f)" % (
        err, np.abs(psi[0]).max(), np.abs(psi[1]).max(), np.sqrt(4 * np.pi / npix)))
    assert err <= 1e-12, err
    mass = (got + 1).sum()
    assert abs(mass - (1 + dbh).sum()) <= 1e-12 * (1 + dbh).sum()
    # numpy in, numpy out
    gh = lss.zeldovich_density(phi.cpu().numpy(), delta.cpu().numpy(), dbh, chi, D, f, lmax=lmax)
    assert np.abs(gh - got).max() <= 1e-12 * np.abs(got + 1).max()
    # no growth: nothing moves, the result is the SPH-smoothed biased field
    zero = np.zeros(nchi)
    psi0 = lss.zeldovich_displacement_device(phi, chi, zero, f, lmax=lmax)
    assert not bool(psi0.any())
    got0 = lss.zeldovich_density_device(phi, delta, db, chi, zero, f, lmax=lmax).cpu().numpy()
    ref0 = zo.za_density_sph(np.zeros((3, nchi, npix)), dbh, np.zeros((nchi, npix)), chi, np.zeros((nchi, npix)))
    assert np.abs(got0 - ref0).max() <= 1e-12 * np.abs(ref0 + 1).max()


def test_working_size_memory_and_mass(ctx):
    """One call at working size (nside 1024, 16 slices, lmax 2048): finite, mass conserved, and the peak device memory
    within what the docstring of zeldovich_density_device states."""
    import torch
    from cora_amd.signal import lss, lssutil

    nside, nchi, lmax = 1024, 16, 2048
    npix = 12 * nside * nside
    rng = np.random.default_rng(51)
    phi = ctx.empty((nchi, npix))
    for c0 in range(0, nchi, 4):                                       # (host a_lm four slices at a time)
        part, _ = _smooth_maps(ctx, nside, lmax, 4, 50 + c0, amp=0.1)
        phi[c0:c0 + 4] = part
        del part
    g = torch.Generator(device=ctx.device).manual_seed(5)
    delta = 0.8 * torch.randn((nchi, npix), dtype=torch.float64, device=ctx.device, generator=g)
    db = 0.4 * torch.randn((nchi, npix), dtype=torch.float64, device=ctx.device, generator=g)
    chi = 1000.0 + 5.0 * np.arange(nchi) + rng.uniform(-0.5, 0.5, nchi)
    D = rng.uniform(0.5, 0.9, nchi)
    f = rng.uniform(0.7, 1.0, nchi)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated(ctx.device)
    torch.cuda.reset_peak_memory_stats(ctx.device)
    out = lss.zeldovich_density_device(phi, delta, db, chi, D, f, lmax=lmax)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated(ctx.device) - base
    budget = 5 * nchi * npix * 8 + lssutil.gradient_bytes(nside, lmax)
    print("working size: peak device memory beyond the inputs %.2f GB, stated bound %.2f GB (gradient_bytes %.2f GB)" % (
        peak / 1e9, budget / 1e9, lssutil.gradient_bytes(nside, lmax) / 1e9))
    assert bool(torch.isfinite(out).all())
    total = float((1 + db).sum())
    assert abs(float((out + 1).sum()) - total) <= 1e-12 * total
    assert peak <= budget, (peak, budget)
