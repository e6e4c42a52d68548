"""The constrained-galaxy kernels (csrc/galaxy.hip) and ``ConstrainedGalaxy`` on the GPU against the oracles of
tests/_galaxy_oracle.py, whose module docstring derives every tolerance used here (eps = 2^-52, u = eps / 2; none is
tuned), and against the reference's own outputs (tests/golden/galaxy_vectors.npz).  tests/test_galaxy_host.py pins the
oracles to the reference first.  Every test prints its worst error over tolerance."""
import functools
import os

import numpy as np
import pytest

import _galaxy_oracle as go
import _pointsource_oracle as po
from test_galaxy_host import getsky_inputs

pytestmark = pytest.mark.gpu

EPS, U, LD = go.EPS, go.U, go.LD


@pytest.fixture(scope="module")
def gold():
    return go.load_golden()


def _poisoned(ctx, shape):
    import torch

    return torch.full(shape, float("nan"), dtype=torch.float64, device=ctx.device)


# ---- reorder -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nmap", [1, 3])
@pytest.mark.parametrize("nside", [1, 2, 4, 16])
def test_reorder(ctx, nside, nmap):
    import torch

    from cora_amd.util import hputil

    npix = 12 * nside * nside
    m = np.random.default_rng(nside + nmap).integers(-50, 50, (nmap, npix)).astype(np.float64)
    d = ctx.to_device(m)
    nest = ctx.healpix_reorder(d, True, out=_poisoned(ctx, (nmap, npix)))
    ring = ctx.healpix_reorder(d, False, out=_poisoned(ctx, (nmap, npix)))
    assert np.array_equal(nest.cpu().numpy(), go.reorder(m, True)) and np.array_equal(ring.cpu().numpy(), go.reorder(m, False))
    assert torch.equal(ctx.healpix_reorder(nest, False), d) and torch.equal(ctx.healpix_reorder(ring, True), d)
    # the public front end: numpy in, numpy out; a tensor stays on the device; one map or several
    assert np.array_equal(hputil.reorder(m, r2n=True), go.reorder(m, True))
    assert np.array_equal(hputil.reorder(m[0], inp="NESTED", out="RING"), go.reorder(m[:1], False)[0])
    assert torch.equal(hputil.reorder(d, n2r=True), ring)
    # against the ud_grade kernel: the 4^k children of a NESTED pixel are neighbours, and integer sums are exact
    k = 1
    while nside >> k >= 1:
        coarse = nest.cpu().numpy().reshape(nmap, -1, 4 ** k).mean(axis=2)
        assert np.array_equal(go.reorder(coarse, False), hputil.ud_grade(m, nside >> k))
        k += 1
    with pytest.raises(ValueError, match="overlaps"):
        ctx.healpix_reorder(d, True, out=d)
    print("reorder nside %d nmap %d: exact, worst err / tol 0" % (nside, nmap))


# ---- block variance ------------------------------------------------------------------------------------------------------

VAR_SHAPES = [(1, 1), (2, 1), (4, 2), (8, 1), (32, 16), (64, 1), (64, 64)]


@functools.lru_cache(maxsize=None)
def _var_case(nside_in, nside_out, nmap):
    """Maps (rows: normal, 1e8 + small integers, constant; the first ``nmap``) and the long-double oracle, once."""
    rng = np.random.default_rng(1000 * nside_in + nside_out)
    npix = 12 * nside_in * nside_in
    maps = np.stack([rng.normal(3.0, 2.0, npix), 1e8 + rng.integers(-20, 21, npix), np.full(npix, 0.1)])[[1, 0, 2][:nmap]]
    return maps, go.block_variance(maps, nside_out)


@pytest.mark.parametrize("nmap", [1, 3])
@pytest.mark.parametrize("nside_in,nside_out", VAR_SHAPES)
def test_block_variance(ctx, nside_in, nside_out, nmap):
    maps, (var, tol, _) = _var_case(nside_in, nside_out, nmap)
    out = ctx.healpix_block_variance(ctx.to_device(maps), nside_out).cpu().numpy()
    assert out.shape == var.shape and np.all(out >= 0)
    err = np.abs(out.astype(LD) - var)
    print("block_variance %d -> %d, nmap %d: worst err / tol %.3g" % (nside_in, nside_out, nmap, go.worst(err, tol)))
    assert np.all(err <= tol)
    if nmap == 3:
        assert np.all(out[2] == 0.0)                               # a constant map: exactly zero
    if nside_in == nside_out:
        assert np.all(out == 0.0)
    else:
        # row 0 is 1e8 + small integers: the one-pass formula misses the bound the kernel is held to
        one = np.abs(go.block_variance_onepass(maps[:1], nside_out).astype(LD) - var[:1])
        assert np.any(one > tol[:1])


def test_block_variance_constant_and_front_end(ctx):
    import torch

    from cora_amd.foreground import galaxy

    for nside_in, nside_out in VAR_SHAPES:
        c = torch.full((2, 12 * nside_in * nside_in), 0.1, dtype=torch.float64, device=ctx.device)
        assert bool((ctx.healpix_block_variance(c, nside_out) == 0).all())
    m = np.random.default_rng(3).normal(size=(2, 12 * 8 * 8))
    dev = galaxy.map_variance(ctx.to_device(m), 2)
    assert isinstance(dev, torch.Tensor) and tuple(dev.shape) == (2, 48)
    host = galaxy.map_variance(m[0], 2)
    assert isinstance(host, np.ndarray) and np.array_equal(host, dev[0].cpu().numpy())
    with pytest.raises(ValueError, match="factor 64"):
        ctx.healpix_block_variance(ctx.empty((1, 12 * 128 * 128)), 1)
    with pytest.raises(ValueError, match="must not exceed"):
        ctx.healpix_block_variance(ctx.empty((1, 48)), 4)
    print("block_variance constant maps: exactly 0, worst err / tol 0")


@pytest.mark.parametrize("case", ["v0", "v1", "v2"])
def test_block_variance_reference(ctx, gold, case):
    m = float(gold[case + "_offset"]) + gold[case + "_map_q"] * float(gold["q"])
    nside_out = int(gold[case + "_nside_out"])
    out = ctx.healpix_block_variance(ctx.to_device(m[None]), nside_out).cpu().numpy()[0]
    var, tol, tol_ref = go.block_variance(m[None], nside_out)
    err_o, err_r = np.abs(out.astype(LD) - var[0]), np.abs(out.astype(LD) - gold[case + "_var"].astype(LD))
    print("block_variance %s: worst err / tol %.3g (oracle), %.3g (reference)"
          % (case, go.worst(err_o, tol[0]), go.worst(err_r, tol[0] + tol_ref[0])))
    assert np.all(err_o <= tol[0]) and np.all(err_r <= tol[0] + tol_ref[0])


# ---- alm_scale_l -----------------------------------------------------------------------------------------------------------

def _l_of_index(lmax):
    return np.concatenate([np.arange(m, lmax + 1) for m in range(lmax + 1)])


@pytest.mark.parametrize("nnu", [1, 4, 5])
@pytest.mark.parametrize("nside,lmax", [(4, 11), (8, 23)])
def test_alm_scale_l(ctx, nside, lmax, nnu):
    import torch

    rng = np.random.default_rng(lmax + nnu)
    nalm, G = (lmax + 1) * (lmax + 2) // 2, (nnu + 3) // 4
    alm = rng.normal(size=(nalm, G, 2, 4))                           # padding channels hold values too
    fl = rng.uniform(0.1, 2.0, (nnu, lmax + 1))
    ell = _l_of_index(lmax)
    want = alm.copy()
    for nu in range(nnu):
        want[:, nu // 4, :, nu % 4] *= fl[nu, ell][:, None]
    d = ctx.to_device(alm)
    res = ctx.alm_scale_l(d, lmax, fl, out=_poisoned(ctx, d.shape))
    assert np.array_equal(res.cpu().numpy(), want) and np.array_equal(d.cpu().numpy(), alm)
    sq, sq0 = ctx.alm_dev_to_square(res, lmax, nnu).cpu().numpy(), ctx.alm_dev_to_square(d, lmax, nnu).cpu().numpy()
    host = sq0.copy()
    host.real *= fl[:, None, :, None]
    host.imag *= fl[:, None, :, None]
    assert np.array_equal(sq.view(np.float64), host.view(np.float64))
    # a vector is broadcast over all channels of the layout
    vec = ctx.alm_scale_l(d, lmax, fl[0]).cpu().numpy()
    assert np.array_equal(vec, alm * fl[0, ell][:, None, None, None])
    # fl = 1 leaves every bit alone, padding included; in place
    assert torch.equal(ctx.alm_scale_l(d, lmax, np.ones((nnu, lmax + 1))), d)
    inplace = d.clone()
    assert ctx.alm_scale_l(inplace, lmax, ctx.to_device(fl), out=inplace) is inplace and np.array_equal(inplace.cpu().numpy(), want)
    with pytest.raises(ValueError, match="fl must be"):
        ctx.alm_scale_l(d, lmax, np.ones((4 * G + 1, lmax + 1)))
    with pytest.raises(ValueError, match="alm must be"):
        ctx.alm_scale_l(d[:-1], lmax, fl)
    big = ctx.empty((nalm + 1, G, 2, 4))
    with pytest.raises(ValueError, match="overlaps alm in part"):
        ctx.alm_scale_l(big[:-1], lmax, fl, out=big[1:])
    print("alm_scale_l nside %d lmax %d nnu %d: exact, worst err / tol 0" % (nside, lmax, nnu))


# ---- smoothing -------------------------------------------------------------------------------------------------------------

def test_smoothing(ctx):
    import torch

    from cora_amd.util import hputil

    nside, lmax = 8, 23
    m = ctx.to_device(np.random.default_rng(8).normal(size=(1, 12 * nside * nside)))
    plain = ctx.alm2map(hputil.map2alm_device(m, nside, lmax, use_weights=False, niter=3), nside, lmax, 1)
    assert torch.equal(hputil.smoothing_device(m, fl=np.ones((1, lmax + 1))), plain)
    assert torch.equal(hputil.smoothing_device(m, fwhm=0.0), plain)
    # two beams on two copies of one map: each row is the single-map call
    two = hputil.smoothing_device(m.expand(2, -1).contiguous(), fwhm=[np.radians(5.0), np.radians(12.0)])
    for row, fwhm in enumerate((np.radians(5.0), np.radians(12.0))):
        assert torch.equal(two[row], hputil.smoothing_device(m, fwhm=fwhm)[0])
    sig = hputil.smoothing_device(m, sigma=np.radians(5.0) / np.sqrt(8 * np.log(2)))
    assert float((sig - two[0]).abs().max()) <= 1e-12 * float(two[0].abs().max())      # the same beam (a unit check)
    assert float(two[1].std()) < float(two[0].std()) < float(plain.std())
    host = hputil.smoothing(m[0].cpu().numpy(), fwhm=np.radians(5.0))
    assert host.shape == (12 * nside * nside,) and np.array_equal(host, two[0].cpu().numpy())
    # a constant map: the beam is exactly 1 at l = 0 and adds no rounding there; the reference is the round trip
    # analysis -> synthesis of the same map without a beam, with a margin of 2
    c = torch.full((1, 12 * nside * nside), 3.7, dtype=torch.float64, device=ctx.device)
    rt = float((ctx.alm2map(hputil.map2alm_device(c, nside, lmax, use_weights=False, niter=3), nside, lmax, 1) - 3.7).abs().max())
    err = float((hputil.smoothing_device(c, fwhm=np.radians(5.0)) - 3.7).abs().max())
    print("smoothing of a constant map: round trip error %.3g, smoothed %.3g, worst err / tol %.3g"
          % (rt, err, err / (2 * rt) if rt else 0.0))
    assert err <= 2 * rt


# ---- combine -----------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _combine_case(nside, nout, skip):
    rng = np.random.default_rng(100 * nside + 10 * nout + skip)
    npix, nchan = 12 * nside * nside, nout + skip
    efreq = rng.uniform(100.0, 1500.0, nchan)
    efreq[skip] = 408.0                                              # a channel at exactly 408 MHz: S == haslam
    haslam, sc, am = rng.uniform(5.0, 80.0, npix), rng.uniform(-3.5, -2.0, npix), rng.uniform(0.3, 8.0, npix)
    mv = 1.3
    sc[4] = 0.0                                                      # S == haslam in every channel
    fg, fgs = rng.normal(0.0, 6.0, (nchan, npix)), rng.normal(0.0, 3.0, (nchan, npix))
    S = haslam[None, :] * (efreq[:, None] / 408.0) ** sc[None, :]
    fgs[:, 0] = fg[:, 0]                                             # x = +0
    fg[:, 1], fgs[:, 1] = -0.0, 0.0                                  # x = -0
    fgs[:, 2] = fg[:, 2] + 40.0 * S[:, 2] * mv / am[2]               # x ~ -40: 1 + tanh cancels to (nearly) 0
    fgs[:, 3] = fg[:, 3] - 1e6 * S[:, 3] * mv / am[3]                # x ~ +1e6
    fgs[:, 4] = fg[:, 4]                                             # sc = 0 and x = 0: out == haslam
    return (fg, fgs, haslam, sc, am, mv, efreq), go.combine(fg, fgs, haslam, sc, am, mv, efreq, skip=skip)


@pytest.mark.parametrize("skip", [0, 2])
@pytest.mark.parametrize("nout", [1, 3, 5])
@pytest.mark.parametrize("nside", [1, 2, 4, 16])
def test_combine(ctx, nside, nout, skip):
    (fg, fgs, haslam, sc, am, mv, efreq), (want, tol, _) = _combine_case(nside, nout, skip)
    npix = 12 * nside * nside
    dfg, dfgs = ctx.to_device(fg), ctx.to_device(fgs)
    out = ctx.galaxy_combine(dfg, dfgs, haslam, sc, am, mv, efreq, skip=skip, out=_poisoned(ctx, (nout, npix))).cpu().numpy()
    err = np.abs(out.astype(LD) - want)
    print("combine nside %d, %d channels, skip %d: worst err / tol %.3g" % (nside, nout, skip, go.worst(err, tol)))
    assert np.all(np.isfinite(out)) and np.all(err <= tol) and np.all(out >= 0)
    d = (fg - fgs)[skip:]
    assert (d < 0).any() and (d > 0).any()                           # both branches
    assert np.array_equal(out[0, :2], haslam[:2])                    # 408 MHz and x = +-0: S == haslam, out == S
    assert np.array_equal(out[:, 4], np.broadcast_to(haslam[4], (nout,)))      # sc = 0
    assert np.all(out[:, 2] <= tol[:, 2].astype(np.float64)) and np.all(out[:, 2] >= 0)        # x ~ -40: 0 or next to it
    S = haslam[None, :] * (efreq[skip:, None] / 408.0) ** sc[None, :]
    assert np.all(np.abs(out[:, 3] / S[:, 3] - (1.0 + 1e6)) < 0.5)   # x ~ +1e6: the linear branch, S (1 + x)
    if skip == 2 and nout == 3:
        with pytest.raises(ValueError, match="overlaps fg"):
            ctx.galaxy_combine(dfg, dfgs, haslam, sc, am, mv, efreq, skip=skip, out=dfg[skip:])
        with pytest.raises(ValueError, match="overlaps fgs"):
            ctx.galaxy_combine(dfg, dfgs, haslam, sc, am, mv, efreq, skip=skip, out=dfgs[:nout])
        with pytest.raises(ValueError, match="haslam must be finite and positive"):
            ctx.galaxy_combine(dfg, dfgs, np.where(np.arange(npix) == 7, 0.0, haslam), sc, am, mv, efreq, skip=skip)
        with pytest.raises(ValueError, match="mv must be"):
            ctx.galaxy_combine(dfg, dfgs, haslam, sc, am, 0.0, efreq, skip=skip)
        with pytest.raises(ValueError, match="fgs has shape"):
            ctx.galaxy_combine(dfg, dfgs[1:], haslam, sc, am, mv, efreq, skip=skip)
        with pytest.raises(ValueError, match="sc has shape"):
            ctx.galaxy_combine(dfg, dfgs, haslam, sc[1:], am, mv, efreq, skip=skip)
        with pytest.raises(ValueError, match="skip must be"):
            ctx.galaxy_combine(dfg, dfgs, haslam, sc, am, mv, efreq, skip=nout + skip)


@pytest.mark.parametrize("case", ["md", "gsm"])
def test_combine_reference(ctx, gold, case):
    fg, fgs, haslam, sc, am, mv, efreq = getsky_inputs(gold, case)
    out = ctx.galaxy_combine(ctx.to_device(fg), ctx.to_device(fgs), haslam, sc, am, mv, efreq,
                             out=_poisoned(ctx, (2, fg.shape[1]))).cpu().numpy()
    want, tol, tol_ref = go.combine(fg, fgs, haslam, sc, am, mv, efreq)
    err_o, err_r = np.abs(out.astype(LD) - want), np.abs(out.astype(LD) - gold[case + "_fgt"].astype(LD))
    print("combine %s: worst err / tol %.3g (oracle), %.3g (reference)"
          % (case, go.worst(err_o, tol), go.worst(err_r, tol + tol_ref)))
    assert np.all(err_o <= tol) and np.all(err_r <= tol + tol_ref)


# ---- ConstrainedGalaxy -----------------------------------------------------------------------------------------------------

NSIDE, FREQ = 32, np.array([400.0, 450.0, 500.0])


def _sky_data():
    from cora_amd.util import hputil

    npix = 12 * NSIDE * NSIDE
    rng = np.random.default_rng(32)
    theta, phi = hputil.pix2ang(NSIDE, np.arange(npix))
    haslam = 20.0 + 60.0 * np.exp(-((theta - np.pi / 2) / 0.2) ** 2) + rng.uniform(0.0, 5.0, npix)
    spectral = {"md": -2.8 + 0.1 * np.cos(theta) + 0.02 * rng.normal(size=npix), "gsm": -2.7 + 0.1 * np.sin(phi)}
    faraday = 30.0 * np.cos(theta) * (1.0 + 0.5 * np.sin(2 * phi)) + 5.0
    return haslam, spectral, faraday


@pytest.fixture(scope="module")
def gal():
    from cora_amd.foreground import galaxy

    haslam, spectral, faraday = _sky_data()
    g = galaxy.ConstrainedGalaxy(haslam=haslam, spectral=spectral, faraday=faraday, amp_nside=NSIDE)
    g.nside, g.frequencies = NSIDE, FREQ
    return g


@pytest.fixture(scope="module")
def debug_run(gal):
    import cora_amd

    return gal.getsky_device(debug=True, celestial=False, rng=cora_amd.DeviceRNG(7))


def test_galaxy_getsky(ctx, gal, debug_run):
    import torch

    import cora_amd
    from cora_amd.util import hputil

    fgt, fg, fgs, fgsmooth, am, mv = debug_run
    npix = 12 * NSIDE * NSIDE
    assert tuple(fgt.shape) == (3, npix) and tuple(fg.shape) == (5, npix) and tuple(fgs.shape) == (5, npix)
    again = gal.getsky_device(celestial=False, rng=cora_amd.DeviceRNG(7))
    assert torch.equal(again, fgt)                                    # same seed: identical bits
    assert bool(torch.isfinite(fgt).all()) and bool((fgt >= 0).all())
    assert not torch.equal(gal.getsky_device(celestial=False, rng=cora_amd.DeviceRNG(8)), fgt)
    # fgt against the oracle on the returned intermediates and the class's data
    efreq = np.concatenate(([408.0, 1420.0], FREQ))
    want, tol, _ = go.combine(fg.cpu().numpy(), fgs.cpu().numpy(), gal._haslam, gal._sp_ind["md"], am.cpu().numpy(), mv, efreq)
    err = np.abs(fgt.cpu().numpy().astype(LD) - want)
    print("getsky fgt against the oracle on (fg, fgs, am, mv): worst err / tol %.3g" % go.worst(err, tol))
    assert np.all(err <= tol)
    S = gal._haslam[None] * (efreq[:, None] / 408.0) ** gal._sp_ind["md"][None]
    assert np.all(np.abs(fgsmooth.cpu().numpy() - S) <= 20 * EPS * S)       # debug product: pow within OpenCL's 16 ulp
    # celestial: the rotation of the galactic result, bit for bit
    cel = gal.getsky_device(rng=cora_amd.DeviceRNG(7))
    assert torch.equal(cel, hputil.rotate_map_device(fgt, hputil.coord_matrix("C", "G")))
    host = gal.getsky(rng=cora_amd.DeviceRNG(7))
    assert isinstance(host, np.ndarray) and np.array_equal(host, cel.cpu().numpy())


def test_galaxy_mv_chain(ctx, gal, debug_run):
    """mv = mean over the sphere of smoothing(sqrt(map_variance(smoothing(fg[0], sigma 0.5 deg), 16)), sigma 2 deg).

    The oracle takes the package's smoothing of fg[0] (a row of the batched call equals the single-map call bit for bit:
    test_smoothing), the block variance in long double, its square root rounded to float64, the package's smoothing
    again and the mean in long double.  The run's variance map differs from the oracle's by tol_v (block-variance bound),
    its root by tol_v / (2 root) + eps root (the rounding of the root, with room); smoothing followed by the mean is linear with gain 1 at
    l = 0 and moves by no more than the largest perturbation of a pixel, with a factor 2 for the part of a pixel-scale
    perturbation that the three Jacobi iterations do not project out; the run's own mean is a pairwise sum of 3072 terms:
    12 u of their mean."""
    from cora_amd.util import hputil

    fg, mv = debug_run[1], debug_run[5]
    sm = hputil.smoothing_device(fg[:1], sigma=np.radians(0.5))
    var, tol_v, _ = go.block_variance(sm.cpu().numpy(), 16)
    root = np.sqrt(var).astype(np.float64)
    vm = hputil.smoothing_device(ctx.to_device(root), sigma=np.radians(2.0)).cpu().numpy().astype(LD)
    want = vm.mean()
    droot = np.where(var > 0, tol_v / (2 * np.where(var > 0, np.sqrt(var), 1)), np.sqrt(tol_v)) + EPS * root
    tol = (2 * droot.max() + 12 * U * np.abs(vm).mean()) * go.SLACK
    print("getsky mv %.6g against the oracle's chain: worst err / tol %.3g" % (mv, go.worst(abs(LD(mv) - want), tol)))
    assert mv > 0 and abs(LD(mv) - want) <= tol


def test_galaxy_gsm_applies_two_constraints(ctx, gal, monkeypatch):
    import cora_amd
    from cora_amd.core import skysim

    seen = []
    real = skysim.mkconstrained

    def spy(corr, constraints, nside):
        seen.append([c[0] for c in constraints])
        return real(corr, constraints, nside)

    monkeypatch.setattr(skysim, "mkconstrained", spy)
    md = gal.getsky_device(celestial=False, rng=cora_amd.DeviceRNG(7))
    monkeypatch.setattr(gal, "spectral_map", "gsm")
    gsm = gal.getsky_device(celestial=False, rng=cora_amd.DeviceRNG(7))
    assert seen == [[0], [0, 1]]
    assert bool((gsm >= 0).all()) and float((gsm - md).abs().max()) > 0
    monkeypatch.setattr(gal, "spectral_map", "gd")
    with pytest.raises(ValueError, match="no such spectral index map"):
        gal.getsky_device(rng=cora_amd.DeviceRNG(7))
    print("gsm: constraints at channels %r; md: %r" % (seen[1], seen[0]))


def test_galaxy_getpolsky(ctx, gal, monkeypatch):
    import cora_amd

    monkeypatch.setattr(gal, "_maxphi", 16.0)
    pol = gal.getpolsky(rng=cora_amd.DeviceRNG(7))
    npix = 12 * NSIDE * NSIDE
    assert pol.shape == (3, 4, npix) and np.all(np.isfinite(pol))
    assert np.array_equal(pol[:, 0], gal.getsky(rng=cora_amd.DeviceRNG(7)))
    assert np.all(pol[:, 3] == 0)
    # |P| < 1 before the rotation, whose weights are non-negative and sum to 1: |Q + iU| <= T up to the rounding of the
    # interpolation sums (4 terms: 4 u each for Q, U and T)
    excess = np.hypot(pol[:, 1], pol[:, 2]) - pol[:, 0]
    print("getpolsky: max (|Q + iU| - T) / T = %.3g, worst err / tol %.3g"
          % ((excess / pol[:, 0]).max(), max(0.0, (excess / (16 * U * pol[:, 0])).max())))
    assert np.all(excess <= 16 * U * pol[:, 0]) and np.abs(pol[:, 1:3]).max() > 0
    gal_nofar = object.__new__(type(gal))
    gal_nofar.__dict__.update(gal.__dict__)
    gal_nofar._faraday = None
    with pytest.raises(ValueError, match="Faraday"):
        gal_nofar.getpolsky()


# ---- command line ------------------------------------------------------------------------------------------------------------

def test_cli_galaxy_and_foreground(ctx, tmp_path):
    from click.testing import CliRunner

    from cora_amd.scripts import makesky

    haslam, spectral, faraday = _sky_data()
    data = str(tmp_path / "skydata.npz")
    np.savez(data, haslam=haslam, spectral_md=spectral["md"], spectral_gsm=spectral["gsm"], spectral_gd=spectral["md"],
             faraday=faraday)
    for cmd, pol, npol in (("galaxy", "none", 1), ("foreground", "zero", 4)):
        out = str(tmp_path / (cmd + ".h5"))
        args = [cmd, "--skydata", data, "--nside", "32", "--freq", "400", "500", "2", "--seed", "1", "--pol", pol, "--filename", out]
        if cmd == "galaxy":
            args += ["--spectral-index", "gsm"]
        r = CliRunner().invoke(makesky.cli, args)
        assert r.exit_code == 0, r.output
        if os.path.exists(out):
            import h5py

            with h5py.File(out, "r") as f:
                sky, freq = f["map"][:], f["index_map/freq"][:]
        else:
            f = np.load(out + ".npz")
            sky, freq = f["map"], f["index_map__freq"]
        assert sky.shape == (2, npol, 12 * 32 * 32) and np.array_equal(freq["centre"], [400.0, 450.0])
        assert np.all(np.isfinite(sky)) and np.all(sky[:, 0] > 0) and np.all(sky[:, 1:] == 0)
    print("cora-makesky galaxy / foreground wrote their containers")
