"""Element-level parity of the ANALYSIS path (K5^T + K4^T, the weighted Jacobi pass, the spin-2 composition) against
the oracle at the kernel shapes of full-size launches.  test_gpu_parity.py (nside <= 64) only reaches the run-time
ringana_kernel; the compile-time K5^T kernels (sht_ringana_ct) take the belt and the Bluestein classes of
nside >= 512.  Here every ring class is isolated in a channel of its own, so that each channel's a_lm come from one
K5^T kernel and any channel cross-talk shows; the aliased lmax = 3 nside - 1 (hputil.sphtrans_real's default),
legendre_adj_kernel<2>, the ring-weighted two-iteration pass, spin-2 analysis at nside 1024 and an independent
direct-sum spot check are covered too.  Run with -m gpu.

Reference code the compared quantities come from: cora/util/hputil.py:195-234 (map2alm), :274-323 (the polarised
branch), :337 (the lmax default)."""
import math

import numpy as np
import pytest
from test_gpu_fullsize import _packed_of, _ring_classes

pytestmark = pytest.mark.gpu


def _class_keys(nside, lmax):
    """Per ring: its ring-FFT class as the plan launches it, with the belt (class 0 like the power-of-two cap rings,
    but a compile-time kernel of its own) as key -1."""
    cls = _ring_classes(nside, lmax)
    i = np.arange(1, 4 * nside)
    key = np.where((i >= nside) & (i <= 3 * nside), -1, cls)
    assert np.array_equal(key, key[::-1])                 # a ring and its mirror are in the same class
    return key


@pytest.mark.parametrize("nside,lmax", [(1024, 2048), (1024, 3071), (512, 1024), (2048, 1024)])
def test_map2alm_per_class_isolation_vs_oracle(ctx, nside, lmax):
    """Channel k holds white noise on the rings of ring class k only (the belt and every Bluestein / direct class of
    the plan), so its a_lm come from one K5^T kernel; each channel against oracle.sht.map2alm_adjoint element by
    element, relative to its own max|ref|.  Two launches: the class count (ragged: padding lanes of the compile-time
    K5^T kernels) and that count padded to a multiple of 16 channels with full-sky noise (legendre_adj_kernel<2>).
    (1024, 3071) is the aliased default lmax; (2048, 1024) has the belt <4096, 2> and the P = 8192 / 6144 caps on the
    run-time kernel.

    Bounds: 1e-12 for the belt and the Bluestein classes P >= 1024 (compile-time kernels; measured <= 1.1e-13).  The
    polar classes on the run-time kernel (direct caps 0, P <= 512: rings i <= 128) measured 1.1e-12 .. 4.7e-12, growing
    with lmax (2.2e-12 at lmax 2048, 4.7e-12 at 3071): next to the pole lambda_lm of low m does not decay with l, so
    max|ref| sits at l ~ lmax, where the recurrence has accumulated ~lmax roundings in the oracle's and the kernel's
    (different) operation orders; they are held to 1e-11."""
    import torch
    from oracle import healpix, sht

    key = _class_keys(nside, lmax)
    keys = sorted(set(key.tolist()))
    nk = len(keys)
    npad = (nk + 15) // 16 * 16
    npix = 12 * nside * nside
    npair = 2 * nside
    ri = healpix.ring_info(nside)
    pixkey = torch.from_numpy(np.repeat(key.astype(np.int32), ri["nphi"])).to(ctx.device)
    gen = torch.Generator(device=ctx.device).manual_seed(nside + lmax)
    x = torch.randn((npad, npix), generator=gen, device=ctx.device, dtype=torch.float64)
    for k, c in enumerate(keys):
        x[k].masked_fill_(pixkey != c, 0.0)
    del pixkey
    refs = [sht.map2alm_adjoint(x[k].cpu().numpy(), nside, lmax, None, pairs=np.flatnonzero(key[:npair] == c))
            for k, c in enumerate(keys)]
    errs = {}
    for nnu in (nk, npad):
        alm = ctx.map2alm(x[:nnu], nside, lmax, None)
        for k, c in enumerate(keys):
            e = np.abs(_packed_of(alm, k) - refs[k]).max() / np.abs(refs[k]).max()
            name = "belt" if c == -1 else int(c)
            errs[name] = max(errs.get(name, 0.0), float(e))
        del alm
    del x
    torch.cuda.empty_cache()
    print("nside %d lmax %d map2alm (%d and %d channels) max|err|/max|ref| per class (0 = direct caps, else Bluestein "
          "P): %s" % (nside, lmax, nk, npad, errs))
    ct = {c: e for c, e in errs.items() if c == "belt" or c >= 1024}
    assert len(ct) >= 4 and max(ct.values()) <= 1e-12, ct
    assert max(errs.values()) <= 1e-11, errs


@pytest.fixture(scope="module")
def band_limited_map(ctx):
    """One band-limited map at nside 1024 / lmax 2048 (a_lm ~ N(0, 1) / (1 + l), a_l0 real), synthesised on the
    device: (device maps [1, npix], host copy, packed a_lm)."""
    import torch

    nside, lmax = 1024, 2048
    L = lmax + 1
    rng = np.random.default_rng(2048)
    nalm = L * (L + 1) // 2
    l_of = np.concatenate([np.arange(m, L) for m in range(L)])
    a = (rng.standard_normal(nalm) + 1j * rng.standard_normal(nalm)) / (1.0 + l_of)
    a[:L] = a[:L].real
    alm = ctx.alm_packed_to_dev(torch.from_numpy(a[None]).to(ctx.device), lmax)
    maps = ctx.alm2map(alm, nside, lmax, 1)
    del alm
    yield maps, maps[0].cpu().numpy(), a
    del maps
    torch.cuda.empty_cache()


def test_map2alm_weighted_two_iterations_vs_oracle(ctx, band_limited_map):
    """hputil.map2alm_device at full size with the reference's defaults (ring weights, iter = 2: three weighted
    quadrature passes and two syntheses) against oracle.sht.map2alm(map, 1024, 2048, True, 2)."""
    from cora_amd.util import hputil
    from oracle import sht

    nside, lmax = 1024, 2048
    maps, host, _ = band_limited_map
    got = _packed_of(hputil.map2alm_device(maps, nside, lmax), 0)
    ref = sht.map2alm(host, nside, lmax, True, 2)
    err = np.abs(got - ref).max() / np.abs(ref).max()
    print("nside 1024 / lmax 2048 weighted map2alm, iter 2: max|err|/max|ref| = %.3e" % err)
    assert err <= 1e-12, err


# (l, m) of the spot check: l <= 40, both ends of the m range
_SPOTS = [(0, 0), (1, 0), (1, 1), (2, 2), (3, 1), (7, 4), (12, 0), (20, 13), (31, 30), (40, 1), (40, 40)]


def test_weighted_pass_spot_check_by_direct_pixel_sum(ctx, band_limited_map):
    """Coefficients l <= 40 of the full-size weighted quadrature pass by a direct pixel sum
    a_lm = sum_pix w (4 pi / npix) x conj(Y_lm) with scipy.special.sph_harm_y (not the lambda recurrence the kernel
    and the oracle share): the e^{-i m phi} sums of each ring in long double, the ring sum with math.fsum."""
    from scipy.special import sph_harm_y

    from cora_amd.util import hputil
    from oracle import healpix

    nside, lmax = 1024, 2048
    maps, host, _ = band_limited_map
    w = hputil.ring_weights(nside)
    got = _packed_of(ctx.map2alm(maps, nside, lmax, ctx.to_device(w)), 0)
    nring, npix = 4 * nside - 1, 12 * nside * nside
    ri = healpix.ring_info(nside)
    start = ri["start"].astype(np.int64)
    theta, phi = healpix.pix2ang_ring(nside)
    theta_r = theta[start]
    wr = np.array([w[min(r, nring - 1 - r)] for r in range(nring)]) * (4.0 * np.pi / npix)
    xl = host.astype(np.longdouble)
    ref = {}
    for m in sorted({m for _, m in _SPOTS}):
        re = np.add.reduceat(xl * np.cos(m * phi), start).astype(np.float64)
        im = -np.add.reduceat(xl * np.sin(m * phi), start).astype(np.float64)
        for l, mm in _SPOTS:
            if mm == m:
                y = wr * sph_harm_y(l, m, theta_r, 0.0).real
                ref[(l, m)] = complex(math.fsum((y * re).tolist()), math.fsum((y * im).tolist()))
    scale = max(abs(v) for v in ref.values())
    err = {(l, m): abs(got[m * (2 * lmax + 1 - m) // 2 + l] - ref[(l, m)]) / scale for l, m in _SPOTS}
    print("weighted pass vs direct pixel sum, |err| / max|a| per (l, m):", {k: "%.1e" % v for k, v in err.items()})
    assert max(err.values()) <= 1e-12, err


def test_spin2_analysis_fullsize_vs_oracle(ctx):
    """(Q, U) -> (E, B) at nside 1024 / lmax 2048, two pairs: one white noise, one noise on the polar rings i <= 8 only
    (where the ring scaling 1/sin^2 theta of the six scalar passes is largest, ~1.5e6).  Coefficients of
    m in {0..4, 511, 1024, 2046, 2047, 2048} against oracle.sht.map2alm_spin2_adjoint(ms=...), relative to the pair's
    max |E|, |B| over those m."""
    import torch
    from cora_amd.util import hputil
    from oracle import healpix, sht

    nside, lmax, nf = 1024, 2048, 2
    ms = [0, 1, 2, 3, 4, 511, 1024, 2046, 2047, 2048]
    npix = 12 * nside * nside
    start = healpix.ring_info(nside)["start"].astype(np.int64)
    gen = torch.Generator(device=ctx.device).manual_seed(1024)
    qu = torch.randn((2 * nf, npix), generator=gen, device=ctx.device, dtype=torch.float64)
    qu[2:, int(start[8]) : int(start[4 * nside - 1 - 8])] = 0.0          # pair 1: rings i <= 8 of both caps
    w = hputil.ring_weights(nside)
    dev = ctx.map2alm_spin2(qu, nside, lmax, ctx.to_device(w))
    host = qu.cpu().numpy()
    m_of = np.concatenate([np.full(lmax + 1 - m, m) for m in range(lmax + 1)])
    sel = np.isin(m_of, ms)
    errs = []
    for f in range(nf):
        e, b = sht.map2alm_spin2_adjoint(host[2 * f], host[2 * f + 1], nside, lmax, w, ms=ms)
        ge, gb = _packed_of(dev, 2 * f), _packed_of(dev, 2 * f + 1)
        scale = max(np.abs(e[sel]).max(), np.abs(b[sel]).max())
        errs.append(max(np.abs(ge[sel] - e[sel]).max(), np.abs(gb[sel] - b[sel]).max()) / scale)
    del qu, dev
    torch.cuda.empty_cache()
    print("nside 1024 / lmax 2048 spin-2 analysis max|err|/max|ref|: white %.3e, polar rings %.3e" % tuple(errs))
    # measured 1.2e-12 (white) and 3.7e-11 (polar rings): W and X are differences of terms scaled by 1/sin^2 theta
    # (1.5e6 on ring 1), formed as such in the oracle and, with another operation order, from the device's scaled
    # scalar passes - the amplification test_gpu_fullsize.py bounds at 1e-9 on the polar rings of the spin-2 synthesis
    assert errs[0] <= 5e-12, errs
    assert errs[1] <= 1e-10, errs
