"""Zel'dovich SPH assignment on the device (csrc/pmesh.hip through cora_amd.signal.lss) against the reference's
golden output (tests/golden/lss_vectors.npz) and the numpy oracle (tests/_za_oracle.py).  The kernel sums with
float atomics (LDS tile, then global), so results are compared to a tolerance, never bit for bit.  It uses no
workspace.  Run with -m gpu."""
import os

import numpy as np
import pytest

import _za_oracle as zo

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lg():
    g = dict(np.load(os.path.join(ROOT, "tests", "golden", "lss_vectors.npz")))
    g["psi"] = g["psi_q"].astype(np.float64) * np.array([g["q_r"], g["q_a"], g["q_a"]])[:, None, None]
    g["delta_bias"] = g["delta_bias_q"].astype(np.float64) * g["q_a"]
    g["delta_m"] = g["delta_m_q"].astype(np.float64) * g["q_a"]
    return g


def _fields(nside, nchi, seed, pix_shift=1.0):
    rng = np.random.default_rng(seed)
    npix = 12 * nside * nside
    res = np.sqrt(4 * np.pi / npix)
    chi = 800.0 + 8.0 * np.arange(nchi) + rng.uniform(-1.0, 1.0, nchi)
    psi = np.stack([rng.normal(0, 3.0, (nchi, npix)), rng.normal(0, pix_shift * res, (nchi, npix)),
                    rng.normal(0, 2 * pix_shift * res, (nchi, npix))])
    delta_bias = rng.normal(0, 0.4, (nchi, npix))
    delta_m = rng.normal(0, 0.8, (nchi, npix))
    return psi, delta_bias, delta_m, chi


@pytest.mark.parametrize("nside", [1, 3, 6, 16, 1024])     # 3, 6: not a power of two
def test_device_neighbours_match_host(ctx, nside):
    from cora_amd.util import hputil

    npix = 12 * nside * nside
    dev = ctx.healpix_neighbours(nside).cpu().numpy()
    assert dev.shape == (npix, 9) and dev.dtype == np.int32
    assert np.array_equal(dev[:, 0], np.arange(npix))
    step = 1 if npix <= 1 << 16 else 7
    rows = np.arange(0, npix, step)
    rows = np.union1d(rows, np.r_[0:4 * nside, npix - 4 * nside:npix])      # every cap-edge ring near the poles
    assert np.array_equal(dev[rows, 1:].T, zo.get_all_neighbours(nside, rows))
    # the public healpy-style entry point
    assert np.array_equal(hputil.get_all_neighbours(nside, rows[:50]), dev[rows[:50], 1:].T)
    assert np.array_equal(hputil.get_all_neighbours(nside, int(rows[3])), dev[rows[3], 1:])


def test_matches_golden(lg):
    from cora_amd.signal import lss

    out = np.full(lg["delta_bias"].shape, float(lg["out0"]))
    got = lss.za_density_sph(lg["psi"], lg["delta_bias"], lg["delta_m"], lg["chi"], out)
    assert got is out
    ref = lg["out"]
    err = np.abs(out - ref).max() / np.abs(ref + 1).max()
    assert err <= 1e-12, err
    rel = abs((out + 1 - float(lg["out0"])).sum() - (1 + lg["delta_bias"]).sum()) / (1 + lg["delta_bias"]).sum()
    assert rel <= 1e-12, rel


def test_matches_oracle_nside256(ctx):
    from cora_amd.signal import lss

    nside, nchi = 256, 16
    psi, db, dm, chi = _fields(nside, nchi, 7, pix_shift=1.5)
    out0 = np.random.default_rng(8).normal(0, 0.1, db.shape)
    ref = zo.za_density_sph(psi, db, dm, chi, out0.copy())
    t = [ctx.to_device(a) for a in (psi, db, dm, chi, out0)]
    keep = [x.clone() for x in t[:4]]
    got = lss.za_density_sph_device(*t).cpu().numpy()
    for a, b in zip(t[:4], keep):                                        # inputs untouched
        assert bool((a == b).all())
    err = np.abs(got - ref).max() / np.abs(ref + 1).max()
    assert err <= 1e-12, err
    mass = (got + 1 - out0).sum()
    assert abs(mass - (1 + db).sum()) <= 1e-12 * (1 + db).sum()
    # a second call: the same to rounding (float atomics), not necessarily bit for bit
    t2 = ctx.to_device(out0)
    again = lss.za_density_sph_device(t[0], t[1], t[2], t[3], t2).cpu().numpy()
    assert np.abs(again - got).max() <= 1e-13 * np.abs(got + 1).max()


def test_edge_cases_small_nside(ctx):
    """Large displacements (many pixels, across poles and phi = 0, out of the chi range), both clip bounds, a
    non-default sigma_chi and the smallest maps: every target off the LDS tile goes to the global path."""
    from cora_amd.signal import lss

    for nside, nchi, shift in ((1, 3, 0.5), (2, 5, 2.0), (3, 5, 3.0), (4, 9, 4.0), (16, 11, 6.0)):
        psi, db, dm, chi = _fields(nside, nchi, 100 + nside, pix_shift=shift)
        psi[0, 0] -= 40.0
        psi[0, -1] += 40.0
        dm[:, ::3] = -0.97
        dm[:, 1::3] = 4.0
        for sigma_chi in (None, 2.5):
            ref = zo.za_density_sph(psi, db, dm, chi, np.zeros(db.shape), sigma_chi=sigma_chi)
            got = lss.za_density_sph(psi, db, dm, chi, np.zeros(db.shape), sigma_chi=sigma_chi)
            err = np.abs(got - ref).max() / np.abs(ref + 1).max()
            assert err <= 1e-12, (nside, nchi, sigma_chi, err)


def test_bad_shapes_raise(ctx):
    from cora_amd.signal import lss

    nside, nchi = 4, 4
    npix = 12 * nside * nside
    psi, db, dm, chi = (ctx.to_device(a) for a in _fields(nside, nchi, 3))
    out = ctx.empty((nchi, npix))
    with pytest.raises(ValueError):
        lss.za_density_sph_device(psi[:2], db, dm, chi, out)
    with pytest.raises(ValueError):
        lss.za_density_sph_device(psi, db, dm[:, :-1], chi, out)
    with pytest.raises(ValueError):
        lss.za_density_sph_device(psi, db, dm, chi[:3], out)
    with pytest.raises(ValueError):
        lss.za_density_sph_device(psi, db, dm, chi, out[:3])
    with pytest.raises(ValueError):
        lss.za_density_sph_device(psi[:, :2], db[:2], dm[:2], chi[:2], out[:2])
    # below the Python layer the C ABI refuses nchi < 3 itself
    from cora_amd import _lib

    with pytest.raises(_lib.CoraHipError):
        ctx.za_density_sph(psi[:, :2].contiguous(), db[:2].contiguous(), dm[:2].contiguous(), chi[:2].contiguous(),
                           out[:2].contiguous(), 0.1, 1.0)
