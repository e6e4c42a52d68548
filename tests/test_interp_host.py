"""Host side of the HEALPix bilinear interpolation (cora_amd.util.hputil.get_interp_weights / coord_x2y,
cora_amd.signal.lss.za_density_grid): the numpy oracle of the scheme (tests/_interp_oracle.py) is held to the
properties that define it, ``coord_matrix`` to orthonormality and two catalogue positions, and the oracle's grid
scatter to the golden output of the reference's own ``za_density_grid`` (tests/golden/zagrid_vectors.npz).  healpy is
not installed: nothing here is compared with healpy's numbers.  No GPU needed."""
import os

import numpy as np
import pytest

import _interp_oracle as io
from cora_amd.util import hputil

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NSIDES = [1, 2, 4, 16]


def _queries(nside, seed=0, nrand=20000):
    """random directions, 100 within 1e-3 of the poles, and the special ones: theta = 0, pi, phi = 0, phi just below
    2 pi, queries exactly on ring latitudes (pixel centres included)."""
    rng = np.random.default_rng(seed + nside)
    th = [np.arccos(rng.uniform(-1, 1, nrand)), rng.uniform(0, 1e-3, 50), np.pi - rng.uniform(0, 1e-3, 50)]
    ph = [rng.uniform(0, 2 * np.pi, nrand + 100)]
    ring = io.ring_theta(nside, np.arange(1, 4 * nside))
    below = np.nextafter(2 * np.pi, 0)
    for t in np.r_[0.0, np.pi, ring, rng.uniform(0, np.pi, 8)]:
        for p in (0.0, below, 1.0, rng.uniform(0, 2 * np.pi)):
            th.append([t])
            ph.append([p])
    tc, pc = hputil.pix2ang(nside, np.arange(12 * nside * nside))
    return np.concatenate(th + [tc]), np.concatenate(ph + [pc]), nrand


@pytest.mark.parametrize("nside", NSIDES)
def test_weights_sum_to_one_and_are_positive(nside):
    th, ph, nrand = _queries(nside)
    pix, w = io.interp_weights(nside, th, ph)
    assert pix.shape == (4, th.size) and pix.dtype == np.int64 and w.shape == (4, th.size)
    assert pix.min() >= 0 and pix.max() < 12 * nside * nside
    assert np.abs(w.sum(axis=0) - 1).max() <= 2.3e-16
    assert (w[:, :nrand + 100] > 0).all()                    # random directions: strictly inside a cell
    # on a pixel centre phi / dphi lands on an integer to rounding: 16 ulp of the largest ring co-ordinate 4 nside
    assert w.min() >= -64 * nside * 2.0 ** -52


@pytest.mark.parametrize("nside", NSIDES)
def test_pixel_centre_gets_its_own_pixel(nside):
    npix = 12 * nside * nside
    tc, pc = hputil.pix2ang(nside, np.arange(npix))
    pix, w = io.interp_weights(nside, tc, pc)
    own = np.where(pix == np.arange(npix)[None], w, 0.0).sum(axis=0)
    assert own.min() >= 1 - 1.8e-14, 1 - own.min()


@pytest.mark.parametrize("nside", NSIDES)
def test_map_linear_in_ring_latitude_is_reproduced(nside):
    th, ph, _ = _queries(nside)
    tc, _ = hputil.pix2ang(nside, np.arange(12 * nside * nside))
    sel = (th >= tc.min()) & (th <= tc.max())
    val = io.interp_val(tc[None], th[sel], ph[sel])[0]
    assert np.abs(val - th[sel]).max() <= 1.4e-15


@pytest.mark.parametrize("nside", NSIDES)
def test_weighted_pixels_are_near_the_query(nside):
    th, ph, _ = _queries(nside)
    pix, w = io.interp_weights(nside, th, ph)
    vq = hputil.ang2vec(th, ph).T
    vp = np.array(hputil.pix2vec(nside, pix))
    cross = np.cross(vp, vq[:, None, :], axis=0)
    dist = np.arctan2(np.sqrt((cross ** 2).sum(axis=0)), (vp * vq[:, None, :]).sum(axis=0))
    assert dist[w > 1e-9].max() <= 1.8 * hputil.nside2resol(nside)


def test_poles_are_the_mean_of_the_polar_ring():
    for nside in NSIDES:
        npix = 12 * nside * nside
        for theta, ring in ((0.0, np.arange(4)), (np.pi, np.arange(npix - 4, npix))):
            pix, w = io.interp_weights(nside, [theta], [0.7])
            assert sorted(pix[:, 0]) == list(ring)
            assert np.abs(w - 0.25).max() <= 1e-16


def test_phi_wraps_round():
    for nside in NSIDES:
        th = np.linspace(0.05, np.pi - 0.05, 23)
        a = io.interp_weights(nside, th, np.full(th.size, 0.3))
        b = io.interp_weights(nside, th, np.full(th.size, 0.3 - 2 * np.pi))
        r = np.random.default_rng(3).normal(size=12 * nside * nside)
        assert np.abs((a[1] * r[a[0]]).sum(0) - (b[1] * r[b[0]]).sum(0)).max() <= 64 * nside * 2.0 ** -52 * np.abs(r).max()


# ---- coord_matrix ----------------------------------------------------------------------------
def _lonlat(v):
    return np.degrees(np.arctan2(v[1], v[0])) % 360.0, np.degrees(np.arctan2(v[2], np.hypot(v[0], v[1])))


def _sep_deg(lon1, lat1, lon2, lat2):
    a, b = hputil.ang2vec(np.radians(90 - lat1), np.radians(lon1)), hputil.ang2vec(np.radians(90 - lat2), np.radians(lon2))
    return np.degrees(np.arctan2(np.linalg.norm(np.cross(a, b)), a @ b))


def test_coord_matrix_is_a_rotation():
    for x in "CGE":
        for y in "CGE":
            R = hputil.coord_matrix(x, y)
            assert np.abs(R @ R.T - np.eye(3)).max() <= 4e-16, (x, y)
            assert abs(np.linalg.det(R) - 1) <= 1e-15
            assert np.array_equal(R, hputil.coord_matrix(y, x).T)
        assert np.array_equal(hputil.coord_matrix(x, x), np.eye(3))
    with pytest.raises(Exception, match="Co-ordinate system invalid."):
        hputil.coord_matrix("G", "X")


def test_coord_matrix_catalogue_positions():
    """The galactic pole and the galactic centre in J2000 equatorial co-ordinates, within 1e-4 deg on the sky (the
    angular separation; the matrix puts the centre at RA 266.40499, Dec -28.93617, 9.2e-5 deg from the quoted
    266.40510, -28.93617)."""
    R = hputil.coord_matrix("G", "C")
    pole, centre = _lonlat(R @ [0.0, 0.0, 1.0]), _lonlat(R @ [1.0, 0.0, 0.0])
    print("galactic pole %.5f %.5f, centre %.5f %.5f" % (pole + centre))
    assert _sep_deg(pole[0], pole[1], 192.85948, 27.12825) <= 1e-4
    assert _sep_deg(centre[0], centre[1], 266.40510, -28.93617) <= 1e-4
    # ecliptic: the pole of the ecliptic lies at RA 270, Dec 90 - obliquity
    epole = _lonlat(hputil.coord_matrix("E", "C") @ [0.0, 0.0, 1.0])
    assert _sep_deg(epole[0], epole[1], 270.0, 90 - 23.4392911) <= 1e-10


# ---- the grid form of the Zel'dovich step against the reference's own function -------------------
@pytest.fixture(scope="module")
def zg():
    g = dict(np.load(os.path.join(ROOT, "tests", "golden", "zagrid_vectors.npz")))
    g["psi"] = g["psi_q"].astype(np.float64) * np.array([g["q_r"], g["q_a"], g["q_a"]])[:, None, None]
    g["delta_bias"] = g["delta_bias_q"].astype(np.float64) * g["q_a"]
    g["delta_m"] = g["delta_m_q"].astype(np.float64) * g["q_a"]
    return g


def test_golden_file_is_small_and_has_the_edge_cases(zg):
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "zagrid_vectors.npz")) < 100000
    nside, chi, psi = int(zg["nside"]), zg["chi"], zg["psi"]
    assert nside == 8 and psi.shape == (3, 6, 768)
    th, ph = hputil.pix2ang(nside, np.arange(768))
    assert ((th + psi[1] < 0).any() and (th + psi[1] > np.pi).any())                 # pole crossings
    assert ((ph + psi[2] < 0).any() and (ph + psi[2] > 2 * np.pi).any())             # phi = 0 crossings
    new_chi = chi[:, None] + psi[0]
    assert (new_chi < chi[0]).any() and (new_chi > chi[-1]).any()                    # both radial ends
    assert (new_chi < 2 * chi[0] - chi[1]).any() and (new_chi > 2 * chi[-1] - chi[-2]).any()
    assert not psi[0, 2].any()                                                       # a slice that stays on its chi


def test_oracle_grid_matches_golden(zg):
    out = np.full(zg["delta_bias"].shape, float(zg["out0"]))
    io.za_density_grid(zg["psi"], zg["delta_bias"], zg["delta_m"], zg["chi"], out)
    ref = zg["out"]
    bound = 1e-13 * np.abs(ref + 1).max()
    assert np.abs(out - ref).max() <= bound, np.abs(out - ref).max()
    # the reference's own scatter: row stride 4
    flat = np.zeros(zg["delta_bias"].shape)
    io.za_density_grid(zg["psi"], zg["delta_bias"], zg["delta_m"], zg["chi"], flat, stride=4)
    n = zg["bin_delta_ref"].size
    assert n == (6 - 1) * 4 + 768 and not flat.ravel()[n:].any()
    assert np.abs(flat.ravel()[:n] - zg["bin_delta_ref"]).max() <= bound


def test_grid_radial_bins():
    """np.digitize on the extended chi: a particle on chi[ii] puts weight 1 on bin ii (at the last slice too), shares
    outside [0, nchi) are marked -1."""
    chi = np.array([10.0, 11.0, 13.0, 14.5])
    ind, w = io.radial_bins(chi.copy(), chi)
    assert np.array_equal(ind[:, 0], np.arange(4)) and np.array_equal(w[:, 0], np.ones(4))
    assert np.array_equal(w[:, 1], [0, 0, 0, -1])
    ind, w = io.radial_bins(np.array([8.0, 9.5, 14.75, 15.5, 16.5]), chi)
    assert (w[0] == -1).all() and (w[4] == -1).all()
    assert w[1, 0] == -1 and w[1, 1] == 0.5 and ind[1, 1] == 0
    assert ind[2, 0] == 3 and abs(w[2, 0] - (16.0 - 14.75) / 1.5) <= 1e-15 and w[2, 1] == -1


# ---- second-order accuracy of the scheme -----------------------------------------------------------
def _field(v):
    return v[0] * 0.3 - v[1] * 0.5 + v[2] * 0.8 + 0.5 * v[0] * v[1] + 0.25 * (3 * v[2] ** 2 - 1)


def test_rotation_is_second_order_accurate():
    R = hputil.coord_matrix("G", "C")
    rms = {}
    for nside in (16, 32):
        v = np.array(hputil.pix2vec(nside, np.arange(12 * nside * nside)))
        th, ph = io.rotated_angles(nside, R)
        got = io.interp_val(_field(v)[None], th, ph)[0]
        rms[nside] = np.sqrt(np.mean((got - _field(R @ v)) ** 2))
    print("rotation rms error: nside 16 %.3e, nside 32 %.3e, ratio %.2f" % (rms[16], rms[32], rms[16] / rms[32]))
    assert rms[16] < 1.0e-3 and rms[32] < 2.6e-4 and rms[16] / rms[32] >= 3


# ---- the Python layer refuses what it cannot take before it reaches the device ------------------------------
def test_arguments_checked_before_the_device():
    from cora_amd.signal import lss

    npix = 48
    ok = dict(psi=np.zeros((3, 3, npix)), delta_bias=np.zeros((3, npix)), delta_m=np.zeros((3, npix)),
              chi=np.arange(3.0), out=np.zeros((3, npix)))
    for bad in (dict(psi=np.zeros((2, 3, npix))), dict(delta_m=np.zeros((3, npix - 1))), dict(chi=np.arange(4.0)),
                dict(out=np.zeros((2, npix))), dict(chi=np.array([2.0, 1.0, 0.0])), dict(chi=np.array([0.0, 1.0, 1.0]))):
        with pytest.raises(ValueError):
            lss.za_density_grid(**dict(ok, **bad))
    with pytest.raises(ValueError):
        lss.za_density_grid(np.zeros((3, 1, npix)), np.zeros((1, npix)), np.zeros((1, npix)), np.arange(1.0),
                            np.zeros((1, npix)))
    with pytest.raises(NotImplementedError):
        hputil.get_interp_weights(4, 0.3, 0.2, nest=True)
    with pytest.raises(NotImplementedError):
        hputil.get_interp_val(np.zeros(npix), 0.3, 0.2, nest=True)
    with pytest.raises(Exception, match="Co-ordinate system invalid."):
        hputil.coord_x2y(np.zeros(npix), "G", "Q")
