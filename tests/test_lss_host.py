"""Host side of the Zel'dovich SPH assignment (cora_amd.signal.lss.za_density_sph): the numpy oracle
(tests/_za_oracle.py) against the reference's own pmesh natives (tests/golden/lss_vectors.npz), the reference's
stride-9 scatter, calculate_positions and the HEALPix neighbour list.  No GPU needed."""
import os

import numpy as np
import pytest

import _za_oracle as zo
from cora_amd.util import hputil, pmesh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lg():
    g = dict(np.load(os.path.join(ROOT, "tests", "golden", "lss_vectors.npz")))
    g["psi"] = g["psi_q"].astype(np.float64) * np.array([g["q_r"], g["q_a"], g["q_a"]])[:, None, None]
    g["delta_bias"] = g["delta_bias_q"].astype(np.float64) * g["q_a"]
    g["delta_m"] = g["delta_m_q"].astype(np.float64) * g["q_a"]
    return g


def _terms(g, form):
    nside = int(g["nside"])
    nchi, npix = g["delta_bias"].shape
    angpos = np.array(hputil.pix2ang(nside, np.arange(npix)))
    per = [zo.slice_terms(g["psi"][:, ii], g["delta_bias"][ii], g["delta_m"][ii], g["chi"][ii], g["chi"], nside,
                          float(g["sigma_ang"]), float(g["sigma_chi"]), angpos, form) for ii in range(nchi)]
    return [np.concatenate([p[k] for p in per]) for k in range(5)]


def test_golden_inputs_cover_the_edge_cases(lg):
    nside = int(lg["nside"])
    nchi, npix = lg["delta_bias"].shape
    th, ph = hputil.pix2ang(nside, np.arange(npix))
    new_th = th[None] + lg["psi"][1]
    new_ph = ph[None] + lg["psi"][2]
    new_chi = lg["chi"][:, None] + lg["psi"][0]
    assert (new_th < 0).any() and (new_th > np.pi).any()                  # across both poles
    assert (new_ph < 0).any() and (new_ph >= 2 * np.pi).any()             # across phi = 0 both ways
    assert (new_chi < lg["chi"][0]).any() and (new_chi > lg["chi"][-1]).any()
    assert (1 + lg["delta_m"] < 0.1).any() and (1 + lg["delta_m"] > 3.0).any()
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "lss_vectors.npz")) < 1 << 20


def test_calculate_positions_matches_reference(lg):
    nside = int(lg["nside"])
    nchi, npix = lg["delta_bias"].shape
    angpos = np.array(hputil.pix2ang(nside, np.arange(npix)))
    sel = lg["sel"]
    got = np.concatenate([pmesh.calculate_positions(angpos, lg["psi"][1:, ii])[:, sel[sel // npix == ii] % npix].T
                          for ii in range(nchi)])
    assert np.array_equal(got, lg["sel_pos"])
    assert (got[:, 0] >= 0).all() and (got[:, 0] <= np.pi).all()
    assert (got[:, 1] >= 0).all() and (got[:, 1] <= 2 * np.pi).all()


def test_calculate_positions_wraps_like_numpy_floor_mod():
    ang = np.array([[0.1, 3.0, 0.5, 1.0], [0.2, 6.0, 6.2, 0.1]])
    disp = np.array([[-0.3, 0.5, 0.0, -7.0], [0.0, 0.0, 0.2, -0.3]])
    got = pmesh.calculate_positions(ang, disp)
    th = np.array([0.2, 2 * np.pi - 3.5, 0.5, np.pi - ((1.0 - 7.0) % np.pi)])
    ph = np.array([0.2 + np.pi, 6.0 + np.pi - 2 * np.pi, 6.4 - 2 * np.pi, (-0.2 + np.pi) % (2 * np.pi)])
    assert np.allclose(got[0], th, rtol=0, atol=1e-15) and np.allclose(got[1], ph, rtol=0, atol=1e-14)


def test_oracle_reproduces_reference_weights(lg):
    rho, pind, pw, rind, rw = _terms(lg, "dot")
    sel = lg["sel"]
    assert np.array_equal(pind[sel], lg["sel_pind"])
    assert np.array_equal(rind[sel], lg["sel_rind"])
    assert np.abs(pw[sel] - lg["sel_pw"]).max() <= 1e-13
    assert np.abs(rw[sel] - lg["sel_rw"]).max() <= 1e-13
    # the kernel's |v x w|^2 form of the same weights
    _, pind_c, pw_c, _, _ = _terms(lg, "cross")
    assert np.array_equal(pind_c, pind) and np.abs(pw_c - pw).max() <= 1e-12


@pytest.mark.parametrize("form", ["dot", "cross"])
def test_oracle_reproduces_golden_out(lg, form):
    out = np.full(lg["delta_bias"].shape, float(lg["out0"]))
    zo.za_density_sph(lg["psi"], lg["delta_bias"], lg["delta_m"], lg["chi"], out, form=form)
    ref = lg["out"]
    assert np.abs(out - ref).max() <= 1e-13 * np.abs(ref + 1).max()
    # mass: every particle deposits exactly its 1 + delta_bias
    assert abs((out + 1 - float(lg["out0"])).sum() - (1 + lg["delta_bias"]).sum()) <= 1e-12 * (1 + lg["delta_bias"]).sum()


def test_reference_bin_delta_uses_row_stride_nine(lg):
    """The reference's C scatter puts bin ri of pixel pi at flat index 9 ri + pi, not ri npix + pi."""
    nchi, npix = lg["delta_bias"].shape
    rho, pind, pw, rind, rw = _terms(lg, "dot")
    v = (rho[:, None] * pw)[:, :, None] * rw[:, None, :]
    flat9 = rind[:, None, :].astype(np.int64) * 9 + pind[:, :, None]
    stride9 = np.bincount(flat9.ravel(), weights=v.ravel(), minlength=(nchi - 1) * 9 + npix)
    bug = lg["bin_delta_ref"]
    assert bug.size == (nchi - 1) * 9 + npix == stride9.size
    assert np.abs(bug - stride9).max() <= 1e-12 * np.abs(bug).max()
    correct = lg["out"] + 1 - float(lg["out0"])
    # same mass, other place: the correct scatter does not start with the recorded prefix
    assert abs(bug.sum() - correct.sum()) <= 1e-12 * correct.sum()
    assert np.abs(correct.ravel()[: bug.size] - bug).max() > 0.1


def _three_face_vertex_pixels(nside):
    """Pixels touching one of the 8 vertices where only three base faces meet (z = +-2/3, phi = k pi / 2)."""
    eps = 1e-7
    th, ph = [], []
    for z in (2.0 / 3.0, -2.0 / 3.0):
        t0 = np.arccos(z)
        sgn = -1.0 if z > 0 else 1.0       # towards the nearer pole
        for k in range(4):
            p0 = k * np.pi / 2
            th += [t0 + sgn * eps, t0 + sgn * eps, t0 - sgn * eps]
            ph += [p0 + eps, p0 - eps, p0]
    return set(hputil.ang2pix(nside, np.array(th), np.mod(np.array(ph), 2 * np.pi)).tolist())


@pytest.mark.parametrize("nside", [1, 2, 4, 16])
def test_host_neighbours_properties(nside):
    npix = 12 * nside * nside
    nb = zo.get_all_neighbours(nside, np.arange(npix)).T          # [npix, 8]
    ok = nb >= 0
    # symmetric
    for p in range(npix):
        for n in nb[p][ok[p]]:
            assert p in nb[n], (nside, p, n)
    # every neighbour centre within about 2 pixel sizes
    v = np.array(hputil.pix2vec(nside, np.arange(npix))).T
    cosang = np.einsum("ij,ikj->ik", v, v[np.where(ok, nb, 0)])
    ang = np.arccos(np.clip(cosang, -1, 1))
    assert ang[ok].max() <= 2.05 * hputil.nside2resol(nside)
    assert (ang[ok] > 0).all()
    # -1 only for pixels that touch a vertex of three base faces (one such corner per pixel, two per face at nside 1)
    missing = set(np.where(~ok.all(axis=1))[0].tolist())
    assert missing == _three_face_vertex_pixels(nside)
    assert set((~ok).sum(axis=1)[sorted(missing)].tolist()) == {2 if nside == 1 else 1}


def test_host_helpers_agree():
    nside = 8
    npix = 12 * nside * nside
    th, ph = hputil.pix2ang(nside, np.arange(npix))
    v = np.array(hputil.pix2vec(nside, np.arange(npix))).T
    w = hputil.ang2vec(th, ph)
    assert np.abs(v - w).max() < 1e-15 * 4
    assert abs(hputil.nside2resol(nside) - np.sqrt(4 * np.pi / npix)) < 1e-17
    ix, iy, f = zo.ring2xyf(nside, np.arange(npix))
    assert np.array_equal(zo.xyf2ring(nside, ix, iy, f), np.arange(npix))


def test_za_density_sph_checks_shapes_before_the_device():
    from cora_amd.signal import lss

    npix = 12 * 4 * 4
    good = dict(psi=np.zeros((3, 4, npix)), delta_bias=np.zeros((4, npix)), delta_m=np.zeros((4, npix)),
                chi=np.arange(4.0), out=np.zeros((4, npix)))
    for name, bad in (("psi", np.zeros((2, 4, npix))), ("delta_m", np.zeros((4, npix + 1))), ("chi", np.arange(5.0)),
                      ("out", np.zeros((4 * npix,))), ("delta_bias", np.zeros((4, 100)))):
        kw = dict(good, **{name: bad})
        with pytest.raises(ValueError):
            lss.za_density_sph(**kw)
    with pytest.raises(ValueError):
        lss.za_density_sph(np.zeros((3, 2, npix)), np.zeros((2, npix)), np.zeros((2, npix)), np.arange(2.0),
                           np.zeros((2, npix)))
