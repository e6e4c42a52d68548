"""Host checks of the displacement-field step: the numpy oracle of the derivative maps (tests/_grad_oracle.py) against
scipy and against the closed form that is handed to the device, and the argument checks of the public functions
(which raise before any device call).  No GPU."""
import numpy as np
import pytest

import _grad_oracle as go


def _rel(a, b):
    return np.abs(a - b).max() / b.std()


@pytest.mark.parametrize("nside", [4, 8])
def test_ladder_matches_scipy(nside):
    """The ladder identities (no division by sin theta) against scipy's spherical harmonics and their theta
    derivative; measured 1.2e-14 (nside 4) and 3.4e-14 (nside 8) of the map's standard deviation."""
    lmax = 3 * nside - 1
    alm = go.random_alm(np.random.default_rng(nside), lmax, 1)[0]
    dth, dph = go.der1_ladder(alm, nside, lmax)
    bth, bph = go.der1_bruteforce(alm, nside, lmax)
    et, ep = _rel(dth, bth), _rel(dph, bph)
    print("ladder vs scipy nside %d: theta %.2e phi %.2e" % (nside, et, ep))
    assert et <= 1e-12 and ep <= 1e-12, (et, ep)


@pytest.mark.parametrize("nside", [32, 64])
@pytest.mark.parametrize("power", [0.0, 3.0])
def test_composed_matches_ladder(nside, power):
    """The closed form (x S[l a] - S[c a]) / sin theta, S[i m a] / sin theta in numpy fp64 against the ladder
    oracle: the formula handed to the device is right (measured <= 5.4e-13 of the component's std)."""
    lmax = 3 * nside - 1
    alm = go.random_alm(np.random.default_rng(100 + nside), lmax, 1, power)[0]
    lt, lp = go.der1_ladder(alm, nside, lmax)
    ct, cp = go.der1_composed(alm, nside, lmax)
    et, ep = _rel(ct, lt), _rel(cp, lp)
    print("composed vs ladder nside %d power %g: theta %.2e phi %.2e" % (nside, power, et, ep))
    assert et <= 1e-11 and ep <= 1e-11, (et, ep)


def test_ring_selection_and_batch_agree_with_full_maps():
    nside, lmax = 8, 20
    alm = go.random_alm(np.random.default_rng(5), lmax, 3, 3.0)
    full = go.der1_ladder(alm, nside, lmax)
    rings = [0, 7, 15, 30]
    from oracle import healpix

    ri = healpix.ring_info(nside)
    for fun in (go.der1_ladder, go.der1_composed):
        sel = fun(alm, nside, lmax, rings=rings)
        one = fun(alm[1], nside, lmax, rings=rings)
        for k, r in enumerate(rings):
            s, n = int(ri["start"][r]), int(ri["nphi"][r])
            for c in range(2):
                assert np.abs(sel[k][c] - full[c][:, s:s + n]).max() <= 1e-11 * full[c].std()
                # (a batch goes through another BLAS path than a single field: equal to rounding)
                assert np.abs(one[k][c] - sel[k][c][1]).max() <= 1e-13 * full[c].std()
    tt, tp = go.tolerances(alm, nside, lmax)
    assert tt.shape == (3, 4 * nside - 1) and (tt > 0).all() and (tp > 0).all()
    assert go.per_pixel(nside, tt).shape == (3, 12 * nside * nside)
    zt, zp = go.tolerances(np.zeros_like(alm[0]), nside, lmax)
    assert not zt.any() and not zp.any()


def test_parseval_rms():
    from oracle import sht as osht

    nside, lmax = 16, 20
    alm = go.random_alm(np.random.default_rng(9), lmax, 1, 3.0)[0]
    alm[0] = 0.0
    m = osht.alm2map(alm, nside, lmax)
    assert abs(np.sqrt((m ** 2).mean()) / go.map_rms(alm, lmax) - 1) < 1e-3


def test_gradient_coefficients_are_numpys():
    from cora_amd import _lib

    rng = np.random.default_rng(3)
    for n in (2, 3, 7, 33):
        for sign in (1.0, -1.0):
            x = sign * np.cumsum(rng.uniform(0.5, 2.0, n))
            coef = _lib.Context.gradient_coefficients(x)
            f = rng.normal(size=(n, 5))
            fm, fp = np.vstack([f[:1], f[:-1]]), np.vstack([f[1:], f[-1:]])
            got = coef[:, :1] * fm + coef[:, 1:2] * f + coef[:, 2:] * fp
            ref = np.gradient(f, x, axis=0)
            assert np.abs(got - ref).max() <= 1e-13 * np.abs(ref).max()
    with pytest.raises(ValueError):
        _lib.Context.gradient_coefficients([1.0])


def test_assert_shape_moved():
    from cora_amd.signal import lss, lssutil

    assert lss._assert_shape is lssutil.assert_shape
    with pytest.raises(ValueError, match="wrong number of dimensions"):
        lssutil.assert_shape(np.zeros((2, 3)), (6,), "a")
    with pytest.raises(ValueError, match="has the wrong shape"):
        lssutil.assert_shape(np.zeros((2, 3)), (3, 2), "a")


def test_bad_arguments_raise_before_any_device_call(monkeypatch):
    from cora_amd import _lib
    from cora_amd.signal import lss, lssutil
    from cora_amd.util import hputil

    def no_device(*a, **k):
        raise AssertionError("a device call was made before the arguments were checked")

    monkeypatch.setattr(_lib, "get_context", no_device)
    nside, nchi = 4, 5
    npix = 12 * nside * nside
    phi = np.zeros((nchi, npix))
    chi = 100.0 + np.arange(nchi)
    D = np.ones(nchi)
    # lssutil.gradient
    with pytest.raises(ValueError):
        lssutil.gradient(phi[0], chi)                          # wrong number of dimensions
    with pytest.raises(ValueError, match="not a HEALPix map"):
        lssutil.gradient(phi[:, :-1], chi)
    with pytest.raises(ValueError, match="wrong shape"):
        lssutil.gradient(phi, chi[:-1])
    with pytest.raises(ValueError, match="at least 2"):
        lssutil.gradient(phi[:1], chi[:1])
    # lss.zeldovich_displacement
    with pytest.raises(ValueError):
        lss.zeldovich_displacement(phi[0], chi, D)
    with pytest.raises(ValueError, match="not a HEALPix map"):
        lss.zeldovich_displacement(phi[:, :-1], chi, D)
    with pytest.raises(ValueError, match="wrong shape"):
        lss.zeldovich_displacement(phi, chi[:-1], D)
    with pytest.raises(ValueError, match="wrong shape"):
        lss.zeldovich_displacement(phi, chi, D[:-1])
    with pytest.raises(ValueError, match="wrong shape"):
        lss.zeldovich_displacement(phi, chi, D, f=np.ones(nchi + 1))
    with pytest.raises(ValueError, match="at least 2"):
        lss.zeldovich_displacement(phi[:1], chi[:1], D[:1])
    # lss.zeldovich_density
    with pytest.raises(ValueError, match="wrong shape"):
        lss.zeldovich_density(phi, phi[:-1], phi, chi, D)
    with pytest.raises(ValueError, match="wrong shape"):
        lss.zeldovich_density(phi, phi, phi[:, :-1], chi, D)
    with pytest.raises(ValueError, match="wrong shape"):
        lss.zeldovich_density(phi, phi, phi, chi[:-1], D)
    with pytest.raises(ValueError, match="not a HEALPix map"):
        lss.zeldovich_density(phi[:, :-1], phi[:, :-1], phi[:, :-1], chi, D)
    with pytest.raises(ValueError, match="at least 3"):
        lss.zeldovich_density(phi[:2], phi[:2], phi[:2], chi[:2], D[:2])
    # hputil.alm2map_der1
    with pytest.raises(ValueError):
        hputil.alm2map_der1(np.zeros(7, dtype=complex), 4)
    with pytest.raises(ValueError):
        hputil.alm2map_der1(np.zeros((2, 6), dtype=complex), 4)
