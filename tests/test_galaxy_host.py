"""Host checks of the constrained galaxy (csrc/galaxy.hip, cora_amd.foreground.galaxy, hputil's reorder / smoothing): the
oracles of tests/_galaxy_oracle.py against the outputs of the reference's own code (tests/golden/galaxy_vectors.npz,
written by tests/golden/make_golden_galaxy.py), the host functions of the package, the new symbols, argument checking
and the command line.  The GPU is then held to the oracles in tests/test_gpu_galaxy.py."""
import ctypes
import os

import numpy as np
import pytest

import _galaxy_oracle as go
import _pointsource_oracle as po

EPS, U, LD = go.EPS, go.U, go.LD


@pytest.fixture(scope="module")
def gold():
    return go.load_golden()


def getsky_inputs(g, case):
    """(fg, fgs, haslam, sc, am, mv, efreq) of a getsky golden case as float64."""
    fg, fgs = g["in_fg_q"] * float(g["in_fg_s"]), g["in_fgs_q"] * float(g["in_fgs_s"])
    haslam, am = g["in_haslam_q"] * float(g["in_haslam_s"]), g["in_am_q"] * float(g["in_am_s"])
    sc = g[case + "_sc_q"] * float(g[case + "_sc_s"])
    efreq = np.concatenate(([408.0, 1420.0], g["in_freq"]))
    return fg, fgs, haslam, sc, am, float(g[case + "_mv"]), efreq


@pytest.mark.parametrize("case", ["v0", "v1", "v2"])
def test_oracle_matches_reference_map_variance(gold, case):
    m = float(gold[case + "_offset"]) + gold[case + "_map_q"] * float(gold["q"])
    var, _, tol_ref = go.block_variance(m[None], int(gold[case + "_nside_out"]))
    err = np.abs(gold[case + "_var"].astype(LD) - var[0])
    print("%s: reference map_variance against the oracle, worst err / tol %.3g" % (case, go.worst(err, tol_ref[0])))
    assert np.all(err <= tol_ref[0])


@pytest.mark.parametrize("case", ["md", "gsm"])
def test_oracle_matches_reference_getsky(gold, case):
    fg, fgs, haslam, sc, am, mv, efreq = getsky_inputs(gold, case)
    out, _, tol_ref = go.combine(fg, fgs, haslam, sc, am, mv, efreq)
    err = np.abs(gold[case + "_fgt"].astype(LD) - out)
    print("%s: reference fgt against the oracle, worst err / tol %.3g" % (case, go.worst(err, tol_ref)))
    assert np.all(err <= tol_ref)
    x0 = fg[2:, :16] == fgs[2:, :16]
    assert x0.all() and np.all(out[:, :16] > 0)
    # mv of the reference: the mean over the sphere of sqrt(map_variance(fg[0], 16)) (the smoothings are the identity in
    # the golden run).  sqrt halves the relative error of the variance and rounds once; a mean of N terms in any order
    # errs by (N - 1) u of the mean of the (non-negative) terms
    var, _, tol_ref_v = go.block_variance(fg[:1], 16)
    root = np.sqrt(var[0])
    tol = (np.where(var[0] > 0, tol_ref_v[0] / (2 * np.where(var[0] > 0, root, 1)), 0) + U * root).mean() + (root.size - 1) * U * root.mean()
    assert abs(LD(mv) - root.mean()) <= tol * go.SLACK


def test_ring_nest_permutations():
    from cora_amd.util import hputil

    for k in range(6):
        nside = 1 << k
        npix = 12 * nside * nside
        a = np.arange(npix)
        r2n, n2r = hputil.ring2nest(nside, a), hputil.nest2ring(nside, a)
        assert np.array_equal(np.sort(r2n), a) and np.array_equal(np.sort(n2r), a)
        assert np.array_equal(n2r[r2n], a) and np.array_equal(r2n[n2r], a)
        assert np.array_equal(n2r, po.nest2ring(nside, a)) and np.array_equal(r2n, po.ring2nest(nside, a))
        if nside == 1:
            assert np.array_equal(r2n, a)
        else:
            # the children 4 P .. 4 P + 3 of NESTED pixel P share their parent in the ud_grade oracle's hierarchy
            par = po.parent(nside, nside // 2, n2r)
            assert np.array_equal(par, hputil.nest2ring(nside // 2, a // 4))
    assert hputil.ring2nest(4, 7) == int(po.ring2nest(4, np.array([7]))[0]) and isinstance(hputil.nest2ring(4, 7), int)
    assert hputil.get_nside(np.zeros(192)) == 4 and hputil.get_nside(np.zeros((3, 48))) == 2


def test_gauss_beam_formula():
    """exp(-l (l + 1) sigma^2 / 2) in long double.  sigma = fwhm / sqrt(8 ln 2) carries log's ulp, a product, a root
    and a quotient (< 2 eps), sigma^2 twice that and a rounding, the product with l (l + 1) / 2 (exact) one more: the
    exponent A errs by < 6 eps A, which exp turns into a relative error; exp's own ulp and a margin: (6 A + 2) eps."""
    from cora_amd.util import hputil

    for fwhm, lmax in ((np.radians(1.0), 95), (np.radians(5.8), 47), (0.0, 11), (np.radians(10.0), 383)):
        b = hputil.gauss_beam(fwhm, lmax)
        ell = np.arange(lmax + 1).astype(LD)
        A = ell * (ell + 1) * (LD(fwhm) / np.sqrt(8 * np.log(LD(2)))) ** 2 / 2
        ref = np.exp(-A)
        tol = (6 * A + 2) * EPS * ref
        print("gauss_beam fwhm %.3g lmax %d: worst err / tol %.3g" % (fwhm, lmax, go.worst(np.abs(b - ref), tol)))
        assert b.shape == (lmax + 1,) and b[0] == 1.0 and np.all(np.abs(b - ref) <= tol)


def test_abi_symbols_present():
    from cora_amd import _lib

    names = ["corahip_healpix_reorder", "corahip_healpix_block_variance", "corahip_alm_scale_l", "corahip_galaxy_combine"]
    lib = ctypes.CDLL(_lib.LIB_PATH)
    header = open(os.path.join(os.path.dirname(_lib._HERE), "include", "corahip.h")).read()
    for n in names:
        assert n in _lib.SIGNATURES and hasattr(lib, n) and ("int %s(" % n) in header
        assert n[len("corahip_"):] in header.split("#define CORAHIP_ABI_MINOR")[1].split("\n")[0]
    for m in ("healpix_reorder", "healpix_block_variance", "alm_scale_l", "galaxy_combine"):
        assert callable(getattr(_lib.Context, m))


def test_argument_errors():
    from cora_amd.foreground import galaxy
    from cora_amd.util import hputil

    with pytest.raises(ValueError, match="not part of cora_amd"):
        galaxy.ConstrainedGalaxy()
    good = np.ones(12 * 16 * 16)
    with pytest.raises(ValueError, match="haslam must be finite and positive"):
        galaxy.ConstrainedGalaxy(haslam=np.zeros(12 * 16 * 16), spectral=good)
    with pytest.raises(ValueError, match="haslam must be finite and positive"):
        galaxy.ConstrainedGalaxy(haslam=np.where(np.arange(good.size) == 5, np.nan, good), spectral=good)
    with pytest.raises(ValueError, match="Wrong pixel number"):
        galaxy.ConstrainedGalaxy(haslam=np.ones(13), spectral=good)
    with pytest.raises(ValueError, match="one RING map"):
        galaxy.ConstrainedGalaxy(haslam=good, spectral=np.ones((2, good.size)))
    with pytest.raises(ValueError, match="keyed by"):
        galaxy.ConstrainedGalaxy(haslam=good, spectral={"xx": good})
    with pytest.raises(ValueError, match="power of two"):
        galaxy.ConstrainedGalaxy(haslam=good, spectral=good, amp_nside=48)
    with pytest.raises(ValueError, match="nside >= 16"):
        galaxy.ConstrainedGalaxy(haslam=np.ones(12 * 8 * 8), spectral=good)
    gal = object.__new__(galaxy.ConstrainedGalaxy)
    gal.nside, gal.frequencies = 16, np.array([400.0, 500.0])
    with pytest.raises(ValueError, match="nside >= 32"):
        gal.getsky_device()
    with pytest.raises(ValueError, match="nside >= 32"):
        gal.getsky()

    with pytest.raises(ValueError, match="power of two"):
        hputil.reorder(np.zeros(12 * 9), r2n=True)
    with pytest.raises(ValueError, match="Wrong pixel number"):
        hputil.reorder(np.zeros(50), n2r=True)
    with pytest.raises(ValueError, match="exclusive"):
        hputil.reorder(np.zeros(48), r2n=True, n2r=True)
    with pytest.raises(ValueError, match="inp and out"):
        hputil.reorder(np.zeros(48))
    with pytest.raises(ValueError, match="power of two"):
        hputil.ring2nest(3, [0])
    with pytest.raises(ValueError, match="out of range"):
        hputil.nest2ring(2, [48])
    assert np.array_equal(hputil.reorder(np.arange(48.0), inp="RING", out="RING"), np.arange(48.0))

    with pytest.raises(ValueError, match="factor 1 to 64"):
        galaxy.map_variance(np.zeros(12 * 128 * 128), 1)
    with pytest.raises(ValueError, match="factor 1 to 64"):
        galaxy.map_variance(np.zeros(48), 4)
    with pytest.raises(ValueError, match="power of two"):
        galaxy.map_variance(np.zeros(12 * 9), 1)
    with pytest.raises(ValueError, match="one map"):
        galaxy.map_variance(np.zeros((2, 2, 48)), 1)
    with pytest.raises(ValueError, match="fl has shape"):
        hputil._beams(2, 5, np.ones((2, 5)), None, None)
    with pytest.raises(ValueError, match="one value per map"):
        hputil._beams(3, 5, None, [0.1, 0.2], None)
    assert hputil._beams(3, 5, None, None, None).tolist() == np.ones((3, 6)).tolist()


def test_chunk_var():
    from cora_amd.foreground import galaxy

    rng = np.random.default_rng(5)
    for a in (rng.normal(3.0, 2.0, (7, 13)), rng.normal(size=40) + 1j * rng.normal(size=40), np.array([2.0, 4.0])):
        v = galaxy.chunk_var(a)
        assert abs(v - np.var(a)) <= 64 * EPS * np.var(a) + 1e-300 and np.isrealobj(v)


def test_cli_refusals():
    from click.testing import CliRunner

    from cora_amd.scripts import makesky

    for cmd in ("galaxy", "foreground"):
        r = CliRunner().invoke(makesky.cli, [cmd, "--nside", "32", "--freq", "400", "500", "4"])
        assert r.exit_code != 0 and "not part of cora_amd" in r.output and "--skydata" in r.output
        # fewer than two frequencies: the reference prints this and returns
        r = CliRunner().invoke(makesky.cli, [cmd, "--nside", "32", "--freq", "400", "500", "1"])
        assert r.exit_code == 0 and "Number of frequencies must be more than two." in r.output
        assert "--skydata" in CliRunner().invoke(makesky.cli, [cmd, "--help"]).output
