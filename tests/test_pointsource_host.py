"""Host checks of the point-source path (csrc/pointsource.hip, cora_amd.foreground.pointsource / poisson): the oracles
of tests/_pointsource_oracle.py against the outputs of the reference's own code (tests/golden/pointsource_vectors.npz,
written by tests/golden/make_golden_pointsource.py), the host functions of the package, the ud_grade hierarchy, argument
checking and the command line.  The GPU is then held to the oracles in tests/test_gpu_pointsource.py."""
import ctypes
import os

import numpy as np
import pytest

import _pointsource_oracle as po

EPS, U, LD = po.EPS, po.U, po.LD
MODEL_CASES = ["dm4", "dm8", "pl4", "pl8"]


@pytest.fixture(scope="module")
def cases():
    return po.load_golden()


def _worst(err, tol):
    return float(np.max(np.asarray(err, dtype=np.float64) / np.maximum(tol, np.finfo(np.float64).tiny))) if np.size(err) else 0.0


def test_abi_symbols_present():
    from cora_amd import _lib

    names = ["corahip_pointsource_population", "corahip_pointsource_paint", "corahip_polarise_rotate",
             "corahip_faraday_rotate", "corahip_healpix_ud_grade"]
    lib = ctypes.CDLL(_lib.LIB_PATH)
    header = open(os.path.join(os.path.dirname(_lib._HERE), "include", "corahip.h")).read()
    for n in names:
        assert n in _lib.SIGNATURES and hasattr(lib, n) and ("int %s(" % n) in header
    assert "#define CORAHIP_ABI_MINOR 12 " in header and lib.corahip_abi_minor() == 12
    for m in ("pointsource_population", "pointsource_paint", "polarise_rotate", "faraday_rotate", "healpix_ud_grade"):
        assert callable(getattr(_lib.Context, m))


def test_poisson_matches_reference(cases):
    """``total`` and ``av`` exact, the events to the spline's tolerance (1e-13, tests/test_host.py), under the
    reference's seed: numpy's legacy stream is consumed as the reference consumes it."""
    from cora_amd.foreground import pointsource, poisson

    c = cases["poi"]
    m = pointsource.DiMatteo()
    m.flux_min = c["flux_min"]
    t = np.log(c["flux_max"] / c["flux_min"])
    rate = m._log_rate(c["area"])
    assert poisson.expected_events(t, rate) == c["av"]
    np.random.seed(int(c["seed"]))
    ev = poisson.inhomogeneous_process_approx(t, rate)
    err = max(np.abs(ev[:64] - c["first"]).max(), np.abs(ev[-64:] - c["last"]).max())
    print("poisson: total %d (reference %d), worst event error %.3g (bound 1e-13)" % (len(ev), c["total"], err))
    assert len(ev) == c["total"] and err < 1e-13
    # the next draw of the global state is the one the reference would make
    np.random.seed(int(c["seed"]))
    np.random.poisson(c["av"])
    np.random.rand(int(c["total"]))
    follow = np.random.rand()
    np.random.seed(int(c["seed"]))
    poisson.inhomogeneous_process_approx(t, rate)
    assert np.random.rand() == follow
    # the two exact processes: events lie in [0, t], ascending, and their number is Poisson about rate t
    np.random.seed(5)
    hp = poisson.homogeneous_process(200.0, 3.0)
    assert np.all(np.diff(hp) > 0) and hp[0] > 0 and hp[-1] <= 200.0 and abs(len(hp) - 600) < 5 * 600**0.5
    ip = poisson.inhomogeneous_process(10.0, lambda s: 50.0 + 5.0 * s)
    assert ip.min() >= 0 and ip.max() <= 10.0 and abs(len(ip) - 750) < 5 * 750**0.5


@pytest.mark.parametrize("name", MODEL_CASES)
def test_generate_population_matches_reference(cases, name):
    """``generate_population`` under the legacy seed gives the reference's fluxes: the same count, values to the
    spline's tolerance in log flux (1e-13) plus exp and the product."""
    from cora_amd.foreground import pointsource

    c = cases[name]
    seed = {"dm4": 11, "dm8": 12, "pl4": 13, "pl8": 14}[name]
    m = (pointsource.DiMatteo if name.startswith("dm") else pointsource.PowerLawModel)()
    m.flux_min = c["flux_min"]
    m.flux_max = 200.0 if name == "pl4" else None
    np.random.seed(seed)
    flux = m.generate_population(4 * np.pi)
    assert flux.shape == c["flux"].shape
    r = _worst(np.abs(flux / c["flux"] - 1), 1e-13 + 4 * EPS)
    print("%s: %d fluxes, worst relative error / (1e-13 + 4 eps) %.3g" % (name, len(flux), r))
    assert r <= 1
    assert (m.spectral_mean, m.spectral_width, m.spectral_pivot) == (c["spectral_mean"], c["spectral_width"], c["spectral_pivot"])


@pytest.mark.parametrize("dtype", [np.float64, LD], ids=["f64", "longdouble"])
@pytest.mark.parametrize("name", MODEL_CASES)
def test_oracles_reproduce_reference_sky(cases, name, dtype):
    """Both paint oracles, then the rotation oracle, against the reference's ``getpolsky``: plane 0 (its ``getsky``)
    under the paint bound, planes 1, 2 under the rotation bound on top of the paint bound carried through it."""
    c = cases[name]
    x, den, c2, npix = po.power_law_inputs(c)
    order = np.argsort(c["pix"], kind="stable")
    sky, tol = po.paint(c["pix"][order], c["flux"][order], c["index"][order], None, None, x, den, c2, npix, dtype=dtype)
    ref = c["sky_pol"]
    r0 = _worst(np.abs(sky - ref[:, 0]), tol)
    q, u, rtol = po.rotate(sky * c["q_frac"][None, :].astype(dtype), sky * c["u_frac"][None, :].astype(dtype),
                           po.wavelengths(c["freq"]), c["rm"], dtype=dtype)
    carried = tol * np.hypot(c["q_frac"], c["u_frac"])[None, :] * 2**0.5
    r1 = _worst(np.abs(q - ref[:, 1]), rtol + carried)
    r2 = _worst(np.abs(u - ref[:, 2]), rtol + carried)
    print("%s %s: worst err / tol  sky %.3g  Q %.3g  U %.3g  (largest |a| %.0f)"
          % (name, np.dtype(dtype).name, r0, r1, r2, np.abs(2 * po.wavelengths(c["freq"])[:, None] * c["rm"][None, :]).max()))
    assert r0 <= 1 and r1 <= 1 and r2 <= 1
    assert np.array_equal(sky == 0, ref[:, 0] == 0)


@pytest.mark.parametrize("dtype", [np.float64, LD], ids=["f64", "longdouble"])
def test_oracles_reproduce_reference_catalogue_cube(cases, dtype):
    from cora_amd.util import hputil

    c = cases["cat"]
    nside = int(c["nside"])
    npix = 12 * nside * nside
    pix = hputil.ang2pix(nside, np.pi / 2.0 - np.radians(c["DEC"]), np.radians(c["RA"]))
    flux, beta, gamma, polw = po.catalogue_inputs(c, pix)
    assert np.isnan(c["POLANG"]).sum() >= 1 and not polw[np.isnan(c["POLANG"])].any()
    order = np.argsort(pix, kind="stable")
    den, c2 = po.conversion(c["freq"], nside)
    x = np.log(c["freq"] / 600.0)
    cube, tol = po.paint(pix[order], flux[order], beta[order], gamma[order], polw[order], x, den, c2, npix, npol=4, dtype=dtype)
    r = [_worst(np.abs(cube[:, k] - c["cube"][:, k]), tol[:, k]) for k in range(3)]
    q, u, rtol = po.rotate(cube[:, 1], cube[:, 2], po.wavelengths(c["freq"]), c["rm"], dtype=dtype)
    carried = (tol[:, 1] + tol[:, 2])
    rq = _worst(np.abs(q - c["cube_rot"][:, 1]), rtol + carried)
    ru = _worst(np.abs(u - c["cube_rot"][:, 2]), rtol + carried)
    print("catalogue %s: worst err / tol  I %.3g  Q %.3g  U %.3g  rotated Q %.3g  U %.3g" % (np.dtype(dtype).name, *r, rq, ru))
    assert max(r) <= 1 and rq <= 1 and ru <= 1
    assert np.array_equal(c["cube_rot"][:, 0], c["cube"][:, 0]) and not cube[:, 3].any()


@pytest.mark.parametrize("dtype", [np.float64, LD], ids=["f64", "longdouble"])
def test_rotation_oracle_reproduces_faraday_rotate(cases, dtype):
    c = cases["far"]
    q, u, tol = po.rotate(c["cube"][:, 1], c["cube"][:, 2], po.wavelengths(c["freq"]), c["rm"], dtype=dtype)
    r = max(_worst(np.abs(q - c["rotated"][:, 1]), tol), _worst(np.abs(u - c["rotated"][:, 2]), tol))
    print("faraday_rotate %s: worst err / tol %.3g" % (np.dtype(dtype).name, r))
    assert r <= 1
    assert np.array_equal(c["rotated"][:, 0], c["cube"][:, 0]) and np.array_equal(c["rotated"][:, 3], c["cube"][:, 3])


@pytest.mark.parametrize("hi,lo", [(2, 1), (8, 1), (8, 4), (16, 2), (32, 8)])
def test_ud_grade_hierarchy(hi, lo):
    """The parent of fine pixel p is the coarse pixel its centre falls into (an independent route to the hierarchy:
    a child's centre lies strictly inside its parent); upgrading then degrading is the identity bit for bit; degrading
    keeps the mean to (4^k) u."""
    from cora_amd.util import hputil

    p = np.arange(12 * hi * hi)
    assert np.array_equal(po.parent(hi, lo, p), hputil.ang2pix(lo, *hputil.pix2ang(hi, p)))
    assert np.array_equal(po.nest2ring(hi, po.ring2nest(hi, p)), p)
    assert np.array_equal(np.sort(po.ring2nest(hi, p)), p)
    rng = np.random.default_rng(hi * 100 + lo)
    coarse = rng.normal(size=(3, 12 * lo * lo))
    fine = po.ud_grade(coarse, hi)
    assert fine.shape == (3, 12 * hi * hi) and np.array_equal(po.ud_grade(fine, lo), coarse)
    assert np.array_equal(np.sort(np.bincount(po.parent(hi, lo, p))), np.full(12 * lo * lo, (hi // lo) ** 2))
    m = rng.normal(size=(3, 12 * hi * hi)) + 3.0
    d = po.ud_grade(m, lo)
    k4 = (hi // lo) ** 2
    # both means in long double, so that only the degrading's own roundings are seen: each coarse pixel is within
    # (4^k - 1) u mean |children| of its exact mean, plus u for the division
    r = _worst(np.abs(d.astype(LD).mean(axis=1) - m.astype(LD).mean(axis=1)), k4 * U * np.abs(m).mean(axis=1))
    print("ud_grade %d -> %d: mean kept to %.3g of its bound" % (hi, lo, r))
    assert r <= 1
    assert np.array_equal(po.ud_grade(m, hi), m)


def test_constructors_and_messages():
    from cora_amd.foreground import gaussianfg, pointsource

    ub = pointsource.CombinedPointSources._UnresolvedBackground()
    assert isinstance(ub, gaussianfg.PointSources) and (ub.A, ub.nu_0, ub.l_0, ub.oversample) == (3.55e-5, 408.0, 100.0, 0)
    assert isinstance(pointsource.UnresolvedBackground(), gaussianfg.PointSources)
    dm, pl = pointsource.DiMatteo(), pointsource.PowerLawModel()
    assert (dm.flux_min, dm.flux_max, dm.faraday, dm.sigma_pol_frac) == (1e-4, None, True, 0.03)
    assert (dm.gamma1, dm.gamma2, dm.S_0, dm.k1) == (1.75, 2.51, 0.88, 1.52e3)
    assert (pl.source_index, pl.source_pivot, pl.source_amplitude) == (2.5, 1.0, 2.396e3)
    s = np.array([0.3, 2.0])
    assert np.array_equal(dm.source_count(s), 1.52e3 / ((s / 0.88) ** 1.75 + (s / 0.88) ** 2.51))
    assert np.array_equal(pl.source_count(s), 2.396e3 * s ** -2.5)
    rr = pointsource.CombinedPointSources._RandomResolved
    assert rr.flux_min == 0.1 and rr.flux_max == 4.0 * (151.0 / 600.0) ** -0.7
    assert pointsource.CombinedPointSources._RealResolved.flux_min == 4.0 and pointsource.RealPointSources.flux_min == 10.0
    dm.nside = 4
    with pytest.raises(ValueError, match="faraday_map="):
        dm._rm_device()
    with pytest.raises(ValueError, match="catalogue="):
        pointsource.RealPointSources()
    with pytest.raises(ValueError, match="GAMMA"):
        pointsource.RealPointSources(catalogue=np.zeros(3, dtype=[(k, "f8") for k in pointsource.CATALOGUE_FIELDS[:-1]]))
    with pytest.raises(Exception):
        dm.nside = 6
    cat = np.zeros(4, dtype=[(k, "f8") for k in pointsource.CATALOGUE_FIELDS])
    cat["S600"] = [1.0, 5.0, 20.0, 400.0]
    real = pointsource.RealPointSources(catalogue=cat)
    real._generate_catalogue()
    assert list(real._masked_catalogue["S600"]) == [20.0, 400.0]
    real.flux_max = 100.0
    real._generate_catalogue()
    assert list(real._masked_catalogue["S600"]) == [20.0]
    comb = pointsource.CombinedPointSources()
    comb.nside, comb.frequencies, comb.flux_max = 4, np.array([400.0, 500.0]), 2.0
    with pytest.warns(UserWarning, match="catalogue="):
        pointsource._warned_no_catalogue = False
        _, rnd_obj, real_obj = comb._components()
    assert real_obj is None and rnd_obj.flux_max == 2.0 and rnd_obj.nside == 4 and list(rnd_obj.frequencies) == [400.0, 500.0]
    comb = pointsource.CombinedPointSources(catalogue=cat, faraday_map=np.zeros(12))
    comb.nside, comb.flux_max = 2, 50.0
    _, rnd_obj, real_obj = comb._components()
    assert real_obj.flux_max == 50.0 and real_obj.flux_min == 4.0 and rnd_obj.flux_max == rr.flux_max and real_obj.nside == 2


def test_catalogue_file_is_read(tmp_path, cases):
    from cora_amd.foreground import pointsource

    c = cases["cat"]
    path = tmp_path / "cat.dat"
    with open(path, "w") as f:
        f.write(" ".join(pointsource.CATALOGUE_FIELDS) + " NAME\n")
        for i in range(len(c["RA"])):
            f.write(" ".join(repr(float(c[k][i])) for k in pointsource.CATALOGUE_FIELDS) + " SRC_%d\n" % i)
    cat = pointsource.load_catalogue(str(path))
    for k in pointsource.CATALOGUE_FIELDS:
        assert np.array_equal(cat[k], c[k], equal_nan=True)
    real = pointsource.RealPointSources(catalogue=str(path))
    real.nside, real.frequencies, real.flux_min = int(c["nside"]), c["freq"], 1.0
    pix, flux, beta, gamma, polw = real._sources()
    oflux, obeta, ogamma, opolw = po.catalogue_inputs(c, pix)
    assert np.array_equal(flux, oflux) and np.array_equal(polw, opolw) and np.array_equal(gamma, ogamma)


class _Untouchable:
    def __getattr__(self, name):
        raise AssertionError("the library was touched (%s) before the arguments were checked" % name)


def test_python_layer_checks_arguments_before_the_library():
    import torch

    from cora_amd._lib import Context

    ctx = Context.__new__(Context)
    ctx.lib, ctx.h, ctx.device = _Untouchable(), None, torch.device("cpu")
    pix = torch.zeros(5, dtype=torch.int64)
    v = torch.zeros(5, dtype=torch.float64)
    x, den = np.zeros(3), np.ones(3)
    bad = [dict(pix=torch.zeros(5, dtype=torch.int32)), dict(flux=torch.zeros(4, dtype=torch.float64)),
           dict(beta=torch.zeros(5, dtype=torch.float32)), dict(npol=2), dict(polw=torch.zeros((5, 2), dtype=torch.float64)),
           dict(polw=torch.zeros((5, 3), dtype=torch.float64), npol=4), dict(den=np.ones(4)), dict(accumulate=True),
           dict(out=torch.zeros((3, 47), dtype=torch.float64)), dict(gamma=torch.zeros(6, dtype=torch.float64)),
           dict(out=torch.zeros((3, 4, 48), dtype=torch.float64))]
    for kw in bad:
        args = dict(pix=pix, flux=v, beta=v, x=x, den=den, c2=1.0, npix=48)
        args.update(kw)
        with pytest.raises(ValueError):
            ctx.pointsource_paint(**args)
    cube = torch.zeros((3, 4, 48), dtype=torch.float64)
    for kw in (dict(polmap=torch.zeros((3, 2, 48), dtype=torch.float64)), dict(polmap=cube.numpy()), dict(rm=np.zeros(47)),
               dict(wv=np.zeros(4)), dict(polmap=torch.zeros((3, 4, 48), dtype=torch.float32))):
        args = dict(polmap=cube, rm=np.zeros(48), wv=np.zeros(3))
        args.update(kw)
        with pytest.raises(ValueError):
            ctx.faraday_rotate(**args)
    sky = torch.zeros((3, 48), dtype=torch.float64)
    for kw in (dict(intensity=cube), dict(qfrac=np.zeros(47)), dict(rm=np.zeros(48), wv=None), dict(wv=np.zeros(2)),
               dict(out=torch.zeros((3, 3, 48), dtype=torch.float64))):
        args = dict(intensity=sky, qfrac=np.zeros(48), ufrac=np.zeros(48), wv=np.zeros(3))
        args.update(kw)
        with pytest.raises(ValueError):
            ctx.polarise_rotate(**args)
    for maps, ns in ((torch.zeros((2, 48), dtype=torch.float64), 3), (torch.zeros((2, 108), dtype=torch.float64), 2),
                     (torch.zeros((2, 47), dtype=torch.float64), 2), (torch.zeros(48, dtype=torch.float64), 2),
                     (torch.zeros((1, 12 * 128 * 128), dtype=torch.float64), 1)):
        with pytest.raises(ValueError):
            ctx.healpix_ud_grade(maps, ns)
    with pytest.raises(ValueError):
        ctx.pointsource_population(1, 5, np.array([0.1, 0.5, 1.0]), np.zeros(3), np.zeros(3), 1.0, -0.7, 0.1, 48)
    with pytest.raises(ValueError):
        ctx.pointsource_population(1, -1, np.array([0.0, 0.5, 1.0]), np.zeros(3), np.zeros(3), 1.0, -0.7, 0.1, 48)


def test_pointsource_command_writes_a_map(tmp_path, monkeypatch):
    """The ``pointsource`` command under click's runner with the model's map functions patched: options reach the model,
    a map of the right shape is written, ``--pol full`` without a rotation-measure map is a ClickException."""
    from click.testing import CliRunner

    from cora_amd.foreground import pointsource
    from cora_amd.scripts import makesky

    seen = {}

    def getsky(self, rng=None):
        seen.update(nside=self.nside, freq=np.array(self.frequencies), flux_max=self.flux_max, cat=self._catalogue,
                    far=self._faraday, rng=rng)
        return np.full((len(self.frequencies), 12 * self.nside**2), 2.0)

    def getpolsky(self, rng=None):
        sky = getsky(self, rng)
        out = np.zeros((sky.shape[0], 4, sky.shape[1]))
        out[:, 0] = sky
        return out

    monkeypatch.setattr(pointsource.CombinedPointSources, "getsky", getsky)
    monkeypatch.setattr(pointsource.CombinedPointSources, "getpolsky", getpolsky)
    base = ["pointsource", "--nside", "4", "--freq", "400", "800", "4", "--freq-mode", "edge"]
    out = str(tmp_path / "ps.h5")
    r = CliRunner().invoke(makesky.cli, base + ["--pol", "none", "--maxflux", "7.5", "--seed", "3", "--filename", out])
    assert r.exit_code == 0, r.output
    f = np.load(out if os.path.exists(out) else out + ".npz")
    assert f["map"].shape == (4, 1, 192) and np.all(f["map"] == 2.0) and list(f["index_map__pol"]) == ["I"]
    assert seen["nside"] == 4 and seen["flux_max"] == 7.5 and seen["cat"] is None and seen["far"] is None
    assert np.array_equal(seen["freq"], [450.0, 550.0, 650.0, 750.0]) and isinstance(seen["rng"], np.random.Generator)
    r = CliRunner().invoke(makesky.cli, base + ["--pol", "full", "--filename", out])
    assert r.exit_code != 0 and "--faraday-map" in r.output
    rm = str(tmp_path / "rm.npy")
    np.save(rm, np.arange(48.0))
    cat = str(tmp_path / "cat.dat")
    with open(cat, "w") as fh:
        fh.write(" ".join(pointsource.CATALOGUE_FIELDS) + "\n10.0 20.0 30.0 0.1 45.0 -0.7 0.0\n")
    out2 = str(tmp_path / "pol.h5")
    r = CliRunner().invoke(makesky.cli, base + ["--pol", "full", "--faraday-map", rm, "--catalogue", cat, "--filename", out2])
    assert r.exit_code == 0, r.output
    f = np.load(out2 if os.path.exists(out2) else out2 + ".npz")
    assert f["map"].shape == (4, 4, 192) and list(f["index_map__pol"]) == ["I", "Q", "U", "V"]
    assert np.array_equal(seen["far"], np.arange(48.0)) and seen["cat"]["S600"][0] == 30.0 and seen["rng"] is None
    r = CliRunner().invoke(makesky.cli, ["foreground", "--nside", "8"])
    assert r.exit_code != 0 and "not part of cora_amd" in r.output


def test_normal_mapping_is_the_specified_one():
    """``first_normal`` of the oracle, which writes the words -> normal mapping out, gives on the a_lm stream's own words
    the bits of oracle/philox.py's ``boxmuller_counter``: one mapping, two streams."""
    from oracle import philox

    lo = np.arange(5000)
    r = philox.philox4x32_10(lo, 3, 0, 0, 77, 1)
    assert np.array_equal(po.first_normal(*r), philox.boxmuller_counter(77 + (1 << 32), lo, 3)[0])


DIST_SEEDS = (1, 2, 3, 4, 5)


def test_generator_distribution_on_the_oracle():
    """The population stream, evaluated by the oracle alone: over 5 fixed seeds of 2e5 sources the counts in 20
    logarithmic flux bins lie within 5 sigma of the integral of ``source_count``, the pixel counts at nside 2 within
    5 sigma of uniform, and the indices have the stated mean and width.  Also the exclusion rule of the pixel test: fewer
    than 1 in 1000 sources lie within npix eps of a pixel boundary (none, in fact)."""
    from scipy.integrate import quad

    from cora_amd.foreground import pointsource, poisson

    m = pointsource.DiMatteo()
    m.flux_min, m.flux_max = 0.01, 100.0
    area, n, npix = 4 * np.pi, 200000, 48
    t = np.log(m.flux_max / m.flux_min)
    data, y2 = poisson.inverse_cdf(t, m._log_rate(area)).data()
    edges = np.exp(np.linspace(np.log(m.flux_min), np.log(m.flux_max), 21))
    expect = np.array([quad(m.source_count, a, b)[0] for a, b in zip(edges[:-1], edges[1:])])
    expect = expect / expect.sum() * n
    worst_flux = worst_pix = 0.0
    for seed in DIST_SEEDS:
        p = po.population(seed, n, data[:, 0], data[:, 1], y2, m.flux_min, m.spectral_mean, m.spectral_width, npix)
        assert p["flux"].min() >= m.flux_min and p["flux"].max() <= m.flux_max * (1 + 1e-12)
        counts = np.histogram(p["flux"], bins=edges)[0]
        worst_flux = max(worst_flux, (np.abs(counts - expect) / np.sqrt(expect)).max())
        pc = np.bincount(p["pix"], minlength=npix)
        worst_pix = max(worst_pix, (np.abs(pc - n / npix) / np.sqrt(n / npix * (1 - 1 / npix))).max())
        assert p["pix"].min() >= 0 and p["pix"].max() < npix
        assert abs(p["index"].mean() - m.spectral_mean) < 5 * m.spectral_width / n**0.5
        assert abs(p["index"].std() / m.spectral_width - 1) < 5 / (2 * n) ** 0.5
        assert (~p["pix_safe"]).sum() < n / 1000
        assert 0 <= p["u1"].min() and p["u1"].max() < 1 and 0 <= p["u2"].min() and p["u2"].max() < 1
    print("distribution: worst flux bin %.2f sigma, worst pixel %.2f sigma (bound 5)" % (worst_flux, worst_pix))
    assert worst_flux <= 5 and worst_pix <= 5
    # the stream shares no block with the a_lm stream and its two blocks differ
    from oracle import philox

    a = po.population_words(7, np.arange(4), 0)
    b = po.population_words(7, np.arange(4), 1)
    alm = philox.philox4x32_10(np.arange(4), 0, 0, 0, 7, 0)
    assert not np.array_equal(a[0], alm[0]) and not np.array_equal(a[0], b[0])
