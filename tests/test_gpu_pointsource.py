"""The point-source kernels (csrc/pointsource.hip) on the GPU against the oracles of tests/_pointsource_oracle.py, whose
module docstring derives every tolerance used here (eps = 2^-52, u = eps / 2; none is tuned), and against the
reference's own outputs (tests/golden/pointsource_vectors.npz).  tests/test_pointsource_host.py pins the oracles to the
reference first.  Every test prints its worst error over tolerance."""
import functools
import os

import numpy as np
import pytest

import _pointsource_oracle as po

pytestmark = pytest.mark.gpu

EPS, U, LD = po.EPS, po.U, po.LD
TINY = np.finfo(np.float64).tiny


def _worst(err, tol):
    return float(np.max(np.asarray(err, dtype=np.float64) / np.maximum(tol, TINY))) if np.size(err) else 0.0


@pytest.fixture(scope="module")
def cases():
    return po.load_golden()


# ---- paint -------------------------------------------------------------------------------------------------------------

PAINT_SHAPES = {
    "empty": (0, 3, 1), "single": (1, 1, 1), "wave+1": (65, 3, 2), "block+1": (257, 17, 4), "one_pixel": (1000, 130, 4),
    "one_each": (3072, 16, 16), "random": (5000, 130, 8), "cat": (26, 5, 4), "cat_pol": (26, 5, 4),
}


@functools.lru_cache(maxsize=None)
def _paint_case(name):
    """Inputs (sorted by pixel), the long-double oracle and its tolerance: computed once per case."""
    N, F, nside = PAINT_SHAPES[name]
    npix = 12 * nside * nside
    rng = np.random.default_rng(sorted(PAINT_SHAPES).index(name) + 100)
    freq = np.linspace(400.0, 800.0, F) if F > 1 else np.array([612.5])
    gamma = polw = None
    pivot = 151.0
    if name.startswith("cat"):
        from cora_amd.util import hputil

        c = po.load_golden()["cat"]
        freq, pivot = c["freq"], 600.0
        pix = hputil.ang2pix(nside, np.pi / 2.0 - np.radians(c["DEC"]), np.radians(c["RA"]))
        flux, beta, gamma, polw = po.catalogue_inputs(c, pix)
        if name == "cat":
            polw = None
    else:
        flux = np.exp(rng.uniform(np.log(0.1), np.log(10.0), N))
        beta = -0.7 + 0.1 * rng.normal(size=N)
        pix = rng.integers(0, npix, N)
        if name == "one_pixel":
            pix[:] = 77
        elif name == "one_each":
            pix = rng.permutation(npix)
        elif name == "random":
            pix[0], pix[1] = 0, npix - 1
            flux[10:40] = 0.0                                                    # zero-flux sources
            pix[100:140] = 301
            flux[100:140] = np.exp(np.linspace(np.log(1e-4), np.log(1e4), 40))   # eight decades in one pixel
            polw = 0.1 * rng.normal(size=(N, 2))
        elif name == "block+1":
            gamma = 0.05 * rng.normal(size=N)
    order = np.argsort(pix, kind="stable")
    pix, flux, beta = pix[order].astype(np.int64), flux[order], beta[order]
    gamma = None if gamma is None else gamma[order]
    polw = None if polw is None else np.ascontiguousarray(polw[order])
    den, c2 = po.conversion(freq, nside)
    x = np.log(freq / pivot)
    npol = 4 if polw is not None else 1
    ref, tol = po.paint(pix, flux, beta, gamma, polw, x, den, c2, npix, npol=npol)
    for a in (pix, flux, beta, x, den, ref, tol):
        a.setflags(write=False)
    return dict(pix=pix, flux=flux, beta=beta, gamma=gamma, polw=polw, x=x, den=den, c2=c2, npix=npix, npol=npol, ref=ref,
                tol=tol, F=len(freq))


@pytest.mark.parametrize("name", list(PAINT_SHAPES))
def test_paint_against_longdouble_oracle(ctx, name):
    """Overwrite mode onto NaN, inputs unchanged, a second call and a channel subset bit-identical, accumulate mode
    onto a random base: all under the paint bound of the oracle's docstring."""
    import torch

    c = _paint_case(name)
    F, npix, npol = c["F"], c["npix"], c["npol"]
    dev = {k: None if c[k] is None else ctx.to_device(c[k], dtype=np.int64 if k == "pix" else np.float64)
           for k in ("pix", "flux", "beta", "gamma", "polw")}
    keep = {k: None if v is None else v.clone() for k, v in dev.items()}
    shape = (F, npix) if npol == 1 else (F, 4, npix)

    def run(x, den, out=None, accumulate=False):
        return ctx.pointsource_paint(dev["pix"], dev["flux"], dev["beta"], x, den, c["c2"], npix, gamma=dev["gamma"],
                                     polw=dev["polw"], npol=npol, out=out, accumulate=accumulate)

    out = run(c["x"], c["den"], out=torch.full(shape, float("nan"), dtype=torch.float64, device=ctx.device))
    got = out.cpu().numpy()
    assert np.all(np.isfinite(got))
    r = _worst(np.abs(got - c["ref"]), c["tol"])
    empty = np.bincount(c["pix"], minlength=npix) == 0
    assert not got[..., empty].any()
    if npol == 4:
        assert not got[:, 3].any()
    for k, v in dev.items():
        assert v is None or torch.equal(v, keep[k])
    assert torch.equal(run(c["x"], c["den"]), out)
    sub = np.arange(F)[::3] if F > 2 else np.arange(F)[-1:]
    part = run(c["x"][sub], c["den"][sub])
    assert torch.equal(part, out[torch.as_tensor(sub, device=ctx.device)])
    # accumulate: occupied pixels get base + sum, everything else keeps its bits
    base = np.random.default_rng(5).normal(size=shape) * (np.abs(c["ref"]).astype(np.float64).max() + 1.0)
    acc = run(c["x"], c["den"], out=ctx.to_device(base), accumulate=True).cpu().numpy()
    want = base.astype(LD)
    if npol == 1:
        want[:, ~empty] += c["ref"][:, ~empty]
    else:
        want[:, :3][:, :, ~empty] += c["ref"][:, :3][:, :, ~empty]
    # the sum carries tol; the one rounding of the addition is at most u of the computed result, itself within tol of
    # `want`, whose own long-double rounding is 2^-11 u: nothing to spare is needed beyond that
    ra = _worst(np.abs(acc - want), c["tol"] + U * (np.abs(want).astype(np.float64) + c["tol"]) * (1 + 2.0**-11))
    assert np.array_equal(acc[..., empty], base[..., empty])
    if npol == 4:
        assert np.array_equal(acc[:, 3], base[:, 3])
    print("paint %s (N, F, nside) = %r: worst err / tol  overwrite %.3g  accumulate %.3g; most sources in a pixel %d"
          % (name, PAINT_SHAPES[name], r, ra, np.bincount(c["pix"], minlength=1).max() if len(c["pix"]) else 0))
    assert r <= 1 and ra <= 1


def test_paint_sorts_and_refuses_bad_pixels(ctx):
    """``paint_sources_device`` sorts by pixel itself (stable) and takes host arrays; a pixel out of range is an error."""
    from cora_amd.foreground import pointsource

    c = _paint_case("wave+1")
    perm = np.random.default_rng(1).permutation(len(c["pix"]))
    freq = 151.0 * np.exp(c["x"])
    got = pointsource.paint_sources_device(c["pix"][perm], c["flux"][perm], c["beta"][perm], freq, 151.0, 2).cpu().numpy()
    den = po.conversion(freq, 2)[0]
    ref, tol = po.paint(c["pix"], c["flux"], c["beta"], None, None, np.log(freq / 151.0), den, c["c2"], 48)
    r = _worst(np.abs(got - ref), tol)
    print("paint_sources_device on permuted sources: worst err / tol %.3g" % r)
    assert r <= 1
    with pytest.raises(ValueError):
        pointsource.paint_sources_device(np.array([48]), np.ones(1), np.ones(1), freq, 151.0, 2)


@pytest.mark.parametrize("name", ["dm4", "dm8", "pl4", "pl8"])
def test_paint_and_rotate_against_reference_models(ctx, cases, name):
    """The reference's ``getpolsky`` from its recorded population: plane 0 under the paint bound, planes 1, 2 under the
    rotation bound with the paint bound carried through the rotation; plane 0 of the cube is the painted map's bits."""
    from cora_amd.foreground import pointsource

    c = cases[name]
    nside = int(c["nside"])
    x, den, c2, npix = po.power_law_inputs(c)
    sky = pointsource.paint_sources_device(c["pix"], c["flux"], c["index"], c["freq"], c["spectral_pivot"], nside)
    order = np.argsort(c["pix"], kind="stable")
    _, tol = po.paint(c["pix"][order], c["flux"][order], c["index"][order], None, None, x, den, c2, npix)
    ref = c["sky_pol"]
    got = sky.cpu().numpy()
    r0 = _worst(np.abs(got - ref[:, 0]), tol)
    cube = ctx.polarise_rotate(sky, c["q_frac"], c["u_frac"], wv=po.wavelengths(c["freq"]), rm=c["rm"]).cpu().numpy()
    _, _, rtol = po.rotate(ref[:, 0] * c["q_frac"][None, :], ref[:, 0] * c["u_frac"][None, :], po.wavelengths(c["freq"]), c["rm"])
    carried = tol * np.hypot(c["q_frac"], c["u_frac"])[None, :] * 2**0.5
    r1 = _worst(np.abs(cube[:, 1] - ref[:, 1]), rtol + carried)
    r2 = _worst(np.abs(cube[:, 2] - ref[:, 2]), rtol + carried)
    print("%s: worst err / tol against the reference  sky %.3g  Q %.3g  U %.3g" % (name, r0, r1, r2))
    assert r0 <= 1 and r1 <= 1 and r2 <= 1
    assert np.array_equal(cube[:, 0], got) and not cube[:, 3].any()


@pytest.mark.parametrize("faraday", [False, True])
def test_real_sources_against_reference_cube(ctx, cases, faraday):
    from cora_amd.foreground import pointsource
    from cora_amd.util import hputil

    c = cases["cat"]
    cat = np.zeros(len(c["RA"]), dtype=[(k, "f8") for k in pointsource.CATALOGUE_FIELDS])
    for k in pointsource.CATALOGUE_FIELDS:
        cat[k] = c[k]
    real = pointsource.RealPointSources(catalogue=cat, faraday_map=c["rm"])
    real.nside, real.frequencies, real.flux_min, real.faraday = int(c["nside"]), c["freq"], c["flux_min"], faraday
    got = real.getpolsky()
    nside = int(c["nside"])
    pix = hputil.ang2pix(nside, np.pi / 2.0 - np.radians(c["DEC"]), np.radians(c["RA"]))
    flux, beta, gamma, polw = po.catalogue_inputs(c, pix)
    order = np.argsort(pix, kind="stable")
    den, c2 = po.conversion(c["freq"], nside)
    _, tol = po.paint(pix[order], flux[order], beta[order], gamma[order], polw[order], np.log(c["freq"] / 600.0), den, c2,
                      12 * nside * nside, npol=4)
    ref = c["cube_rot"] if faraday else c["cube"]
    t1, t2 = tol[:, 1], tol[:, 2]
    if faraday:
        _, _, rtol = po.rotate(c["cube"][:, 1], c["cube"][:, 2], po.wavelengths(c["freq"]), c["rm"])
        t1 = t2 = rtol + tol[:, 1] + tol[:, 2]
    r = [_worst(np.abs(got[:, 0] - ref[:, 0]), tol[:, 0]), _worst(np.abs(got[:, 1] - ref[:, 1]), t1),
         _worst(np.abs(got[:, 2] - ref[:, 2]), t2)]
    print("catalogue cube, faraday %s: worst err / tol  I %.3g  Q %.3g  U %.3g" % (faraday, *r))
    assert got.shape == (len(c["freq"]), 4, 12 * nside * nside) and max(r) <= 1 and not got[:, 3].any()
    assert np.array_equal(real.getsky(), got[:, 0])


# ---- population --------------------------------------------------------------------------------------------------------

POP_SEED = {1: 2**40 + 17, 63: 5, 4097: 6, 100003: 7}


@functools.lru_cache(maxsize=None)
def _spline():
    from cora_amd.foreground import pointsource, poisson

    m = pointsource.DiMatteo()
    m.flux_min, m.flux_max = 1e-3, 50.0
    data, y2 = poisson.inverse_cdf(np.log(m.flux_max / m.flux_min), m._log_rate(4 * np.pi)).data()
    return m, data[:, 0].copy(), data[:, 1].copy(), y2.copy()


@pytest.mark.parametrize("n", [1, 63, 4097, 100003])
def test_population_against_oracle(ctx, n):
    """Interval index exact; spline value within 8 eps sum |terms|; flux within (|t| + 3) eps relative on top; index
    under the package's Box-Muller bound; pixel exact wherever u2 npix is further than npix eps from an integer (fewer
    than 1 in 1000 sources are not, by the oracle alone)."""
    m, xs, ys, y2 = _spline()
    npix = 12 * 16 * 16
    seed = POP_SEED[n]
    o = po.population(seed, n, xs, ys, y2, m.flux_min, m.spectral_mean, m.spectral_width, npix, dtype=LD)
    pix, flux, index, iv, t = ctx.pointsource_population(seed, n, xs, ys, y2, m.flux_min, m.spectral_mean, m.spectral_width,
                                                         npix, interval=True)
    pix, flux, index, iv, t = (v.cpu().numpy() for v in (pix, flux, index, iv, t))
    assert np.array_equal(iv, o["interval"])
    ttol = 8 * EPS * o["tabs"]
    ftol = (ttol + (np.abs(o["t"]).astype(np.float64) + 3) * EPS) * np.abs(o["flux"]).astype(np.float64)
    rf = _worst(np.abs(flux - o["flux"]), ftol)
    rt = _worst(np.abs(t - o["t"]), ttol)               # the spline value itself, from the kernel's test hook
    assert np.array_equal(flux, m.flux_min * np.exp(t)) or _worst(np.abs(flux - m.flux_min * np.exp(t)), 2 * EPS * flux) <= 1
    itol = abs(m.spectral_width) * 4e-15 * np.maximum(1.0, np.abs(o["z"])) + U * (np.abs(m.spectral_width * o["z"]) + np.abs(index))
    ri = _worst(np.abs(index - o["index"]), itol)
    safe = o["pix_safe"]
    assert (~safe).sum() < max(n / 1000, 1) and np.array_equal(pix[safe], o["pix"][safe])
    assert pix.min() >= 0 and pix.max() < npix
    print("population n = %d: worst err / tol  flux %.3g  spline %.3g  index %.3g; %d pixels left out"
          % (n, rf, rt, ri, (~safe).sum()))
    assert rf <= 1 and rt <= 1 and ri <= 1
    # a second call gives the same bits
    again = ctx.pointsource_population(seed, n, xs, ys, y2, m.flux_min, m.spectral_mean, m.spectral_width, npix)
    assert np.array_equal(again[1].cpu().numpy(), flux) and np.array_equal(again[0].cpu().numpy(), pix)


# ---- rotation ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("F", [1, 3, 130])
@pytest.mark.parametrize("npix", [12, 48, 3072])
def test_polarise_and_faraday_rotate(ctx, npix, F):
    import torch

    from cora_amd.foreground import pointsource

    rng = np.random.default_rng(npix * 1000 + F)
    freq = np.linspace(400.0, 800.0, F) if F > 1 else np.array([400.0])
    wv = po.wavelengths(freq)
    sky = rng.uniform(0.5, 30.0, (F, npix))
    q, u = 0.03 * rng.normal(size=npix), 0.03 * rng.normal(size=npix)
    rm = rng.uniform(-1.0, 1.0, npix) * 4000.0 / (2 * wv.max())
    rm[0] = 4000.0 / (2 * wv.max())                         # |a| = 4000 at the longest wavelength
    skyd = ctx.to_device(sky)
    flat = ctx.polarise_rotate(skyd, q, u, wv=wv, rm=np.zeros(npix)).cpu().numpy()
    assert np.array_equal(flat[:, 0], sky) and not flat[:, 3].any()
    assert np.array_equal(flat[:, 1], sky * q[None, :]) and np.array_equal(flat[:, 2], sky * u[None, :])
    assert np.array_equal(ctx.polarise_rotate(skyd, q, u).cpu().numpy(), flat)
    got = ctx.polarise_rotate(skyd, q, u, wv=wv, rm=rm)
    rq, ru, tol = po.rotate(sky * q[None, :], sky * u[None, :], wv, rm)
    g = got.cpu().numpy()
    r = max(_worst(np.abs(g[:, 1] - rq), tol), _worst(np.abs(g[:, 2] - ru), tol))
    assert np.array_equal(g[:, 0], sky) and not g[:, 3].any() and torch.equal(skyd, ctx.to_device(sky))
    # in place on a cube equals out of place; a numpy cube is rotated in place too and returned
    cube = ctx.to_device(flat)
    assert pointsource.faraday_rotate(cube, rm, freq) is cube and torch.equal(cube, got)
    host = flat.copy()
    host[:, 3] = 7.0
    assert pointsource.faraday_rotate(host, rm, freq) is host
    assert np.array_equal(host[:, 1:3], g[:, 1:3]) and np.array_equal(host[:, 0], sky) and np.all(host[:, 3] == 7.0)
    print("rotate npix %d F %d: worst err / tol %.3g (largest |a| %.0f)" % (npix, F, r, np.abs(2 * wv[:, None] * rm[None, :]).max()))
    assert r <= 1


# ---- ud_grade ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nin,nout", [(1, 8), (8, 1), (4, 4), (16, 2)])
def test_ud_grade(ctx, nin, nout):
    import torch

    from cora_amd.util import hputil

    maps = np.random.default_rng(nin * 100 + nout).normal(size=(3, 12 * nin * nin))
    want = po.ud_grade(maps, nout)
    got = hputil.ud_grade(maps, nout)
    assert isinstance(got, np.ndarray) and got.shape == (3, 12 * nout * nout)
    if nout >= nin:
        assert np.array_equal(got, want)
        r = 0.0
    else:
        m = (nin // nout) ** 2
        bound = (m - 1) * U * po.ud_grade(np.abs(maps), nout)
        r = _worst(np.abs(got - po.ud_grade(maps, nout, dtype=LD)), bound)
    dev = hputil.ud_grade(ctx.to_device(maps), nout)
    assert isinstance(dev, torch.Tensor) and dev.device == ctx.device and np.array_equal(dev.cpu().numpy(), got)
    one = hputil.ud_grade(maps[1], nout)
    assert one.shape == (12 * nout * nout,) and np.array_equal(one, got[1])
    if nout > nin:                                         # up then down: the identity, bit for bit
        assert np.array_equal(hputil.ud_grade(got, nin), maps)
    print("ud_grade %d -> %d: worst err / tol %.3g" % (nin, nout, r))
    assert r <= 1


# ---- end to end --------------------------------------------------------------------------------------------------------

def test_dimatteo_getsky_equals_the_oracle_population_painted_by_the_oracle(ctx):
    """``DiMatteo.getsky(rng=DeviceRNG(seed))`` at nside 8: the oracle generates the population of that seed (count
    from the same Poisson draw), sorts it and paints it in long double; the map agrees under the paint bound with the
    population's own bounds (flux, index) carried into every term."""
    import cora_amd
    from cora_amd.foreground import pointsource, poisson

    m = pointsource.DiMatteo()
    m.nside, m.frequencies, m.flux_min, m.flux_max = 8, np.array([400.0, 520.0, 640.0, 800.0]), 1.0, 300.0
    seed = 20261018
    got = m.getsky(rng=cora_amd.DeviceRNG(seed))
    t = np.log(m.flux_max / m.flux_min)
    rate = m._log_rate(4 * np.pi)
    total = int(np.random.default_rng([seed, po.DOMAIN]).poisson(poisson.expected_events(t, rate)))
    data, y2 = poisson.inverse_cdf(t, rate).data()
    o = po.population(seed, total, data[:, 0], data[:, 1], y2, m.flux_min, m.spectral_mean, m.spectral_width, 768, dtype=LD)
    assert o["pix_safe"].all()
    order = np.argsort(o["pix"], kind="stable")
    rel = 8 * EPS * o["tabs"] + (np.abs(o["t"]).astype(np.float64) + 3) * EPS
    relx = abs(m.spectral_width) * 4e-15 * np.maximum(1.0, np.abs(o["z"])) + EPS * (np.abs(m.spectral_width * o["z"]) + 1.0)
    den, c2 = po.conversion(m.frequencies, 8)
    ref, tol = po.paint(o["pix"][order], o["flux"][order], o["index"][order], None, None, np.log(m.frequencies / 151.0), den,
                        c2, 768, rel=rel[order], relx=relx[order])
    r = _worst(np.abs(got - ref), tol)
    print("DiMatteo.getsky, %d sources at nside 8 (at most %d in a pixel): worst err / tol %.3g"
          % (total, np.bincount(o["pix"]).max(), r))
    assert got.shape == (4, 768) and r <= 1
    assert np.array_equal(m.getsky(rng=cora_amd.DeviceRNG(seed)), got)
    # population_device is the same population
    pix, flux, index = pointsource.population_device(m, 4 * np.pi, seed)
    assert len(pix) == total and np.array_equal(pix.cpu().numpy(), o["pix"])


def test_combined_point_sources_and_command(ctx, cases, tmp_path):
    """``CombinedPointSources.getpolsky`` with the golden catalogue rows and a coarse rotation-measure map: shape, plane
    3 zero, Stokes I above the Gaussian background where the brightest source sits; without the map a sentence says what
    to pass; ``cora-makesky pointsource`` writes a map."""
    from click.testing import CliRunner

    from cora_amd.foreground import pointsource
    from cora_amd.scripts import makesky
    from cora_amd.util import hputil

    c = cases["cat"]
    cat = np.zeros(len(c["RA"]), dtype=[(k, "f8") for k in pointsource.CATALOGUE_FIELDS])
    for k in pointsource.CATALOGUE_FIELDS:
        cat[k] = c[k]
    rm = np.random.default_rng(2).uniform(-100.0, 100.0, 12 * 4 * 4)
    ps = pointsource.CombinedPointSources(catalogue=cat, faraday_map=rm)
    ps.nside, ps.frequencies = 8, np.array([400.0, 600.0, 800.0])
    cube = ps.getpolsky(rng=np.random.default_rng(5))
    assert cube.shape == (3, 4, 768) and np.all(np.isfinite(cube)) and not cube[:, 3].any()
    bright = hputil.ang2pix(8, np.pi / 2.0 - np.radians(c["DEC"][0]), np.radians(c["RA"][0]))
    assert cube[1, 0, bright] == cube[1, 0].max() and cube[:, 1].any() and cube[:, 2].any()
    sky = ps.getsky(rng=np.random.default_rng(5))
    assert sky.shape == (3, 768) and sky[1, bright] == sky[1].max()
    with pytest.raises(ValueError, match="faraday_map="):
        pointsource.CombinedPointSources.like_map(ps, catalogue=cat).getpolsky()
    out = str(tmp_path / "ps.h5")
    r = CliRunner().invoke(makesky.cli, ["pointsource", "--nside", "8", "--freq", "400", "800", "2", "--freq-mode", "edge",
                                         "--pol", "none", "--seed", "1", "--filename", out])
    assert r.exit_code == 0, r.output
    f = np.load(out if os.path.exists(out) else out + ".npz")
    assert f["map"].shape == (2, 1, 768) and np.all(np.isfinite(f["map"])) and f["map"].max() > 0
