"""HEALPix bilinear interpolation on the device (csrc/hpinterp.hip through cora_amd.util.hputil and
cora_amd.signal.lss) against the numpy oracle (tests/_interp_oracle.py) and the golden output of the reference's
own za_density_grid (tests/golden/zagrid_vectors.npz).

Weights are compared through ``sum_k w_k r[pix_k]`` for random maps r: the interpolant is continuous across cell
boundaries, so the comparison does not care which side of a tie (a query on a pixel centre or a ring latitude) either
side took.  Tolerance ``64 nside 2^-52 max|r|``: 16 ulp of the largest ring co-ordinate 4 nside, the rounding scale of
phi / dphi; the theta weight's error is about 10 times smaller.

64-bit indexing (nmap npix and nchi npix beyond 2^31) needs more than 16 GiB of maps and does not fit a test of a few
seconds: it is exercised by tools/bench_interp.py at nside 1024 x 256 channels.  Run with -m gpu."""
import os

import numpy as np
import pytest

import _interp_oracle as io

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NSIDES = [1, 2, 4, 16]
EPS = 2.0 ** -52


def _tol(nside, r):
    return 64 * nside * EPS * np.abs(r).max()


def _queries(nside, nrand=4000):
    """(theta, phi, nrand): random continuous directions first, then the special ones: pixel centres, ring latitudes,
    the poles, phi = 0 and just below 2 pi, 100 directions within 1e-3 of the poles."""
    from cora_amd.util import hputil

    rng = np.random.default_rng(100 + nside)
    th = [np.arccos(rng.uniform(-1, 1, nrand)), rng.uniform(0, 1e-3, 50), np.pi - rng.uniform(0, 1e-3, 50)]
    ph = [rng.uniform(0, 2 * np.pi, nrand + 100)]
    ring = io.ring_theta(nside, np.arange(1, 4 * nside))
    for t in np.r_[0.0, np.pi, ring, rng.uniform(0, np.pi, 8)]:
        for p in (0.0, np.nextafter(2 * np.pi, 0), 1.0, rng.uniform(0, 2 * np.pi)):
            th.append([t])
            ph.append([p])
    tc, pc = hputil.pix2ang(nside, np.arange(12 * nside * nside))
    return np.concatenate(th + [tc]), np.concatenate(ph + [pc]), nrand


def _maps(nside, n, seed):
    return np.random.default_rng(seed).normal(size=(n, 12 * nside * nside))


@pytest.mark.parametrize("nside", NSIDES)
def test_weights_match_oracle(ctx, nside):
    th, ph, nrand = _queries(nside)
    npix = 12 * nside * nside
    pix, w = ctx.healpix_interp_weights(nside, ctx.to_device(th), ctx.to_device(ph))
    pix, w = pix.cpu().numpy(), w.cpu().numpy()
    assert pix.shape == (4, th.size) and pix.dtype == np.int64 and w.shape == (4, th.size) and w.dtype == np.float64
    assert pix.min() >= 0 and pix.max() < npix
    rpix, rw = io.interp_weights(nside, th, ph)
    r = _maps(nside, 3, 7)
    err = np.abs((r[:, pix] * w[None]).sum(axis=1) - (r[:, rpix] * rw[None]).sum(axis=1)).max()
    same = (np.sort(pix[:, :nrand], axis=0) == np.sort(rpix[:, :nrand], axis=0)).all(axis=0).mean()
    print("nside %d: worst err / tol %.3g, same index set on %.4f of the random queries" % (nside, err / _tol(nside, r), same))
    assert err <= _tol(nside, r)
    assert same >= 0.99
    assert np.abs(w.sum(axis=0) - 1).max() <= 4 * EPS


def test_public_weights_take_healpy_shapes(ctx):
    from cora_amd.util import hputil

    nside = 4
    th = np.array([[0.3, 1.2, 2.9], [0.0, np.pi / 2, np.pi]])
    ph = np.array([[0.1, 3.0, 6.2], [1.0, 0.0, 2.0]])
    pix, w = hputil.get_interp_weights(nside, th, ph)
    assert pix.shape == (4, 2, 3) and w.shape == (4, 2, 3) and pix.dtype == np.int64
    rpix, rw = io.interp_weights(nside, th.ravel(), ph.ravel())
    r = _maps(nside, 1, 3)[0]
    assert np.abs((w * r[pix]).sum(0).ravel() - (rw * r[rpix]).sum(0)).max() <= _tol(nside, r)
    # scalars; lonlat in degrees; pixel indices for theta
    p1, w1 = hputil.get_interp_weights(nside, 1.2, 3.0)
    assert p1.shape == (4,) and np.array_equal(p1, pix[:, 0, 1]) and np.array_equal(w1, w[:, 0, 1])
    p2, w2 = hputil.get_interp_weights(nside, np.degrees(3.0), 90 - np.degrees(1.2), lonlat=True)
    assert np.abs((w2 * r[p2]).sum() - (w1 * r[p1]).sum()) <= _tol(nside, r)
    p3, w3 = hputil.get_interp_weights(nside, np.arange(12 * nside * nside))
    own = np.where(p3 == np.arange(12 * nside * nside)[None], w3, 0).sum(0)
    assert own.min() >= 1 - 64 * nside * EPS
    with pytest.raises(ValueError):
        hputil.get_interp_weights(nside, 3.5, 0.0)
    with pytest.raises(ValueError):
        hputil.get_interp_weights(nside, [12 * nside * nside])
    # get_interp_val: one map or several, scalar or array directions
    m = _maps(nside, 2, 4)
    v = hputil.get_interp_val(m, th, ph)
    assert v.shape == (2, 2, 3)
    assert np.abs(v.reshape(2, -1) - io.interp_val(m, th.ravel(), ph.ravel())).max() <= _tol(nside, m)
    assert np.array_equal(hputil.get_interp_val(m[1], th, ph), v[1])
    assert hputil.get_interp_val(m[0], 1.2, 3.0) == v[0, 0, 1]


@pytest.mark.parametrize("nside", NSIDES)
def test_interp_val_device_matches_oracle(ctx, nside):
    from cora_amd.util import hputil

    th, ph, _ = _queries(nside)
    m = _maps(nside, 5, 11)
    md = ctx.to_device(m)
    got = hputil.get_interp_val_device(md, ctx.to_device(th), ctx.to_device(ph)).cpu().numpy()
    assert got.shape == (5, th.size)
    err = np.abs(got - io.interp_val(m, th, ph)).max()
    print("nside %d: interp_val worst err / tol %.3g" % (nside, err / _tol(nside, m)))
    assert err <= _tol(nside, m)
    # pixel-centre queries return the map itself
    tc, pc = hputil.pix2ang(nside, np.arange(12 * nside * nside))
    back = hputil.get_interp_val_device(md, ctx.to_device(tc), ctx.to_device(pc)).cpu().numpy()
    assert np.abs(back - m).max() <= _tol(nside, m)
    with pytest.raises(ValueError):
        hputil.get_interp_val_device(md[:, :-1].contiguous(), ctx.to_device(tc), ctx.to_device(pc))


@pytest.mark.parametrize("nside", NSIDES)
def test_rotate_map_device(ctx, nside):
    from cora_amd.util import hputil

    m = _maps(nside, 3, 21)
    md = ctx.to_device(m)
    same = hputil.rotate_map_device(md, np.eye(3)).cpu().numpy()
    assert np.abs(same - m).max() <= _tol(nside, m)
    R = hputil.coord_matrix("G", "C")
    got = hputil.rotate_map_device(md, R).cpu().numpy()
    th, ph = io.rotated_angles(nside, R)
    err = np.abs(got - io.interp_val(m, th, ph)).max()
    print("nside %d: rotation worst err / tol %.3g" % (nside, err / _tol(nside, m)))
    assert err <= _tol(nside, m)
    assert bool((md == ctx.to_device(m)).all())                         # input untouched


def test_rotate_refuses_aliasing_and_bad_shapes(ctx):
    from cora_amd.util import hputil

    nside = 4
    npix = 12 * nside * nside
    buf = ctx.to_device(np.zeros((5, npix)))
    R = hputil.coord_matrix("C", "G")
    with pytest.raises(ValueError):
        hputil.rotate_map_device(buf[:3], R, out=buf[:3])
    with pytest.raises(ValueError):
        hputil.rotate_map_device(buf[:3], R, out=buf[2:5])
    hputil.rotate_map_device(buf[:2], R, out=buf[2:4])
    with pytest.raises(ValueError):
        hputil.rotate_map_device(buf[:2], np.eye(4), out=buf[2:4])
    with pytest.raises(ValueError):
        hputil.rotate_map_device(buf[:2], R, out=buf[2:5])
    with pytest.raises(ValueError):
        hputil.rotate_map_device(buf[:2].float(), R)
    with pytest.raises(ValueError):
        hputil.rotate_map_device(buf[:2], R, out=buf[2:4].float())
    with pytest.raises(ValueError):
        hputil.rotate_map_device(buf[:2].cpu(), R)
    th = ctx.to_device(np.array([0.3, 1.0]))
    for args in ((buf[:2], th.float(), th), (buf[:2], th.cpu(), th.cpu()), (buf[:2].t().contiguous().t(), th, th)):
        with pytest.raises(ValueError):
            hputil.get_interp_val_device(*args)


def test_coord_g2c_equals_planewise_rotation(ctx):
    from cora_amd.util import hputil

    nside = 16
    cube = np.random.default_rng(31).normal(size=(3, 4, 12 * nside * nside))
    keep = cube.copy()
    got = hputil.coord_g2c(cube)
    assert got.shape == cube.shape and got is not cube and np.array_equal(cube, keep)
    R = hputil.coord_matrix("C", "G")                 # output pixel p (celestial) samples the galactic map at R n_p
    for f in range(3):
        ref = hputil.rotate_map_device(ctx.to_device(cube[f]), R).cpu().numpy()
        assert np.array_equal(got[f], ref)
    back = hputil.coord_c2g(got)
    assert np.array_equal(back, hputil.coord_x2y(got, "C", "G"))
    with pytest.raises(Exception, match="Co-ordinate system invalid."):
        hputil.coord_x2y(cube, "G", "B")


def test_channel_chunks_give_the_same_bits(ctx):
    from cora_amd.util import hputil

    nside = 64
    npix = 12 * nside * nside
    cube = np.random.default_rng(32).normal(size=(5, npix))
    one = hputil.coord_x2y(cube, "G", "E")
    chunked = hputil.coord_x2y(cube, "G", "E", max_bytes=2 * 2 * npix * 8)      # 2 channels at a time: 3 chunks
    assert np.array_equal(one, chunked)
    assert np.array_equal(one, hputil.coord_x2y(cube, "G", "E", max_bytes=1))   # never less than one map


# ---- the grid form of the Zel'dovich step --------------------------------------------------------
@pytest.fixture(scope="module")
def zg():
    g = dict(np.load(os.path.join(ROOT, "tests", "golden", "zagrid_vectors.npz")))
    g["psi"] = g["psi_q"].astype(np.float64) * np.array([g["q_r"], g["q_a"], g["q_a"]])[:, None, None]
    g["delta_bias"] = g["delta_bias_q"].astype(np.float64) * g["q_a"]
    g["delta_m"] = g["delta_m_q"].astype(np.float64) * g["q_a"]
    return g


def _grid_dev(ctx, psi, db, dm, chi, out):
    from cora_amd.signal import lss

    t = [ctx.to_device(a) for a in (psi, db, dm, chi, out)]
    res = lss.za_density_grid_device(*t)
    assert res is t[4]
    return res.cpu().numpy()


def test_grid_matches_golden(ctx, zg):
    from cora_amd.signal import lss

    ref = zg["out"]
    bound = 1e-12 * np.abs(ref + 1).max()
    out = np.full(zg["delta_bias"].shape, float(zg["out0"]))
    got = lss.za_density_grid(zg["psi"], zg["delta_bias"], zg["delta_m"], zg["chi"], out)
    assert got is out
    err = np.abs(out - ref).max()
    print("za_density_grid vs golden: err / bound %.3g" % (err / bound))
    assert err <= bound
    # out pre-filled with 0.25 gains exactly that offset: the same run from zeros differs by it
    zero = _grid_dev(ctx, zg["psi"], zg["delta_bias"], zg["delta_m"], zg["chi"], np.zeros(ref.shape))
    assert np.abs((out - zero) - float(zg["out0"])).max() <= bound
    # poisoned scratch: delta_m is not read
    nan = _grid_dev(ctx, zg["psi"], zg["delta_bias"], np.full(ref.shape, np.nan), zg["chi"], np.zeros(ref.shape))
    assert np.isfinite(nan).all() and np.abs(nan - zero).max() <= bound
    # a second call: the same to rounding (float atomics)
    again = _grid_dev(ctx, zg["psi"], zg["delta_bias"], zg["delta_m"], zg["chi"], np.zeros(ref.shape))
    assert np.abs(again - zero).max() <= 1e-13 * np.abs(ref + 1).max()


@pytest.mark.parametrize("nside,nchi", [(1, 2), (2, 3), (4, 5), (16, 7)])
def test_grid_properties_and_oracle(ctx, nside, nchi):
    rng = np.random.default_rng(200 + nside)
    npix = 12 * nside * nside
    res = np.sqrt(4 * np.pi / npix)
    chi = 800.0 + 8.0 * np.arange(nchi) + rng.uniform(-1.0, 1.0, nchi)
    db = rng.normal(0, 0.4, (nchi, npix))
    dm = rng.normal(0, 0.8, (nchi, npix))
    # nothing moves: every particle sits on its own pixel centre and on chi[ii]
    got = _grid_dev(ctx, np.zeros((3, nchi, npix)), db, dm, chi, np.zeros((nchi, npix)))
    assert np.abs(got - db).max() <= 64 * nside * EPS * np.abs(1 + db).max()
    # angular displacements only (across the poles and phi = 0 at these sizes): mass is conserved
    psi = np.stack([np.zeros((nchi, npix)), rng.normal(0, 2 * res, (nchi, npix)), rng.normal(0, 4 * res, (nchi, npix))])
    got = _grid_dev(ctx, psi, db, dm, chi, np.zeros((nchi, npix)))
    mass = (1 + db).sum()
    assert abs((got + 1).sum() - mass) <= 1e-12 * mass
    # radial displacements too, some beyond both ends: against the oracle
    psi[0] = rng.normal(0, 5.0, (nchi, npix))
    psi[0, 0, ::3] -= 12.0
    psi[0, -1, ::3] += 12.0
    ref = io.za_density_grid(psi, db, dm, chi, np.zeros((nchi, npix)))
    got = _grid_dev(ctx, psi, db, dm, chi, np.zeros((nchi, npix)))
    # a particle within rounding of a cell boundary may take the other cell: the scatter is continuous there too
    err = np.abs(got - ref).max() / np.abs(ref + 1).max()
    print("nside %d nchi %d: za_density_grid vs oracle %.3g" % (nside, nchi, err))
    assert err <= 64 * nside * EPS + 1e-12


def test_grid_bad_arguments_raise(ctx):
    from cora_amd import _lib
    from cora_amd.signal import lss

    nside, nchi = 4, 4
    npix = 12 * nside * nside
    psi, db, dm, out = (ctx.to_device(np.zeros(s)) for s in ((3, nchi, npix), (nchi, npix), (nchi, npix), (nchi, npix)))
    chi = ctx.to_device(np.arange(nchi) + 1.0)
    lss.za_density_grid_device(psi, db, dm, chi, out)
    for bad in (ctx.to_device(np.arange(nchi, 0.0, -1.0)), ctx.to_device(np.array([1.0, 2.0, 2.0, 3.0]))):
        with pytest.raises(ValueError):
            lss.za_density_grid_device(psi, db, dm, bad, out)
    with pytest.raises(ValueError):
        lss.za_density_grid_device(psi[:, :1], db[:1], dm[:1], chi[:1], out[:1])
    with pytest.raises(ValueError):
        lss.za_density_grid_device(psi[:2], db, dm, chi, out)
    with pytest.raises(ValueError):
        lss.za_density_grid_device(psi, db, dm[:, :-1], chi, out)
    # the kernels read raw float64 memory: another dtype, a strided view or a host tensor is a ValueError, not an assert
    import torch

    for bad in (dict(psi=psi.float()), dict(db=db.t().contiguous().t()), dict(out=out.cpu()), dict(chi=chi.float())):
        a = dict(psi=psi, db=db, dm=dm, chi=chi, out=out)
        a.update(bad)
        with pytest.raises(ValueError):
            lss.za_density_grid_device(a["psi"], a["db"], a["dm"], a["chi"], a["out"])
    # below the Python layer the C ABI refuses nchi < 2 itself
    with pytest.raises(_lib.CoraHipError):
        ctx.za_density_grid(psi[:, :1].contiguous(), db[:1].contiguous(), chi[:1].contiguous(), out[:1].contiguous())
    assert _lib.load().corahip_abi_minor() >= 9


def test_zeldovich_density_sph_switch(ctx):
    from cora_amd.signal import lss

    nside, nchi, lmax = 16, 4, 32
    npix = 12 * nside * nside
    rng = np.random.default_rng(61)
    phi = ctx.to_device(rng.normal(0, 0.05, (nchi, npix)))
    chi = 800.0 + 8.0 * np.arange(nchi) + rng.uniform(-1.0, 1.0, nchi)
    D = rng.uniform(0.5, 0.9, nchi)
    f = rng.uniform(0.7, 1.0, nchi)
    delta = ctx.to_device(rng.normal(0, 0.8, (nchi, npix)))
    db = ctx.to_device(rng.normal(0, 0.4, (nchi, npix)))
    psi = lss.zeldovich_displacement_device(phi, chi, D, f, lmax=lmax)
    dm = delta * ctx.to_device(D)[:, None]
    chid = ctx.to_device(chi)
    grid = lss.zeldovich_density_device(phi, delta, db, chi, D, f, lmax=lmax, sph=False).cpu().numpy()
    ref = lss.za_density_grid_device(psi, db, dm, chid, ctx.to_device(np.zeros((nchi, npix)))).cpu().numpy()
    assert np.abs(grid - ref).max() <= 1e-12 * np.abs(ref + 1).max()
    # sph=True and the default are what the function gave before: displacement, then the SPH step (float atomics:
    # to rounding)
    sph_ref = lss.za_density_sph_device(psi, db, dm, chid, ctx.to_device(np.zeros((nchi, npix)))).cpu().numpy()
    for kw in ({}, {"sph": True}):
        got = lss.zeldovich_density_device(phi, delta, db, chi, D, f, lmax=lmax, **kw).cpu().numpy()
        assert np.abs(got - sph_ref).max() <= 1e-12 * np.abs(sph_ref + 1).max()
    assert np.abs(grid - sph_ref).max() > 1e-3                            # the two forms are different assignments
    # numpy in, numpy out, and through the chain
    gh = lss.zeldovich_density(phi.cpu().numpy(), delta.cpu().numpy(), db.cpu().numpy(), chi, D, f, lmax=lmax, sph=False)
    assert np.abs(gh - grid).max() <= 1e-12 * np.abs(grid + 1).max()
    kw = dict(b1=1.3, lmax=lmax, polarisation=False)
    m_grid = lss.tracer_map_device(phi, delta, chi, D, f, sph=False, **kw).cpu().numpy()
    m_sph = lss.tracer_map_device(phi, delta, chi, D, f, **kw).cpu().numpy()
    bias = lss.biased_field_device(delta, D, 1.3)
    want = lss.zeldovich_density_device(phi, delta, bias, chi, D, f, lmax=lmax, sph=False).cpu().numpy()
    assert m_grid.shape == (nchi, 1, npix) and np.abs(m_grid[:, 0] - want).max() <= 1e-12 * np.abs(want + 1).max()
    assert np.abs(m_grid - m_sph).max() > 1e-3
