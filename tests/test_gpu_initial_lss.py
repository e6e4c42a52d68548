"""The joint xi(r) -> C_l kernels (``corahip_xi_multi_average``, ``corahip_cl_blocks`` of cora_amd/csrc/corrfunc.hip) and
the initial-LSS step built on them (``signal.lss.multifrequency_aps_device``, ``generate_initial_lss_device``), held to
the derived bounds of tests/_corrfunc_oracle.py function by function: ``xi_table_average`` with that function's f_t,
``legendre_project`` with the xi bound passed on; the gate is err / bound <= 1 and no constant is fitted to device
output.  Every output tensor handed to a kernel is filled with the 0xFF byte pattern first.  Run with -m gpu.

Each test prints its worst err / bound.  Observed on the MI355X:

  spline point sets through the multi kernel, worst over the three slots     kind 0   kind 1   kind 2
    nk4 / uniform64                                                           0.306    0.332    0.377  /  0.281  0.348  0.415
    log300 / mirror300                                                        0.425    0.364    0.392  /  0.314  0.379  0.404
    close / plateau                                                           0.262    0.334    0.371  /  0.250  0.436  0.331
    kinked (kind 0) / zero end-slope (kind 1; slot 1 is ys - 1)               0.224    0.161
    max, 2925 knots                                                           0.378    0.361    0.432
    max, 2926 knots (one more than the LDS kernel takes)                      0.396    0.369    0.436
    max, 6002 knots                                                           0.416    0.357    0.415
    max, 40 000 knots (63 106 points, thinned by 16)                          0.401    0.368    0.437
  pair decode and bin average (kind 2), F x xint x nm      1x1x3 0.146, 1x9x3 0.067, 5x3x3 0.160, 17x2x3 0.299, 257x1x17 0.407
  projection and assembly (L 48, F 5, 188 nodes in 192 rows)                  0.011
  65 536 knots                                                                0.435
  6002 knots end to end, delta delta / phi delta / phi phi                    0.035 / 0.024 / 0.032
  the draw, seed 1: z(delta^2) 0.48 -0.61 -1.15 -0.58, z(phi delta) 0.00 0.39 0.04 -1.46 (cap 5); the phi delta
    expectation lies 11.0 .. 13.7 sigma from zero
  indefinite blocks: smallest eigenvalue of the unit-diagonal block -8.9e-09 .. -4.2e-13, negative at 48 of 48 l
  numpy forms with frequencies= and the default cosmology: the bits of the device forms

The 40 000-knot point sets take 4 / 7 / 12 s (kinds 0 / 1 / 2), nearly all of it the longdouble oracle on the host;
every other case runs in under 3 s.
"""
import numpy as np
import pytest

import _corrfunc_oracle as co
import _initial_lss_oracle as io

pytestmark = pytest.mark.gpu

KINDS = (0, 1, 2)
CHUNK = 96                       # separations per call of the point-set tests (F = CHUNK + 1)
MU2 = np.array([1.0, 0.25])      # mu = 1: |r_i - r_j| exactly; 0.25: general separations
F_T2 = 3.0e-3                    # the other f_t of slot 2


def _poisoned(ctx, shape):
    import torch

    t = ctx.empty(shape)
    t.view(torch.uint8).fill_(0xFF)            # every double a NaN: an element the kernel does not write shows
    return t


def _multi(ctx, kind, xs, ky, ky2, f_t, mu, xa, xw, F, xint, nm_rows=None):
    """-> packed [nm_rows, nfun, F (F + 1) / 2] on the host."""
    import torch

    rows = len(mu) if nm_rows is None else nm_rows
    out = _poisoned(ctx, (rows, ky.shape[0], F * (F + 1) // 2))
    d = ctx.to_device
    ctx.xi_multi_average(d(xs), d(ky), d(ky2), kind, co.X_T, f_t, d(mu), d(xa), d(xw), F, xint, nm_rows=rows, out=out)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


@pytest.mark.parametrize("nk", (2925, 2926, 6002, 40000))
@pytest.mark.parametrize("kind", KINDS)
def test_multi_spline_point_sets(ctx, kind, nk):
    """The point sets of test_gpu_corrfunc.py::test_spline_point_sets (xint = 1, xa[0] = 0, chunks of 96) through the
    multi kernel with three slots: the table, its negative (kind 1: ys - 1), the table with another f_t.  nk = 2925 runs
    every layout of ``spline_cases`` (its largest table has 2925 knots, the most the LDS kernel takes); the larger nk run
    the table of that many knots, which only this kernel takes.  Points of the large tables are thinned by 16."""
    cases = [c for c in co.spline_cases(kind, nk) if nk == 2925 or c[0] == "max"]
    for name, xs, ys, y2, r in cases:
        ky, ky2, f_t = io.multi_tables(kind, xs, ys, y2, F_T2)
        f_eq = np.full(3, co.F_T)
        worst, pts = 0.0, r[1:]
        starts = list(range(0, pts.size, CHUNK))
        for c0 in starts:
            xa = np.concatenate([[0.0], pts[c0:c0 + CHUNK]])
            F = xa.size
            got = _multi(ctx, kind, xs, ky, ky2, f_t, MU2, xa, np.ones(1), F, 1)
            if kind == 2:
                val, bound = io.xi_multi_reference(kind, xs, ky, ky2, co.X_T, f_t, MU2, xa, np.ones(1), F, 1)
                if c0 in (starts[0], starts[-1]):       # equal f_t: slots 0 and 2 are the same function
                    eq = _multi(ctx, kind, xs, ky, ky2, f_eq, MU2, xa, np.ones(1), F, 1)
                    assert _same_bits(eq[:, 0], eq[:, 2]) and _same_bits(eq[:, :2], got[:, :2]), (kind, name, c0)
            else:
                # f_t does not enter kinds 0 and 1: slot 2 is slot 0, for the oracle (one evaluation) and bit for bit
                val, bound = io.xi_multi_reference(kind, xs, ky[:2], ky2[:2], co.X_T, f_t[:2], MU2, xa, np.ones(1), F, 1)
                val, bound = (np.concatenate([v, v[:, :1]], axis=1) for v in (val, bound))
                assert _same_bits(got[:, 0], got[:, 2]), (kind, name, c0)
            worst = max(worst, co.worst_ratio(got, io.pack(val), io.pack(bound)))
        print("multi spline kind %d %-10s nk %5d %5d points  err/bound %.3f" % (kind, name, xs.size, r.size, worst))
        assert worst <= 1.0, (kind, name, worst)


@pytest.mark.parametrize("F,xint,nm", [(1, 1, 3), (1, 9, 3), (5, 3, 3), (17, 2, 3), (257, 1, 17)])
def test_multi_pair_decode_and_bin_average(ctx, F, xint, nm):
    """kind 2, uniform table, weights neither normalised nor symmetric.  F = 257 with 17 nodes: more items than the
    capped grid holds in one trip.  nfun 1 and 3, with and without padding rows."""
    import torch

    xs, ys, y2 = co.table(2, "uniform64")
    ky, ky2, f_t = io.multi_tables(2, xs, ys, y2, F_T2)
    _, xa, xw = co.bin_average_case(2, F, xint)
    mu = np.polynomial.legendre.leggauss(nm)[0]
    if nm == 17:
        ncu = torch.cuda.get_device_properties(ctx.device).multi_processor_count
        assert nm * F * (F + 1) // 2 > 8 * ncu * 256, ncu
    val, bound = io.xi_multi_reference(2, xs, ky, ky2, co.X_T, f_t, mu, xa, xw, F, xint)
    val, bound = io.pack(val), io.pack(bound)
    rows16 = (nm + 15) // 16 * 16
    assert rows16 > nm
    first = None
    for rows in (nm, rows16):
        got3 = _multi(ctx, 2, xs, ky, ky2, f_t, mu, xa, xw, F, xint, nm_rows=rows)
        got1 = _multi(ctx, 2, xs, ky[:1], ky2[:1], f_t[:1], mu, xa, xw, F, xint, nm_rows=rows)
        again = _multi(ctx, 2, xs, ky, ky2, f_t, mu, xa, xw, F, xint, nm_rows=rows)
        assert got3.shape == (rows, 3, F * (F + 1) // 2) and got1.shape == (rows, 1, F * (F + 1) // 2)
        assert _same_bits(got3, again)
        assert _same_bits(got1[:, 0], got3[:, 0])
        assert _same_bits(got3[nm:], np.zeros_like(got3[nm:])) and _same_bits(got1[nm:], np.zeros_like(got1[nm:]))
        ratio = co.worst_ratio(got3[:nm], val, bound)
        print("multi pair decode F %d xint %d nm %d rows %d err/bound %.3f" % (F, xint, nm, rows, ratio))
        assert ratio <= 1.0
        first = got3[:nm] if first is None else first
        assert _same_bits(first, got3[:nm])


def test_projection_and_assembly(ctx):
    """L = 48, F = 5, 188 nodes (not a multiple of 16): xi_multi_average into 192 rows, legendre_project on the buffer as it
    is with zero weights for the padding, cl_blocks; against the oracle's three projections placed by four numpy
    assignments.  Slot 1 is half of slot 0 and slot 2 has another f_t: a swapped slot shows."""
    import scipy.special as ss
    import torch

    from oracle import corrfunc as ocf

    L, F, nm, rows = 48, 5, 188, 192
    xs, ys, y2 = co.table(2, "log300")
    ky, ky2, f_t = np.stack([ys, 0.5 * ys, ys]), np.stack([y2, 0.5 * y2, y2]), np.array([co.F_T, co.F_T, F_T2])
    mu, w, wsum = ss.roots_legendre(nm, mu=True)
    wt = w * 4.0 * np.pi / wsum
    pts, xw, xint = ocf.radial_nodes(1400.0 + 12.5 * np.arange(F) + 3.0 * np.sin(np.arange(F)), 1)
    npair = F * (F + 1) // 2
    d = ctx.to_device
    xi = _poisoned(ctx, (rows, 3, npair))
    mu_p, wt_p = np.zeros(rows), np.zeros(rows)
    mu_p[:nm], wt_p[:nm] = mu, wt
    mu_d = d(mu_p)
    ctx.xi_multi_average(d(xs), d(ky), d(ky2), 2, co.X_T, f_t, mu_d[:nm], d(pts), d(xw), F, xint, nm_rows=rows, out=xi)
    packed = _poisoned(ctx, (L, 3 * npair))
    ctx.legendre_project(mu_d, d(wt_p), L - 1, xi.reshape(rows, 3 * npair), out=packed)
    ext = _poisoned(ctx, (L, 2 * F, 2 * F))
    ctx.cl_blocks(packed.reshape(L, 3, npair), F, out=ext)
    one = _poisoned(ctx, (L, F, F))
    ctx.cl_blocks(packed.reshape(L, 3, npair)[:, 1].contiguous(), F, out=one)
    torch.cuda.synchronize()
    ext, one = ext.cpu().numpy(), one.cpu().numpy()

    xv, xb = io.xi_multi_reference(2, xs, ky, ky2, co.X_T, f_t, mu, pts, xw, F, xint)
    cl = [co.legendre_project(mu, wt, L - 1, xv[:, f].reshape(nm, -1), xb[:, f].reshape(nm, -1)) for f in range(3)]
    val = io.extended(*(c[0].reshape(L, F, F) for c in cl))
    bound = io.extended(*(c[1].reshape(L, F, F) for c in cl))
    ratio = co.worst_ratio(ext, val, bound)
    print("projection and assembly err/bound %.3f" % ratio)
    assert ratio <= 1.0
    assert _same_bits(ext, ext.transpose(0, 2, 1))
    assert _same_bits(one, ext[:, :F, F:]) and _same_bits(one, one.transpose(0, 2, 1))


def test_arguments_the_kernels_cannot_take(ctx):
    """CORAHIP_EINVAL with a message, nothing written; and a 65 536-knot table runs."""
    import torch

    from cora_amd import _lib

    xs, ys, y2 = co.table(0, "uniform64")
    d = ctx.to_device
    mu, xa, xw = d(MU2), d(np.array([0.0, 10.0, 250.0])), d(np.ones(1))
    out = _poisoned(ctx, (2, 5, 6))
    with pytest.raises(_lib.CoraHipError, match="nfun = 5 tables"):
        ctx.xi_multi_average(d(xs), d(np.tile(ys, (5, 1))), d(np.tile(y2, (5, 1))), 0, 1.0, np.ones(5), mu, xa, xw, 3, 1, out=out)
    out = _poisoned(ctx, (1, 1, 6))
    with pytest.raises(_lib.CoraHipError, match="nm_rows = 1 output rows for nm = 2"):
        ctx.xi_multi_average(d(xs), d(ys[None]), d(y2[None]), 0, 1.0, np.ones(1), mu, xa, xw, 3, 1, nm_rows=1, out=out)
    with pytest.raises(_lib.CoraHipError, match="nk = 3 knots"):
        ctx.xi_multi_average(d(xs[:3]), d(ys[None, :3]), d(y2[None, :3]), 0, 1.0, np.ones(1), mu, xa, xw, 3, 1)
    blocks = _poisoned(ctx, (4, 6, 6))
    with pytest.raises(_lib.CoraHipError, match="nfun = 2"):
        ctx.cl_blocks(ctx.empty((4, 2, 6)), 3, out=blocks)
    torch.cuda.synchronize()
    assert np.all(np.isnan(out.cpu().numpy())) and np.all(np.isnan(blocks.cpu().numpy()))

    xs, ys, y2 = co.table(2, "max", 65536)
    r = co.spline_points(2, xs, stride=4096)
    xa = np.concatenate([[0.0], r[1::max(1, (r.size - 1) // CHUNK)][:CHUNK]])
    got = _multi(ctx, 2, xs, ys[None], y2[None], np.array([co.F_T]), MU2, xa, np.ones(1), xa.size, 1)
    val, bound = co.xi_table_average(2, xs, ys, y2, co.X_T, co.F_T, MU2, xa, np.ones(1), xa.size, 1)
    ratio = co.worst_ratio(got[:, 0], io.pack(val), io.pack(bound))
    print("65536 knots err/bound %.3f" % ratio)
    assert ratio <= 1.0


def _aps(chi, **kw):
    from cora_amd.signal import lss

    corrs = lss.calculate_correlations(io.ps, ksmooth=io.KSMOOTH, **kw)
    aps = lss.multifrequency_aps_device(corrs, io.NSIDE, redshift=np.linspace(0.8, 1.1, len(chi)),
                                        cosmology=io.StandInCosmology(chi))
    return corrs, aps


def test_large_table_end_to_end(ctx):
    """calculate_correlations at its defaults (6002 knots, more than the LDS kernel takes) -> multifrequency_aps_device
    at nside 16; the three C_l arrays against the oracle on the knots the interpolaters hold."""
    corrs, aps = _aps(io.CHI_DRAW)
    cs = [corrs["corr0"], corrs["corr2"], corrs["corr4"]]
    assert all(c._data.shape == (6002, 2) for c in cs) and ctx.xi_table_max_knots() < 6002
    assert np.array_equal(aps["ell"], np.arange(48)) and np.array_equal(aps["chi"], io.CHI_DRAW) and aps["freq"] is None
    val, bound = io.aps_reference(cs, 47, io.CHI_DRAW, 2, 4)
    for n, name in enumerate(("Cl_delta_delta", "Cl_phi_delta", "Cl_phi_phi")):
        got = aps[name].cpu().numpy()
        assert got.shape == (48, 4, 4) and _same_bits(got, got.transpose(0, 2, 1))
        ratio = co.worst_ratio(got, val[n], bound[n])
        print("6002 knots %s err/bound %.3f" % (name, ratio))
        assert ratio <= 1.0, name


_DRAW = {}


def _draw_case(chi):
    key = float(chi[1])
    if key not in _DRAW:
        _DRAW[key] = _aps(chi, samples_per_decade=100)
    return _DRAW[key]


def _check_draw_is_mkfullsky(aps):
    import torch

    from cora_amd.core import skysim
    from cora_amd.signal import lss

    ext = lss.initial_lss_covariance_device(aps)
    ext_h = ext.cpu().numpy()
    phi, delta = lss.generate_initial_lss_device(aps, seed=1)
    ref = skysim.mkfullsky_device(ext, io.NSIDE, rng=np.random.default_rng(1))
    torch.cuda.synchronize()
    phi, delta, ref = phi.cpu().numpy(), delta.cpu().numpy(), ref.cpu().numpy()
    assert phi.shape == delta.shape == (4, 12 * io.NSIDE**2)
    assert _same_bits(phi, ref[:4]) and _same_bits(delta, ref[4:])
    return ext_h, phi, delta


def test_the_draw(ctx):
    """602 knots, chi = 1500 + 150 i, seed 1: nside from the spectra, the blocks positive definite, (phi, delta) the two
    halves of mkfullsky_device on the extended blocks bit for bit, delta^2 and phi delta within 5 sigma per slice."""
    from cora_amd.signal import lss

    corrs, aps = _draw_case(io.CHI_DRAW)
    assert corrs["corr0"]._data.shape == (602, 2)
    with pytest.raises(RuntimeError, match=r"Requested nside \(32\) cannot exceed nside used for input C_l \(16\)"):
        lss.generate_initial_lss_device(aps, nside=32, seed=1)
    ext, phi, delta = _check_draw_is_mkfullsky(aps)
    assert ext.shape == (48, 8, 8) and _same_bits(ext, ext.transpose(0, 2, 1))
    assert _same_bits(ext, io.extended(*(aps[k].cpu().numpy() for k in ("Cl_delta_delta", "Cl_phi_delta", "Cl_phi_phi"))))
    assert io.is_positive_definite(ext)
    z, pd_signal = io.draw_z_scores(phi, delta, ext)
    print("draw seed 1: z(delta^2) %s  z(phi delta) %s  phi delta expectation / sigma %s"
          % (np.round(z[0], 2), np.round(z[1], 2), np.round(pd_signal, 1)))
    assert np.all(np.abs(z) <= 5.0), z


def test_indefinite_blocks(ctx):
    """chi = 2300 + 8 i: the blocks are indefinite at most l (the reference's own behaviour at coarse quadrature, which
    matrix_root_manynull is there for).  Finite maps, and the draw is mkfullsky_device's bit for bit."""
    corrs, aps = _draw_case(io.CHI_INDEFINITE)
    ext, phi, delta = _check_draw_is_mkfullsky(aps)
    assert np.all(np.isfinite(phi)) and np.all(np.isfinite(delta))
    unit = ext / np.sqrt(np.einsum("lii,ljj->lij", ext, ext))
    lowest = np.linalg.eigvalsh(unit)[:, 0]
    print("indefinite blocks: smallest eigenvalue of the unit-diagonal block %.1e .. %.1e, negative at %d of %d l"
          % (lowest.min(), lowest.max(), (lowest < 0).sum(), lowest.size))
    # the condition on the input that makes this test mean something: eigenvalues below the jitter of 1e-14 at most l,
    # so that the Cholesky route fails there and the draw goes through the eigen-decomposition
    assert (lowest < -1e-13).sum() > lowest.size // 2 and not io.is_positive_definite(ext)


def test_numpy_forms_and_frequencies(ctx):
    """``multifrequency_aps`` / ``generate_initial_lss`` (numpy in and out) with ``frequencies=`` and the default
    cosmology at 602 knots: the bits of the device forms, ``redshift`` and ``chi`` from ``nu21`` and
    ``Cosmology().comoving_distance``; the spectra are ``corr_to_clarray_multi_device`` of the three functions; the
    covariance is assembled from the ``Cl_*`` entries as they stand (an edited cross term is what is drawn from)."""
    import torch

    from cora_amd.signal import corrfunc, lss
    from cora_amd.util import constants
    from cora_amd.util.cosmology import Cosmology

    corrs, _ = _draw_case(io.CHI_DRAW)
    freq = np.array([700.0, 660.0, 620.0, 580.0])
    host = lss.multifrequency_aps(corrs, io.NSIDE, redshift=np.zeros(4), frequencies=freq)
    dev = lss.multifrequency_aps_device(corrs, io.NSIDE, frequencies=freq)
    z = constants.nu21 / freq - 1.0
    chi = np.asarray(Cosmology().comoving_distance(z), dtype=np.float64)
    assert set(host) == set(dev) == {"ell", "chi", "redshift", "freq", "cosmology", "Cl_delta_delta", "Cl_phi_delta", "Cl_phi_phi"}
    for aps in (host, dev):
        assert np.array_equal(aps["freq"], freq) and np.array_equal(aps["redshift"], z) and np.array_equal(aps["chi"], chi)
        assert np.array_equal(aps["ell"], np.arange(48)) and isinstance(aps["cosmology"], Cosmology)
    full = corrfunc.corr_to_clarray_multi_device([corrs["corr0"], corrs["corr2"], corrs["corr4"]], 47, chi, xromb=2, q=4)
    assert tuple(full.shape) == (3, 48, 4, 4)
    for n, name in enumerate(("Cl_delta_delta", "Cl_phi_delta", "Cl_phi_phi")):
        assert isinstance(host[name], np.ndarray) and isinstance(dev[name], torch.Tensor)
        assert _same_bits(host[name], dev[name].cpu().numpy()) and _same_bits(host[name], full[n].cpu().numpy())
    ext_h = lss.initial_lss_covariance_device(host).cpu().numpy()
    assert _same_bits(ext_h, lss.initial_lss_covariance_device(dev).cpu().numpy())
    assert _same_bits(ext_h, io.extended(host["Cl_delta_delta"], host["Cl_phi_delta"], host["Cl_phi_phi"]))
    phi, delta = lss.generate_initial_lss(host, seed=3)
    phi_d, delta_d = lss.generate_initial_lss_device(dev, rng=np.random.default_rng(3))
    assert isinstance(phi, np.ndarray) and phi.shape == delta.shape == (4, 12 * io.NSIDE**2)
    assert _same_bits(phi, phi_d.cpu().numpy()) and _same_bits(delta, delta_d.cpu().numpy())
    edited = dict(host)
    edited["Cl_phi_delta"] = np.zeros_like(host["Cl_phi_delta"])
    ext_e = lss.initial_lss_covariance_device(edited).cpu().numpy()
    assert _same_bits(ext_e, io.extended(host["Cl_delta_delta"], edited["Cl_phi_delta"], host["Cl_phi_phi"]))
    xs, ys, y2 = co.table(0, "uniform64")
    with pytest.raises(ValueError, match="contiguous"):
        ctx.cl_blocks(ctx.empty((4, 3, 6))[:, 1], 3)
    with pytest.raises(ValueError, match="contiguous"):
        d = ctx.to_device
        ctx.xi_multi_average(d(xs), d(np.stack([ys, ys], axis=1)).T, d(np.stack([y2, y2], axis=1)).T, 0, 1.0, np.ones(2),
                             d(MU2), d(np.array([0.0, 10.0])), d(np.ones(1)), 2, 1)
