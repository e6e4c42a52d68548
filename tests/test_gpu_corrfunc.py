"""The xi(r) -> C_l kernels (cora_amd/csrc/corrfunc.hip) called directly - ctx.xi_table_average, ctx.legendre_project
- and held pointwise to the derived bounds of tests/_corrfunc_oracle.py: the spline at every knot, look-up-cell edge
and table end, the short transcendentals at their branch switches and range ends, the pair decode past one grid
trip, the Legendre recurrence to lmax 2048 and the MFMA GEMM at every tile boundary.  Every output tensor is filled
with a NaN byte pattern first.  tests/test_corrfunc_oracle_host.py shows that the same bounds reject each of seven
deliberate defects.  Run with -m gpu.

Each test prints its worst err / bound per case group.  Observed on the MI355X (derived constants: see the oracle;
the device reports 163840 bytes of LDS per workgroup: a limit of 2925 knots):

  spline point sets, worst over every element      kind 0   kind 1   kind 2
    nk4                                             0.306    0.332    0.377
    uniform64                                       0.281    0.348    0.415
    log300 (forward walk)                           0.425    0.364    0.392
    mirror300                                       0.314    0.379    0.404
    close (knots 2^-40 apart)                       0.262    0.334    0.371
    max (2925 knots)                                0.378    0.361    0.432
    plateau (|y| 1e-300 .. 708, exp tail to -744)   0.250    0.436    0.331
    kinked (kind 0) / zero end-slope (kind 1)       0.224    0.114
  pair decode and bin average, kind 0               0.012 .. 0.129; F 257 x 17 nodes (second grid trip) 0.277
  bin average, kinds 1 and 2                        0.122 / 0.015, 0.200 / 0.126   (F 3 xint 2 / F 2 xint 9)
  Legendre matrix, lmax 2048 / 0 / 1                0.947 / 0 / 0.947   (the single rounding of wt * mu at l = 1)
  GEMM tile edges, nm 1 / 15 / 16 / 17 / 33         0.119 / 0.219 / 0.153 / 0.088 / 0.079
  dirty scratch                                     0.050
  corr_to_clarray per (l, i, j), kinds 0 / 1 / 2    0.005 / 0.025 / 0.018;  4000 knots through the host path 0.022
"""
import numpy as np
import pytest

import _corrfunc_oracle as co

pytestmark = pytest.mark.gpu

KINDS = (0, 1, 2)
CHUNK = 96                       # separations per xi_table_average call of the point-set tests (F = CHUNK + 1)
MU2 = np.array([1.0, 0.25])      # mu = 1: |r_i - r_j| exactly; 0.25: general separations


def _poisoned(ctx, shape):
    import torch

    t = ctx.empty(shape)
    t.view(torch.uint8).fill_(0xFF)            # every double a NaN: an element the kernel does not write shows
    return t


def _xi(ctx, kind, xs, ys, y2, mu, xa, xw, F, xint):
    import torch

    out = _poisoned(ctx, (len(mu), F, F))
    d = ctx.to_device
    ctx.xi_table_average(d(xs), d(ys), d(y2), kind, co.X_T, co.F_T, d(mu), d(xa), d(xw), F, xint, out=out)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _project(ctx, mu, wt, lmax, xi):
    import torch

    out = _poisoned(ctx, (lmax + 1, xi.shape[1]))
    ctx.legendre_project(ctx.to_device(mu), ctx.to_device(wt), lmax, ctx.to_device(np.ascontiguousarray(xi)), out=out)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


@pytest.mark.parametrize("kind", KINDS)
def test_spline_point_sets(ctx, kind):
    """xint = 1, xw = [1], xa = [0, r_1, ...]: row 0 is xi(r_j) at the exact r_j of the point set, the other rows
    |r_i - r_j| (mu = 1) and general separations; every element against the oracle, out == out^T bit for bit."""
    nk_max = ctx.xi_table_max_knots()
    print("knot limit of the device:", nk_max)
    assert nk_max >= 1024
    for name, xs, ys, y2, r in co.spline_cases(kind, nk_max):
        worst, pts = 0.0, r[1:]
        for c0 in range(0, pts.size, CHUNK):
            xa = np.concatenate([[0.0], pts[c0:c0 + CHUNK]])
            got = _xi(ctx, kind, xs, ys, y2, MU2, xa, np.ones(1), xa.size, 1)
            assert _same_bits(got, got.transpose(0, 2, 1)), (kind, name, c0)
            val, bound = co.xi_table_average(kind, xs, ys, y2, co.X_T, co.F_T, MU2, xa, np.ones(1), xa.size, 1)
            worst = max(worst, co.worst_ratio(got, val, bound))
        print("spline kind %d %-10s nk %4d %5d points  err/bound %.3f" % (kind, name, xs.size, r.size, worst))
        assert worst <= 1.0, (kind, name, worst)


@pytest.mark.parametrize("F,xint,nm", [(1, 1, 3), (1, 2, 3), (1, 9, 3), (2, 1, 3), (2, 2, 3), (2, 9, 3), (3, 1, 3), (3, 2, 3),
                                       (3, 9, 3), (17, 1, 3), (17, 2, 3), (17, 9, 3), (257, 1, 17)])
def test_pair_decode_grid_stride_and_bin_average(ctx, F, xint, nm):
    """kind 0, uniform table.  F = 257 with 17 nodes: 563 601 items, more than the 8 * num_cu * 256 threads of the capped
    grid hold in one trip.  Weights neither normalised nor symmetric."""
    import torch

    xs, ys, y2 = co.table(0, "uniform64")
    _, xa, xw = co.bin_average_case(0, F, xint)
    mu = np.polynomial.legendre.leggauss(nm)[0]
    if nm == 17:
        ncu = torch.cuda.get_device_properties(ctx.device).multi_processor_count
        assert nm * F * (F + 1) // 2 > 8 * ncu * 256, ncu
    got = _xi(ctx, 0, xs, ys, y2, mu, xa, xw, F, xint)
    assert _same_bits(got, got.transpose(0, 2, 1))
    val, bound = co.xi_table_average(0, xs, ys, y2, co.X_T, co.F_T, mu, xa, xw, F, xint)
    ratio = co.worst_ratio(got, val, bound)
    print("pair decode F %d xint %d nm %d err/bound %.3f" % (F, xint, nm, ratio))
    assert ratio <= 1.0


@pytest.mark.parametrize("kind", (1, 2))
def test_bin_average_of_transformed_kinds(ctx, kind):
    xs, ys, y2 = co.table(kind, "uniform64")
    for F, xint in ((3, 2), (2, 9)):
        mu, xa, xw = co.bin_average_case(kind, F, xint)
        got = _xi(ctx, kind, xs, ys, y2, mu, xa, xw, F, xint)
        val, bound = co.xi_table_average(kind, xs, ys, y2, co.X_T, co.F_T, mu, xa, xw, F, xint)
        ratio = co.worst_ratio(got, val, bound)
        print("bin average kind %d F %d xint %d err/bound %.3f" % (kind, F, xint, ratio))
        assert ratio <= 1.0 and _same_bits(got, got.transpose(0, 2, 1))


def _legendre_nodes():
    e = 1.0 - 2.0**-52
    return np.concatenate([[1.0, -1.0, 0.0, e, -e], np.polynomial.legendre.leggauss(43)[0]])


@pytest.mark.parametrize("lmax", (2048, 0, 1))
def test_legendre_matrix_elementwise(ctx, lmax):
    """xi = identity: legendre_project returns wt_m P_l(mu_m) itself (the products with 1 and 0 are exact)."""
    mu = _legendre_nodes()
    wt = np.random.default_rng(5).uniform(0.5, 2.0, mu.size)
    got = _project(ctx, mu, wt, lmax, np.eye(mu.size))
    lm, bound = co.legendre_matrix(mu, wt, lmax)
    ratio = co.worst_ratio(got, lm, bound)
    print("legendre matrix lmax %d nm %d err/bound %.3f" % (lmax, mu.size, ratio))
    assert got.shape == (lmax + 1, mu.size) and ratio <= 1.0
    # mu = +-1: the recurrence is exact, only wt * (+-1) remains
    assert np.array_equal(got[:, 0], np.full(lmax + 1, wt[0])) and np.array_equal(np.abs(got[:, 1]), np.full(lmax + 1, wt[1]))


@pytest.mark.parametrize("nm", (1, 15, 16, 17, 33))
def test_gemm_tile_edges(ctx, nm):
    """L x ncol over every tile boundary for one, two and three K chunks, padded-copy and direct B operand; columns
    of xi spanning 1e-100 .. 1e100 with mixed signs, so only a per-element bound can pass."""
    worst = 0.0
    for L in (1, 127, 128, 129, 257):
        for ncol in (1, 127, 128, 129, 400):
            mu, wt, xi = co.projection_case(L, ncol, nm)
            got = _project(ctx, mu, wt, L - 1, xi)
            val, bound = co.legendre_project(mu, wt, L - 1, xi)
            ratio = co.worst_ratio(got, val, bound)
            assert ratio <= 1.0, (L, ncol, nm, ratio)
            worst = max(worst, ratio)
    print("gemm nm %d err/bound %.3f" % (nm, worst))


def test_dirty_scratch_is_not_inherited(ctx):
    """A call that leaves NaN in both scratch slots (Legendre matrix and padded operand), then a smaller finite one
    whose padding rows and columns lie inside what the first one wrote."""
    mu, wt, xi = co.projection_case(300, 400, 33)
    first = _project(ctx, mu, np.full(33, np.nan), 299, np.full((33, 400), np.nan))
    assert np.all(np.isnan(first))
    mu, wt, xi = co.projection_case(129, 129, 17)
    got = _project(ctx, mu, wt, 128, xi)
    val, bound = co.legendre_project(mu, wt, 128, xi)
    ratio = co.worst_ratio(got, val, bound)
    print("dirty scratch err/bound %.3f" % ratio)
    assert np.all(np.isfinite(got)) and ratio <= 1.0


@pytest.mark.parametrize("kind", KINDS)
def test_corr_to_clarray_per_element(ctx, kind):
    """One corr_to_clarray per interpolater kind (lmax 300, 20 distances, xromb 2), every (l, i, j) against the
    oracle's composed bound."""
    from cora_amd.signal import corrfunc

    lmax, xa, ref, bound, interp = co.end_to_end_case(kind)
    got = corrfunc.corr_to_clarray(interp, lmax, xa, xromb=2, q=2)
    assert got.shape == (lmax + 1, 20, 20) and _same_bits(got, got.transpose(0, 2, 1))
    ratio = co.worst_ratio(got.reshape(lmax + 1, -1), ref, bound)
    print("corr_to_clarray kind %d err/bound %.3f" % (kind, ratio))
    assert ratio <= 1.0


def test_knot_limit_follows_the_device(ctx):
    """One knot above the limit: the ordinary argument error naming the limit, nothing launched, the next call fine;
    a 4000-knot Interpolater goes through corr_to_clarray's host-evaluated path and agrees with the oracle."""
    import scipy.special as ss
    import torch

    from cora_amd import _lib
    from cora_amd.signal import corrfunc
    from oracle import corrfunc as ocf

    nk_max = ctx.xi_table_max_knots()
    xs, ys, y2 = co.table(0, "max", nk_max + 1)
    d = ctx.to_device
    mu, xa, xw = d(MU2), d(np.array([0.0, 10.0, 250.0])), d(np.ones(1))
    out = _poisoned(ctx, (2, 3, 3))
    rc = ctx.lib.corahip_xi_table_average(ctx.h, ctx._f64(d(xs)), ctx._f64(d(ys)), ctx._f64(d(y2)), nk_max + 1, 0, 1.0, 1.0,
                                          ctx._f64(mu), 2, ctx._f64(xa), ctx._f64(xw), 3, 1, ctx._f64(out))
    msg = ctx.lib.corahip_last_error().decode()
    assert rc != 0 and "limit of %d" % nk_max in msg, (rc, msg)
    torch.cuda.synchronize()
    assert np.all(np.isnan(out.cpu().numpy()))
    with pytest.raises(_lib.CoraHipError, match="limit of %d" % nk_max):
        ctx.xi_table_average(d(xs), d(ys), d(y2), 0, 1.0, 1.0, mu, xa, xw, 3, 1)
    got = _xi(ctx, 0, xs[:-1], ys[:-1], y2[:-1], MU2, np.array([0.0, 10.0, 250.0]), np.ones(1), 3, 1)
    val, bound = co.xi_table_average(0, xs[:-1], ys[:-1], y2[:-1], 1.0, 1.0, MU2, np.array([0.0, 10.0, 250.0]), np.ones(1), 3, 1)
    assert co.worst_ratio(got, val, bound) <= 1.0

    xs, ys, y2 = co.table(0, "max", 4000)
    assert nk_max < 4000
    lmax, xarr = 24, np.array([900.0, 960.0, 1000.0, 1100.0, 1130.0])
    got = corrfunc.corr_to_clarray(co.interpolater(0, xs, ys, y2), lmax, xarr, xromb=1, q=2)
    m, w, wsum = ss.roots_legendre(2 * lmax, mu=True)
    pts, pw, xint = ocf.radial_nodes(xarr, 1)
    xi, xb = co.xi_table_average(0, xs, ys, y2, 1.0, 1.0, m, pts, pw, 5, xint)
    ref, bound = co.legendre_project(m, w * 4.0 * np.pi / wsum, lmax, xi.reshape(m.size, -1), xb.reshape(m.size, -1))
    ratio = co.worst_ratio(got.reshape(lmax + 1, -1), ref, bound)
    print("4000-knot interpolater through corr_to_clarray err/bound %.3f" % ratio)
    assert ratio <= 1.0
