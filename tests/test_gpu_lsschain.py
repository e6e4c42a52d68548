"""The LSS chain on the device (csrc/lsschain.hip through cora_amd._lib.Context, cora_amd.signal.lssutil and
cora_amd.signal.lss) against the outputs of the reference (tests/golden/lsschain_vectors.npz) and the numpy oracle of
tests/_lsschain_oracle.py.

Tolerances are derived, not tuned:
  slice_mix        (n + 2) eps (|K| @ |f|) per element: the bound of an inner product of length n in any summation
                   order, with FMA or without.
  diff2, linear dynamics, first-order bias: exact equality (the kernels round every product and sum on its own, in
                   the reference's order).
  sums             ncol eps sum |terms| for a sum of ncol terms (worst case of any order), / ncol for a mean.
  second-order bias, lognormal: stated at the tests.
Every test prints its worst error over tolerance.  Run with -m gpu."""
import os

import numpy as np
import pytest

import _lsschain_oracle as lo

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = np.finfo(np.float64).eps


@pytest.fixture(scope="module")
def gv():
    g = dict(np.load(os.path.join(ROOT, "tests", "golden", "lsschain_vectors.npz")))
    q = float(g["q"])
    for k in ("chi", "sigmaP", "D", "phi", "delta", "f3", "b1", "b2", "fr", "map"):
        g[k] = g[k + "_q"].astype(np.float64) * q
    return g


def _dev(ctx, a):
    return ctx.to_device(np.ascontiguousarray(a, dtype=np.float64))


def _host(t):
    return t.cpu().numpy()


def _ratio(err, tol):
    """worst err / tol; a non-zero error where the tolerance is zero counts as inf"""
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(tol > 0, err / np.where(tol > 0, tol, 1.0), np.where(err > 0, np.inf, 0.0))
    return float(np.max(r)) if r.size else 0.0


def _mix_inputs(n, ncol, seed):
    rng = np.random.default_rng(seed)
    K = rng.standard_normal((n, n))
    f = rng.standard_normal((n, ncol))
    f[n // 2] *= 1e6
    if n > 1:
        f[0] = 0.0
    return K, f


def _mix_check(ctx, K, f, label, **kw):
    import torch

    n, ncol = f.shape
    Kd, fd = _dev(ctx, K), _dev(ctx, f)
    K0, f0 = Kd.clone(), fd.clone()
    out = torch.full((n, ncol), float("nan"), dtype=torch.float64, device=ctx.device)
    ctx.slice_mix(Kd, fd, out=out, **kw)
    got = _host(out)
    assert np.isfinite(got).all()
    assert torch.equal(Kd, K0) and torch.equal(fd, f0)
    tol = (n + 2) * EPS * (np.abs(K) @ np.abs(f))
    worst = _ratio(np.abs(got - K @ f), tol)
    print("slice_mix %s n %d ncol %d: worst err / tol %.3g" % (label, n, ncol, worst))
    assert worst <= 1.0
    again = ctx.slice_mix(Kd, fd, **kw)
    assert torch.equal(again, out)
    return out


@pytest.mark.parametrize("ncol", [1, 15, 17, 48, 3072, 3073])
@pytest.mark.parametrize("n", [1, 3, 4, 16, 17, 37, 128, 130, 300])
def test_slice_mix_matches_oracle(ctx, n, ncol):
    K, f = _mix_inputs(n, ncol, 1000 * n + ncol)
    _mix_check(ctx, K, f, "dense")


def test_slice_mix_many_workgroups(ctx):
    K, f = _mix_inputs(128, 49152, 7)
    _mix_check(ctx, K, f, "dense")


def _skip_matrices(n, rng):
    full = rng.standard_normal((n, n))
    i, j = np.indices((n, n))
    zero_block = full.copy()
    zero_block[16:32] = 0.0
    last = np.zeros((n, n))
    last[n // 3, n - 1] = 1.5
    return {"tridiagonal": np.where(np.abs(i - j) <= 1, full, 0.0), "lower": np.tril(full), "upper": np.triu(full),
            "zero_block": zero_block, "last_column": last}


@pytest.mark.parametrize("kind", ["tridiagonal", "lower", "upper", "zero_block", "last_column"])
@pytest.mark.parametrize("n", [37, 130])
def test_slice_mix_skipping(ctx, n, kind):
    import torch

    rng = np.random.default_rng(n)
    K = _skip_matrices(n, rng)[kind]
    _, f = _mix_inputs(n, 145, n + 1)
    skipped = _mix_check(ctx, K, f, kind)
    dense = ctx.slice_mix(_dev(ctx, K), _dev(ctx, f), skip=False)      # ranges forced to [0, n)
    assert torch.equal(skipped, dense)


def test_slice_mix_band_cut_within_documented_bound(ctx, gv):
    """band_cut = 1e-18 on the golden 128-point FoG kernel.  The documented bound is on the dropped terms:
    |sum of dropped K_ij f_jp| <= band_cut max_j |K_ij| sum_j |f_jp|.  Checked three ways: the band_cut call equals the
    exact call on the thresholded matrix K' bit for bit; the product of the dropped part K - K' alone is within the
    bound; and the band_cut call differs from the exact call on K by no more than the bound plus the rounding of the
    two sums ((n + 2) eps |K| @ |f| each - two roundings of sums that differ in their last terms need not agree).
    Measured on an MI355X: dropped part 0.006 of the bound; |banded - exact| up to 5.3 bounds (rounding flips of the
    last bit, 2e-16 of the result, against a bound of 3e-17), 0.004 of bound plus rounding."""
    import torch

    K = gv["fog_128"]
    n, cut = 128, 1e-18
    rng = np.random.default_rng(5)
    f = rng.standard_normal((n, 3073))
    fd = _dev(ctx, f)
    exact = ctx.slice_mix(K, fd)
    banded = ctx.slice_mix(K, fd, band_cut=cut)
    Kc = np.where(np.abs(K) < cut * np.abs(K).max(axis=1, keepdims=True), 0.0, K)
    assert (Kc == 0).sum() > n * n // 2                                  # the cut does drop most of the matrix
    assert torch.equal(banded, ctx.slice_mix(Kc, fd))
    bound = cut * np.abs(K).max(axis=1)[:, None] * np.abs(f).sum(axis=0)[None, :]
    dropped = _host(ctx.slice_mix(K - Kc, fd))
    r_drop = _ratio(np.abs(dropped), bound)
    rounding = 2 * (n + 2) * EPS * (np.abs(K) @ np.abs(f))
    diff = np.abs(_host(banded) - _host(exact))
    print("band_cut 1e-18: dropped part / bound %.3g, |banded - exact| / bound max %.3g, / (bound + rounding) %.3g"
          % (r_drop, _ratio(diff, bound), _ratio(diff, bound + rounding)))
    assert r_drop <= 1.0
    assert _ratio(diff, bound + rounding) <= 1.0


def test_slice_mix_rejects_overlap_and_bad_shapes(ctx):
    import torch

    n, ncol = 8, 64
    buf = torch.zeros((2 * n, ncol), dtype=torch.float64, device=ctx.device)
    K = np.eye(n)
    with pytest.raises(ValueError):
        ctx.slice_mix(K, buf[:n], out=buf[:n])
    with pytest.raises(ValueError):
        ctx.slice_mix(K, buf[:n], out=buf[2:n + 2])
    ctx.slice_mix(K, buf[:n], out=buf[n:])
    with pytest.raises(ValueError):
        ctx.slice_mix(np.eye(n + 1), buf[:n])


# ------------------------------------------------------------------------------------------------ diff2
def _nonuniform(n, seed):
    rng = np.random.default_rng(seed)
    return 1500.0 + np.cumsum(rng.uniform(3.0, 7.0, n))


def test_diff2_equals_golden(ctx, gv):
    from cora_amd.signal import lssutil

    got = _host(lssutil.diff2_device(_dev(ctx, gv["phi"]), gv["chi"]))
    assert np.array_equal(got, gv["diff2_2d"])
    assert np.array_equal(lssutil.diff2(gv["phi"], gv["chi"], axis=0), gv["diff2_2d"])
    got3 = lssutil.diff2(gv["f3"], gv["chi"], axis=1)
    assert got3.shape == gv["f3"].shape and np.array_equal(got3, gv["diff2_3d"])


@pytest.mark.parametrize("ncol", [1, 47, 48, 3073])
@pytest.mark.parametrize("n", [4, 5, 6, 33])
def test_diff2_equals_oracle(ctx, n, ncol):
    import torch

    from cora_amd.signal import lssutil

    rng = np.random.default_rng(100 * n + ncol)
    x = _nonuniform(n, n)
    f = rng.standard_normal((n, ncol))
    fd = _dev(ctx, f)
    out = torch.full((n, ncol), float("nan"), dtype=torch.float64, device=ctx.device)
    lssutil.diff2_device(fd, x, out=out)
    ref = lo.diff2(f, x, axis=0)
    got = _host(out)
    print("diff2 n %d ncol %d: max |got - oracle| %.3g" % (n, ncol, np.abs(got - ref).max()))
    assert np.array_equal(got, ref)
    assert np.array_equal(_host(fd), f)
    with pytest.raises(ValueError):
        lssutil.diff2_device(fd, x, out=fd)


def test_linear_dynamics_equals_golden(ctx, gv):
    from cora_amd.signal import lss

    args = [_dev(ctx, gv[k]) for k in ("phi", "delta", "bias_b1b2")]
    assert np.array_equal(_host(lss.linear_dynamics_device(*args, gv["chi"], gv["D"])), gv["linear_real"])
    assert np.array_equal(_host(lss.linear_dynamics_device(*args, gv["chi"], gv["D"], gv["fr"])), gv["linear_rsd"])
    assert np.array_equal(lss.linear_dynamics(gv["phi"], gv["delta"], gv["bias_b1b2"], gv["chi"], gv["D"], gv["fr"]),
                          gv["linear_rsd"])


@pytest.mark.parametrize("with_f", [False, True])
@pytest.mark.parametrize("nside", [4, 16])
@pytest.mark.parametrize("n", [4, 9])
def test_linear_dynamics_equals_oracle(ctx, n, nside, with_f):
    from cora_amd.signal import lss

    npix = 12 * nside * nside
    rng = np.random.default_rng(10 * n + nside)
    phi, delta, bias = (rng.standard_normal((n, npix)) * s for s in (3.0, 0.5, 0.7))
    chi = _nonuniform(n, 3 * n)
    D = np.linspace(0.8, 0.6, n)
    f = np.linspace(0.8, 0.95, n) if with_f else None
    got = _host(lss.linear_dynamics_device(_dev(ctx, phi), _dev(ctx, delta), _dev(ctx, bias), chi, D, f))
    assert np.array_equal(got, lo.linear_dynamics(phi, delta, bias, chi, D, f))
    with pytest.raises(ValueError):
        lss.linear_dynamics_device(_dev(ctx, phi[:3]), _dev(ctx, delta[:3]), _dev(ctx, bias[:3]), chi[:3], D[:3], None)


# ------------------------------------------------------------------------------------------------ moments
def _moment_tols(f):
    """(tolerance of the mean, of the variance) per row: ncol eps sum |terms| / ncol"""
    mean = f.mean(axis=1, keepdims=True)
    return EPS * np.abs(f).sum(axis=1), EPS * ((f - mean) ** 2).sum(axis=1)


@pytest.mark.parametrize("ncol", [1, 48, 3073, 196608])
def test_slice_moments_match_numpy(ctx, ncol):
    import torch

    from cora_amd.signal import lssutil

    n = 5
    rng = np.random.default_rng(ncol)
    f = rng.standard_normal((n, ncol)) * np.array([1.0, 0.1, 30.0, 1.0, 2.0])[:, None] + np.array([0, 5, -2, 100, 0])[:, None]
    fd = _dev(ctx, f)
    mean, var = lssutil.slice_moments_device(fd)
    tm, tv = _moment_tols(f)
    rm, rv = _ratio(np.abs(_host(mean) - f.mean(axis=1)), tm), _ratio(np.abs(_host(var) - f.var(axis=1)), tv)
    print("slice_moments ncol %d: mean err / tol %.3g, var err / tol %.3g" % (ncol, rm, rv))
    assert rm <= 1.0 and rv <= 1.0
    mean2, var2 = lssutil.slice_moments_device(fd)
    assert torch.equal(mean, mean2) and torch.equal(var, var2)
    # a strided view: the same rows inside a wider array (odd and even row strides)
    for pad in (5, 6):
        wide = torch.full((n, ncol + pad), float("nan"), dtype=torch.float64, device=ctx.device)
        wide[:, :ncol] = fd
        ms, vs = lssutil.slice_moments_device(wide[:, :ncol])
        assert _ratio(np.abs(_host(ms) - f.mean(axis=1)), tm) <= 1.0
        assert _ratio(np.abs(_host(vs) - f.var(axis=1)), tv) <= 1.0


# ------------------------------------------------------------------------------------------------ bias, lognormal
def _lognormal_tol(x, var, var_tol):
    """8 eps (1 + |x| + var / 2) exp(x - var / 2) (rounding of the argument and of exp, within 1 ulp) +
    exp(x - var / 2) / 2 * (tolerance of the variance)"""
    e = np.exp(x - var / 2)
    return 8 * EPS * (1 + np.abs(x) + var / 2) * e + e / 2 * var_tol


def test_biased_field_first_order_exact(ctx, gv):
    from cora_amd.signal import lss

    got = _host(lss.biased_field_device(_dev(ctx, gv["delta"]), gv["D"], gv["b1"]))
    assert np.array_equal(got, gv["bias_b1"])
    assert np.array_equal(got, lo.biased_field(gv["delta"], gv["D"], gv["b1"]))
    assert np.array_equal(lss.biased_field(gv["delta"], gv["D"], gv["b1"]), gv["bias_b1"])
    # scalars broadcast
    assert np.array_equal(lss.biased_field(gv["delta"], 0.5, 2.0), lo.biased_field(gv["delta"], np.full(12, 0.5), np.full(12, 2.0)))


def _bias_tol(delta, D, b1, b2):
    m2 = (delta**2).mean(axis=1)[:, None]
    m2_tol = EPS * (delta**2).sum(axis=1)[:, None]
    c1, c2 = np.abs(D * b1)[:, None], np.abs(D**2 * b2)[:, None]
    return 4 * EPS * (c1 * np.abs(delta) + c2 * (delta**2 + m2)) + c2 * m2_tol


def test_biased_field_second_order(ctx, gv):
    from cora_amd.signal import lss

    delta, D, b1, b2 = gv["delta"], gv["D"], gv["b1"], gv["b2"]
    got = _host(lss.biased_field_device(_dev(ctx, delta), D, b1, b2))
    tol = _bias_tol(delta, D, b1, b2)
    r = _ratio(np.abs(got - gv["bias_b1b2"]), tol)
    print("biased_field with b2: worst err / tol %.3g" % r)
    assert r <= 1.0
    # b2 alone: the first-order term is skipped
    got2 = _host(lss.biased_field_device(_dev(ctx, delta), D, None, b2))
    assert _ratio(np.abs(got2 - lo.biased_field(delta, D, None, b2)), tol) <= 1.0


@pytest.mark.parametrize("lightcone", [True, False])
def test_biased_field_lognormal(ctx, gv, lightcone):
    from cora_amd.signal import lss

    delta, D, b1 = gv["delta"], gv["D"], gv["b1"]
    x = lo.biased_field(delta, D, b1)                       # exact on the device too (first order only)
    axis = 1 if lightcone else None
    var = x.var(axis=axis, keepdims=True)
    var_tol = EPS * ((x - x.mean(axis=axis, keepdims=True)) ** 2).sum(axis=axis, keepdims=True)
    got = _host(lss.biased_field_device(_dev(ctx, delta), D, b1, lognormal=True, lightcone=lightcone))
    r = _ratio(np.abs(got - lo.biased_field(delta, D, b1, lognormal=True, lightcone=lightcone)),
               _lognormal_tol(x, var, var_tol) * np.ones_like(x))
    print("biased_field lognormal lightcone=%s: worst err / tol %.3g" % (lightcone, r))
    assert r <= 1.0


def test_biased_field_second_order_lognormal_golden(ctx, gv):
    """The golden of bias (b1, b2) + lognormal: the lognormal bound plus the bias tolerance carried through the
    exponential (d exp(x - var/2) = exp(x - var/2) dx)."""
    from cora_amd.signal import lss

    delta, D, b1, b2 = gv["delta"], gv["D"], gv["b1"], gv["b2"]
    x = gv["bias_b1b2"]
    var = x.var(axis=1, keepdims=True)
    btol = _bias_tol(delta, D, b1, b2)
    # the variance moves by at most 2 sqrt(var) max|dx| + its summation bound
    var_tol = EPS * ((x - x.mean(axis=1, keepdims=True)) ** 2).sum(axis=1, keepdims=True) \
        + 4 * np.sqrt(var) * btol.max(axis=1, keepdims=True)
    tol = _lognormal_tol(x, var, var_tol) + np.exp(x - var / 2) * btol
    got = _host(lss.biased_field_device(_dev(ctx, delta), D, b1, b2, lognormal=True))
    r = _ratio(np.abs(got - gv["bias_b1b2_lognormal"]), tol)
    print("biased_field b1, b2, lognormal vs golden: worst err / tol %.3g" % r)
    assert r <= 1.0


@pytest.mark.parametrize("axis", [1, None])
def test_lognormal_transform_device(ctx, gv, axis):
    import torch

    from cora_amd.signal import lssutil

    x = gv["delta"]
    n, npix = x.shape
    ref = gv["lognormal_axis1" if axis == 1 else "lognormal_none"]
    var = x.var(axis=axis, keepdims=True)
    var_tol = EPS * ((x - x.mean(axis=axis, keepdims=True)) ** 2).sum(axis=axis, keepdims=True)
    tol = _lognormal_tol(x, var, var_tol) * np.ones_like(x)
    xd = _dev(ctx, x)
    got = lssutil.lognormal_transform_device(xd, axis=axis)
    r = _ratio(np.abs(_host(got) - ref), tol)
    print("lognormal_transform axis=%s: worst err / tol %.3g" % (axis, r))
    assert r <= 1.0 and np.array_equal(_host(xd), x)
    assert _ratio(np.abs(lssutil.lognormal_transform(x, axis=axis) - ref), tol) <= 1.0
    # into plane 0 of a NaN-filled map: the other planes are not touched
    m = torch.full((n, 4, npix), float("nan"), dtype=torch.float64, device=ctx.device)
    res = lssutil.lognormal_transform_device(xd, out=m[:, 0], axis=axis)
    assert res.data_ptr() == m.data_ptr() and torch.equal(m[:, 0], got) and bool(torch.isnan(m[:, 1:]).all())
    # in place
    inplace = xd.clone()
    assert lssutil.lognormal_transform_device(inplace, out=inplace, axis=axis) is inplace
    assert torch.equal(inplace, got)
    with pytest.raises(ValueError, match="Given output array is incompatible."):
        lssutil.lognormal_transform_device(xd, out=m[:, :1, :-1].reshape(n, -1), axis=axis)
    with pytest.raises(ValueError):
        lssutil.lognormal_transform_device(xd, axis=0)


# ------------------------------------------------------------------------------------------------ FoG, map, composition
def test_fingers_of_god_matches_golden(ctx, gv):
    from cora_amd.signal import lss

    a = float(gv["alpha_fog"])
    K = gv["fog_K"]
    f2 = gv["linear_rsd"]
    got = _host(lss.fingers_of_god_device(_dev(ctx, f2), gv["chi"], gv["sigmaP"], gv["D"], a))
    r2 = _ratio(np.abs(got - gv["fog_2d"]), (12 + 2) * EPS * (np.abs(K) @ np.abs(f2)))
    m = gv["map"]
    md = _dev(ctx, m)
    gotm = lss.fingers_of_god_device(md, gv["chi"], gv["sigmaP"], gv["D"], a)
    assert tuple(gotm.shape) == m.shape
    tolm = ((12 + 2) * EPS * (np.abs(K) @ np.abs(m).reshape(12, -1))).reshape(m.shape)
    rm = _ratio(np.abs(_host(gotm) - gv["fog_map"]), tolm)
    print("fingers_of_god: worst err / tol %.3g (field), %.3g (map)" % (r2, rm))
    assert r2 <= 1.0 and rm <= 1.0
    assert _ratio(np.abs(lss.fingers_of_god(m, gv["chi"], gv["sigmaP"], gv["D"], a) - gv["fog_map"]), tolm) <= 1.0
    assert lss.fingers_of_god_device(md, gv["chi"], gv["sigmaP"], gv["D"], alpha_FoG=0.0) is md
    assert lss.fingers_of_god(m, gv["chi"], gv["sigmaP"], alpha_FoG=0.0) is m


def test_biased_lss_to_map(ctx, gv):
    import torch

    from cora_amd.signal import lss, lssutil

    x = gv["delta"]
    n, npix = x.shape
    xd = _dev(ctx, x)
    T_b = np.linspace(1e-4, 2e-4, n)
    m = lss.biased_lss_to_map_device(xd)
    assert tuple(m.shape) == (n, 4, npix) and torch.equal(m[:, 0], xd) and not bool(m[:, 1:].any())
    m1 = lss.biased_lss_to_map_device(xd, map_prefactor=3.0, T_b=T_b, polarisation=False)
    assert tuple(m1.shape) == (n, 1, npix)
    assert np.array_equal(_host(m1), lo.biased_lss_to_map(x, False, 3.0, T_b, False))
    ml = lss.biased_lss_to_map_device(xd, lognormal=True, map_prefactor=3.0, T_b=T_b)
    ln = lssutil.lognormal_transform_device(xd, axis=1)
    assert np.array_equal(_host(ml[:, 0]), (_host(ln) * 3.0) * T_b[:, None]) and not bool(ml[:, 1:].any())
    assert np.array_equal(lss.biased_lss_to_map(x, True, 3.0, T_b), _host(ml))


@pytest.mark.parametrize("dynamics", ["linear", "zeldovich"])
def test_tracer_map_is_the_composition(ctx, dynamics, monkeypatch):
    """tracer_map_device against the same four calls made one by one, bit for bit (nside 16, 8 slices).

    The Zel'dovich density step adds with float atomics (csrc/pmesh.hip): two runs of it on the same inputs agree to
    rounding only (measured here: 6.5e-19 on the final map), so no composition through it can equal a second,
    independent run bit for bit.  For that dynamics the step's result inside tracer_map_device is recorded: its
    inputs must be bit for bit the ones the step-by-step sequence passes, and everything downstream of its output
    must equal the step-by-step calls on that same output bit for bit.  The figure of an independent run is printed."""
    import torch

    from cora_amd.signal import lss

    nside, n = 16, 8
    npix = 12 * nside * nside
    rng = np.random.default_rng(16)
    phi = _dev(ctx, rng.standard_normal((n, npix)) * 2.0)
    delta = _dev(ctx, rng.standard_normal((n, npix)) * 0.3)
    chi = 1000.0 + 10.0 * np.arange(n) + np.array([0.0, 0.3, -0.2, 0.1, 0.0, 0.4, -0.1, 0.2])
    D, f = np.linspace(0.8, 0.7, n), np.linspace(0.8, 0.9, n)
    b1, b2, sig, T_b = np.full(n, 1.3), np.full(n, -0.2), np.full(n, 1.93), np.linspace(1e-4, 2e-4, n)
    calls = []
    za = lss.zeldovich_density_device

    def recording(*args, **kw):
        res = za(*args, **kw)
        calls.append((args, kw, res.clone()))
        return res

    monkeypatch.setattr(lss, "zeldovich_density_device", recording)
    got = lss.tracer_map_device(phi, delta, chi, D, f, b1, b2, sigmaP=sig, dynamics=dynamics, fog_D=D, alpha_FoG=0.8,
                                map_lognormal=True, map_prefactor=2.0, T_b=T_b)
    monkeypatch.undo()
    bias = lss.biased_field_device(delta, D, b1, b2)
    if dynamics == "linear":
        assert not calls
        final = lss.linear_dynamics_device(phi, delta, bias, chi, D, f)
    else:
        (args, kw, final), = calls
        assert args[0] is phi and args[1] is delta and torch.equal(args[2], bias)
        assert all(np.array_equal(np.asarray(u), v) for u, v in zip(args[3:6], (chi, D, f)))
        assert kw == dict(sigma_chi=None, lmax=None, niter=3)
        indep = lss.zeldovich_density_device(phi, delta, bias, chi, D, f)
        print("zeldovich_density_device, two runs: max |difference| %.3g (float atomics)" % float((indep - final).abs().max()))
    fog = lss.fingers_of_god_device(final, chi, sig, D, 0.8)
    ref = lss.biased_lss_to_map_device(fog, True, 2.0, T_b)
    assert tuple(got.shape) == (n, 4, npix) and bool(torch.isfinite(got).all())
    print("tracer_map %s: max |composition - steps| %.3g" % (dynamics, float((got - ref).abs().max())))
    assert torch.equal(got, ref)
    with pytest.raises(ValueError):
        lss.tracer_map_device(phi, delta, chi, D, f, b1, dynamics="other")


# ------------------------------------------------------------------------------------------------ index width
def test_index_width_past_2_31(ctx):
    """n = 4, ncol = 2^30 + 16: 4.3e9 elements per field, element offsets past 2^31 (and past 2^32 in bytes)."""
    import torch

    from cora_amd.signal import lssutil

    free, _ = torch.cuda.mem_get_info(ctx.device)
    if free < 120e9:
        pytest.skip("needs 120 GB of free device memory (%.0f GB free)" % (free / 1e9))
    n, ncol = 4, 2**30 + 16
    g = torch.Generator(device=ctx.device).manual_seed(3)
    f = torch.randn((n, ncol), dtype=torch.float64, device=ctx.device, generator=g)
    cols = torch.cat([torch.arange(0, ncol - 4096, 1048573, device=ctx.device),
                      torch.arange(ncol - 4096, ncol, device=ctx.device)])
    fs = _host(f[:, cols])
    rng = np.random.default_rng(4)
    K = rng.standard_normal((n, n))
    x = _nonuniform(n, 1)

    out = lssutil.slice_mix_device(K, f)
    r = _ratio(np.abs(_host(out[:, cols]) - K @ fs), (n + 2) * EPS * (np.abs(K) @ np.abs(fs)))
    print("index width: slice_mix worst err / tol %.3g" % r)
    assert r <= 1.0
    out.fill_(float("nan"))
    lssutil.diff2_device(f, x, out=out)
    assert np.array_equal(_host(out[:, cols]), lo.diff2(fs, x, axis=0))
    del out
    mean, var = lssutil.slice_moments_device(f)
    tv, tm = torch.var_mean(f, dim=1, unbiased=False)
    sabs = _host(torch.linalg.vector_norm(f, ord=1, dim=1))          # sum |f|, no temporary
    ssq = _host(tv) * ncol                                            # sum (f - mean)^2
    rm = _ratio(np.abs(_host(mean) - _host(tm)), EPS * sabs)
    rv = _ratio(np.abs(_host(var) - _host(tv)), EPS * ssq)
    print("index width: mean err / tol %.3g, var err / tol %.3g" % (rm, rv))
    assert rm <= 1.0 and rv <= 1.0
    # the last columns count: a spike there must show in the sums
    f[:, -1] += 1.0e6
    mean2, _ = lssutil.slice_moments_device(f)
    assert np.allclose(_host(mean2 - mean) * ncol, 1.0e6, rtol=1e-6)
