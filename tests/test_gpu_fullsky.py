"""The exact curved-sky C_l on the GPU (csrc/fullsky.hip, RedshiftCorrelation.angular_powerspectrum_full) against
tests/_fullsky_oracle.py: the radial table against the longdouble table within tol E(x) (tol: 8 x what the float64
restatement of the scheme shows, a constant of the oracle module), the Gram product against the longdouble sum within its
derived bound, symmetric and subset-invariant bit for bit, the chunked driver, the model at broadcast points and through
``clarray`` (the average-before-product identity), and the three entry points on poisoned memory.  Every comparison prints
err / bound."""
import functools

import numpy as np
import pytest

import _fullsky_oracle as fo
import _poison

pytestmark = pytest.mark.gpu

LD, U = fo.LD, fo.U
CASES = fo.radial_cases()


def _worst(err, bound):
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(bound > 0, err.astype(np.float64) / bound, np.where(err > 0, np.inf, 0.0))
    return float(r.max())


def _modes(name):
    c = CASES[name]
    if c["chi"].shape[1] == 1:          # unit coefficients: j_l alone, j_l'' alone
        return [("j_l", c["cb"], c["cf"]), ("j_l''", 0.0 * c["cb"], -np.ones_like(c["cf"]))]
    return [("mixed", c["cb"], c["cf"])]


@pytest.mark.parametrize("name", list(CASES))
def test_radial_table_against_oracle(ctx, name):
    import torch

    c = CASES[name]
    F, nsub = c["chi"].shape
    assert (name, c["lmax"], F, nsub, c["k"].size) in [("single", 0, 1, 1, 1), ("k0", 3, 2, 1, 5), ("log", 200, 3, 1, 130),
                                                      ("sub", 200, 3, 3, 70), ("turn", 3071, 2, 1, 64), ("tiny", 12, 1, 1, 8)]
    for mode, cb, cf in _modes(name):
        ref, bound = fo.radial_table_ld(c, cb, cf, tables=fo.case_tables(name))
        A = ctx.sphbessel_radial(c["k"], c["chi"], cb, cf, c["lmax"])
        got = A.cpu().numpy()
        assert got.shape == ref.shape and np.isfinite(got).all()
        err = np.abs(got.astype(LD) - ref)
        print("radial %s %s: max err / bound %.3g, max err %.3g" % (name, mode, _worst(err, bound), float(err.max())))
        assert np.all(err <= bound)
        assert torch.equal(ctx.sphbessel_radial(c["k"], c["chi"], cb, cf, c["lmax"]), A)        # the same bits again
        if name == "k0":
            # x = 0: j_0 = 1, j_0'' = -1/3, j_2'' = 2/15 and zeros, exactly
            want = [1.0, 0.0, 0.0, 0.0] if mode == "j_l" else [-1.0 / 3.0, 0.0, 2.0 / 15.0, 0.0]
            assert np.array_equal(got[:, 0, 0], np.array(want)) and np.array_equal(got[:, 1, 0], np.array(want))
    if name == "sub":
        # a padded row length: the same table, zeros behind it
        P = ctx.sphbessel_radial(c["k"], c["chi"], c["cb"], c["cf"], c["lmax"], ld_k=80)
        assert P.shape == (201, 3, 70) and P.stride() == (240, 80, 1) and torch.equal(P, A)
        full = torch.as_strided(P, (201, 3, 80), (240, 80, 1))
        assert not bool(full[:, :, 70:].any())


# ---- Gram product ------------------------------------------------------------------------------------------------------

# (lmax, F, nk); the last one has two tiles of channels
GRAM_CASES = [(3, 1, 1), (5, 3, 17), (2, 17, 130), (1, 33, 515), (0, 130, 21)]


@functools.lru_cache(maxsize=None)
def gram_inputs(shape):
    lmax, F, nk = shape
    rng = np.random.default_rng(7000 + 100 * F + nk)
    A = rng.standard_normal((lmax + 1, F, nk))
    g = rng.standard_normal(nk)                     # both signs
    C0 = rng.standard_normal((lmax + 1, F, F))
    C0 = C0 + C0.transpose(0, 2, 1)
    return A, g, C0


@pytest.mark.parametrize("shape", GRAM_CASES)
def test_gram_against_longdouble_sum(ctx, shape):
    import torch

    lmax, F, nk = shape
    A, g, C0 = gram_inputs(shape)
    assert nk == 1 or (g.min() < 0 < g.max())
    dA, dg = ctx.to_device(A), ctx.to_device(g)
    C = ctx.cl_gram(dA, dg)
    got = C.cpu().numpy()
    ref, S = fo.gram_ld(A, g)
    err, bound = np.abs(got.astype(LD) - ref), fo.gram_bound(S, nk)
    print("gram %r: max err / bound %.3g" % (shape, _worst(err, bound)))
    assert np.isfinite(got).all() and np.all(err <= bound)
    assert torch.equal(C, C.transpose(1, 2))                               # symmetric bit for bit
    assert torch.equal(ctx.cl_gram(dA, dg), C)
    # accumulate onto a non-zero C
    acc = ctx.to_device(C0)
    out = ctx.cl_gram(dA, dg, out=acc, accumulate=True)
    assert out is acc
    got = acc.cpu().numpy()
    ref, S = fo.gram_ld(A, g, C0)
    err, bound = np.abs(got.astype(LD) - ref), fo.gram_bound(S, nk)
    print("gram %r accumulate: max err / bound %.3g" % (shape, _worst(err, bound)))
    assert np.all(err <= bound) and torch.equal(acc, acc.transpose(1, 2))
    # a padded row length gives the same bits
    wide = torch.full((lmax + 1, F, nk + 5), float("nan"), dtype=torch.float64, device=ctx.device)
    wide[:, :, :nk] = dA
    assert torch.equal(ctx.cl_gram(wide[:, :, :nk], dg), C)


@pytest.mark.parametrize("F,sub", [(5, [1, 3]), (130, [0, 5, 127, 128, 129])])
def test_gram_channel_subset_has_the_bits_of_the_full_call(ctx, F, sub):
    import torch

    rng = np.random.default_rng(99 + F)
    A = rng.standard_normal((3, F, 75))
    g = rng.standard_normal(75)
    dA, dg = ctx.to_device(A), ctx.to_device(g)
    full = ctx.cl_gram(dA, dg)
    part = ctx.cl_gram(dA[:, sub].contiguous(), dg)
    idx = torch.as_tensor(sub, device=ctx.device)
    assert torch.equal(part, full[:, idx][:, :, idx])


# ---- driver ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("chunk", [16, 48, 33, 1000])
def test_driver_in_chunks(ctx, chunk):
    import torch

    c = CASES["sub"]
    nk = c["k"].size
    assert chunk > nk or nk % chunk != 0
    g = np.random.default_rng(5).standard_normal(nk)
    A, B = fo.radial_table_ld(c, tables=fo.case_tables("sub"))
    ref, S = fo.gram_ld(A, g)
    bound = fo.gram_bound(S, nk) + fo.gram_table_bound(A, B, g)
    C = ctx.clarray_fullsky(c["k"], g, c["chi"], c["cb"], c["cf"], c["lmax"], nk_chunk=chunk)
    got = C.cpu().numpy()
    err = np.abs(got.astype(LD) - ref)
    print("driver chunk %d: max err / bound %.3g" % (chunk, _worst(err, bound)))
    assert np.isfinite(got).all() and np.all(err <= bound)
    assert torch.equal(C, C.transpose(1, 2))
    assert torch.equal(ctx.clarray_fullsky(c["k"], g, c["chi"], c["cb"], c["cf"], c["lmax"], nk_chunk=chunk), C)
    # the byte budget picks the chunk: 201 x 3 x 8 bytes a column
    assert ctx.clarray_fullsky_chunk(200, 3, nk, max_bytes=201 * 3 * 8 * 40) == 32
    assert ctx.clarray_fullsky_chunk(200, 3, nk, max_bytes=1) == 16 and ctx.clarray_fullsky_chunk(200, 3, nk) == 80
    assert torch.equal(ctx.clarray_fullsky(c["k"], g, c["chi"], c["cb"], c["cf"], c["lmax"], max_bytes=201 * 3 * 8 * 40),
                       ctx.clarray_fullsky(c["k"], g, c["chi"], c["cb"], c["cf"], c["lmax"], nk_chunk=32))


# ---- model -------------------------------------------------------------------------------------------------------------

KSTAR, KMAX, LMAX = 0.02, 0.14, 40
REDSHIFTS = np.array([0.8, 1.0, 1.3])


def _oracle_cl(model, z, lmax=LMAX):
    """(C [lmax + 1, nz, nz] longdouble, bound) of the model's definition on the oracle's grid for the redshifts z."""
    chi, pfd, f, b = model._z_quantities(z)
    k, w = fo.fullsky_grid(chi.max(), KMAX, 4)
    g = fo.trapezoid_g(fo.toy_ps(KSTAR), k, w)
    case = dict(lmax=lmax, k=k, chi=chi[:, None], cb=(pfd * b)[:, None], cf=(pfd * f)[:, None])
    A, B = fo.radial_table_ld(case)
    C, S = fo.gram_ld(A, g)
    # (+ 4 u S: g and the coefficients are formed on the host by the model, in its own order)
    return C, fo.gram_bound(S, k.size) + fo.gram_table_bound(A, B, g) + 4 * U * S


def _models():
    from cora_amd.signal import corr, corr21cm
    from cora_amd.util import constants

    rc = corr.RedshiftCorrelation(ps_vv=fo.toy_ps(KSTAR), redshift=0.0)
    cr = corr21cm.Corr21cm(ps=fo.toy_ps(KSTAR), redshift=0.0)
    rc.fullsky_kmax = cr.fullsky_kmax = KMAX
    return [("RedshiftCorrelation", rc, lambda z: z, {}), ("Corr21cm", cr, lambda z: constants.nu21 / (1.0 + z), {})]


@pytest.mark.parametrize("which", [0, 1])
def test_model_at_broadcast_points(ctx, which):
    name, model, coord, _ = _models()[which]
    from cora_amd.util import constants

    x = coord(REDSHIFTS)                        # redshift, or frequency for Corr21cm
    zz = REDSHIFTS if which == 0 else constants.nu21 / x - 1.0
    ref, bound = _oracle_cl(model, zz)
    l = np.arange(LMAX + 1)
    got = model.angular_powerspectrum_full(l[:, None, None], x[None, :, None], x[None, None, :], kmax=KMAX)
    assert got.shape == (LMAX + 1, 3, 3) and np.isfinite(got).all()
    err = np.abs(got.astype(LD) - ref)
    print("%s points: max err / bound %.3g, max err / max |C| %.3g" % (name, _worst(err, bound),
                                                                         float(err.max() / np.abs(ref).max())))
    assert np.all(err <= bound)
    # a scalar in, a float out; a few scattered points give the same numbers as the full block's entries
    one = model.angular_powerspectrum_full(7, x[0], x[2], kmax=KMAX)
    assert isinstance(one, float)
    pts = model.angular_powerspectrum_full(np.array([7, 0, 40]), x[[0, 1, 2]], x[[2, 1, 0]], kmax=KMAX)
    assert pts.shape == (3,) and abs(one - float(ref[7, 0, 2])) <= bound[7, 0, 2]
    assert np.all(np.abs(pts.astype(LD) - ref[[7, 0, 40], [0, 1, 2], [2, 1, 0]]) <= bound[[7, 0, 40], [0, 1, 2], [2, 1, 0]])


@pytest.mark.parametrize("which", [0, 1])
def test_clarray_averages_before_the_product(ctx, which):
    """clarray(aps_full, zromb = 1) against the Romberg reduction of the pointwise values on the F x 3 grid."""
    from cora_amd.core import skysim
    from cora_amd.util import constants

    name, model, coord, _ = _models()[which]
    x = coord(REDSHIFTS)
    got = skysim.clarray(model.angular_powerspectrum_full, LMAX, x, zromb=1)
    # the sub-samples clarray takes: the channel centre -/+ half the spacing of the first two sorted channels
    xs = np.sort(x)
    half = abs(xs[1] - xs[0]) / 2.0
    xa = (x[:, None] + np.linspace(-half, half, 3)[None, :]).ravel()
    za = xa if which == 0 else constants.nu21 / xa - 1.0
    C, bound = _oracle_cl(model, za)
    w = skysim.romberg_weights(1).astype(LD)
    W = np.einsum("a,b->ab", w, w)
    ref = np.einsum("ab,liajb->lij", W, C.reshape(LMAX + 1, 3, 3, 3, 3))
    rb = np.einsum("ab,liajb->lij", np.abs(W).astype(np.float64), bound.reshape(LMAX + 1, 3, 3, 3, 3))
    rb = rb + 12 * U * np.einsum("ab,liajb->lij", np.abs(W).astype(np.float64), np.abs(C).astype(np.float64).reshape(LMAX + 1, 3, 3, 3, 3))
    assert got.shape == (LMAX + 1, 3, 3) and np.isfinite(got).all()
    err = np.abs(got.astype(LD) - ref)
    print("%s clarray: max err / bound %.3g, max err / max |C| %.3g" % (name, _worst(err, rb), float(err.max() / np.abs(ref).max())))
    assert np.all(err <= rb)
    assert np.array_equal(got, got.transpose(0, 2, 1))
    # and it is not the flat-sky table model
    assert model._clarray_plan(model.angular_powerspectrum_full)["kind"] == "fullsky"


# ---- poison ------------------------------------------------------------------------------------------------------------

def test_entry_points_on_poisoned_memory(ctx):
    import torch

    c = CASES["sub"]
    g = np.random.default_rng(5).standard_normal(c["k"].size)
    dk, dg = ctx.to_device(c["k"]), ctx.to_device(g)
    dchi, dcb, dcf = (ctx.to_device(c[n]) for n in ("chi", "cb", "cf"))
    A = ctx.sphbessel_radial(dk, dchi, dcb, dcf, c["lmax"]).clone()

    def radial():
        P = ctx.sphbessel_radial(dk, dchi, dcb, dcf, c["lmax"], ld_k=75)
        return torch.as_strided(P, (201, 3, 75), (225, 75, 1))             # the padding columns too

    ref, _ = _poison.poisoned_runs(ctx, radial, label="sphbessel_radial")
    assert torch.equal(ref[0][:, :, :70], A) and not bool(ref[0][:, :, 70:].any())
    ref, _ = _poison.poisoned_runs(ctx, lambda: ctx.cl_gram(A, dg), label="cl_gram")
    assert torch.equal(ref[0], ctx.cl_gram(A, dg))
    ref, _ = _poison.poisoned_runs(ctx, lambda: ctx.clarray_fullsky(dk, dg, dchi, dcb, dcf, c["lmax"], nk_chunk=48),
                                   label="clarray_fullsky")
    assert torch.equal(ref[0], ctx.clarray_fullsky(dk, dg, dchi, dcb, dcf, c["lmax"], nk_chunk=48))
