"""K1 (csrc/clarray.hip) against the host oracle of tests/_clarray_oracle.py, element by element: every call goes
through the public entry points with SYNTHETIC tables (random O(1) entries of both signs, so that no part of the output
is small enough to hide an error) and every test asserts |got - reference| / bound <= 1 with the pointwise bound derived
in the oracle.  The cases are the smallest that reach each path of clarray21_kernel; that they do is asserted from the
kernel's own predicates (oracle.expect) before the kernel runs:

  interior_z{3,5,9}     all_fast, the row-major build, nsp = 2, the one clamped lane (the l = 0 sentinel)
  interior_z{1,2,4,17}  ZINT = 0 (run-time zint), fast interpolation over the generic build
  top_clamped           the high clamp, slot nkperp in the generic build, not fast with a compiled ZINT
  top_fast_slot(_odd)   all_fast with xhi == nkperp and the slot READ (x in [nkperp - 1, nkperp - 1e-5]); nkperp 40, 41
  top_fast_below        all_fast with xhi == nkperp, last multipole in the last table interval
  low_clamp             the low clamp for l >= 1
  kpar_edge             y0 = nkpar - 2, wy = 1 next to pairs inside the table and at separation 0
  nsp0 / nsp32          no early entry (range starting at l = 200) / the cap (511-row table, xscale = 170)
  few_l{0,5}_nl{1,2,3}  one to three multipoles: a dense part of a single entry (nsp = n - 1; nsp >= n cannot happen)
  two_launches          nl = 2400: the second launch, l_base = 2304
  guard_2305/2049       one multipole in the second launch / the ninth-multipole lane
  layout_F*             band enumeration, tail rows, finish and mirror kernels at F = 1 .. 100

Worst |got - reference| / bound on an MI355X (n = 2 zint + 21, K_X = 16 with LOG10_ULP = 3 assumed, K_Y = 4):
  interior_z3 0.111  z5 0.100  z9 0.033  z1 0.180  z2 0.213  z4 0.061  z17 0.039
  top_clamped 0.248  top_fast_slot 0.088  top_fast_slot_odd 0.034  top_fast_below 0.034  low_clamp 0.129
  kpar_edge 0.155  nsp0 0.059  nsp32 0.053  few_l0_nl1..3 0.003 0.098 0.078  few_l5_nl1..3 0.030 0.045 0.058
  two_launches 0.032  guard_2305 0.094  guard_2049 0.082
  layout_F1 .. F100 0.044 0.046 0.094 0.159 0.135 0.178 0.224; pair shards: bit-identical, hence 0.135 (F = 40), 0.178 (65)
  aps points 0.361 (0.302 among the clamped points)
  romb_reduce at most 0.215 (F = 33, zint = 3), 0 at zint = 1 (w = [1]); clarray_separable at most 0.272 (F = 33, zint = 3)
They agree with the float64 restatement on the host (tests/test_clarray_oracle_host.py) to the second digit.  With the
slot-nkperp write of the row-major build taken from row nkperp - 2 and wy left at its fraction at the k_par edge, built
once for that purpose, top_clamped, top_fast_slot, top_fast_slot_odd, kpar_edge and layout_F100 failed with ratios of
1e9 to 1e14 and the other 51 tests passed.

Run with -m gpu."""
import numpy as np
import pytest

import _clarray_oracle as co

pytestmark = pytest.mark.gpu
LD = co.LD


def _dev(ctx, c):
    d = lambda k: ctx.to_device(c[k])
    return ((d("dd"), d("dv"), d("vv"), c["kperpmin"], c["kperpmax"], c["kparmax"], d("chi"), d("pfd"), d("f"), d("b"),
             c["F"], c["zint"], d("w"), d("log10l")))


def _poison(ctx, *shape):
    """The entry points allocate their own output: a NaN-filled block of the same size, released just before, is normally what
    the caching allocator hands them - an element the kernels leave unwritten is then NaN, not the stale (and possibly
    right) result of an earlier call."""
    t = ctx.empty(shape)
    t.fill_(float("nan"))
    del t


def _clarray(ctx, c):
    _poison(ctx, c["log10l"].size, c["F"], c["F"])
    return ctx.clarray_table21cm(*_dev(ctx, c)).cpu().numpy()


def _check(name, got, what="clarray"):
    """got [nl, F, F] against the oracle of the named case: every [l, i, j] with j >= i, by its own bound."""
    c = co.case(name)
    C, B = co.reference_of(name)
    pairs = co.all_pairs(c["F"])
    assert got.shape == (c["log10l"].size, c["F"], c["F"]) and np.all(np.isfinite(got))
    up = got[:, pairs[:, 0], pairs[:, 1]].T.astype(LD)          # [npairs, nl]
    assert np.all(B > 0)
    r = np.abs(up - C) / B
    worst = float(r.max())
    p, l = np.unravel_index(int(np.argmax(r)), r.shape)
    print("%s %s: worst bound ratio %.3f at pair (%d, %d), entry %d" % (what, name, worst, pairs[p, 0], pairs[p, 1], l))
    return worst


@pytest.mark.parametrize("name", co.PATH_CASES)
def test_clarray_path_case_within_bound(ctx, name):
    co.expect(name)
    assert _check(name, _clarray(ctx, co.case(name))) <= 1.0


@pytest.mark.parametrize("F", co.LAYOUT_F)
def test_clarray_layout_within_bound_and_symmetric(ctx, F):
    """Random per-sub-sample pfd, f, b: a pair written to another pair's place is an O(1) error."""
    name = "layout_F%d" % F
    got = _clarray(ctx, co.case(name))
    assert np.array_equal(got, got.transpose(0, 2, 1))          # bitwise: the lower triangle is a copy
    assert _check(name, got) <= 1.0


@pytest.mark.parametrize("W", (2, 3, 8))
@pytest.mark.parametrize("F", (40, 65))
def test_pair_shards_bit_identical_and_within_bound(ctx, F, W):
    """W 'ranks' integrate pairs r, r + W, ... into [l block][slot][l] slabs; block q of every rank, stacked as the
    all-to-all would deliver them, finishes into C[q l_block : ...].  npairs = 820 and 2145: every W here leaves padding
    pairs (npairs % W != 0) at one of the two F at least, W = 8 at both; both F cross a band, and l_block = 7 does not
    divide nl = 40 (a short last block)."""
    import torch

    name = "layout_F%d" % F
    c = co.case(name)
    nl, lb = c["log10l"].size, 7
    assert any((G * (G + 1) // 2) % W != 0 for G in (40, 65)) and any((F * (F + 1) // 2) % V != 0 for V in (2, 3, 8))
    assert nl % lb != 0 and F > co.CL_BAND
    args = _dev(ctx, c)
    _poison(ctx, nl, F, F)
    full = ctx.clarray_table21cm(*args)
    slabs = [ctx.clarray_table21cm_pairs(*args, r, W, lb) for r in range(W)]
    parts = []
    for q in range((nl + lb - 1) // lb):
        n = min(nl, (q + 1) * lb) - q * lb
        _poison(ctx, n, F, F)
        parts.append(ctx.clarray_pairs_finish(torch.stack([slabs[r][q] for r in range(W)]), F, n))
    got = torch.cat(parts)
    assert torch.equal(got, full)
    assert _check(name, got.cpu().numpy(), "pair shards W=%d" % W) <= 1.0


def test_aps_points_within_bound(ctx):
    c = co.case("interior_z3")
    pts = co.make_points(c, 400, 5)
    cl = co.points_clamps(c, *pts[:3])
    assert all(cl[k].sum() >= 10 for k in ("x_low", "x_high", "y_high", "y_zero"))
    ref, bound = co.reference_points(c, *pts)
    d = ctx.to_device
    _poison(ctx, 400)
    got = ctx.aps_table21cm_points(d(c["dd"]), d(c["dv"]), d(c["vv"]), c["kperpmin"], c["kperpmax"], c["kparmax"],
                                   *[d(v) for v in pts]).cpu().numpy()
    assert got.shape == ref.shape and np.all(np.isfinite(got))
    r = np.abs(got.astype(LD) - ref) / bound
    print("aps points: worst bound ratio %.3f (worst clamped %.3f)" %
          (float(r.max()), float(r[cl["x_low"] | cl["x_high"] | cl["y_high"]].max())))
    assert float(r.max()) <= 1.0


def _romb_inputs(F, zint):
    rng = np.random.default_rng(1000 * F + zint)
    w = co.make_case(F + zint, F=1, zint=zint, chan=[300.0], half=0.1, log10l=co.log10l_range(1))["w"]
    return rng, w


@pytest.mark.parametrize("zint", (1, 3, 9))
@pytest.mark.parametrize("F", (1, 5, 33))
def test_romb_reduce_within_bound(ctx, F, zint):
    rng, w = _romb_inputs(F, zint)
    nl = 7
    X = rng.standard_normal((nl, F, zint, F, zint))
    val, bound = co.weighted_sum(X, w)
    _poison(ctx, nl, F, F)
    got = ctx.romb_reduce(ctx.to_device(X), nl, F, zint, ctx.to_device(w)).cpu().numpy()
    r = float((np.abs(got.astype(LD) - val) / bound).max())
    print("romb_reduce F=%d zint=%d: worst bound ratio %.3f" % (F, zint, r))
    assert r <= 1.0


@pytest.mark.parametrize("zint", (1, 3, 9))
@pytest.mark.parametrize("F", (1, 5, 33))
def test_clarray_separable_within_bound(ctx, F, zint):
    """bcov is NOT symmetric here: a transposed read shows."""
    rng, w = _romb_inputs(F, zint)
    nl = 7
    bcov = rng.standard_normal((F * zint, F * zint))
    al = rng.standard_normal(nl)
    val, bound = co.weighted_sum(bcov.reshape(1, F, zint, F, zint), w, scale=al)
    _poison(ctx, nl, F, F)
    got = ctx.clarray_separable(ctx.to_device(al), ctx.to_device(bcov), F, zint, ctx.to_device(w)).cpu().numpy()
    assert got.shape == val.shape
    r = float((np.abs(got.astype(LD) - val) / bound).max())
    print("clarray_separable F=%d zint=%d: worst bound ratio %.3f" % (F, zint, r))
    assert r <= 1.0
