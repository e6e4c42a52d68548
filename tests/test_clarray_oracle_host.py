"""The K1 oracle (tests/_clarray_oracle.py) checked on the host.  No GPU.

  * clarray21_kernel's arithmetic restated in float64 lies within HALF the bound of the extended-precision reference on
    every case tests/test_gpu_clarray.py uses (a condition, not a measurement);
  * each mutant of that restatement exceeds the bound a thousandfold on the case aimed at it, and stays inside it on a
    case that does not reach the mutated path;
  * the pair enumeration is a bijection with the band structure the finish kernel relies on;
  * paths() reports, for every named case, the branch the case was written for, and the cases together reach every
    branch of the kernel.

Worst |restatement - reference| / bound with n = 2 zint + 21, K_X = 16 (LOG10_ULP = 3), K_Y = 4, as measured here:
  interior_z3 0.109  z5 0.101  z9 0.033  z1 0.180  z2 0.213  z4 0.061  z17 0.038
  top_clamped 0.248  top_fast_slot 0.087  top_fast_slot_odd 0.029  top_fast_below 0.035  low_clamp 0.129
  kpar_edge 0.154  nsp0 0.059  nsp32 0.053  few_l0_nl1..3 0.003 0.098 0.078  few_l5_nl1..3 0.030 0.047 0.058
  two_launches 0.032  guard_2305 0.094  guard_2049 0.082  layout_F1 .. F100 0.044 0.047 0.095 0.160 0.134 0.178 0.223
  points 0.361
"""
import numpy as np
import pytest

import _clarray_oracle as co

LD = co.LD


def _ratio(got, ref, bound):
    got = np.asarray(got).astype(LD)
    assert got.shape == ref.shape and np.all(np.isfinite(got)) and np.all(bound > 0)
    return float((np.abs(got - ref) / bound).max())


# ---------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("name", co.CASE_NAMES)
def test_restatement_within_half_the_bound(name):
    C, B = co.reference_of(name)
    r = _ratio(co.kernel_restatement(co.case(name)), C, B)
    print("%s: restatement bound ratio %.3f" % (name, r))
    assert r <= 0.5


def test_points_restatement_within_half_the_bound():
    c = co.case("interior_z3")
    pts = co.make_points(c, 400, 5)
    ref, bound = co.reference_points(c, *pts)
    r = _ratio(co.points_restatement(c, *pts), ref, bound)
    print("points: restatement bound ratio %.3f" % r)
    assert r <= 0.5
    cl = co.points_clamps(c, *pts[:3])
    assert all(cl[k].sum() >= 10 for k in ("x_low", "x_high", "y_high", "y_zero")), {k: v.sum() for k, v in cl.items()}
    assert (~(cl["x_low"] | cl["x_high"] | cl["y_high"] | cl["y_zero"])).sum() >= 50


def test_reference_against_a_scalar_loop():
    """The vectorised reference against the formulas of the module written out point by point in plain Python."""
    import math

    c = co.make_case(1, F=3, zint=2, chan=[20.0, 300.0, 345.0], half=3.0, log10l=co.log10l_range(200)[::40])
    C, B = co.reference(c)
    pairs = co.all_pairs(3)
    xs = (c["nkperp"] - 1) / math.log10(c["kperpmax"] / c["kperpmin"])
    ys = c["kparmax"] / math.pi
    for p, (i, j) in enumerate(pairs):
        for li, ll in enumerate(c["log10l"]):
            tot = 0.0
            for a in range(2):
                for b in range(2):
                    za, zb = i * 2 + a, j * 2 + b
                    xc = (c["chi"][za] + c["chi"][zb]) / 2
                    x = min(max(ll * xs - math.log10(xc * c["kperpmin"]) * xs, 0.0), c["nkperp"] - 1e-5)
                    y = min(max(abs(c["chi"][zb] - c["chi"][za]) * ys, 0.0), c["nkpar"] - 1e-5)
                    x0, y0 = int(x), int(y)
                    x1, y1 = min(x0 + 1, c["nkperp"] - 1), min(y0 + 1, c["nkpar"] - 1)
                    wx, wy = x - x0, y - y0
                    look = lambda T: ((1 - wx) * ((1 - wy) * T[x0, y0] + wy * T[x0, y1]) +
                                      wx * ((1 - wy) * T[x1, y0] + wy * T[x1, y1]))
                    W = c["w"][a] * c["w"][b] * c["pfd"][za] * c["pfd"][zb] / (xc * xc * math.pi)
                    tot += W * (c["b"][za] * c["b"][zb] * look(c["dd"]) +
                                (c["f"][za] * c["b"][zb] + c["f"][zb] * c["b"][za]) * look(c["dv"]) +
                                c["f"][za] * c["f"][zb] * look(c["vv"]))
            assert abs(LD(tot) - C[p, li]) <= B[p, li], (i, j, li)


def test_points_reference_is_the_single_sub_pair_form():
    """reference() at zint = 1 is reference_points() with the coefficients of that one sub-pair."""
    c = co.case("interior_z1")
    C, B = co.reference_of("interior_z1")
    pairs = co.all_pairs(c["F"])
    i, j = pairs[:, 0], pairs[:, 1]
    nl = c["log10l"].size
    rep = lambda v: np.repeat(v, nl)
    W = c["w"][0] ** 2 * c["pfd"][i] * c["pfd"][j]
    ref, bound = co.reference_points(c, np.tile(c["log10l"], len(pairs)), rep(c["chi"][i]), rep(c["chi"][j]),
                                     rep(W * c["b"][i] * c["b"][j]),
                                     rep(W * (c["f"][i] * c["b"][j] + c["f"][j] * c["b"][i])),
                                     rep(W * c["f"][i] * c["f"][j]))
    # (the coefficient triples were rounded to float64 on the way in: three roundings of W, three of c_T)
    assert np.all(np.abs(ref.reshape(len(pairs), nl) - C) <= B)


# ---------------------------------------------------------------------------------------- mutants
AIMED = [("slot_prev_row", "top_clamped"), ("slot_prev_row", "top_fast_slot"), ("slot_prev_row", "top_fast_slot_odd"),
         ("wy_kept", "kpar_edge"), ("no_low_clamp_first", "interior_z3"), ("w_reversed_a", "interior_z3"),
         ("w_reversed_a", "interior_z9"), ("fb_partner", "interior_z3"), ("fb_partner", "layout_F33"),
         ("drop_subpair", "interior_z9"), ("drop_subpair", "interior_z17")]
BLIND = [("slot_prev_row", "top_fast_below"), ("slot_prev_row", "interior_z3"), ("wy_kept", "interior_z3"),
         ("no_low_clamp_first", "nsp0")]


@pytest.mark.parametrize("mutant,name", AIMED)
def test_mutant_exceeds_the_bound(mutant, name):
    """(A literal exchange of w[a] and w[b] in W = w_a w_b ..., or of the roles of a and b altogether, only relabels
    the double sum: the mutant is the weight of the WRONG sub-sample, w[zint - 1 - a], which the asymmetric weights of
    make_case show and true Romberg weights, being symmetric, would not.)"""
    C, B = co.reference_of(name)
    r = _ratio(co.kernel_restatement(co.case(name), mutant=mutant), C, B)
    print("%s on %s: bound ratio %.3g" % (mutant, name, r))
    assert r > 1e3


@pytest.mark.parametrize("mutant,name", BLIND)
def test_mutant_is_invisible_where_its_path_is_not_reached(mutant, name):
    """Why the aimed cases are needed: the same mutants pass on cases that do not read slot nkperp, do not take the
    k_par edge, or whose first entry needs no clamp."""
    C, B = co.reference_of(name)
    assert _ratio(co.kernel_restatement(co.case(name), mutant=mutant), C, B) <= 0.5


# ---------------------------------------------------------------------------------------- enumeration
@pytest.mark.parametrize("F", (1, 2, 31, 32, 33, 40, 64, 65, 100))
def test_pair_of_index_is_a_bijection(F):
    pairs = co.all_pairs(F)
    i, j = pairs[:, 0], pairs[:, 1]
    assert np.all((0 <= i) & (i <= j) & (j < F))
    assert len(set(map(tuple, pairs))) == F * (F + 1) // 2
    # bands of 32 diagonals, in order
    band = (j - i) // co.CL_BAND
    assert np.all(np.diff(band) >= 0)
    for B in range(band.max() + 1):
        sel = np.flatnonzero(band == B)
        n = F - co.CL_BAND * B
        nfull = n - (co.CL_BAND - 1) if n >= co.CL_BAND else 0
        assert nfull == 0 or sel[0] % 8 == 0            # a band with full rows starts at a multiple of 8: p mod 8 is its x
        full = pairs[sel[:nfull * co.CL_BAND]].reshape(nfull, co.CL_BAND, 2)
        # 32 consecutive p are the 32 separations of one row; p mod 8 = x holds the adjacent separations 4x .. 4x + 3
        assert np.all(full[:, :, 0] == np.arange(nfull)[:, None])
        d = full[:, :, 1] - full[:, :, 0] - co.CL_BAND * B
        assert np.all(np.sort(d, axis=1) == np.arange(co.CL_BAND)[None, :])
        assert np.all(d // 4 == (np.arange(co.CL_BAND) % 8)[None, :])
        tail = pairs[sel[nfull * co.CL_BAND:]]
        assert np.all(np.diff(tail[:, 0]) >= 0) and np.all(tail[:, 0] >= nfull)
        same_row = np.diff(tail[:, 0]) == 0
        assert np.all(np.diff(tail[:, 1])[same_row] == 1)                        # tail rows: i-major, j ascending


# ---------------------------------------------------------------------------------------- branch coverage
@pytest.mark.parametrize("name", co.CASE_NAMES)
def test_case_reaches_its_path(name):
    co.expect(name)


def test_cases_cover_every_branch():
    P = {n: co.paths(co.case(n)) for n in co.PATH_CASES}
    launches = [(n, p) for n in P for p in P[n]]
    hit = lambda pred: [n for n, p in launches if pred(p)]
    assert hit(lambda p: p["zint_inst"] > 0 and p["all_fast"].all())                       # all_fast, row-major build
    assert hit(lambda p: p["zint_inst"] > 0 and (~p["all_fast"]).any())                    # not fast, compiled ZINT
    assert hit(lambda p: p["zint_inst"] == 0 and p["all_fast"].all())                      # ZINT = 0 (fast interpolation)
    assert {p["zint_inst"] for _, p in launches} == {0, 3, 5, 9}
    assert hit(lambda p: (p["fast_build"] & p["xhi_top"]).any())                           # xhi == nkperp under all_fast
    assert hit(lambda p: (p["fast_build"] & p["slot_read"]).any())
    assert hit(lambda p: (~p["all_fast"] & p["slot_read"]).any())
    assert hit(lambda p: p["kpar_edge"].any())
    assert hit(lambda p: p["clamp_low_later"].any()) and hit(lambda p: p["clamp_high"].any())
    assert hit(lambda p: p["fast_build"].all() and p["clamp_low_first"].all())             # the one clamped lane of a fast launch
    nsp = {p["nsp"] for _, p in launches if p["fast_build"].all()}
    assert 0 in nsp and 32 in nsp and nsp & set(range(1, 32))
    assert hit(lambda p: p["fast_build"].all() and p["n"] - p["nsp"] == 1)                 # a dense part of one entry
    assert not hit(lambda p: p["every_individual"])                                        # (unreachable: nsp <= n - 1)
    assert hit(lambda p: p["l_base"] == co.L_LAUNCH and p["n"] > 1) and hit(lambda p: p["l_base"] == co.L_LAUNCH and p["n"] == 1)
    assert hit(lambda p: p["n"] == 2049)


def test_weighted_sum_bound_holds_for_the_kernels_order():
    rng = np.random.default_rng(3)
    for F, zint in ((1, 1), (5, 3), (33, 9)):
        c = co.make_case(F, F=F, zint=zint, chan=np.arange(F) + 300.0, half=0.2, log10l=co.log10l_range(2))
        X = rng.standard_normal((4, F, zint, F, zint))
        val, bound = co.weighted_sum(X, c["w"])
        got = np.zeros((4, F, F))
        for a in range(zint):               # the kernels' order: t over b, then s += w_a t
            t = np.zeros((4, F, F))
            for b in range(zint):
                t = t + c["w"][b] * X[:, :, a, :, b]
            got = got + c["w"][a] * t
        assert np.all(np.abs(got.astype(LD) - val) <= bound)
