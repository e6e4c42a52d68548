"""Host checks of the LSS chain (csrc/lsschain.hip, cora_amd.signal.lss / lssutil): the numpy oracle
(tests/_lsschain_oracle.py) and the package's host functions against the outputs of the reference itself
(tests/golden/lsschain_vectors.npz, written by tests/golden/make_golden_lsschain.py), and argument checking."""
import os

import numpy as np
import pytest

import _lsschain_oracle as lo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = np.finfo(np.float64).eps


@pytest.fixture(scope="module")
def gv():
    g = dict(np.load(os.path.join(ROOT, "tests", "golden", "lsschain_vectors.npz")))
    q = float(g["q"])
    for k in ("chi", "sigmaP", "D", "phi", "delta", "f3", "b1", "b2", "fr", "map"):
        g[k] = g[k + "_q"].astype(np.float64) * q
    return g


def _rel(a, b):
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), np.finfo(np.float64).tiny)))


def test_oracle_diff2_equals_golden(gv):
    assert np.array_equal(lo.diff2(gv["phi"], gv["chi"], axis=0), gv["diff2_2d"])
    assert np.array_equal(lo.diff2(gv["f3"], gv["chi"], axis=1), gv["diff2_3d"])


def test_oracle_process_formulas_equal_golden(gv):
    D, b1, b2 = gv["D"], gv["b1"], gv["b2"]
    assert np.array_equal(lo.biased_field(gv["delta"], D, b1), gv["bias_b1"])
    bias = lo.biased_field(gv["delta"], D, b1, b2)
    assert np.array_equal(bias, gv["bias_b1b2"])
    assert np.array_equal(lo.biased_field(gv["delta"], D, b1, b2, lognormal=True), gv["bias_b1b2_lognormal"])
    assert np.array_equal(lo.linear_dynamics(gv["phi"], gv["delta"], bias, gv["chi"], D), gv["linear_real"])
    assert np.array_equal(lo.linear_dynamics(gv["phi"], gv["delta"], bias, gv["chi"], D, gv["fr"]), gv["linear_rsd"])
    assert np.array_equal(lo.lognormal_transform(gv["delta"], axis=1), gv["lognormal_axis1"])
    assert np.array_equal(lo.lognormal_transform(gv["delta"], axis=None), gv["lognormal_none"])
    # K itself to 4 eps (next test); the product with the golden's own K exactly
    assert np.array_equal(np.matmul(gv["fog_K"], gv["linear_rsd"]), gv["fog_2d"])
    got = lo.fingers_of_god(gv["map"], gv["chi"], gv["sigmaP"], D, float(gv["alpha_fog"]))
    tol = (12 + 2) * EPS * (np.abs(gv["fog_K"]) @ np.abs(gv["map"]).reshape(12, -1)).reshape(got.shape)
    assert np.all(np.abs(got - gv["fog_map"]) <= tol)


def test_width_and_fog_kernel_match_golden(gv):
    from cora_amd.signal import lssutil

    worst = 0.0
    for mod in (lo, lssutil):
        worst = max(worst, _rel(mod.calculate_width(gv["chi"]), gv["width"]))
        worst = max(worst, _rel(mod.exponential_FoG_kernel(gv["chi"], 1.93, 1.0), gv["fog_scalar"]))
        worst = max(worst, _rel(mod.exponential_FoG_kernel(gv["chi"], gv["sigmaP"], gv["D"]), gv["fog_array"]))
        worst = max(worst, _rel(mod.exponential_FoG_kernel(np.linspace(1800.0, 2400.0, 128), 1.93, 1.0), gv["fog_128"]))
        worst = max(worst, _rel(mod.exponential_FoG_kernel(gv["chi"], float(gv["alpha_fog"]) * gv["sigmaP"], gv["D"]),
                                gv["fog_K"]))
    print("calculate_width / exponential_FoG_kernel: worst relative difference %.3g (bound %.3g)" % (worst, 4 * EPS))
    assert worst <= 4 * EPS


def test_diff2_coefficients_in_kernel_order_equal_golden(gv):
    from cora_amd._lib import Context

    coef, first = Context.diff2_coefficients(gv["chi"])
    assert coef.shape == (12, 4) and np.array_equal(first, np.clip(np.arange(12) - 2, 0, 8))
    assert np.array_equal(lo.diff2_kernel_order(coef, first, gv["phi"]), gv["diff2_2d"])
    f3 = np.moveaxis(gv["f3"], 1, 0).reshape(12, -1)
    got = np.moveaxis(lo.diff2_kernel_order(coef, first, f3).reshape(12, 5, 7), 0, 1)
    assert np.array_equal(got, gv["diff2_3d"])
    # 4 and 5 points: every row is an edge row or the single interior row
    for n in (4, 5):
        x = gv["chi"][:n]
        c, fi = Context.diff2_coefficients(x)
        assert np.array_equal(lo.diff2_kernel_order(c, fi, gv["phi"][:n]), lo.diff2(gv["phi"][:n], x, axis=0))


def test_slice_mix_ranges():
    from cora_amd._lib import Context

    n = 37
    K = np.zeros((n, n))
    K[np.arange(n), np.arange(n)] = 1.0
    K[np.arange(1, n), np.arange(n - 1)] = 0.5
    K[np.arange(n - 1), np.arange(1, n)] = 0.25
    Kc, r = Context.slice_mix_ranges(K)
    assert Kc is not None and r.dtype == np.int32 and r.tolist() == [[0, 20], [12, 36], [28, 40]]
    K[16:32] = 0.0
    assert Context.slice_mix_ranges(K)[1].tolist() == [[0, 20], [0, 0], [28, 40]]
    K[:] = 0.0
    K[3, n - 1] = 1.0
    assert Context.slice_mix_ranges(K)[1].tolist() == [[36, 40], [0, 0], [0, 0]]
    # band_cut zeroes relative to the row maximum, in a copy
    K = np.full((4, 4), 1e-20) + np.eye(4)
    Kc, r = Context.slice_mix_ranges(K, band_cut=1e-18)
    assert np.array_equal(Kc, np.eye(4) * (1 + 1e-20)) and K[0, 1] == 1e-20 and r.tolist() == [[0, 4]]


def test_value_errors(gv):
    from cora_amd._lib import Context
    from cora_amd.signal import lss, lssutil

    with pytest.raises(ValueError):
        Context.diff2_coefficients(gv["chi"][:3])
    with pytest.raises(ValueError):
        lssutil.diff2(gv["phi"][:3], gv["chi"][:3], axis=0)                   # n < 4
    with pytest.raises(ValueError):
        lssutil.diff2(gv["phi"], gv["chi"][:-1], axis=0)                      # x does not match the axis
    with pytest.raises(ValueError):
        lssutil.lognormal_transform(gv["delta"], axis=0)                      # unsupported axis
    with pytest.raises(ValueError):
        lssutil.lognormal_transform(gv["f3"], axis=1)                         # not the last axis of a 2-D field
    with pytest.raises(ValueError, match="Given output array is incompatible."):
        lssutil.lognormal_transform(gv["delta"], out=np.zeros((12, 47)), axis=1)
    with pytest.raises(ValueError, match="Given output array is incompatible."):
        lssutil.lognormal_transform(gv["delta"], out=np.zeros((12, 48), dtype=np.float32))
    with pytest.raises(ValueError):
        lssutil.exponential_FoG_kernel(gv["chi"], gv["sigmaP"][:-1], 1.0)
    with pytest.raises(ValueError):
        lss.linear_dynamics(gv["phi"][:3], gv["delta"][:3], gv["delta"][:3], gv["chi"][:3], gv["D"][:3])   # n < 4
    with pytest.raises(ValueError):
        lss.linear_dynamics(gv["phi"], gv["delta"][:, :-1], gv["delta"], gv["chi"], gv["D"])
    with pytest.raises(ValueError):
        lss.biased_field(gv["delta"], gv["D"][:-1], gv["b1"])
    with pytest.raises(ValueError):
        lss.biased_field(gv["delta"][0], gv["D"], gv["b1"])
    with pytest.raises(ValueError):
        lss.fingers_of_god(gv["delta"], gv["chi"][:-1], 1.93)
    with pytest.raises(ValueError):
        lss.fingers_of_god(gv["delta"][0], gv["chi"], 1.93)
    assert lss.fingers_of_god(gv["delta"], gv["chi"], 1.93, alpha_FoG=0.0) is gv["delta"]
