"""The initial-LSS step without a GPU: the two new entry points in the header and the ctypes table, the argument checks
of ``corr_to_clarray_multi_device`` that run before any device call, ``lssutil.linspace``, and the restated CPU pipeline
(tests/_initial_lss_oracle.py) whose draw statistics say why tests/test_gpu_initial_lss.py may cap them at 5 sigma.

Observed: the blocks at chi = 1500 + 150 i are positive definite at every l; seed 1 gives |z| <= 1.46 over the eight
statistics (bound here: 3), the phi delta expectation lies 11 sigma from zero."""
import os
import re

import numpy as np
import pytest

import _corrfunc_oracle as co
import _initial_lss_oracle as io

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("xi_multi_average", "cl_blocks")


def test_new_entry_points_are_declared():
    from cora_amd import _lib

    header = open(os.path.join(ROOT, "include", "corahip.h")).read()
    minor = [line for line in header.splitlines() if line.startswith("#define CORAHIP_ABI_MINOR")]
    assert len(minor) == 1 and re.match(r"#define CORAHIP_ABI_MINOR 12\s", minor[0])
    for name in NEW:
        assert re.search(r"^int corahip_%s\(corahip_ctx \*ctx," % name, header, re.M), name
        assert re.search(r"\b%s\b" % name, minor[0]), name
        assert "corahip_" + name in _lib.SIGNATURES
        assert callable(getattr(_lib.Context, name))


def _three(kind=2):
    xs, ys, y2 = co.table(kind, "uniform64")
    return [co.interpolater(kind, xs, ys, y2), co.interpolater(kind, xs, -ys, -y2), co.interpolater(kind, xs, ys, y2)]


def test_multi_refuses_mixed_tables_before_the_device(monkeypatch):
    from cora_amd import _lib
    from cora_amd.signal import corrfunc

    def no_device():
        raise AssertionError("the device was touched")

    monkeypatch.setattr(_lib, "get_context", no_device)
    chi = np.array([1000.0, 1010.0, 1020.0])

    cs = _three()
    xs, ys, y2 = co.table(0, "uniform64")
    cs[1] = co.interpolater(0, xs, ys, y2)
    with pytest.raises(ValueError, match="function 1 differs from function 0 in kind"):
        corrfunc.corr_to_clarray_multi_device(cs, 8, chi)

    cs = _three()
    cs[2]._data = cs[2]._data.copy()
    cs[2]._data[5, 0] = np.nextafter(cs[2]._data[5, 0], np.inf)
    with pytest.raises(ValueError, match="function 2 differs from function 0 in its knots: knot 5 "):
        corrfunc.corr_to_clarray_multi_device(cs, 8, chi)

    cs = _three()
    cs[1]._data = cs[1]._data[:-1].copy()
    cs[1]._y2 = cs[1]._y2[:-1].copy()
    with pytest.raises(ValueError, match="function 1 differs from function 0 in its knots: 63, not 64"):
        corrfunc.corr_to_clarray_multi_device(cs, 8, chi)

    cs = _three()
    cs[1].x_t = 2.0
    with pytest.raises(ValueError, match="function 1 differs from function 0 in x_t: 2.0, not 1.0"):
        corrfunc.corr_to_clarray_multi_device(cs, 8, chi)

    with pytest.raises(ValueError, match="function 0 .* is not one of this package's"):
        corrfunc.corr_to_clarray_multi_device([np.cos], 8, chi)
    with pytest.raises(ValueError, match="1 to 4 correlation functions"):
        corrfunc.corr_to_clarray_multi_device(_three() + _three(), 8, chi)

    # tables that agree pass the check: kind, shared knots, stacked ordinates, one f_t each
    cs = _three()
    cs[2].f_t = 3.0
    kind, kx, ky, ky2, x_t, f_t = corrfunc.joint_spline_tables(cs)
    assert kind == 2 and kx.shape == (64,) and ky.shape == ky2.shape == (3, 64) and x_t == co.X_T
    assert np.array_equal(f_t, [co.F_T, co.F_T, 3.0]) and np.array_equal(ky[1], -ky[0])


def test_aps_needs_redshifts_or_frequencies():
    from cora_amd.signal import lss

    with pytest.raises(RuntimeError, match="Redshifts or frequencies must be specified!"):
        lss.multifrequency_aps_device({}, 16)


def test_linspace():
    from cora_amd.signal import lssutil

    assert np.array_equal(lssutil.linspace({"start": 0.5, "stop": 2.5, "num": 5}), np.linspace(0.5, 2.5, 5))
    assert np.array_equal(lssutil.linspace({"start": 0.5, "stop": 2.5, "num": 4, "endpoint": False}),
                          np.linspace(0.5, 2.5, 4, endpoint=False))
    assert np.array_equal(lssutil.linspace([400.0, 800.0, 9]), np.linspace(400.0, 800.0, 9))
    assert np.array_equal(lssutil.linspace([400.0, 800.0, 8, False]), np.linspace(400.0, 800.0, 8, endpoint=False))
    a = np.array([3.0, 1.0, 2.0])
    assert lssutil.linspace(a) is a
    for bad in ((0.0, 1.0, 3), 3.0, "0:1:3"):
        with pytest.raises(TypeError, match="linspace takes a dict, a list or an array"):
            lssutil.linspace(bad)


def test_host_pipeline_draw_statistics():
    """P(k) -> xi (nine Richardson levels, 602 knots) -> C_l -> extended blocks -> oracle mkfullsky with seed 1."""
    from oracle import skysim as osk

    corrs = io.host_correlations(100, 9)
    assert all(c._data.shape == (602, 2) for c in corrs.values())
    ext = io.host_extended(corrs, io.CHI_DRAW)
    assert ext.shape == (48, 8, 8) and np.allclose(ext, ext.transpose(0, 2, 1), rtol=1e-9, atol=0)
    assert io.is_positive_definite(ext)
    sky = osk.mkfullsky(ext, io.NSIDE, rng=np.random.default_rng(1))
    z, pd_signal = io.draw_z_scores(sky[:4], sky[4:], ext)
    print("host pipeline seed 1: z(delta^2) %s  z(phi delta) %s  phi delta expectation / sigma %s"
          % (np.round(z[0], 2), np.round(z[1], 2), np.round(pd_signal, 1)))
    assert np.all(np.abs(z) <= 3.0), z
    assert np.all(np.abs(pd_signal) > 6.0), pd_signal          # a missing or sign-flipped cross block fails the cap of 5
