"""The shot-noise step without a GPU: the new entry point in the header and the ctypes table, the redshift models,
growth functions, volumes and shot-noise standard deviations against vectors made by the reference
(tests/golden/shotnoise_vectors.npz, written by tests/golden/make_golden_shotnoise.py), and every argument check that
runs before a device call.

Bound of the comparisons: 8 ulp of the sum of the absolute terms of the expression (a handful of double operations and
one ``pow``, which may differ by an ulp between numpy builds); for a pure product that sum is the value itself."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = np.finfo(np.float64).eps


@pytest.fixture(scope="module")
def gv():
    g = dict(np.load(os.path.join(ROOT, "tests", "golden", "shotnoise_vectors.npz")))
    g["z"] = g["z_q"] * float(g["q"])
    return g


def _within(got, want, mag=None):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape
    mag = np.abs(want) if mag is None else mag
    err = np.abs(got - want)
    assert np.all(err <= 8 * EPS * mag), (err / (EPS * mag)).max()


def _no_device(monkeypatch):
    from cora_amd import _lib

    def no_device():
        raise AssertionError("the device was touched")

    monkeypatch.setattr(_lib, "get_context", no_device)


def test_new_entry_point_is_declared():
    from cora_amd import _lib

    header = open(os.path.join(ROOT, "include", "corahip.h")).read()
    minor = [line for line in header.splitlines() if line.startswith("#define CORAHIP_ABI_MINOR")]
    assert len(minor) == 1 and re.match(r"#define CORAHIP_ABI_MINOR 12\s", minor[0])
    name = "normal_rows_pcg64"
    assert re.search(r"^int corahip_%s\(corahip_ctx \*ctx," % name, header, re.M)
    assert re.search(r"\b%s\b" % name, minor[0])
    assert "corahip_" + name in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["corahip_" + name][1]) == 10
    assert callable(getattr(_lib.Context, name))


@pytest.mark.parametrize("cls_name", ["bias", "omega_HI", "sigma_P"])
def test_model_sets_match_the_reference(gv, cls_name):
    from cora_amd.signal import lssmodels

    cls = getattr(lssmodels, cls_name)
    stored = sorted(k.split("__")[1] for k in gv if k.startswith(cls_name + "__"))
    assert sorted(cls.models()) == stored
    z = gv["z"]
    for name in cls.models():
        x0, coeffs, *powers = cls._models[name]
        powers = powers[0] if powers else range(len(coeffs))
        mag = sum(np.abs(c * (z - x0) ** p) for p, c in zip(powers, coeffs))
        want = gv["%s__%s" % (cls_name, name)]
        _within(cls.evaluate(z, model=name), want, mag)
        _within(cls[name](z), want, mag)
        _within(cls.get(name)(z), want, mag)


def test_model_set_surface():
    from cora_amd.signal import lssmodels as lm

    assert lm.bias["HI"](1.0) == 0.489
    assert np.allclose(lm.bias.evaluate(np.array([0.5, 1.5]), "eboss_qso"), [0.195495, 1.309695], rtol=0, atol=5e-7)
    assert lm.omega_HI.default_model == "Crighton2015"
    z = np.array([0.5, 1.0])
    assert np.array_equal(lm.omega_HI.evaluate(z), lm.omega_HI.evaluate(z, model="Crighton2015"))
    assert np.array_equal(lm.omega_HI.get()(z), lm.omega_HI.evaluate(z))
    assert lm.PolyModelSet.evaluate_poly(2.0, 1.0, [1.0, 2.0, 3.0]) == 6.0
    assert lm.PolyModelSet.evaluate_poly(3.0, 1.0, [5.0], [2]) == 20.0
    with pytest.raises(ValueError, match="No model provided"):
        lm.bias.evaluate(z)
    with pytest.raises(ValueError, match='Model "nope" not known'):
        lm.sigma_P.get("nope")


def test_temperature_and_number_density_match_the_reference(gv):
    from cora_amd.signal import lssmodels as lm
    from cora_amd.util.cosmology import Cosmology

    c, z = Cosmology(), gv["z"]
    for name in lm.omega_HI.models():
        om = lm.omega_HI.evaluate(z, model=name)
        _within(lm.mean_21cm_temperature(c, z, om), gv["T_b__" + name])
        _within(lm.log_M_HI_g_to_n_eff(float(gv["log_M_HI_g"]), c, z, model=name), gv["n_eff__" + name])
    _within(lm.log_M_HI_g_to_n_eff(float(gv["log_M_HI_g"]), c, z), gv["n_eff__default"])
    assert np.array_equal(gv["n_eff__default"], gv["n_eff__Crighton2015"])


def test_constants_for_the_number_density():
    from cora_amd.util import constants

    assert constants.G == 6.6742e-11 and constants.solar_mass == 1.98892e30


def test_growth_functions_match_the_reference(gv):
    from cora_amd.util.cosmology import Cosmology

    c, z = Cosmology(), gv["z"]
    _within(c.growth_factor(z), gv["growth_factor"])
    _within(c.growth_factor(0), gv["growth_factor_0"])
    x = ((1.0 / c.omega_m) - 1.0) / (1.0 + z) ** 3
    num = 1.0 + 1.175 * x + 0.3064 * x**2 + 0.005355 * x**3
    den = 1.0 + 1.857 * x + 1.021 * x**2 + 0.1530 * x**3
    mag = (1.0 + 1.5 * x / (1.0 + x) + 3.0 * x * (1.175 + 0.6127 * x + 0.01607 * x**2) / num
           + 3.0 * x * (1.857 + 2.042 * x + 0.4590 * x**2) / den)
    _within(c.growth_rate(z), gv["growth_rate"], mag)
    assert np.all(np.diff(c.growth_factor(z)) < 0) and np.all((c.growth_rate(z) > 0.5) & (c.growth_rate(z) < 1))
    curved = Cosmology(omega_l=0.6)
    for fn in (curved.growth_factor, curved.growth_rate):
        with pytest.raises(RuntimeError, match="only valid in a flat universe"):
            fn(z)


def test_existing_cosmology_is_unchanged(gv):
    from cora_amd.util.cosmology import Cosmology

    c = Cosmology()
    _within(c.H(gv["z"]), gv["H"])
    assert np.allclose(c.comoving_distance(gv["z"]), gv["chi"], rtol=1e-12, atol=0)


def test_volumes_match_the_reference(gv, monkeypatch):
    from cora_amd.signal import lss

    _no_device(monkeypatch)
    # chi comes out of an ODE integrator (same scipy call as the reference's): the bound is on the expression around it
    _within(lss.differential_comoving_volume(gv["z"]), gv["dVdz"])
    for flag, key in ((False, "voxvol_fixed"), (True, "voxvol_freq")):
        nfreq, npol, ipol, scale_f, attrs = lss._flat_spectrum_plan(int(gv["nside"]), gv["freq5"], True, ("I",), None, 3.0, flag, None)
        assert (nfreq, npol, ipol) == (5, 4, [0])
        _within(attrs["voxvol_ref"], gv[key])
        assert attrs["central_redshift"] == gv["central_redshift"]
        _within(scale_f, np.ones(5) * (3.0**0.5 / gv[key] ** 0.5))
    _, _, _, scale_f, _ = lss._flat_spectrum_plan(4, gv["freq5"], True, ("I",), 2.0, None, False, None)
    assert np.array_equal(scale_f, np.full(5, 2.0**0.5))


def test_shot_noise_std_matches_the_reference(gv, monkeypatch):
    from cora_amd.signal import lss
    from cora_amd.util.cosmology import Cosmology

    _no_device(monkeypatch)
    q, nside = float(gv["q"]), int(gv["nside"])
    chi = gv["chi6_q"] * q
    _within(lss.shot_noise_std(nside, chi, np.ones(6) * 2.0**-9), gv["sn_std_scalar"])
    _within(lss.shot_noise_std(nside, chi, gv["ne6_q"] * q), gv["sn_std_slices"])
    ne = lss._shot_noise_n_eff(6, None, float(gv["log_M_HI_g"]), gv["z6_q"] * q, Cosmology(), "Crighton2015")
    _within(ne, gv["n_eff6_mass"])
    _within(lss.shot_noise_std(nside, chi, ne), gv["sn_std_mass"])
    # n_eff wins over log_M_HI_g; a scalar is spread over the slices
    assert np.array_equal(lss._shot_noise_n_eff(6, 0.25, 9.5, None, None, "Crighton2015"), np.full(6, 0.25))


def test_shot_noise_seed_is_adler32_of_the_corner():
    import zlib

    from cora_amd.signal import lss

    rng = np.random.default_rng(5)
    wide, narrow = rng.standard_normal((3, 192)), rng.standard_normal((3, 48))
    assert lss.shot_noise_seed(wide) == zlib.adler32(wide[:, :100].copy().tobytes())
    assert lss.shot_noise_seed(narrow) == zlib.adler32(narrow.tobytes())
    assert lss.shot_noise_seed(wide[:, ::-1]) == zlib.adler32(wide[:, ::-1][:, :100].copy().tobytes())


def test_polynomial_bias_precedence_and_alpha_b():
    from cora_amd.signal import lss, lssmodels

    z = np.array([0.4, 1.1, 2.0])
    # (alpha_b = 1 still goes through the statement: 1.0 * b + 1.0 - 1.0 rounds, it is not b)
    model = 1.0 * lssmodels.bias["eboss_lrg"](z) + 1.0 - 1.0
    assert np.array_equal(lss.polynomial_bias(z, model="eboss_lrg"), model)
    own = 1.0 * lssmodels.PolyModelSet.evaluate_poly(z, 0.5, [0.2, 0.3]) + 1.0 - 1.0
    assert not np.array_equal(own, model)
    # explicit coefficients win over the model; one of the pair alone does not
    assert np.array_equal(lss.polynomial_bias(z, model="eboss_lrg", z_eff=0.5, bias_coeff=[0.2, 0.3]), own)
    assert np.array_equal(lss.polynomial_bias(z, model="eboss_lrg", z_eff=0.5), model)
    assert np.array_equal(lss.polynomial_bias(z, model="eboss_lrg", bias_coeff=[0.2, 0.3]), model)
    assert np.array_equal(lss.polynomial_bias(z, model="HI", alpha_b=1.5), 1.5 * lssmodels.bias["HI"](z) + 1.5 - 1.0)
    for kw in ({}, {"z_eff": 0.5}, {"bias_coeff": [1.0]}):
        with pytest.raises(ValueError, match="Either `model` must be set, or `z_eff` and `bias_coeff`"):
            lss.polynomial_bias(z, **kw)


def test_blend_power_spectrum_end_points():
    from cora_amd.signal import lss

    k = np.logspace(-3, 1, 9)

    def lin(k):
        return 1e4 * k / (1 + (k / 0.02) ** 2.5)

    def nl(k):
        return lin(k) * (1 + (k / 0.3) ** 1.5)

    assert np.array_equal(lss.blend_power_spectrum(lin, nl, 0.0)(k), lin(k))
    assert np.array_equal(lss.blend_power_spectrum(lin, nl)(k), nl(k))
    assert np.array_equal(lss.blend_power_spectrum(lin, nl, 0.25)(k), lin(k) * (1 - 0.25) + nl(k) * 0.25)


def test_tracer_models_are_the_reference_statements(gv, monkeypatch):
    from cora_amd.signal import lss, lssmodels
    from cora_amd.util.cosmology import Cosmology

    _no_device(monkeypatch)
    c, z = Cosmology(), gv["z"]
    m = lss.tracer_models(z, bias_model="eboss_elg", alpha_b=1.25, sigma_P_model="ELG", use_mean_21cmT=True, omega_HI_model="SKA")
    assert np.array_equal(m["D"], c.growth_factor(z) / c.growth_factor(0))
    assert np.array_equal(m["f"], c.growth_rate(z)) and np.array_equal(m["fog_D"], c.growth_factor(z))
    assert np.array_equal(m["chi"], c.comoving_distance(z))
    assert np.array_equal(m["b1"], lss.polynomial_bias(z, model="eboss_elg", alpha_b=1.25))
    assert np.array_equal(m["sigmaP"], lssmodels.sigma_P["ELG"](z))
    _within(m["T_b"], gv["T_b__SKA"])
    m = lss.tracer_models(z)
    assert m["sigmaP"] is None and m["T_b"] is None


def test_validation_errors_come_before_the_device(gv, monkeypatch):
    import torch

    from cora_amd.signal import lss

    _no_device(monkeypatch)
    delta = torch.zeros((6, 192), dtype=torch.float64)
    chi = gv["chi6_q"] * float(gv["q"])
    for fn in (lss.add_correlated_shot_noise_device, lss.add_correlated_shot_noise):
        arg = delta if fn is lss.add_correlated_shot_noise_device else delta.numpy()
        with pytest.raises(RuntimeError, match="One of `n_eff` or `log_M_HI_g` must be set."):
            fn(arg, chi)
        with pytest.raises(ValueError, match="redshift"):
            fn(arg, chi, log_M_HI_g=9.5)
        with pytest.raises(ValueError):
            fn(arg, chi[:5], n_eff=1e-3)
        with pytest.raises(ValueError):
            fn(arg, chi, n_eff=np.ones(5))
    for fn in (lss.generate_flat_spectrum_map_device, lss.generate_flat_spectrum_map):
        with pytest.raises(ValueError, match="Only one of variance or P_SN can be specified."):
            fn(4, gv["freq5"])
        with pytest.raises(ValueError, match="Only one of variance or P_SN can be specified."):
            fn(4, gv["freq5"], variance=1.0, P_SN=2.0)
        with pytest.raises(RuntimeError, match="Must have full_pol=True if nonzero non-I maps are desired."):
            fn(4, gv["freq5"], full_pol=False, pol=("I", "Q"), variance=1.0)
        with pytest.raises(ValueError):
            fn(4, gv["freq5"], pol=("I", "X"), variance=1.0)
    phi = torch.zeros((6, 192), dtype=torch.float64)
    with pytest.raises(ValueError, match="dynamics must be"):
        lss.tracer_map_from_models_device(phi, delta, gv["z6_q"] * float(gv["q"]), dynamics="nbody")
    with pytest.raises(TypeError, match="unexpected keywords"):
        lss.tracer_map_from_models_device(phi, delta, gv["z6_q"] * float(gv["q"]), chi=chi)
    with pytest.raises(ValueError, match='Model "nope" not known'):
        lss.tracer_map_from_models_device(phi, delta, gv["z6_q"] * float(gv["q"]), bias_model="nope")


def test_row_off_bounds_are_checked_on_the_host():
    import torch

    from cora_amd import _lib

    out = torch.zeros((3, 4, 10), dtype=torch.float64)
    scale = np.ones(3)
    ok = np.array([0, 40, 110], dtype=np.int64)
    nrow, ro = _lib.Context.check_rows(scale, 10, out, ok)
    assert nrow == 3 and ro.dtype == np.int64 and np.array_equal(ro, ok)
    assert _lib.Context.check_rows(scale, 40, out, None) == (3, None)
    for bad in ([0, 40, 111], [0, -1, 50], [120, 0, 10]):
        with pytest.raises(ValueError, match="would leave out"):
            _lib.Context.check_rows(scale, 10, out, np.array(bad, dtype=np.int64))
    with pytest.raises(ValueError, match="3 rows of 41 need 123"):
        _lib.Context.check_rows(scale, 41, out, None)
    with pytest.raises(ValueError, match="row_off must be 3 integers"):
        _lib.Context.check_rows(scale, 10, out, np.array([0, 40]))
    with pytest.raises(ValueError, match="row_off must be 3 integers"):
        _lib.Context.check_rows(scale, 10, out, np.array([0.0, 40.0, 80.0]))
    with pytest.raises(ValueError, match="one value per row"):
        _lib.Context.check_rows(np.ones((3, 1)), 10, out, None)
    with pytest.raises(ValueError, match="contiguous float64"):
        _lib.Context.check_rows(scale, 10, out.to(torch.float32), None)
    # the method itself refuses before it uses the context (an object without one)
    with pytest.raises(ValueError, match="would leave out"):
        _lib.Context.normal_rows_pcg64(object.__new__(_lib.Context), 1, 1, scale, 10, out, row_off=[0, 40, 111])


def test_normal_rows_device_wants_a_generator(monkeypatch):
    import torch

    from cora_amd.util import nputil

    _no_device(monkeypatch)
    out = torch.zeros((2, 8), dtype=torch.float64)
    for rng in (None, 5, np.random.RandomState(1)):
        with pytest.raises(TypeError, match="numpy.random.Generator"):
            nputil.normal_rows_device(rng, np.ones(2), 8, out)
