"""Correlated shot noise on the GPU: ``corahip_normal_rows_pcg64`` and everything built on it against numpy itself.

Every comparison is ``np.array_equal`` on the uint64 view against ``Generator.normal`` of an identically seeded
generator: no tolerance.  Standard deviations and voxel volumes come from tests/golden/shotnoise_vectors.npz (made by
the reference, tests/golden/make_golden_shotnoise.py)."""
import os
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (nrow, ncol, skip): where the (ordinal -> row, column) sink can go wrong
CASES = [
    (1, 1, 0),                       # smallest
    (3, 1, 1),                       # ncol of 1
    (1000, 3, 0),                    # many field rows inside one 64-lane row
    (5, 63, 3), (4, 64, 0), (7, 65, 1),          # around the 64-lane row width
    (12, 48, 0),                     # nside 2
    (9, 1023, 0), (2, 1025, 2),      # a block edge inside a row
    (5, 4097, 0),                    # several blocks per row
    (16, 12288, 1),                  # nside 32: 1.97e5 values, which hold wedge and tail samples
    (1, 3 * 4096 * 64 + 5, 0),       # one long row
]


@pytest.fixture(scope="module")
def gv():
    g = dict(np.load(os.path.join(ROOT, "tests", "golden", "shotnoise_vectors.npz")))
    g["z"] = g["z_q"] * float(g["q"])
    return g


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same(got, want):
    got = got.cpu().numpy() if hasattr(got, "cpu") else np.asarray(got)
    assert got.shape == np.shape(want)
    return np.array_equal(_bits(got), _bits(want))


def _pair(seed, skip=0, kind=np.random.PCG64):
    a, b = np.random.Generator(kind(seed)), np.random.Generator(kind(seed))
    if skip:
        a.standard_normal(skip)
        b.standard_normal(skip)
    return a, b


def _state_eq(a, b):
    """bit generator states, which hold arrays for SFC64 and Philox"""
    if isinstance(a, dict):
        return isinstance(b, dict) and a.keys() == b.keys() and all(_state_eq(a[k], b[k]) for k in a)
    return bool(np.array_equal(a, b))


def _scales(nrow, seed):
    return np.random.default_rng(1000 + seed).uniform(0.25, 4.0, nrow) * 2.0 ** np.random.default_rng(seed).integers(-20, 20, nrow)


@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("nrow,ncol,skip", CASES)
def test_entry_point_equals_numpy(ctx, nrow, ncol, skip, accumulate):
    from cora_amd import _lib
    from cora_amd.util import nputil

    rng, ref_rng = _pair(20261020 + ncol, skip)
    s = _scales(nrow, ncol)
    ref = ref_rng.normal(scale=s[:, None], size=(nrow, ncol))
    if accumulate:
        base = np.random.default_rng(7).standard_normal((nrow, ncol))
        out = ctx.to_device(base)
        want = base + ref
    else:
        out = ctx.to_device(np.full((nrow, ncol), np.nan))
        want = ref
    # the entry point itself: the raw-draw count leads to numpy's state
    st = rng.bit_generator.state["state"]
    probe = out.clone()
    n_raw = ctx.normal_rows_pcg64(st["state"], st["inc"], s, ncol, probe, accumulate=accumulate)
    assert _same(probe, want)
    assert _lib.pcg64_advance(st["state"], st["inc"], n_raw) == ref_rng.bit_generator.state["state"]["state"]
    # and through the generator
    assert nputil.normal_rows_device(rng, s, ncol, out, accumulate=accumulate) is out
    assert _same(out, want)
    assert _state_eq(rng.bit_generator.state, ref_rng.bit_generator.state)


def test_row_off_scatters_rows_and_touches_nothing_else(ctx):
    from cora_amd.util import nputil

    nrow, ncol = 11, 777
    rng, ref_rng = _pair(31, 2)
    s = _scales(nrow, 5)
    ref = ref_rng.normal(scale=s[:, None], size=(nrow, ncol))
    plane = np.array([2, 0, 3, 1, 1, 3, 0, 2, 2, 1, 0])
    row_off = (np.arange(nrow) * 4 + plane) * ncol
    out = ctx.to_device(np.full((nrow, 4, ncol), np.nan))
    nputil.normal_rows_device(rng, s, ncol, out, row_off=row_off)
    got = out.cpu().numpy()
    assert _same(got[np.arange(nrow), plane], ref)
    mask = np.ones((nrow, 4), dtype=bool)
    mask[np.arange(nrow), plane] = False
    assert np.isnan(got[mask]).all()
    assert _state_eq(rng.bit_generator.state, ref_rng.bit_generator.state)
    bad = row_off.copy()
    bad[5] += 1                                                 # plane 3 of row 5: one element past ... the next row's plane 0
    bad[10] = out.numel() - ncol + 1                            # one element past the end of out
    with pytest.raises(ValueError, match=r"row_off\[10\] = .* would leave out"):
        nputil.normal_rows_device(rng, s, ncol, out, row_off=bad)
    assert _state_eq(rng.bit_generator.state, ref_rng.bit_generator.state)


def test_zero_scale_gives_positive_zero(ctx):
    from cora_amd.util import nputil

    nrow, ncol = 6, 200
    rng, ref_rng = _pair(17)
    s = np.array([1.5, 0.0, 2.0, 0.0, 0.0, 3.0])
    ref = ref_rng.normal(scale=s[:, None], size=(nrow, ncol))
    assert not np.signbit(ref[[1, 3, 4]]).any()                  # numpy: 0.0 + scale * z = +0.0 whatever the sign of z
    out = ctx.to_device(np.full((nrow, ncol), np.nan))
    nputil.normal_rows_device(rng, s, ncol, out)
    got = out.cpu().numpy()
    assert _same(got, ref)
    assert not np.signbit(got[[1, 3, 4]]).any() and (got[[1, 3, 4]] == 0).all()
    assert _state_eq(rng.bit_generator.state, ref_rng.bit_generator.state)


def test_larger_case_accumulates_bit_equal(ctx):
    from cora_amd.util import nputil

    nrow, ncol = 24, 786432                                  # nside 256: tail samples across block and tile boundaries
    rng, ref_rng = _pair(256, 1)
    s = _scales(nrow, 9)
    want = np.random.default_rng(3).standard_normal((nrow, ncol))
    out = ctx.to_device(want)
    want += ref_rng.normal(scale=s[:, None], size=(nrow, ncol))
    nputil.normal_rows_device(rng, s, ncol, out, accumulate=True)
    assert _same(out, want)
    assert _state_eq(rng.bit_generator.state, ref_rng.bit_generator.state)


def _field(seed, n, npix):
    return np.random.default_rng(seed).standard_normal((n, npix))


@pytest.mark.parametrize("how", ["scalar", "slices", "mass"])
def test_add_correlated_shot_noise(ctx, gv, how):
    from cora_amd.signal import lss

    q, nside = float(gv["q"]), int(gv["nside"])
    chi, z6 = gv["chi6_q"] * q, gv["z6_q"] * q
    kw, std = {
        "scalar": (dict(n_eff=2.0**-9), gv["sn_std_scalar"]),
        "slices": (dict(n_eff=gv["ne6_q"] * q), gv["sn_std_slices"]),
        "mass": (dict(log_M_HI_g=float(gv["log_M_HI_g"]), redshift=z6), gv["sn_std_mass"]),
    }[how]
    delta = _field(41, 6, 12 * nside * nside)
    rng, ref_rng = _pair(77, 1)
    d = ctx.to_device(delta)
    assert lss.add_correlated_shot_noise_device(d, chi, rng=rng, **kw) is d
    assert _same(d, delta + ref_rng.normal(scale=std[:, np.newaxis], size=delta.shape))
    assert _state_eq(rng.bit_generator.state, ref_rng.bit_generator.state)
    # the numpy in/out form, seeded
    got = lss.add_correlated_shot_noise(delta, chi, seed=5, **kw)
    assert _same(got, delta + np.random.default_rng(5).normal(scale=std[:, np.newaxis], size=delta.shape))


def test_shot_noise_seed_comes_from_the_field(ctx, gv):
    from cora_amd.signal import lss

    q, nside = float(gv["q"]), int(gv["nside"])
    chi, std = gv["chi6_q"] * q, gv["sn_std_scalar"]
    delta, other = _field(42, 6, 12 * nside * nside), _field(43, 6, 12 * nside * nside)
    seed = zlib.adler32(delta[:, :100].copy().tobytes())
    assert lss.shot_noise_seed(ctx.to_device(delta)) == seed
    d = lss.add_correlated_shot_noise_device(ctx.to_device(delta), chi, n_eff=2.0**-9)
    assert _same(d, delta + np.random.default_rng(seed).normal(scale=std[:, np.newaxis], size=delta.shape))
    seed2 = zlib.adler32(other[:, :100].copy().tobytes())
    assert seed2 != seed
    d = lss.add_correlated_shot_noise_device(ctx.to_device(delta), chi, n_eff=2.0**-9, seed_from=ctx.to_device(other))
    assert _same(d, delta + np.random.default_rng(seed2).normal(scale=std[:, np.newaxis], size=delta.shape))


@pytest.mark.parametrize("case", ["variance", "psn_fixed", "psn_freq", "iqu", "single"])
def test_generate_flat_spectrum_map(ctx, gv, case):
    from cora_amd.signal import lss

    nside, freq = int(gv["nside"]), gv["freq5"]
    npix, nfreq = 12 * nside * nside, len(freq)
    kw = {
        "variance": dict(variance=2.5),
        "psn_fixed": dict(P_SN=300.0),
        "psn_freq": dict(P_SN=300.0, use_freq_dependent_voxel_volume=True),
        "iqu": dict(P_SN=300.0, use_freq_dependent_voxel_volume=True, pol=("I", "Q", "U"), full_pol=True),
        "single": dict(variance=2.5, full_pol=False),
    }[case]
    freq_dep = kw.get("use_freq_dependent_voxel_volume", False)
    voxvol = gv["voxvol_freq"] if freq_dep else gv["voxvol_fixed"]
    # GenerateFlatSpectrumMap.process, the statements that set the scale
    if "variance" in kw:
        scale = kw["variance"] ** 0.5
    else:
        scale = kw["P_SN"] ** 0.5
        if freq_dep:
            scale = scale / voxvol[:, np.newaxis, np.newaxis] ** 0.5
        else:
            scale /= voxvol**0.5
    ipol = ["IQUV".index(p) for p in kw.get("pol", ("I",))]
    npol = 4 if kw.get("full_pol", True) else 1
    rng, ref_rng = _pair(91, 3)
    ref = ref_rng.normal(scale=scale, size=(nfreq, len(ipol), npix))
    m, attrs = lss.generate_flat_spectrum_map_device(nside, freq, rng=rng, **kw)
    got = m.cpu().numpy()
    assert got.shape == (nfreq, npol, npix)
    assert _same(got[:, ipol, :], ref)
    rest = [p for p in range(npol) if p not in ipol]
    assert (_bits(got[:, rest, :]) == 0).all()                  # exactly +0.0
    assert _state_eq(rng.bit_generator.state, ref_rng.bit_generator.state)
    assert set(attrs) == {"voxvol_ref", "central_redshift"}
    assert np.array_equal(attrs["voxvol_ref"], voxvol) and attrs["central_redshift"] == gv["central_redshift"]
    if case == "variance":
        host, attrs_h = lss.generate_flat_spectrum_map(nside, freq, seed=12, **kw)
        assert _same(host[:, ipol, :], np.random.default_rng(12).normal(scale=scale, size=(nfreq, 1, npix)))
        assert np.array_equal(attrs_h["voxvol_ref"], voxvol)


@pytest.mark.parametrize("kind", [np.random.SFC64, np.random.Philox])
def test_other_generators_take_the_host_route(ctx, kind, monkeypatch):
    from cora_amd.util import nputil

    monkeypatch.setattr(nputil, "_HOST_CHUNK", 4096)             # (several chunks of rows)
    nrow, ncol = 13, 1000
    rng, ref_rng = _pair(3, 0, kind)
    s = _scales(nrow, 2)
    ref = ref_rng.normal(scale=s[:, None], size=(nrow, ncol))
    base = _field(8, nrow, ncol)
    out = ctx.to_device(base)
    nputil.normal_rows_device(rng, s, ncol, out, accumulate=True)
    assert _same(out, base + ref)
    assert _state_eq(rng.bit_generator.state, ref_rng.bit_generator.state)
    # assign mode with scattered rows
    ref = ref_rng.normal(scale=s[:, None], size=(nrow, ncol))
    out = ctx.to_device(np.full((nrow, 2, ncol), np.nan))
    nputil.normal_rows_device(rng, s, ncol, out, row_off=(np.arange(nrow) * 2 + 1) * ncol)
    got = out.cpu().numpy()
    assert _same(got[:, 1], ref) and np.isnan(got[:, 0]).all()
    assert _state_eq(rng.bit_generator.state, ref_rng.bit_generator.state)


def test_pcg64_takes_the_host_route_while_a_session_is_held(ctx):
    from cora_amd import _lib
    from cora_amd.core import skysim
    from cora_amd.util import nputil

    holder = np.random.default_rng(99)
    held = skysim.prepare_numpy_stream(ctx, holder, 150, 72)
    assert held is not None
    try:
        nrow, ncol = 5, 4097
        rng, ref_rng = _pair(11, 1)
        s = _scales(nrow, 4)
        st = rng.bit_generator.state["state"]
        out = ctx.to_device(np.zeros((nrow, ncol)))
        with pytest.raises(_lib.CoraHipError) as e:
            ctx.normal_rows_pcg64(st["state"], st["inc"], s, ncol, out)
        assert e.value.status == _lib.CORAHIP_ESTATE
        assert bool((out == 0).all())
        base = _field(6, nrow, ncol)
        out = ctx.to_device(base)
        nputil.normal_rows_device(rng, s, ncol, out, accumulate=True)
        assert _same(out, base + ref_rng.normal(scale=s[:, None], size=(nrow, ncol)))
        assert _state_eq(rng.bit_generator.state, ref_rng.bit_generator.state)
        assert rng.bit_generator.lock.acquire(False)
        rng.bit_generator.lock.release()
    finally:
        held.abort()
    # the context takes the device route again
    rng, ref_rng = _pair(11, 1)
    out = ctx.to_device(np.zeros((3, 100)))
    nputil.normal_rows_device(rng, np.ones(3), 100, out)
    assert _same(out, ref_rng.normal(scale=np.ones(3)[:, None], size=(3, 100)))


@pytest.mark.parametrize("noise", [False, True])
def test_tracer_map_from_models_is_the_composition(ctx, noise):
    import torch

    from cora_amd.signal import lss

    nside, n = 8, 6
    npix = 12 * nside * nside
    z = np.array([0.80, 0.81, 0.823, 0.835, 0.85, 0.861])
    phi, delta = ctx.to_device(3.0 * _field(1, n, npix)), ctx.to_device(0.5 * _field(2, n, npix))
    models = dict(bias_model="eboss_elg", alpha_b=1.1, sigma_P_model="ELG", use_mean_21cmT=True, omega_HI_model="SKA")
    kw = dict(n_eff=3e-4) if noise else {}
    got = lss.tracer_map_from_models_device(phi, delta, z, b2=0.2, dynamics="linear", alpha_FoG=0.75, **models, **kw)

    m = lss.tracer_models(z, **models)
    if not noise:
        hand = lss.tracer_map_device(phi, delta, m["chi"], m["D"], m["f"], m["b1"], b2=0.2, sigmaP=m["sigmaP"], dynamics="linear",
                                     fog_D=m["fog_D"], alpha_FoG=0.75, T_b=m["T_b"])
    else:
        bias = lss.biased_field_device(delta, m["D"], m["b1"], 0.2)
        final = lss.linear_dynamics_device(phi, delta, bias, m["chi"], m["D"], m["f"])
        final = lss.fingers_of_god_device(final, m["chi"], m["sigmaP"], m["fog_D"], 0.75)
        std = lss.shot_noise_std(nside, m["chi"], np.ones(n) * 3e-4)
        seed = zlib.adler32(delta.cpu().numpy()[:, :100].copy().tobytes())
        noise_h = np.random.default_rng(seed).normal(scale=std[:, np.newaxis], size=(n, npix))
        final = ctx.to_device(final.cpu().numpy() + noise_h)
        hand = lss.biased_lss_to_map_device(final, False, 1.0, m["T_b"], True)
    assert got.shape == (n, 4, npix)
    assert torch.equal(got, hand)
    assert bool((got[:, 0] != 0).any())
