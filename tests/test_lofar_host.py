"""Host checks of the LOFAR synchrotron model (csrc/lofar.hip, cora_amd.foreground.lofar): the oracle of
tests/_lofar_oracle.py against the outputs of the reference's own code (tests/golden/lofar_vectors.npz, written by
tests/golden/make_golden_lofar.py), the new symbols, the class attributes and the range guard.  The GPU is then held to the
oracle in tests/test_gpu_lofar.py."""
import ctypes
import os
import re

import numpy as np
import pytest

import _lofar_oracle as lo


@pytest.fixture(scope="module")
def gold():
    return lo.load_golden()


@pytest.mark.parametrize("tag", lo.CASES)
def test_oracle_matches_reference(gold, tag):
    """The tolerance test_flatsky.py gives a field: 1e-13 relative to max |Tb|."""
    par, A, beta, Tb = lo.golden_case(gold, tag)
    ref, x, _ = lo.model(A, beta, par, lo.golden_attrs(gold))
    numz = (par["x_num"] + par["y_num"]) // 2
    assert Tb.shape == ref.shape == (par["nu_num"], par["x_num"], par["y_num"])
    assert A.shape == (par["x_num"], par["y_num"], numz - numz % 2) and (beta is A) == par["correlated"]
    rel = float(np.abs(Tb - ref).max() / np.abs(Tb).max())
    print("%s: reference Tb against the oracle, max |diff| / max |Tb| = %.3g" % (tag, rel))
    assert rel < 1e-13
    if tag == "c4_6_6":
        assert x.min() < 0 < x.max()           # the band straddles nu_0
    if tag == "c3_8_7":
        assert numz == 7 and A.shape[2] == 6


def test_golden_cases_differ(gold):
    a = lo.golden_case(gold, "c5_12_9")
    b = lo.golden_case(gold, "c5_12_9_corr")
    assert np.array_equal(a[1], b[1]) and not np.array_equal(a[3], b[3])      # the same first draw, another map


def test_abi_symbols_present():
    from cora_amd import _lib

    names = ["corahip_powerlaw_los", "corahip_field_moments"]
    lib = ctypes.CDLL(_lib.LIB_PATH)
    header = open(os.path.join(os.path.dirname(_lib._HERE), "include", "corahip.h")).read()
    minor = [line for line in header.splitlines() if line.startswith("#define CORAHIP_ABI_MINOR")]
    assert len(minor) == 1 and re.match(r"#define CORAHIP_ABI_MINOR 12\s", minor[0]) and lib.corahip_abi_minor() == 12
    for n in names:
        assert n in _lib.SIGNATURES and hasattr(lib, n) and ("int %s(" % n) in header
        assert n[len("corahip_"):] in minor[0]
    assert len(_lib.SIGNATURES["corahip_powerlaw_los"][1]) == 12 and len(_lib.SIGNATURES["corahip_field_moments"][1]) == 5
    for m in ("powerlaw_los", "field_moments", "powerlaw_range_check"):
        assert callable(getattr(_lib.Context, m))
    # the ulp bound of exp that the header states is the one the oracle's bound uses
    doc = header.split("powerlaw_los:")[1].split("field_moments:")[0]
    assert "With E = %d that ulp bound" % lo.EXP_ULP in doc and "(nz + 2 max|x b| + 2 E + 4) 2^-53" in doc
    # argument checks come before anything touches a device: no context
    lib.corahip_powerlaw_los.restype = lib.corahip_field_moments.restype = ctypes.c_int
    assert lib.corahip_field_moments(None, None, ctypes.c_long(1), 1, None) == -1


def test_class_attributes(gold):
    from cora_amd.core import gaussianfield, maps
    from cora_amd.foreground import lofar

    want = lo.golden_attrs(gold)
    for name in ("nu_0", "A_amp", "A_std", "beta_mean", "beta_std", "alpha"):
        assert float(getattr(lofar.LofarGDSE, name)) == want[name], name
    assert lofar.LofarGDSE.correlated is False and want["correlated"] == 0.0
    assert lofar._LofarGDSE_3D.delta == want["delta"] == -4.0
    assert issubclass(lofar.LofarGDSE, maps.Map3d) and issubclass(lofar._LofarGDSE_3D, gaussianfield.RandomField)
    m = lofar.LofarGDSE()
    assert (m.nu_num, m.x_num, m.y_num) == (128, 128, 128)
    # the power law of the 3-d field, DC mode zeroed, no warning from the division by zero there
    f = lofar._LofarGDSE_3D(npix=[4, 4, 4], wsize=[1.0, 1.0, 1.0])
    f.delta = -2.7
    k = np.zeros((2, 2, 2, 3))
    k[1, 0, 1] = (3.0, 0.0, 4.0)
    with np.errstate(all="raise"):
        ps = f.powerspectrum(k)
    assert ps[0, 0, 0] == 0.0 and abs(ps[1, 0, 1] - 25.0 ** (-1.35)) < 1e-15 and np.isinf(ps[0, 0, 1])
    # seeds of the two fields of an integer-seed draw differ, also for neighbouring seeds
    assert lofar.beta_seed(5) == (5 + lofar.BETA_SEED_OFFSET) % 2**64 and lofar.beta_seed(2**64 - 1) == lofar.BETA_SEED_OFFSET - 1
    assert len({5, 6, lofar.beta_seed(5), lofar.beta_seed(6)}) == 4


def test_range_guard_fires():
    from cora_amd import _lib

    chk = _lib.Context.powerlaw_range_check
    chk(1.0, -2.55, 0.1, 4.0)
    chk(0.0, 1e300, 1.0, 1e300)
    chk(511.0, 1.0, 0.0, 7.0)
    for args in ((512.0, 1.0, 0.0, 0.0), (1.0, -500.0, 3.0, 4.0), (2.0, 0.0, -1.0, 256.0), (1.0, 0.0, 1.0, float("nan")),
                 (float("inf"), 1.0, 0.0, 0.0)):
        with pytest.raises(ValueError, match="must stay below 512"):
            chk(*args)
