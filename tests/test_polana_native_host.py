"""Host side of the native spin-2 analysis (no GPU): the two new symbols are declared, bound and exported, the
``method`` keyword of ``map2alm_pol_device`` and the module setting that the other entry points follow are checked
before any device work, and the default route stays the composed one.

The call surfaces of ``map2alm_sky_device``, ``map2alm_sky_bytes``, ``cross_spectra_pol_device`` and ``anafast_pol``
are pinned by tests/test_polspectra_host.py::test_signatures and stay as they are: those four take the route from
``hputil._spin2_method``, which ``hputil.spin2_method`` sets for the duration of a block."""
import inspect
import os
import re

import numpy as np
import pytest

from cora_amd import _lib
from cora_amd.util import hputil

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbols_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "corahip.h")).read()
    assert re.search(r"\bint corahip_map2alm_spin2_workspace_bytes\(const corahip_sht_plan \*\w+, int nfields, size_t \*bytes\);",
                     header)
    assert re.search(r"\bint corahip_map2alm_spin2\(corahip_ctx \*ctx, corahip_sht_plan \*\w+, const double \*maps_qu, int nfields,"
                     r"\s+const double \*ring_w, double \*alm_eb_dev, void \*workspace, size_t workspace_bytes\);", header)
    minor = header.split("#define CORAHIP_ABI_MINOR")[1].split("\n")[0]
    assert minor.split()[0] == "12"
    names = re.split(r"[,;]\s*|\s+", minor)
    assert "map2alm_spin2_workspace_bytes" in names and "map2alm_spin2" in names
    res, args = _lib.SIGNATURES["corahip_map2alm_spin2_workspace_bytes"]
    assert res is _lib.c_int and len(args) == 3
    res, args = _lib.SIGNATURES["corahip_map2alm_spin2"]
    assert res is _lib.c_int and len(args) == 8
    lib = _lib.load()
    assert hasattr(lib, "corahip_map2alm_spin2_workspace_bytes") and hasattr(lib, "corahip_map2alm_spin2")


def test_binding_surface():
    E = inspect.Parameter.empty
    params = lambda f: [(p.name, p.default) for p in inspect.signature(f).parameters.values()]
    assert params(_lib.Context.map2alm_spin2_native)[1:] == [("maps_qu", E), ("nside", E), ("lmax", E), ("ring_w", None),
                                                             ("chunk", None), ("out", None)]
    assert params(_lib.Context.map2alm_spin2_workspace_bytes)[1:] == [("plan", E), ("nfields", E)]
    assert params(_lib.Context.map2alm_spin2)[1:] == [("maps_qu", E), ("nside", E), ("lmax", E), ("ring_w", None),
                                                      ("out", None)]            # the composed pass is as it was
    assert params(hputil.map2alm_pol_device) == [("maps_qu", E), ("nside", E), ("lmax", E), ("use_weights", None),
                                                 ("niter", None), ("method", None)]
    for f in (hputil.map2alm_sky_device, hputil.map2alm_sky_bytes, hputil.cross_spectra_pol_device, hputil.anafast_pol):
        assert "method" not in inspect.signature(f).parameters, f.__name__    # their pinned call surfaces are unchanged


def test_default_method_is_composed():
    assert hputil._spin2_method == "composed"


def test_setting_is_scoped_and_checked():
    with hputil.spin2_method("native") as m:
        assert m == "native" and hputil._spin2_method == "native"
        with hputil.spin2_method("composed"):
            assert hputil._spin2_method == "composed"
        assert hputil._spin2_method == "native"
    assert hputil._spin2_method == "composed"
    with pytest.raises(RuntimeError):
        with hputil.spin2_method("native"):
            raise RuntimeError("inside")
    assert hputil._spin2_method == "composed"                                # restored when the block raises, too
    for bad in ("bogus", "Native", "", 1):
        with pytest.raises(ValueError):
            with hputil.spin2_method(bad):
                pass
        assert hputil._spin2_method == "composed"


def test_unknown_method_raises_before_device_work(monkeypatch):
    import torch

    def no_device():
        raise AssertionError("the method must be checked before a context is asked for")

    monkeypatch.setattr(_lib, "get_context", no_device)
    qu = torch.zeros((2, 48), dtype=torch.float64)
    sky = torch.zeros((1, 3, 48), dtype=torch.float64)
    with pytest.raises(ValueError):
        hputil.map2alm_pol_device(qu, 2, 4, method="bogus")
    with pytest.raises(ValueError):
        hputil.map2alm_pol_device(qu, 2, 4, method="Native")                 # the two names are exact
    # the entry points without the keyword follow the module setting, and check it first as well
    monkeypatch.setattr(hputil, "_spin2_method", "bogus")
    with pytest.raises(ValueError):
        hputil.map2alm_pol_device(qu, 2, 4)
    with pytest.raises(ValueError):
        hputil.map2alm_sky_bytes(2, 4, 3)
    with pytest.raises(ValueError):
        hputil.map2alm_sky_device(sky)
    with pytest.raises(ValueError):
        hputil.cross_spectra_pol_device(sky)
    with pytest.raises(ValueError):
        hputil.anafast_pol(np.zeros((3, 48)))
