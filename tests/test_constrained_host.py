"""Host checks of the device route of skysim.mkconstrained (csrc/constrained.hip): the oracle of
tests/_constrained_oracle.py against the reference's own cv (tests/golden/mkconstrained_vectors.npz, written by
tests/golden/make_golden_mkconstrained.py), the new symbols and argument checking.  The GPU is then held to the oracle in
tests/test_gpu_constrained.py."""
import ctypes
import os

import numpy as np
import pytest

import _constrained_oracle as co


@pytest.fixture(scope="module")
def gold():
    return co.load_golden()


def golden_case(g, case):
    """(corr [L, F, F], f_ind, calm [k, nalm], cv [F, nalm]) of a golden case as float64 / complex128."""
    calm = (g[case + "_calm_re"] + 1j * g[case + "_calm_im"]) * float(g[case + "_calm_s"])
    return g[case + "_corr"].astype(np.float64), [int(f) for f in g[case + "_f_ind"]], calm, g[case + "_cv"]


@pytest.mark.parametrize("case,F,k", [("a", 6, 1), ("b", 18, 2)])
def test_oracle_matches_reference_cv(gold, case, F, k):
    """The reference solves tmat^T amp = c and multiplies by trans^T; the oracle forms W first.  Both start from scipy's
    eigh, so the subspace term of tol_W (with the reference's residual on both sides) covers two runs of it; the k-term
    sum is in tol_cv."""
    corr, f_ind, calm, cv_ref = golden_case(gold, case)
    assert corr.shape == (9, F, F) and len(f_ind) == k and calm.shape == (k, 45) and cv_ref.shape == (F, 45)
    assert np.array_equal(corr, corr.transpose(0, 2, 1))
    cv, W = co.mkconstrained_cv(corr, f_ind, calm)
    tol = co.tol_cv(corr, f_ind, calm)
    err = np.abs(cv - cv_ref)
    larr, marr = co.getlm(8)
    assert np.all(cv[:, larr == 0] == 0) and np.all(W[0] == 0)
    assert np.all(tol[:, larr > 0] > 0)
    print("%s: reference cv against the oracle, worst err / tol %.3g" % (case, (err[:, larr > 0] / tol[:, larr > 0]).max()))
    assert np.all(err <= tol)
    # the constrained channels carry their constraints: W[l, f_ind[j], :] is the j-th unit vector
    for j, f in enumerate(f_ind):
        assert np.all(np.abs(cv[f] - np.where(larr > 0, calm[j], 0)) <= tol[f] + 4 * co.U * np.abs(calm[j]))


def test_abi_symbols_present():
    from cora_amd import _lib

    names = ["corahip_eig_top_batched", "corahip_eig_top_max_f", "corahip_constrained_weights", "corahip_alm_mix_l"]
    lib = ctypes.CDLL(_lib.LIB_PATH)
    header = open(os.path.join(os.path.dirname(_lib._HERE), "include", "corahip.h")).read()
    assert "#define CORAHIP_ABI_MINOR 12 " in header
    for n in names:
        assert n in _lib.SIGNATURES and hasattr(lib, n) and ("int %s(" % n) in header
        assert n[len("corahip_"):] in header.split("#define CORAHIP_ABI_MINOR")[1].split("\n")[0]
    for m in ("eig_top_batched", "eig_top_max_f", "constrained_weights", "alm_mix_l"):
        assert callable(getattr(_lib.Context, m))
    # the test hook that fills the scratch of the context (and the per-call scratch of the eigen routes) with a poison byte
    n = "corahip_debug_poison_scratch"
    assert n in _lib.SIGNATURES and hasattr(lib, n) and ("int %s(corahip_ctx *ctx, int byte, size_t *slot_bytes);" % n) in header
    assert "debug_poison_scratch (test hook)" in header.split("#define CORAHIP_ABI_MINOR")[1].split("\n")[0]
    assert len(_lib.SIGNATURES[n][1]) == 3 and callable(_lib.Context.debug_poison_scratch)
    from cora_amd.core import skysim

    for f in ("constrained_weights_device", "mkconstrained_device", "mkconstrained"):
        assert callable(getattr(skysim, f))


class _Untouchable:
    def __getattr__(self, name):
        raise AssertionError("the library was touched (%s) before the arguments were checked" % name)


def test_argument_errors_before_the_library(monkeypatch):
    import torch

    from cora_amd import _lib
    from cora_amd.core import skysim

    ctx = _lib.Context.__new__(_lib.Context)
    ctx.lib, ctx.h, ctx.device = _Untouchable(), None, torch.device("cpu")
    C = torch.zeros((3, 5, 5), dtype=torch.float64)
    for bad, k in ((C, 0), (C, 6), (torch.zeros((3, 12, 12), dtype=torch.float64), 9), (torch.zeros((3, 5, 4), dtype=torch.float64), 1),
                   (C.float(), 1), (C.numpy(), 1), (C[:, :, ::2], 1), (C[0], 1)):
        with pytest.raises(ValueError):
            ctx.eig_top_batched(bad, k)
    with pytest.raises(ValueError, match="max_iter"):
        ctx.eig_top_batched(C, 1, max_iter=-1)
    V, th, info = torch.zeros((3, 5, 2), dtype=torch.float64), torch.zeros((3, 2), dtype=torch.float64), torch.zeros(3, dtype=torch.int32)
    for out in ((V[:, :, :1], th, info), (V, th[:2], info), (V, th, info.long()), (V, V.reshape(-1)[:6].reshape(3, 2), info)):
        with pytest.raises(ValueError):
            ctx.eig_top_batched(C, 2, out=out)
    for f_ind in ([0], [0, 5], [-1, 0], [0.0, 1.0], [0, 1, 2]):
        with pytest.raises(ValueError, match="f_ind"):
            ctx.constrained_weights(V, f_ind)
    with pytest.raises(ValueError, match="V must be"):
        ctx.constrained_weights(V.numpy(), [0, 1])
    with pytest.raises(ValueError, match="k must be"):
        ctx.constrained_weights(torch.zeros((3, 12, 9), dtype=torch.float64), list(range(9)))
    lmax = 2
    alm = torch.zeros((6, 1, 2, 4), dtype=torch.float64)
    W = torch.zeros((3, 5, 2), dtype=torch.float64)
    with pytest.raises(ValueError, match="alm must be"):
        ctx.alm_mix_l(alm[:5], lmax, W)
    with pytest.raises(ValueError, match="W must be"):
        ctx.alm_mix_l(alm, lmax, W[:2])
    with pytest.raises(ValueError, match="W must be"):
        ctx.alm_mix_l(alm, lmax, torch.zeros((3, 5, 5), dtype=torch.float64))
    with pytest.raises(ValueError, match="out must be"):
        ctx.alm_mix_l(alm, lmax, W, out=torch.zeros((6, 1, 2, 4), dtype=torch.float64))
    big = torch.zeros((6 * 2 * 8 + 60,), dtype=torch.float64)
    with pytest.raises(ValueError, match="overlaps"):
        ctx.alm_mix_l(big[:48].reshape(6, 1, 2, 4), lmax, W, out=big[8:104].reshape(6, 2, 2, 4))

    # skysim: refused before a context is asked for
    monkeypatch.setattr(_lib, "get_context", lambda *a, **k: (_ for _ in ()).throw(AssertionError("context asked for")))
    m = torch.zeros(48, dtype=torch.float64)
    with pytest.raises(ValueError, match="at most 8 constraints"):
        skysim.mkconstrained(np.zeros((4, 12, 12)), [(i, m) for i in range(9)], 2)
    with pytest.raises(ValueError, match="all device tensors or all arrays"):
        skysim.mkconstrained(np.zeros((4, 12, 12)), [(0, m), (1, np.zeros(48))], 2)
