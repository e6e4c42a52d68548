"""The wide shape of the fused-RNG draw (csrc/draw.hip, draw_wide_kernel): launches whose widest channel chunk has more
than 128 columns run 256-column items of 64 m with the real and the imaginary rows interleaved in one MFMA tile.

Bits: the k-slots and the order of the k-steps are those of the 128-column shape, so one wide call must be ``torch.equal``
to the concatenation of narrow calls over 128-channel ranges (the sharded ranks run the narrow shapes and must agree
with the 1-rank step bit for bit).  Values: against the materialised Philox stream through ``draw_alm`` with the tolerance
of the existing draw tests, 1e-13 max|a| (fixtures as in test_gpu_parity.py: factors of A A^T).  Contract: on a poisoned
output every cell of the call is written and nothing around it is touched.  Run with -m gpu."""
import numpy as np
import pytest

import _poison
from test_gpu_poison import _channels, _mk_cl

pytestmark = pytest.mark.gpu

_KEEP = {}


def _factors(ctx, F, lmax):
    """(T, info, all-ones info) of lmax + 1 random positive definite blocks A A^T, built once per shape."""
    import torch

    key = (F, lmax)
    if key not in _KEEP:
        A = np.random.default_rng(1000 * F + lmax).standard_normal((lmax + 1, F, F + 5))
        T, info = ctx.factor_batched(ctx.to_device(A @ A.transpose(0, 2, 1)))
        assert not info.any()
        _KEEP[key] = (T, info, torch.ones_like(info))
    return _KEEP[key]


def _upto(fac, lmax):
    """The factors of the multipoles 0 .. lmax of a larger set."""
    return tuple(t[:lmax + 1].contiguous() for t in fac)


def _narrow(ctx, T, info, seed, lmax, F):
    import torch

    return torch.cat([ctx.draw_alm_philox(T, info, seed, lmax, F, nu0=n0, nnu=128) for n0 in range(0, F, 128)], dim=1)


# lmax: edges of the 8-m wave tile (7, 8) and of the 64-m item (63, 64), a ragged second item (70), three items (130)
@pytest.mark.parametrize("lmax", [0, 7, 8, 63, 64, 70, 130])
def test_wide_bits_equal_two_narrow_calls(ctx, lmax):
    import torch

    F = 256
    T, tri, dense = _upto(_factors(ctx, F, 130), lmax)
    for info in (tri, dense):
        wide = ctx.draw_alm_philox(T, info, 41 + lmax, lmax, F)
        assert torch.isfinite(wide).all()
        assert torch.equal(wide, _narrow(ctx, T, info, 41 + lmax, lmax, F)), (lmax, bool(info.any()))


def test_wide_bits_equal_four_narrow_calls_at_512(ctx):
    import torch

    F, lmax = 512, 10
    T, tri, dense = _factors(ctx, F, lmax)
    for info in (tri, dense):
        wide = ctx.draw_alm_philox(T, info, 5, lmax, F)
        assert torch.equal(wide, _narrow(ctx, T, info, 5, lmax, F)), bool(info.any())


def _check_values(ctx, T, info, seed, lmax, F, nu0, nnu):
    import torch

    g = ctx.normals_philox(seed, lmax, F)
    a = ctx.alm_dev_to_square(ctx.draw_alm(T, info, g, lmax, F, nu0=nu0, nnu=nnu), lmax, nnu)
    b = ctx.alm_dev_to_square(ctx.draw_alm_philox(T, info, seed, lmax, F, nu0=nu0, nnu=nnu), lmax, nnu)
    assert torch.isfinite(b).all()
    err, scale = (a - b).abs().max().item(), a.abs().max().item()
    print("F=%d lmax=%d nu0=%d nnu=%d: max|diff| %.3e, max|a| %.3e" % (F, lmax, nu0, nnu, err, scale))
    assert err <= 1e-13 * scale, (F, lmax, nu0, nnu, err, scale)
    # the row-sliced entry
    rows = T[:, nu0:nu0 + nnu, :].contiguous()
    c = ctx.alm_dev_to_square(ctx.draw_alm_philox_rows(rows, info, seed, lmax, F, nu0, nnu), lmax, nnu)
    assert torch.equal(b, c), (F, lmax, nu0, nnu)


# partial tiles and partial cells (132 = 8 tiles + one cell, 144 = 9 tiles, 200 = 12.5 tiles), the full group (256),
# one wide group plus a 4-column group (260), a channel range off the chunk grid (the "every tile" path)
@pytest.mark.parametrize("F,lmax,nu0,nnu", [(132, 70, 0, 132), (144, 70, 0, 144), (200, 70, 0, 200), (256, 130, 0, 256),
                                            (260, 20, 0, 260), (256, 130, 3, 200)])
def test_wide_values_against_materialised_stream(ctx, F, lmax, nu0, nnu):
    T, tri, dense = _factors(ctx, F, lmax)
    _check_values(ctx, T, tri, 7 + F, lmax, F, nu0, nnu)
    _check_values(ctx, T, dense, 8 + F, lmax, F, nu0, nnu)


# (8, 264): both chunks off the chunk grid; (32, 320): on it, chunk 0 with one full chunk and eight of the tail, chunk 1
# cut at F after six chunks of its tail
@pytest.mark.parametrize("first", [(8, 264), (32, 320)])
def test_wide_folded_set_of_two_132_channel_chunks(ctx, first):
    import torch

    F, lmax, n = 512, 10, 132
    T, tri, dense = _factors(ctx, F, lmax)
    g = ctx.normals_philox(19, lmax, F)
    rows = torch.cat([T[:, a:a + n] for a in first], dim=1).contiguous()
    for info in (tri, dense):
        got = ctx.draw_alm_philox_chunks(rows, info, 19, lmax, F, [(a, n) for a in first])
        want = torch.cat([ctx.draw_alm(T, info, g, lmax, F, nu0=a, nnu=n) for a in first], dim=1)
        err, scale = (got - want).abs().max().item(), want.abs().max().item()
        print("chunks %r: max|diff| %.3e, max|a| %.3e" % (first, err, scale))
        assert torch.isfinite(got).all() and err <= 1e-13 * scale, (first, err, scale)


@pytest.mark.parametrize("F", [144, 256])
def test_wide_on_poisoned_output(ctx, F):
    """As test_gpu_poison_modules.py::test_k3_draw_alm_and_philox (factors with a zero and an indefinite block: the eigen
    route writes dense factors for those l), and with the output inside a larger buffer whose other cells must stay."""
    import torch

    lmax = 70
    key = ("poison", F)
    if key not in _KEEP:
        _KEEP[key] = ctx.factor_batched(ctx.to_device(_mk_cl(F, lmax + 1, 7 * F + lmax)))
    T, info = _KEEP[key]
    label = "draw_alm_philox wide F=%d" % F
    ref, report = _poison.poisoned_runs(ctx, lambda: _channels(ctx.draw_alm_philox(T, info, 77, lmax, F), F), slots=(3,),
                                        label=label)
    print("%s: %s" % (label, ", ".join("0x%02X -> %r" % (b, report[b]) for b in sorted(report))))
    for b, (nalloc, nbytes, sbytes) in report.items():
        assert sbytes > 0 and nalloc > 0 and nbytes > 0, (label, hex(b), report[b])
    nalm, G, pad = (lmax + 1) * (lmax + 2) // 2, F // 4, 64
    for byte in (0xFF, 0x7E):
        buf = torch.empty((nalm + 2 * pad, G, 2, 4), dtype=torch.float64, device=ctx.device)
        buf.view(torch.uint8).fill_(byte)
        out = ctx.draw_alm_philox(T, info, 77, lmax, F, out=buf[pad:pad + nalm])
        assert torch.equal(_channels(out, F), ref[0]), (label, hex(byte))
        for guard in (buf[:pad], buf[pad + nalm:]):
            assert bool((guard.contiguous().view(torch.uint8) == byte).all()), (label, hex(byte), "a cell outside the call was written")
