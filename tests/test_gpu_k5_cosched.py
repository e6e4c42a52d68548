"""K5 (ring FFT of alm2map) with the belt class and the cap classes side by side on disjoint CU sets, the belt drawing its
items from a device counter (sht_ringfft in csrc/sht_ringfft.hip, ringfft_direct_ct in csrc/sht_ringfft_ct.hip).

The schedule must not change a single bit of the maps: every (ring, channel group) item is computed by the same code
whichever workgroup of whichever launch takes it.  So every comparison here is torch.equal against the alternating
schedule (CORAHIP_K5_BELT_WGS=0), on output buffers pre-filled with NaN: an item that no workgroup took leaves NaN
behind, an item taken twice is harmless but a ticket that skips one is not.

The compile-time belt kernel exists for ring half-lengths 2048 and 4096 only, so the smallest shape that reaches the
co-scheduled form is nside 1024 / lmax 2048 (8 channels: a few ms per call once the plan is cached).
"""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SWITCH = "CORAHIP_K5_BELT_WGS"


def _num_cu(ctx):
    import torch

    return torch.cuda.get_device_properties(ctx.device).multi_processor_count


def _settings(ctx):
    """today's schedule; automatic; W = 8 (the helper launch does nearly all of the belt); W = num_cu - 8 (a side grid of
    one workgroup per XCD); a value that is not a multiple of 8"""
    return ["0", None, "8", str(_num_cu(ctx) - 8), "93"]


class _switch:
    def __init__(self, value):
        self.value = value

    def __enter__(self):
        self.old = os.environ.get(SWITCH)
        if self.value is None:
            os.environ.pop(SWITCH, None)
        else:
            os.environ[SWITCH] = self.value

    def __exit__(self, *a):
        if self.old is None:
            os.environ.pop(SWITCH, None)
        else:
            os.environ[SWITCH] = self.old


def _alm(ctx, lmax, nnu, seed):
    import torch

    L = lmax + 1
    nalm = L * (L + 1) // 2
    gen = torch.Generator(device=ctx.device).manual_seed(seed)
    l_of = torch.cat([torch.arange(m, L, device=ctx.device) for m in range(L)])
    a = torch.randn((nalm, (nnu + 3) // 4, 2, 4), generator=gen, device=ctx.device, dtype=torch.float64)
    a *= (1.0 / (1.0 + l_of.double()))[:, None, None, None]
    a[:L, :, 1, :] = 0.0
    return a


def _synth(ctx, alm, nside, lmax, nnu, setting, out=None, sync=True):
    import torch

    maps = out if out is not None else ctx.empty((nnu, 12 * nside * nside))
    maps.fill_(float("nan"))
    with _switch(setting):
        ctx.alm2map(alm, nside, lmax, nnu, out=maps)
    if sync:
        torch.cuda.synchronize()
    return maps


def _check_parity(ctx, nside, lmax, nnu, settings, seed):
    import torch

    alm = _alm(ctx, lmax, nnu, seed)
    ref = _synth(ctx, alm, nside, lmax, nnu, settings[0]).clone()
    assert not bool(torch.isnan(ref).any()), (nside, lmax, nnu, settings[0], "an item was skipped")
    got = ctx.empty(tuple(ref.shape))
    for s in settings[1:]:
        _synth(ctx, alm, nside, lmax, nnu, s, out=got)
        nnan = int(torch.isnan(got).sum().item())
        diff = (torch.nan_to_num(got) - ref).abs()
        nbad = int((diff > 0).sum().item())
        print("nside %d lmax %d nnu %d %s=%s: NaN pixels %d, differing pixels %d, max |diff| %.3e"
              % (nside, lmax, nnu, SWITCH, s, nnan, nbad, diff.max().item()))
        assert nnan == 0, (nside, lmax, nnu, s, "an item was skipped")
        assert torch.equal(got, ref), (nside, lmax, nnu, s, nbad)
    del alm, ref, got
    torch.cuda.empty_cache()


@pytest.mark.parametrize("nnu", [8, 1, 3, 5, 64])
def test_schedule_parity(ctx, nnu):
    """Every setting of the switch gives the same maps, bit for bit, with full and ragged channel groups (1, 3, 5) and at
    the 64-column shard shape."""
    _check_parity(ctx, 1024, 2048, nnu, _settings(ctx), 300 + nnu)


def test_fewer_items_than_workgroups(ctx):
    """Four channels: one channel group, so the items of a class are its rings - and the plan has cap classes of fewer rings
    than either grid of an even split (their grids are cut to the item count; the rest of the side CUs idle)."""
    nside, lmax, nnu = 1024, 2048, 4
    ncu = _num_cu(ctx)
    W = 8 * (ncu // 16)
    cls = ctx.sht_ring_classes(nside, lmax)
    caps = np.r_[cls[:nside - 1], cls[3 * nside:]]
    lengths, counts = np.unique(caps, return_counts=True)
    items = counts * ((nnu + 3) // 4)          # (2- and 1-channel classes have more items per ring: none is smaller)
    assert items.min() < min(W, ncu - W), (dict(zip(lengths.tolist(), items.tolist())), W, ncu)
    _check_parity(ctx, nside, lmax, nnu, ["0", None, str(W), "8", str(ncu - 8)], 404)


def test_counter_reset_between_calls(ctx):
    """Two calls back to back on one context with nothing between them (the counters are zeroed on the stream, ahead of the
    fork, in every call), then one call under a forced W: three identical maps."""
    import torch

    nside, lmax, nnu = 1024, 2048, 8
    alm = _alm(ctx, lmax, nnu, 505)
    ncu = _num_cu(ctx)
    ref = _synth(ctx, alm, nside, lmax, nnu, "0").clone()
    a = ctx.empty(tuple(ref.shape))
    b = ctx.empty(tuple(ref.shape))
    c = ctx.empty(tuple(ref.shape))
    _synth(ctx, alm, nside, lmax, nnu, str(ncu // 2), out=a, sync=False)
    _synth(ctx, alm, nside, lmax, nnu, str(ncu // 2), out=b, sync=False)
    _synth(ctx, alm, nside, lmax, nnu, "16", out=c, sync=True)
    for name, t in (("first", a), ("second", b), ("forced", c)):
        nnan = int(torch.isnan(t).sum().item())
        print("call %s: NaN pixels %d, differing pixels %d" % (name, nnan, int((torch.nan_to_num(t) != ref).sum().item())))
        assert nnan == 0, name
        assert torch.equal(t, ref), name
    assert torch.equal(a, b) and torch.equal(b, c)
    del alm, ref, a, b, c
    torch.cuda.empty_cache()


def test_fallback_shape(ctx):
    """nside 64 / lmax 128: no compile-time belt kernel, every class goes to the run-time kernels on the alternating
    schedule whatever the switch says."""
    _check_parity(ctx, 64, 128, 8, _settings(ctx), 606)


def test_schedule_parity_nside2048(ctx):
    """The length-4096 belt (two channels per item, one ticket counter per XCD label) beside the P = 8192 / 6144 caps:
    three channels, so the last group of every ring is ragged."""
    ncu = _num_cu(ctx)
    _check_parity(ctx, 2048, 2048, 3, ["0", None, "8", str(ncu - 8), str(ncu // 2)], 707)
