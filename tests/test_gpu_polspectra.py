"""Polarised spectra on the GPU: Context.alm_gather_channels (csrc/spectra.hip), hputil.map2alm_sky_device /
cross_spectra_pol_device / anafast_pol and skysim.clarray_from_maps on [F, npol, npix], against tests/_polspectra_oracle.py
(layouts, references and the derivation of every bound are there).  Every test prints its worst error over tolerance.
Run with -m gpu."""
import ctypes

import numpy as np
import pytest

import _polspectra_oracle as po

pytestmark = pytest.mark.gpu

CORAHIP_EINVAL = -1
PAD = 7.5                                  # what the padding channels of a hand-built source hold
FILLS = (float("nan"), 3.0e300)            # what dst holds before a gather


# ---- 1. the gather -----------------------------------------------------------------------------------------------
def _index_sets(nsrc, rng):
    """a permutation, a subset and a set with repeats of the nsrc source channels"""
    perm = rng.permutation(nsrc)
    subset = np.sort(rng.choice(nsrc, size=max(1, nsrc // 2), replace=False))
    repeats = rng.integers(0, nsrc, size=nsrc + 2)
    repeats[-1] = repeats[0]
    return {"permutation": perm, "subset": subset, "repeats": repeats}


@pytest.mark.parametrize("lmax", (0, 1, 5, 33))
@pytest.mark.parametrize("nsrc", (1, 3, 4, 5, 9))
def test_gather_moves_the_channels_and_nothing_else(ctx, nsrc, lmax):
    import torch

    rng = np.random.default_rng(100 * nsrc + lmax)
    nalm = (lmax + 1) * (lmax + 2) // 2
    a = rng.standard_normal((nsrc, nalm)) + 1j * rng.standard_normal((nsrc, nalm))
    src = torch.from_numpy(po.to_layout(a, PAD)).to(ctx.device)
    keep = src.clone()
    ncase = 0
    for kind, idx in _index_sets(nsrc, rng).items():
        n = len(idx)
        for dst_first in (0, 1, 3, 4, 6):
            ndst = dst_first + n + (ncase % 4)                       # the range ends on, or 1 .. 3 short of, the end
            G = (ndst + 3) // 4
            for fill in FILLS:
                dst = torch.full((nalm, G, 2, 4), fill, dtype=torch.float64, device=ctx.device)
                res = ctx.alm_gather_channels(src, nsrc, idx.astype(np.int32), dst, ndst, dst_first=dst_first)
                assert res is dst
                got = po.from_layout(dst.cpu().numpy())              # [4 G, nalm], padding channels included
                tag = (kind, dst_first, ndst, fill)
                assert np.array_equal(got[dst_first:dst_first + n], a[idx]), tag         # bit for bit (no NaN in a)
                rest = np.delete(got, np.arange(dst_first, dst_first + n), axis=0)
                for part in (rest.real, rest.imag):                  # every other element still holds its fill
                    assert np.isnan(part).all() if np.isnan(fill) else np.array_equal(part, np.full(part.shape, fill)), tag
            again = torch.full((nalm, G, 2, 4), FILLS[1], dtype=torch.float64, device=ctx.device)
            ctx.alm_gather_channels(src, nsrc, torch.from_numpy(idx.astype(np.int32)).to(ctx.device), again, ndst, dst_first)
            assert torch.equal(again, dst), (kind, dst_first)         # identical bits; idx as a device tensor
            ncase += 1
    assert torch.equal(src, keep)                                    # the source is not touched
    print("gather nsrc %d lmax %d: %d layouts, every one exact" % (nsrc, lmax, ncase))


def test_gather_from_a_buffer_padded_to_eight(ctx):
    """nsrc = 4 G addresses the padding channels of an 8-padded buffer like any other; a wide destination (more than one
    workgroup along the row: 300 channels = 75 groups = 300 pairs) and a wide source"""
    import torch

    lmax = 5
    nalm = (lmax + 1) * (lmax + 2) // 2
    rng = np.random.default_rng(8)
    a = rng.standard_normal((6, nalm)) + 1j * rng.standard_normal((6, nalm))
    src = torch.from_numpy(po.to_layout(a, PAD)).to(ctx.device)                       # 6 channels in 2 groups
    dst = torch.full((nalm, 1, 2, 4), float("nan"), dtype=torch.float64, device=ctx.device)
    ctx.alm_gather_channels(src, 8, [7, 0, 5], dst, 3)
    got = po.from_layout(dst.cpu().numpy())
    assert np.array_equal(got[0], np.full(nalm, PAD + 1j * PAD)) and np.array_equal(got[1], a[0]) and np.array_equal(got[2], a[5])
    assert np.isnan(got[3].real).all()
    with pytest.raises(ValueError):
        ctx.alm_gather_channels(src, 6, [6], dst, 3)                                  # beyond nsrc as given
    nsrc, ndst = 301, 300
    b = rng.standard_normal((nsrc, nalm)) + 1j * rng.standard_normal((nsrc, nalm))
    wide = torch.from_numpy(po.to_layout(b)).to(ctx.device)
    idx = rng.permutation(nsrc)[:297]
    out = torch.full((nalm, 75, 2, 4), float("nan"), dtype=torch.float64, device=ctx.device)
    ctx.alm_gather_channels(wide, nsrc, idx, out, ndst, dst_first=2)
    got = po.from_layout(out.cpu().numpy())
    assert np.array_equal(got[2:299], b[idx]) and np.isnan(got[:2].real).all() and np.isnan(got[299:].imag).all()


def test_gather_refuses_overlap_and_bad_counts(ctx):
    import torch

    lmax, nsrc, ndst = 4, 5, 6
    nalm = (lmax + 1) * (lmax + 2) // 2
    buf = torch.zeros((2, nalm, 2, 2, 4), dtype=torch.float64, device=ctx.device)
    src, dst = buf[0], buf[1]
    idx = ctx.to_device(np.array([0, 4, 2], dtype=np.int32), dtype=np.int32)
    f = ctx.lib.corahip_alm_gather_channels
    s, d, i = (ctypes.c_void_p(t.data_ptr()) for t in (src, dst, idx))
    assert f(ctx.h, s, nsrc, i, 3, lmax, d, ndst, 3) == 0
    for args in ((None, nsrc, i, 3, lmax, d, ndst, 0), (s, nsrc, None, 3, lmax, d, ndst, 0), (s, nsrc, i, 3, lmax, None, ndst, 0),
                 (s, 0, i, 3, lmax, d, ndst, 0), (s, nsrc, i, 0, lmax, d, ndst, 0), (s, nsrc, i, 3, lmax, d, 0, 0),
                 (s, nsrc, i, 3, -1, d, ndst, 0), (s, nsrc, i, 3, lmax, d, ndst, -1), (s, nsrc, i, 3, lmax, d, ndst, 4),
                 (s, nsrc, i, 3, lmax, d, 2, 0),
                 (s, nsrc, i, 3, lmax, s, ndst, 0),                                    # dst is src
                 (s, nsrc, i, 3, lmax, ctypes.c_void_p(src.data_ptr() + 64), ndst, 0),  # dst inside src
                 (s, nsrc, i, 3, lmax, ctypes.c_void_p(dst.data_ptr() + 8), ndst, 0)):  # not 16-byte aligned
        assert f(ctx.h, *args) == CORAHIP_EINVAL, args[1:]
    assert not bool(buf.any())                                       # a refused call (and the zero source) wrote nothing
    good = [0, 4, 2]
    for bad in ([0, 5], [-1], [], [[0, 1]], np.array([0.0, 1.0]), torch.tensor([0, 1], dtype=torch.int64, device=ctx.device)):
        with pytest.raises(ValueError):
            ctx.alm_gather_channels(src, nsrc, bad, dst, ndst)
    with pytest.raises(ValueError):
        ctx.alm_gather_channels(src, nsrc, good, dst, ndst, dst_first=4)
    with pytest.raises(ValueError):
        ctx.alm_gather_channels(src, nsrc, good, dst, ndst, dst_first=-1)
    with pytest.raises(ValueError):
        ctx.alm_gather_channels(src, 9, good, dst, ndst)              # 3 groups asked of a source of 2
    with pytest.raises(ValueError):
        ctx.alm_gather_channels(src, nsrc, good, dst, 3)
    with pytest.raises(ValueError):
        ctx.alm_gather_channels(src, nsrc, good, src, nsrc)           # overlap
    with pytest.raises(ValueError):
        ctx.alm_gather_channels(src, nsrc, good, torch.zeros((nalm + 1, 2, 2, 4), dtype=torch.float64, device=ctx.device), ndst)
    with pytest.raises(ValueError):
        ctx.alm_gather_channels(src.float(), nsrc, good, dst, ndst)


# ---- 2. the coefficients of a polarised sky -----------------------------------------------------------------------
_sky = {}


def _sky_case(nside, lmax, F=9, seed=0, pure_e=False):
    """(maps [F, 4, npix], oracle coefficients [4 F, nalm] with use_weights=True, niter=2), computed once per case and
    not modified; fewer channels or 3 planes are slices of it (the analysis treats every channel on its own)"""
    key = (nside, lmax, F, seed, pure_e)
    if key not in _sky:
        alm = po.random_sky_alm(np.random.default_rng(1000 * nside + seed), lmax, F, 4, pure_e=pure_e)
        maps = po.synth_sky(alm, nside, lmax)
        _sky[key] = (maps, po.analyse_sky(maps, nside, lmax, use_weights=True, niter=2))
    return _sky[key]


def _subset(maps, ref, F, npol):
    Fall = maps.shape[0]
    rows = np.concatenate([p * Fall + np.arange(F) for p in range(npol)])
    return np.ascontiguousarray(maps[:F, :npol]), ref[rows]


@pytest.mark.parametrize("npol", (3, 4))
@pytest.mark.parametrize("nside, lmax, F", ((16, 24, 1), (16, 24, 3), (16, 24, 5), (16, 24, 9), (8, 16, 3)))
def test_sky_coefficients_against_the_oracle(ctx, nside, lmax, F, npol):
    """chunk = 4: F = 9 makes three chunks with a remainder of one, F = 5 a remainder that shares its groups with the
    chunk before.  Every channel within 1e-11 max|a| of its field in the oracle."""
    from cora_amd.util import hputil

    maps, ref = _subset(*_sky_case(nside, lmax, 9 if nside == 16 else 3), F, npol)
    alm = hputil.map2alm_sky_device(ctx.to_device(maps), lmax=lmax, use_weights=True, niter=2, chunk=4)
    n = npol * F
    nalm = (lmax + 1) * (lmax + 2) // 2
    assert tuple(alm.shape) == (nalm, (n + 3) // 4, 2, 4)
    full = po.from_layout(alm.cpu().numpy())
    got = full[:n]
    assert not full[n:].any()                                                          # padding channels are zero
    assert np.array_equal(got, po.device_packed(ctx, alm, lmax, n))                    # (the library's own unpacking agrees)
    l, _ = po.lm(lmax)
    assert not got[F:3 * F][:, l < 2].any()                                            # no spin-2 power below l = 2
    r = np.abs(got - ref).max(axis=1) / (po.ALM_GATE * np.abs(ref).max(axis=1))
    print("sky coefficients nside %d lmax %d F %d npol %d: worst err / tol %.3g (channel %d, field %d)"
          % (nside, lmax, F, npol, r.max(), int(r.argmax()) % F, int(r.argmax()) // F))
    assert r.max() <= 1.0
    # the default chunk, and the defaults of the module (use_weights=True, niter=2): the same numbers within the gate
    dflt = po.device_packed(ctx, hputil.map2alm_sky_device(ctx.to_device(maps), lmax=lmax), lmax, n)
    assert (np.abs(dflt - ref).max(axis=1) <= po.ALM_GATE * np.abs(ref).max(axis=1)).all()


def test_sky_analysis_on_poisoned_allocations(ctx):
    """Every fresh allocation (the output among them), the cached workspace and the library's scratch hold 0x00, then
    0xFF (NaN), then 0x7E bytes: the result is finite and the same - every channel of the output is written by a gather,
    the padding channel by the driver.  Criterion "atomic": the analysis ends in the run-time ring kernel."""
    from _poison import poisoned_runs
    from cora_amd.util import hputil

    nside, lmax, F, npol = 8, 16, 5, 3                                                 # 15 channels: one padding channel
    maps, _ = _subset(*_sky_case(nside, lmax, 3), 3, npol)
    dev = ctx.to_device(np.concatenate([maps, 0.5 * maps[:2]]))
    assert dev.shape[0] == F
    poisoned_runs(ctx, lambda: hputil.map2alm_sky_device(dev, lmax=lmax, chunk=4), criterion="atomic",
                  label="map2alm_sky_device F 5 npol 3 chunk 4")


def test_sky_analysis_refuses_host_tensors_and_other_dtypes(ctx):
    import torch
    from cora_amd.util import hputil

    for bad in (torch.zeros((2, 3, 48), dtype=torch.float64), torch.zeros((2, 3, 48), dtype=torch.float32, device=ctx.device),
                np.zeros((2, 3, 48))):
        with pytest.raises(ValueError):
            hputil.map2alm_sky_device(bad)


# ---- 3. the spectra ----------------------------------------------------------------------------------------------
def _device_sky_alm(ctx, maps, lmax, **kw):
    from cora_amd.util import hputil

    n = maps.shape[0] * maps.shape[1]
    return po.device_packed(ctx, hputil.map2alm_sky_device(ctx.to_device(maps), lmax=lmax, **kw), lmax, n)


def test_spectra_against_the_gram_of_the_device_coefficients(ctx):
    import torch
    from cora_amd.core import skysim
    from cora_amd.util import hputil

    nside, lmax = 16, 24
    big, ref = _sky_case(nside, lmax)
    maps, _ = _subset(big, ref, 3, 3)                                                  # F = 3, (T, Q, U)
    maps2 = np.ascontiguousarray(big[5:7])                                             # F2 = 2, (T, Q, U, V)
    dmaps, dmaps2 = ctx.to_device(maps), ctx.to_device(maps2)
    a, b = _device_sky_alm(ctx, maps, lmax), _device_sky_alm(ctx, maps2, lmax)
    S, Sabs = po.gram(a, a, lmax)
    cd = skysim.clarray_from_maps(dmaps, lmax=lmax)
    ch = skysim.clarray_from_maps(maps, lmax=lmax)
    cs = hputil.cross_spectra_pol_device(dmaps, lmax=lmax)
    assert isinstance(cd, torch.Tensor) and isinstance(ch, np.ndarray) and tuple(cd.shape) == ch.shape == (lmax + 1, 9, 9)
    r1 = max(po.ratio(np.abs(x - S), po.gram_tol(Sabs)) for x in (cd.cpu().numpy(), ch, cs.cpu().numpy()))
    for x in (cd, cs):
        assert torch.equal(x, x.transpose(1, 2))                                                   # bitwise symmetric
    assert np.array_equal(ch, ch.transpose(0, 2, 1))
    # identical bits from call to call: the gather and the Gram product on the same coefficients (a second analysis may
    # fold the aliased bins of a ring in another order - tests/test_gpu_poison.py, criterion "atomic" - and is held to
    # the tolerance above instead)
    da, db = hputil.map2alm_sky_device(dmaps, lmax=lmax), hputil.map2alm_sky_device(dmaps2, lmax=lmax)
    g1 = ctx.alm_cross_spectra(da, 9, lmax)
    assert torch.equal(ctx.alm_cross_spectra(da, 9, lmax), g1) and torch.equal(g1, g1.transpose(1, 2))
    gx = ctx.alm_cross_spectra(da, 9, lmax, alm_b=db, ny=8)
    assert torch.equal(ctx.alm_cross_spectra(db, 8, lmax, alm_b=da, ny=9), gx.transpose(1, 2).contiguous())
    # the documented index rule: C.reshape(L, P, F, P, F)[l, p, i, q, j]
    c5 = ch.reshape(lmax + 1, 3, 3, 3, 3)
    assert c5[7, 1, 2, 2, 0] == ch[7, hputil.sky_channel(1, 2, 3), hputil.sky_channel(2, 0, 3)]
    # two stacks, F != F2 and npol != npol2
    Sx, Sxabs = po.gram(a, b, lmax)
    cx = hputil.cross_spectra_pol_device(dmaps, dmaps2, lmax=lmax)
    assert tuple(cx.shape) == (lmax + 1, 9, 8)
    r2 = po.ratio(np.abs(cx.cpu().numpy() - Sx), po.gram_tol(Sxabs))
    cxt = hputil.cross_spectra_pol_device(dmaps2, dmaps, lmax=lmax).cpu().numpy()
    r2 = max(r2, po.ratio(np.abs(cxt.transpose(0, 2, 1) - Sx), po.gram_tol(Sxabs)))
    # default lmax = 3 nside - 1
    assert skysim.clarray_from_maps(dmaps[:1]).shape == (3 * nside, 3, 3)
    # anafast_pol: healpy's defaults (no weights, three refinements), TT EE BB TE EB TB of one (T, Q, U) map
    one, two = maps[1], maps2[0, :3]
    a3 = _device_sky_alm(ctx, one[None], lmax, use_weights=False, niter=3)
    b3 = _device_sky_alm(ctx, two[None], lmax, use_weights=False, niter=3)
    i, j = hputil.spectra_pair_order(3)
    assert list(zip(i.tolist(), j.tolist())) == [(0, 0), (1, 1), (2, 2), (0, 1), (1, 2), (0, 2)]
    S3, S3abs = po.gram(a3, a3, lmax)
    cl = hputil.anafast_pol(one, lmax=lmax)
    assert cl.shape == (6, lmax + 1)
    r3 = po.ratio(np.abs(cl - S3[:, i, j].T), po.gram_tol(S3abs)[:, i, j].T)
    X3, X3abs = po.gram(a3, b3, lmax)
    clx = hputil.anafast_pol(one, two, lmax=lmax)
    r4 = po.ratio(np.abs(clx - X3[:, i, j].T), po.gram_tol(X3abs)[:, i, j].T)
    two_stack = hputil.cross_spectra_pol_device(ctx.to_device(one[None]), ctx.to_device(two[None]), lmax=lmax, use_weights=False,
                                                niter=3).cpu().numpy()
    r4 = max(r4, po.ratio(np.abs(two_stack[:, i, j].T - X3[:, i, j].T), po.gram_tol(X3abs)[:, i, j].T))
    assert hputil.anafast_pol(one).shape == (6, 3 * nside)
    print("spectra: clarray_from_maps / cross_spectra_pol_device %.3f, two stacks %.3f, anafast_pol %.3f, with map2 %.3f"
          % (r1, r2, r3, r4))
    assert max(r1, r2, r3, r4) <= 1.0


# ---- 4. properties -----------------------------------------------------------------------------------------------
def _pair_delta(ref, F):
    """1e-11 max(|a^E|, |a^B|) per frequency channel of field-major oracle coefficients"""
    return po.ALM_GATE * np.maximum(np.abs(ref[F:2 * F]).max(axis=1), np.abs(ref[2 * F:3 * F]).max(axis=1))


def test_pure_e_sky_has_no_more_bb_than_the_gate_allows(ctx):
    """B coefficients zero in the input.  The oracle's own B (the leakage of two refinements, not rounding) has norm_l(B)
    per l; device coefficients within delta of it have sqrt(BB_l) <= norm_l(B_oracle) + delta, the Gram product adds
    (2 (l + 1) + 3) eps BB_l (_polspectra_oracle: properties)."""
    from cora_amd.core import skysim

    nside, lmax, F = 16, 24, 2
    maps, ref = _sky_case(nside, lmax, F, seed=1, pure_e=True)
    maps, ref = _subset(maps, ref, F, 3)
    C = skysim.clarray_from_maps(maps, lmax=lmax).reshape(lmax + 1, 3, F, 3, F)
    bb = np.stack([C[:, 2, f, 2, f] for f in range(F)])                                # [F, L]
    ee = np.stack([C[:, 1, f, 1, f] for f in range(F)])
    l = np.arange(lmax + 1)
    bound = (po.norm_l(ref[2 * F:], lmax) + _pair_delta(ref, F)[:, None]) ** 2 * (1 + (2 * (l + 1) + 3) * po.EPS)
    r = po.ratio(bb[:, 2:], bound[:, 2:])
    print("pure E: worst BB / bound %.3g; BB / EE at most %.3g" % (r, (bb[:, 2:] / ee[:, 2:]).max()))
    assert (bb >= 0).all() and not bb[:, :2].any() and r <= 1.0


def test_rotating_the_polarisation_angle_keeps_ee_plus_bb(ctx):
    """psi = 0.3 on every pixel turns (E, B) by 2 psi in every (l, m): N_l = sqrt(EE_l + BB_l) is unchanged.  With device
    coefficients within delta (delta') of the oracle's, |N' - N| <= |N'_o - N_o| + sqrt(2) (delta + delta') and
    |N'^2 - N^2| = |N' - N| (N' + N), plus the Gram rounding of the four spectra."""
    from cora_amd.core import skysim

    nside, lmax, F = 16, 24, 2
    big, ref = _sky_case(nside, lmax)
    maps, ref = _subset(big, ref, F, 3)
    rot = po.rotate_polarisation(maps, 0.3)
    ref_rot = po.analyse_sky(rot, nside, lmax, use_weights=True, niter=2)

    def power(m):
        C = skysim.clarray_from_maps(m, lmax=lmax).reshape(lmax + 1, 3, F, 3, F)
        return np.stack([C[:, 1, f, 1, f] + C[:, 2, f, 2, f] for f in range(F)])       # [F, L]

    def oracle_norm(r):
        return np.sqrt(po.norm_l(r[F:2 * F], lmax) ** 2 + po.norm_l(r[2 * F:], lmax) ** 2)

    s0, s1 = power(maps), power(rot)
    l = np.arange(lmax + 1)
    dn = np.abs(oracle_norm(ref_rot) - oracle_norm(ref)) + np.sqrt(2.0) * (_pair_delta(ref, F) + _pair_delta(ref_rot, F))[:, None]
    bound = dn * (np.sqrt(s0) + np.sqrt(s1)) + (2 * (l + 1) + 3) * po.EPS * (s0 + s1)
    r = po.ratio(np.abs(s1 - s0)[:, 2:], bound[:, 2:])
    print("rotation by psi = 0.3: worst |EE + BB change| / bound %.3g (relative change at most %.3g)"
          % (r, (np.abs(s1 - s0)[:, 2:] / s0[:, 2:]).max()))
    assert r <= 1.0
    # and the rotation did something: EE alone changes
    C0 = skysim.clarray_from_maps(maps, lmax=lmax).reshape(lmax + 1, 3, F, 3, F)
    C1 = skysim.clarray_from_maps(rot, lmax=lmax).reshape(lmax + 1, 3, F, 3, F)
    assert np.abs(C1[2:, 1, 0, 1, 0] - C0[2:, 1, 0, 1, 0]).max() > 1e-3 * C0[2:, 1, 0, 1, 0].max()


# ---- 5. memory ---------------------------------------------------------------------------------------------------
def test_temporaries_stay_below_the_stated_bound(ctx):
    import torch
    from cora_amd.util import hputil

    nside, F, npol, chunk = 32, 9, 4, 4
    lmax = 3 * nside - 1
    g = torch.Generator(device=ctx.device).manual_seed(3)
    maps = torch.randn((F, npol, 12 * nside * nside), dtype=torch.float64, device=ctx.device, generator=g)
    hputil.ring_weights(nside)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated(ctx.device)
    torch.cuda.reset_peak_memory_stats(ctx.device)
    alm = hputil.map2alm_sky_device(maps, chunk=chunk)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated(ctx.device) - base - alm.numel() * 8
    bound = hputil.map2alm_sky_bytes(nside, lmax, npol, chunk)
    print("map2alm_sky_device nside %d F %d chunk %d: peak beyond input and output %.2f MB, map2alm_sky_bytes %.2f MB"
          % (nside, F, chunk, peak / 1e6, bound / 1e6))
    assert bool(torch.isfinite(alm).all())
    assert peak <= bound, (peak, bound)
