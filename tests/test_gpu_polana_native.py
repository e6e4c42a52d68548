"""The native spin-2 analysis on the GPU: ``Context.map2alm_spin2_native`` (csrc/sht_polana_native.hip: K5^T on the
(Q, U) channels as they are + legendre_adj_pol_kernel, the adjoint of the spin-2 synthesis kernel) and the
native route of ``hputil`` (``map2alm_pol_device(method="native")``; ``spin2_method("native")`` for the entry points
whose call surfaces are pinned).

Bounds - the gates the composed pass is already held to, no new numbers:
  quadrature pass   2e-12 max(|E|, |B|) of the field against oracle.sht.map2alm_spin2_adjoint
                    (tests/test_gpu_parity.py::test_map2alm_spin2_quadrature_vs_oracle); 4e-12 between the two routes
                    (each lies within 2e-12 of the one oracle)
  whole route       1e-11 max|a| against oracle.sht.map2alm_spin2(niter=2) (tests/_polspectra_oracle.py)
  adjointness       2e-11 sum|terms|: the 1e-11 synthesis gate plus the analysis gate
  determinism       none: bit for bit
The oracle of a shape is computed once per session and shared."""
import functools

import numpy as np
import pytest

import _polspectra_oracle as po
from _poison import poisoned_runs

pytestmark = pytest.mark.gpu

PASS_GATE = 2e-12


@functools.lru_cache(maxsize=None)
def _maps(nside, nf):
    """(Q_f, U_f) interleaved [2 nf, npix]; read-only"""
    qu = np.random.default_rng(7 * nside + nf).standard_normal((2 * nf, 12 * nside * nside))
    qu.setflags(write=False)
    return qu


@functools.lru_cache(maxsize=None)
def _oracle(nside, lmax, nf, weights, ms):
    """packed (E, B) [nf, 2, nalm] of one quadrature pass of _maps(nside, nf)"""
    from oracle import sht

    qu = _maps(nside, nf)
    w = sht.ring_weights(nside) if weights else None
    out = np.array([sht.map2alm_spin2_adjoint(qu[2 * f], qu[2 * f + 1], nside, lmax, w, ms=ms) for f in range(nf)])
    out.setflags(write=False)
    return out


def _weights(ctx, nside, weights):
    from oracle import sht

    return ctx.to_device(sht.ring_weights(nside)) if weights else None


def _dev(ctx, a):
    import torch

    return torch.from_numpy(np.array(a, dtype=np.float64)).to(ctx.device)     # (a copy: the shared inputs are read-only)


def _packed_all(ctx, alm_dev, lmax):
    """every channel of alm_dev, padding included, packed [4 G, nalm]"""
    return po.device_packed(ctx, alm_dev, lmax, 4 * alm_dev.shape[1])


# ---- 1. the quadrature pass against the oracle ---------------------------------------------------------------------
@pytest.mark.parametrize("nside,lmax,nf,weights,ms", [
    (4, 8, 1, False, None),                            # 8 of 512 tile lanes live, a single ragged l-block
    (8, 23, 2, True, None),                            # lmax = 3 nside - 1
    (16, 40, 3, True, None),                           # 6 channels padded to 8; L = 41 ends mid-block
    (32, 95, 2, True, None),                           # polar rings with m >= mcut, late lstart
    (32, 64, 5, False, None),                          # 10 channels -> two 8-groups: the other NCT dispatch
    (256, 40, 1, True, (0, 2, 40)),                    # npair = 512: exactly one full ring tile
    (512, 70, 1, True, (0, 1, 2, 3, 35, 69, 70)),      # two ring tiles, three l-blocks: paired and single reduction
])
def test_quadrature_pass_against_the_oracle(ctx, nside, lmax, nf, weights, ms):
    ref = _oracle(nside, lmax, nf, weights, ms)
    dev = ctx.map2alm_spin2_native(_dev(ctx, _maps(nside, nf)), nside, lmax, _weights(ctx, nside, weights))
    assert tuple(dev.shape) == ((lmax + 1) * (lmax + 2) // 2, (2 * nf + 7) // 8 * 2, 2, 4)
    got = _packed_all(ctx, dev, lmax)
    l, m = po.lm(lmax)
    sel = np.ones(l.size, dtype=bool) if ms is None else np.isin(m, ms)
    worst = 0.0
    for f in range(nf):
        e, b = ref[f]
        scale = max(np.abs(e).max(), np.abs(b).max())
        err = max(np.abs(got[2 * f] - e)[sel].max(), np.abs(got[2 * f + 1] - b)[sel].max())
        worst = max(worst, err / scale)
        assert err < PASS_GATE * scale, (f, err, scale)
    print("native pass nside %d lmax %d nf %d: worst error %.3g of the field's max (gate %.0e)" % (nside, lmax, nf, worst, PASS_GATE))
    assert np.isfinite(got.view(np.float64)).all()
    assert not got[:, l < 2].any()                     # l < 2 carries no spin-2 power: exact zeros
    assert not got[2 * nf:].any()                      # and so are the padding channels


# ---- 2. native against composed ------------------------------------------------------------------------------------
@pytest.mark.parametrize("nside,lmax,nf,weights", [(32, 64, 5, False), (512, 70, 1, True)])
def test_native_against_composed(ctx, nside, lmax, nf, weights):
    qu, w = _dev(ctx, _maps(nside, nf)), _weights(ctx, nside, weights)
    a = _packed_all(ctx, ctx.map2alm_spin2_native(qu, nside, lmax, w), lmax)
    c = _packed_all(ctx, ctx.map2alm_spin2(qu, nside, lmax, w), lmax)
    assert a.shape == c.shape
    for f in range(nf):
        scale = np.abs(c[2 * f:2 * f + 2]).max()
        err = np.abs(a[2 * f:2 * f + 2] - c[2 * f:2 * f + 2]).max()
        print("native - composed nside %d lmax %d field %d: %.3g of the field's max" % (nside, lmax, f, err / scale))
        assert err < 2 * PASS_GATE * scale, (f, err, scale)


# ---- 3. determinism and poison -------------------------------------------------------------------------------------
@pytest.mark.parametrize("nside,lmax", [(32, 64), (512, 70)])
def test_bit_identical_on_poisoned_workspace_and_output(ctx, nside, lmax):
    import torch

    nf = 2
    qu, w = _dev(ctx, _maps(nside, nf)), _weights(ctx, nside, True)
    ctx.map2alm_spin2_native(qu, nside, lmax, w)       # plan, tables and workspace exist before the first compared run
    ref, report = poisoned_runs(ctx, lambda: ctx.map2alm_spin2_native(qu, nside, lmax, w), valid=lambda r: r[:, :1],
                                criterion="exact", label="map2alm_spin2_native %d %d" % (nside, lmax))
    assert bool((ref[0] != 0).any())
    again = ctx.map2alm_spin2_native(qu, nside, lmax, w)
    assert torch.equal(again[:, :1], ref[0])           # and from call to call


# ---- 4. chunking ---------------------------------------------------------------------------------------------------
def test_chunks_of_four_fields_against_one_call(ctx):
    import torch

    nside, lmax, nf = 16, 40, 9
    qu, w = _dev(ctx, _maps(nside, nf)), _weights(ctx, nside, True)
    one = ctx.map2alm_spin2_native(qu, nside, lmax, w)
    parts = ctx.map2alm_spin2_native(qu, nside, lmax, w, chunk=4)
    assert one.shape == parts.shape
    a, b = _packed_all(ctx, one, lmax), _packed_all(ctx, parts, lmax)
    for f in range(nf):
        scale = np.abs(a[2 * f:2 * f + 2]).max()
        assert np.abs(a[2 * f:2 * f + 2] - b[2 * f:2 * f + 2]).max() <= PASS_GATE * scale, f
    assert not b[2 * nf:].any()
    print("chunks of 4 fields against one call: bits equal = %s" % torch.equal(one, parts))
    with pytest.raises(AssertionError):
        ctx.map2alm_spin2_native(qu, nside, lmax, w, chunk=6)


# ---- 5. adjointness ------------------------------------------------------------------------------------------------
def test_native_pass_is_the_adjoint_of_the_synthesis(ctx):
    import torch

    nside, lmax = 16, 40
    npix = 12 * nside * nside
    rng = np.random.default_rng(40)
    eb = po.random_sky_alm(rng, lmax, 1, 3)[1:3, 0]                           # band-limited (e, b), zero below l = 2
    qu = rng.standard_normal((2, npix))
    synth = ctx.alm2map_spin2(_dev(ctx, po.to_layout(np.concatenate([eb, np.zeros((6, eb.shape[1]))]))), nside, lmax, 8)[:2]
    lhs_terms = (4.0 * np.pi / npix) * (qu * synth.cpu().numpy())
    ana = _packed_all(ctx, ctx.map2alm_spin2_native(_dev(ctx, qu), nside, lmax), lmax)[:2]
    l, m = po.lm(lmax)
    rhs_terms = np.where(m == 0, 1.0, 2.0) * (np.conj(eb) * ana).real
    lhs, rhs = lhs_terms.sum(), rhs_terms.sum()
    tol = 2e-11 * min(np.abs(lhs_terms).sum(), np.abs(rhs_terms).sum())
    print("<q, S a> = %.15g, <A q, a> = %.15g, difference %.3g, bound %.3g" % (lhs, rhs, abs(lhs - rhs), tol))
    assert abs(lhs) > 1e3 * tol                                                # the products are not trivially small
    assert abs(lhs - rhs) <= tol


# ---- 6. the whole route --------------------------------------------------------------------------------------------
def test_refined_analysis_against_the_oracle(ctx):
    from cora_amd.util import hputil
    from oracle import sht

    nside, lmax = 16, 24
    rng = np.random.default_rng(24)
    eb = po.random_sky_alm(rng, lmax, 1, 3)[1:3, 0]
    q, u = sht.alm2map_spin2(eb[0], eb[1], nside, lmax)
    alm = hputil.map2alm_pol_device(_dev(ctx, np.stack([q, u])), nside, lmax, method="native")
    got = _packed_all(ctx, alm, lmax)                  # (the buffer is padded to 8 channels: two groups)
    assert not got[2:].any()
    e, b = sht.map2alm_spin2(q, u, nside, lmax, use_weights=True, niter=2)
    scale = max(np.abs(e).max(), np.abs(b).max())
    err = max(np.abs(got[0] - e).max(), np.abs(got[1] - b).max())
    print("map2alm_pol_device(method='native') against the oracle: %.3g of max|a| (gate %.0e)" % (err / scale, po.ALM_GATE))
    assert err <= po.ALM_GATE * scale


def test_sky_analysis_puts_the_native_planes_field_major(ctx):
    import torch
    from cora_amd.util import hputil

    nside, F, npol = 16, 3, 4
    lmax = 3 * nside - 1
    npix = 12 * nside * nside
    g = torch.Generator(device=ctx.device).manual_seed(16)
    maps = torch.randn((F, npol, npix), dtype=torch.float64, device=ctx.device, generator=g)
    with hputil.spin2_method("native"):
        sky = po.device_packed(ctx, hputil.map2alm_sky_device(maps), lmax, npol * F)
    assert hputil._spin2_method == "composed"
    scal = po.device_packed(ctx, hputil.map2alm_device(torch.cat([maps[:, 0], maps[:, 3]]), nside, lmax), lmax, 2 * F)
    pol = po.device_packed(ctx, hputil.map2alm_pol_device(maps[:, 1:3].contiguous().view(2 * F, npix), nside, lmax,
                                                          method="native"), lmax, 2 * F)
    for f in range(F):
        assert np.array_equal(sky[hputil.sky_channel(0, f, F)], scal[f])
        assert np.array_equal(sky[hputil.sky_channel(3, f, F)], scal[F + f])
        assert np.array_equal(sky[hputil.sky_channel(1, f, F)], pol[2 * f])
        assert np.array_equal(sky[hputil.sky_channel(2, f, F)], pol[2 * f + 1])
    assert np.abs(pol).max() > 0


# ---- 7. memory -----------------------------------------------------------------------------------------------------
def test_native_temporaries_stay_below_a_smaller_bound(ctx):
    import torch
    from cora_amd.util import hputil

    nside, lmax, F, npol, chunk = 64, 128, 8, 3, 4
    g = torch.Generator(device=ctx.device).manual_seed(64)
    maps = torch.randn((F, npol, 12 * nside * nside), dtype=torch.float64, device=ctx.device, generator=g)
    hputil.ring_weights(nside)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated(ctx.device)
    torch.cuda.reset_peak_memory_stats(ctx.device)
    with hputil.spin2_method("native"):
        alm = hputil.map2alm_sky_device(maps, lmax=lmax, chunk=chunk)
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated(ctx.device) - base - alm.numel() * 8
        native = hputil.map2alm_sky_bytes(nside, lmax, npol, chunk)
    composed = hputil.map2alm_sky_bytes(nside, lmax, npol, chunk)
    print("map2alm_sky_device under spin2_method('native') nside %d F %d chunk %d: peak beyond input and output %.2f MB, bound %.2f MB "
          "(composed bound %.2f MB)" % (nside, F, chunk, peak / 1e6, native / 1e6, composed / 1e6))
    assert bool(torch.isfinite(alm).all())
    assert peak < native, (peak, native)
    assert native < composed, (native, composed)
