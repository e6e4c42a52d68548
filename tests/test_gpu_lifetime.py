"""Lifetime of the library's device memory (csrc/dev_buf.h owns every allocation): a context and its plans are built up
through every owner, destroyed, and the default context is none the worse for it; a plan that is destroyed and made
again computes the same bits.  Free device memory is not looked at: the figure is device-wide, and the card is shared."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NSIDE, LMAX = 8, 23


def _rng(seed):
    return np.random.default_rng(seed)


def _alm_dev(ctx, lmax, nnu, seed):
    """alm_dev [nalm, ceil(nnu / 4), 2, 4] with zero padding lanes, real m = 0 entries and nothing below l = 2"""
    L = lmax + 1
    G = (nnu + 3) // 4
    a = _rng(seed).standard_normal((L * (L + 1) // 2, G, 2, 4))
    a[:L, :, 1, :] = 0.0
    a[[0, 1, L], :, :, :] = 0.0           # (l, m) = (0, 0), (1, 0), (1, 1): the spin-2 transform starts at l = 2
    lane = np.arange(4 * G).reshape(G, 4)
    a *= (lane < nnu)[None, :, None, :]
    return ctx.to_device(a)


def _sht(c, nnu_list=(1, 64)):
    """alm2map at nnu = 1 (K4 shape RT 2) and nnu = 64 (RT 1): both keys of the plan's lazy item list and segment seeds"""
    return [c.alm2map(_alm_dev(c, LMAX, nnu, 10 + nnu), NSIDE, LMAX, nnu).clone() for nnu in nnu_list]


def _spin2(c):
    """four (E, B) pairs: the entry point takes channel counts whose groups of four fill whole groups of eight"""
    return c.alm2map_spin2(_alm_dev(c, LMAX, 8, 7), NSIDE, LMAX, 8).clone()


def _ffts(c):
    """fft_c2c along a strided axis: 16 (power of two), 12 (run-time Bluestein), 20 (compile-time convolution, 256)"""
    import torch

    out = []
    for n in (16, 12, 20):
        r = _rng(n)
        x = torch.from_numpy(r.standard_normal((n, 3)) + 1j * r.standard_normal((n, 3))).to(c.device)
        out.append(c.fft_c2c(x, 0).clone())
    return out


def _spd(F, nl, seed):
    a = _rng(seed).standard_normal((nl, F, F))
    return a @ a.transpose(0, 2, 1) + F * np.eye(F)


def _same(a, b):
    import torch

    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


def test_second_context_built_up_and_destroyed(ctx):
    import torch

    from cora_amd import _lib

    before = _sht(ctx) + _ffts(ctx)

    c2 = _lib.Context(0)
    maps = _sht(c2)
    assert _same(maps, before[:2])                             # the same library, the same bits on either context
    assert bool(torch.isfinite(_spin2(c2)).all())              # d_polc
    alm = c2.map2alm(maps[1], NSIDE, LMAX)
    assert bool(torch.isfinite(alm).all())
    assert c2.k4_mfma_count(NSIDE, LMAX, 1) > 0 and c2.k4_mfma_count(NSIDE, LMAX, 64) > 0
    assert _same(_ffts(c2), before[2:])
    # Philox draws at two lmax: the context's slot table is built, then replaced
    F = 8
    for lmax in (5, 9):
        T, info = c2.factor_batched(c2.to_device(_spd(F, lmax + 1, lmax)))
        assert int(info.abs().sum()) == 0
        assert bool(torch.isfinite(c2.draw_alm_philox(T, None, 99, lmax, F)).all())
    # a 4 x 4 batch with one indefinite matrix: per-call buffers of the eigen route
    C = _spd(4, 4, 3)
    C[2] -= 2.0 * np.linalg.eigvalsh(C[2])[1] * np.eye(4)
    T, info = c2.factor_batched(c2.to_device(C))
    assert info.cpu().tolist() == [0, 0, 1, 0] and bool(torch.isfinite(T).all())
    # eig_top_batched with one product: at F = 8 the block spans the space and the iteration ends at once; at F = 17,
    # the smallest F it does not span, every block goes to the full decomposition and its per-call buffers
    for F, route in ((8, 0), (17, 1)):
        V, theta, info = c2.eig_top_batched(c2.to_device(_spd(F, 3, F)), 2, max_iter=1)
        assert info.cpu().tolist() == [route] * 3, (F, info)
        assert bool(torch.isfinite(V).all()) and bool(torch.isfinite(theta).all())

    c2.sync()
    assert len(c2._plans) >= 1
    for plan in c2._plans.values():
        assert c2.lib.corahip_sht_plan_destroy(c2.h, plan) == 0
    c2._plans.clear()
    assert c2.lib.corahip_ctx_destroy(c2.h) == 0
    c2.h = None

    assert _same(_sht(ctx) + _ffts(ctx), before)


def test_plan_destroyed_and_made_again(ctx):
    before = _sht(ctx, (1,)) + [_spin2(ctx)]
    ctx.sync()
    plan = ctx.sht_plan(NSIDE, LMAX)
    key = next(k for k, v in ctx._plans.items() if v is plan)
    del ctx._plans[key]
    assert ctx.lib.corahip_sht_plan_destroy(ctx.h, plan) == 0
    assert _same(_sht(ctx, (1,)) + [_spin2(ctx)], before)
    assert key in ctx._plans and ctx._plans[key] is not plan
