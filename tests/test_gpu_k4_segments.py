"""legendre_kernel's lane groups walk contiguous quarters of an item's l range (csrc/sht_internal.h: leg_seg).
Entry states of the four segments, maps at the shapes where the segment addressing can go wrong, bit-identity within a
ring-tile height and determinism under the dynamic queue.  Run with -m gpu."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ORACLE_TOL = 1e-11          # of the map's rms: the tolerance of test_gpu_parity.test_alm2map_vs_oracle


def _rand_alm(rng, nnu, lmax):
    nalm = (lmax + 1) * (lmax + 2) // 2
    a = rng.standard_normal((nnu, nalm)) + 1j * rng.standard_normal((nnu, nalm))
    l = np.concatenate([np.arange(m, lmax + 1) for m in range(lmax + 1)])
    return a / (1.0 + l) ** 1.0


@functools.lru_cache(maxsize=None)
def _case(nside, lmax):
    """Four distinct a_lm and their oracle maps, computed once per shape and never modified."""
    from oracle import sht

    alm = _rand_alm(np.random.default_rng(1000 * nside + lmax), 4, lmax)
    ref = np.stack([sht.alm2map(a, nside, lmax) for a in alm])
    alm.setflags(write=False)
    ref.setflags(write=False)
    return alm, ref


def _maps(ctx, alm4, nside, lmax, nnu):
    """The four a_lm repeated over nnu channels through one alm2map call."""
    import torch

    alm = alm4[np.arange(nnu) % 4]
    dev = ctx.alm_packed_to_dev(torch.from_numpy(np.ascontiguousarray(alm)).to(ctx.device), lmax)
    return ctx.alm2map(dev, nside, lmax, nnu).cpu().numpy()


# ------------------------------------------------------------------ 1. entry states
@pytest.mark.parametrize("nside,lmax,rt", [(16, 47, 1), (64, 191, 1), (64, 191, 2)])
def test_lambda_from_the_segment_entry_states(ctx, nside, lmax, rt):
    """Lane group kq owns rows [R_kq, R_kq + 2 T), R_kq = l_begin + 2 kq T.  Its lambda (corahip_sht_lambda_segment_entry)
    must equal the single-start device form from its entry row to the segment's end and be zero elsewhere; the four
    segments partition [l_begin, l_begin + 8 T); the pairs the four groups include are exactly the pairs whose even
    row is >= lstart - 1."""
    from oracle import healpix, sht

    ri = healpix.ring_info(nside)
    npair = 2 * nside
    for m in (0, 1, lmax // 2, lmax - 1, lmax):
        for pair in (0, nside // 2, npair - 2, npair - 1):
            ref = sht.lambda_lm(lmax, m, ri["z"][pair])
            one = ctx.sht_lambda(nside, lmax, m, pair).cpu().numpy()
            scale = max(np.abs(ref).max(), 1e-300)
            nz = np.nonzero(one)[0]
            ls = m + (int(nz[0]) if len(nz) else lmax + 1 - m)         # the plan's first contributing row
            covered = np.zeros(lmax + 1 - m, dtype=int)
            for kq in range(4):
                dev, (l_begin, T, R, erow) = ctx.sht_lambda_segment_entry(nside, lmax, rt, m, pair, kq)
                dev = dev.cpu().numpy()
                tag = (m, pair, kq, l_begin, T, R, erow, ls)
                # geometry: the same item start and macro-step count as ever, four contiguous quarters
                assert (l_begin - m) % 8 == 0 and m <= l_begin and (ls > lmax or l_begin <= ls), tag
                assert T == (lmax - l_begin) // 8 + 1 and R == l_begin + kq * 2 * T, tag
                assert l_begin + 8 * T > lmax, tag
                # entry row: the segment's first row if that is >= lstart - 1, else the first R + 2 t >= lstart - 1 in it
                want = -1
                if ls <= lmax:
                    first = R if R >= ls - 1 else R + 2 * ((ls - 1 - R + 1) // 2)
                    want = first if first < R + 2 * T else -1
                assert erow == want, tag
                if erow < 0 or erow > lmax:
                    assert not dev.any(), tag
                    continue
                end = min(R + 2 * T - 1, lmax)                          # last row of the segment that exists
                assert not dev[: erow - m].any() and not dev[end + 1 - m:].any(), tag
                covered[erow - m: end + 1 - m] += 1
                k0 = max(erow, ls) - m
                base = np.abs(one[k0:] - ref[k0:]).max()
                err = np.abs(dev[erow - m: end + 1 - m] - one[erow - m: end + 1 - m]).max()
                assert err <= max(1e-13 * scale, 0.1 * base) + 2.0**-100, tag + (err, base)
            # the term set of the staggered scheme: pair (P, P + 1), P - m even, is summed iff P >= lstart - 1
            l = np.arange(m, lmax + 1)
            P = l - ((l - m) & 1)
            assert np.array_equal(covered, ((P >= ls - 1) & (ls <= lmax)).astype(int)), (m, pair, ls)


# ------------------------------------------------------------------ 2. maps against the oracle
@pytest.mark.parametrize("nside,lmax", [(64, 6), (64, 7), (64, 8),              # T = 1, 2: segments almost entirely past lmax
                                        (64, 55), (64, 56), (64, 57),           # T = 7, 8: one stage, the rolled tail
                                        (64, 111), (64, 112),                   # T = 14, 15: two stages
                                        (16, 47),                               # 32 ring pairs: a partial tile
                                        (128, 300),                             # two tiles, lstart spread over segments
                                        (8, 40)])                               # lmax > 4 nside
def test_alm2map_segments_vs_oracle(ctx, nside, lmax):
    alm4, ref = _case(nside, lmax)
    maps = _maps(ctx, alm4, nside, lmax, 64)                                    # 64 channels: legendre_kernel<8,1>
    assert maps.shape == (64, ref.shape[1])
    err = np.abs(maps - ref[np.arange(64) % 4]).max() / ref.std()
    print("nside %d lmax %d: max|err|/rms = %.3e" % (nside, lmax, err))
    assert err < ORACLE_TOL, err


# ------------------------------------------------------------------ 3. shapes
def test_bit_identity_within_a_tile_height(ctx):
    """The order in which an accumulator sums its rows depends on the item's l_begin, hence on the ring-tile height:
    128-ring tiles (64 and more channels per call) and 256-ring tiles (fewer) each give bit-identical maps whatever the
    channel count, and the two families agree to rounding."""
    nside, lmax = 64, 191
    alm4, ref = _case(nside, lmax)
    wide = _maps(ctx, alm4, nside, lmax, 64)
    wide128 = _maps(ctx, alm4, nside, lmax, 128)
    assert np.array_equal(wide128[:64], wide) and np.array_equal(wide128[64:], wide)
    narrow = {n: _maps(ctx, alm4, nside, lmax, n) for n in (32, 16, 8)}
    assert np.array_equal(narrow[32][:16], narrow[16]) and np.array_equal(narrow[32][16:], narrow[16])
    assert np.array_equal(narrow[16][:8], narrow[8]) and np.array_equal(narrow[16][8:], narrow[8])
    for maps in (wide, narrow[8]):
        n = maps.shape[0]
        assert np.abs(maps - ref[np.arange(n) % 4]).max() / ref.std() < ORACLE_TOL
    assert np.abs(wide[:8] - narrow[8]).max() / ref.std() < ORACLE_TOL


# ------------------------------------------------------------------ 4. determinism
def test_two_launches_are_bit_identical(ctx):
    """Which workgroup takes which item is decided by the dynamic queue: it must not matter."""
    nside, lmax = 128, 300
    alm4, _ = _case(nside, lmax)
    assert np.array_equal(_maps(ctx, alm4, nside, lmax, 64), _maps(ctx, alm4, nside, lmax, 64))
