"""Parity of the HIP path (through the C ABI) against the CPU oracle.  Run with -m gpu."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _rel(a, b):
    return np.abs(np.asarray(a) - np.asarray(b)).max() / np.abs(b).max()


def _rand_alm(rng, nnu, lmax):
    nalm = (lmax + 1) * (lmax + 2) // 2
    a = rng.standard_normal((nnu, nalm)) + 1j * rng.standard_normal((nnu, nalm))
    # realistic red spectrum so that no single l dominates rounding
    from oracle import sht

    l = np.concatenate([np.arange(m, lmax + 1) for m in range(lmax + 1)])
    return a / (1.0 + l) ** 1.0


# ------------------------------------------------------------------ geometry / Legendre
@pytest.mark.parametrize("nside", [1, 2, 8, 64])
def test_ring_geometry(ctx, nside):
    from oracle import healpix

    ri = healpix.ring_info(nside)
    dv = ctx.sht_rings(nside, 2 * nside)
    assert np.array_equal(dv["start"], ri["start"])
    assert np.array_equal(dv["nphi"], ri["nphi"])
    assert np.allclose(dv["z"], ri["z"], rtol=0, atol=1e-16)
    assert np.allclose(dv["phi0"], ri["phi0"], rtol=0, atol=1e-16)


@pytest.mark.parametrize("nside,lmax,m,pair", [(8, 16, 0, 3), (8, 16, 5, 0), (64, 128, 100, 2), (64, 128, 128, 127),
                                              (256, 512, 500, 0), (256, 512, 400, 30), (1024, 2048, 2000, 5),
                                              (1024, 2048, 1000, 400), (1024, 2048, 2048, 2047)])
def test_lambda_recurrence(ctx, nside, lmax, m, pair):
    """Device recurrence incl. polar seed table vs the oracle's scaled recurrence."""
    from oracle import healpix, sht

    ri = healpix.ring_info(nside)
    ref = sht.lambda_lm(lmax, m, ri["z"][pair])
    dev = ctx.sht_lambda(nside, lmax, m, pair).cpu().numpy()
    scale = max(np.abs(ref).max(), 1e-300)
    # terms below 2^-70 (8.5e-22) are dropped on the device by design (SEED_MIN_EXP, csrc/sht_plan.hip)
    assert np.abs(dev - ref).max() <= 1e-11 * scale + 2.0**-69


@pytest.mark.parametrize("nside,lmax,m,pair", [(8, 16, 0, 3), (8, 16, 5, 0), (8, 16, 16, 1), (64, 128, 100, 2),
                                              (64, 128, 127, 3), (256, 512, 500, 0), (256, 512, 400, 30),
                                              (1024, 2048, 2000, 5), (1024, 2048, 1000, 400), (1024, 2048, 1, 0),
                                              (1024, 2048, 2047, 900), (1024, 2048, 2048, 2047)])
def test_lambda_from_the_lane_group_entry_states(ctx, nside, lmax, m, pair):
    """Round 4: legendre_kernel's lanes enter at a window start from the plan's FOUR entry states per (m, ring)
    (sht_plan.hip seed_kernel, d_seed4: one per lane group kq, in front of row R = m + 2 kq + 8 k >= lstart - 1).  The
    recurrence started from each of them (corahip_sht_lambda_entry) must reproduce the oracle's lambda_lm from its entry
    row on - including the rows lstart - 1 .. lstart - 3 it may carry below the cut, the start at l = m through the
    state (-mu_m, 0), and the last m - and be zero in front of it."""
    from oracle import healpix, sht

    ri = healpix.ring_info(nside)
    ref = sht.lambda_lm(lmax, m, ri["z"][pair])
    one = ctx.sht_lambda(nside, lmax, m, pair).cpu().numpy()
    scale = max(np.abs(ref).max(), 1e-300)
    nz = np.nonzero(one)[0]
    ls = m + (int(nz[0]) if len(nz) else lmax + 1 - m)             # the plan's first contributing row
    for kq in range(4):
        dev = ctx.sht_lambda_entry(nside, lmax, m, pair, kq).cpu().numpy()
        t = ls - 1 - m - 2 * kq
        R = m + 2 * kq + (((t + 7) >> 3) << 3 if t > 0 else 0)
        if ls > lmax or R > lmax:           # the ring (or this lane group) never enters
            assert not dev.any()
            continue
        assert not dev[: max(0, R - m)].any(), (kq, R)
        # as close to the oracle as the single-start form is (the ring next to the pole at m = 1 is ill-conditioned for
        # ANY double recurrence: 5e-11 of the scale there, 1e-13 elsewhere)
        base = np.abs(one[max(ls, R) - m:] - ref[max(ls, R) - m:]).max()
        assert np.abs(dev[R - m:] - ref[R - m:]).max() <= max(1e-11 * scale, 3.0 * base) + 2.0**-69, (kq, R, ls)
        # from the later of the two starts on, the two device forms agree to rounding (times that conditioning)
        k0 = max(R, ls) - m
        assert np.abs(dev[k0:] - one[k0:]).max() <= max(1e-13 * scale, 0.1 * base) + 2.0**-100, (kq, R, ls)


# ------------------------------------------------------------------ K4 + K5
@pytest.mark.parametrize("nside,lmax,nnu", [(1, 2, 1), (2, 5, 3), (4, 11, 8), (8, 16, 4), (8, 23, 9), (16, 32, 16),
                                            (32, 95, 5), (64, 128, 24),
                                            # legendre_kernel<1,2>, <2,2>, <4,2>, <8,1> with head, steady-state and tail stages
                                            (64, 191, 8), (64, 191, 16), (64, 191, 32), (64, 191, 64)])
def test_alm2map_vs_oracle(ctx, nside, lmax, nnu):
    import torch
    from oracle import sht

    rng = np.random.default_rng(100 * nside + nnu)
    alm = _rand_alm(rng, nnu, lmax)
    ref = np.stack([sht.alm2map(a, nside, lmax) for a in alm])
    dev = ctx.alm_packed_to_dev(torch.from_numpy(alm).to(ctx.device), lmax)
    maps = ctx.alm2map(dev, nside, lmax, nnu).cpu().numpy()
    assert maps.shape == ref.shape
    err = np.abs(maps - ref).max() / ref.std()
    assert err < 1e-11, err


def test_alm2map_chunked_workspace(ctx):
    """A workspace too small for all channels forces the chunked path: identical maps."""
    import torch

    nside, lmax, nnu = 16, 32, 20
    rng = np.random.default_rng(5)
    alm = _rand_alm(rng, nnu, lmax)
    dev = ctx.alm_packed_to_dev(torch.from_numpy(alm).to(ctx.device), lmax)
    full = ctx.alm2map(dev, nside, lmax, nnu).cpu().numpy()
    plan = ctx.sht_plan(nside, lmax)
    small = ctx.alm2map_workspace_bytes(plan, 8) + (lmax + 1) * (lmax + 2) // 2 * 16 * 8
    part = ctx.alm2map(dev, nside, lmax, nnu, max_workspace_bytes=small).cpu().numpy()
    assert np.abs(part - full).max() <= 1e-13 * np.abs(full).max()


def test_alm2map_single_modes(ctx):
    """Analytic maps: a_00 -> a/sqrt(4 pi); a_10 -> sqrt(3/4pi) cos(theta); a_11."""
    import torch
    from oracle import healpix

    nside, lmax = 8, 4
    theta, phi = healpix.pix2ang_ring(nside)
    nalm = (lmax + 1) * (lmax + 2) // 2
    alm = np.zeros((3, nalm), dtype=np.complex128)
    alm[0, 0] = 2.5 + 7.0j                      # a_00 (imaginary part must be ignored)
    alm[1, 1] = -1.25                           # a_10
    alm[2, (lmax + 1) + 0] = 0.5 - 0.75j        # a_11: idx = m(2 lmax+1-m)/2 + l = lmax + 1
    dev = ctx.alm_packed_to_dev(torch.from_numpy(alm).to(ctx.device), lmax)
    maps = ctx.alm2map(dev, nside, lmax, 3).cpu().numpy()
    assert np.allclose(maps[0], 2.5 / np.sqrt(4 * np.pi), rtol=0, atol=1e-14)
    assert np.allclose(maps[1], -1.25 * np.sqrt(3 / (4 * np.pi)) * np.cos(theta), rtol=0, atol=1e-14)
    a = 0.5 - 0.75j
    ref = -np.sqrt(3 / (8 * np.pi)) * 2 * (a * np.exp(1j * phi)).real * np.sin(theta)
    assert np.allclose(maps[2], ref, rtol=0, atol=1e-14)


# ------------------------------------------------------------------ K2
def test_factor_cholesky_branch(ctx, golden):
    from oracle import skysim as osk

    C = golden["cla_21cm_F8_l64_zromb3"]
    T, info = ctx.factor_batched(ctx.to_device(C))
    T, info = T.cpu().numpy(), info.cpu().numpy()
    ref = osk.factors(C)
    assert np.all(info == 0)
    for l in range(C.shape[0]):
        assert np.abs(T[l] - ref[l]).max() <= 1e-12 * np.abs(ref[l]).max()
        assert np.all(np.triu(T[l], 1) == 0)


@pytest.mark.parametrize("F", [5, 33, 70, 256])
def test_factor_sizes(ctx, F):
    rng = np.random.default_rng(F)
    A = rng.standard_normal((3, F, F + 3))
    C = A @ A.transpose(0, 2, 1) + 0.1 * np.eye(F)
    T, info = ctx.factor_batched(ctx.to_device(C), jitter_rel=0.0)
    T = T.cpu().numpy()
    assert np.all(info.cpu().numpy() == 0)
    ref = np.linalg.cholesky(C)
    assert np.abs(T - ref).max() <= 1e-12 * np.abs(ref).max()


def test_factor_eigen_branch(ctx, golden):
    """Cholesky failure -> eigen root: T T^T reproduces the PSD part; zero matrix -> zero."""
    R = golden["root_rank3_in"]
    Z = np.zeros_like(R)
    rng = np.random.default_rng(2)
    V = rng.standard_normal((6, 6))
    Ind = V @ np.diag([3.0, 2.0, 1.0, 0.5, -0.2, -1e-3]) @ V.T  # indefinite
    Ind = 0.5 * (Ind + Ind.T)
    C = np.stack([R, Z, Ind])
    T, info = ctx.factor_batched(ctx.to_device(C), jitter_rel=0.0)
    T, info = T.cpu().numpy(), info.cpu().numpy()
    assert list(info) == [1, 1, 1]
    assert np.abs(T[0] @ T[0].T - R).max() <= 1e-13 * np.abs(R).max()
    assert np.all(T[1] == 0)
    ev, evec = np.linalg.eigh(Ind)
    psd = (evec * np.where(ev < ev.max() * 1e-16, 0.0, ev)) @ evec.T
    assert np.abs(T[2] @ T[2].T - psd).max() <= 1e-13 * np.abs(psd).max()


def test_factor_mfma_kernel_failure_path_and_ragged_sizes(ctx):
    """The left-looking MFMA Cholesky (even F >= 64): a block that is not positive definite is flagged and handed to the
    eigen branch (at a late pivot, a first pivot, and the zero matrix), its neighbours in the batch are untouched; sizes
    that are not multiples of the 32-column blocks; the upper triangle comes back exactly zero."""
    rng = np.random.default_rng(64)
    F = 96
    A = rng.standard_normal((4, F, F + 5))
    C = A @ A.transpose(0, 2, 1) + 0.1 * np.eye(F)
    ev, evec = np.linalg.eigh(C[1])
    ev[3] = -0.5                                        # indefinite: the Cholesky fails somewhere in the middle
    C[1] = (evec * ev) @ evec.T
    C[1] = 0.5 * (C[1] + C[1].T)
    C[2] = 0.0                                          # zero block: first pivot
    T, info = ctx.factor_batched(ctx.to_device(C), jitter_rel=0.0)
    T, info = T.cpu().numpy(), info.cpu().numpy()
    assert list(info) == [0, 1, 1, 0]
    for k in (0, 3):
        ref = np.linalg.cholesky(C[k])
        assert np.abs(T[k] - ref).max() <= 1e-12 * np.abs(ref).max()
        assert np.all(np.triu(T[k], 1) == 0)
    e1, v1 = np.linalg.eigh(C[1])
    psd = (v1 * np.where(e1 < e1.max() * 1e-16, 0.0, e1)) @ v1.T
    assert np.abs(T[1] @ T[1].T - psd).max() <= 1e-12 * np.abs(psd).max()
    assert np.all(T[2] == 0)
    # from F = 384 on the kernel takes its tall form (64-row wave tiles, the shared factor block staged once per
    # workgroup): sizes with a partial last block row / an odd number of block rows, and its failure path
    F = 400
    A = rng.standard_normal((3, F, F + 5))
    C = A @ A.transpose(0, 2, 1) + 0.1 * np.eye(F)
    ev, evec = np.linalg.eigh(C[1])
    ev[200] = -0.5
    C[1] = (evec * ev) @ evec.T
    C[1] = 0.5 * (C[1] + C[1].T)
    T, info = ctx.factor_batched(ctx.to_device(C), jitter_rel=0.0)
    T, info = T.cpu().numpy(), info.cpu().numpy()
    assert list(info) == [0, 1, 0]
    for k in (0, 2):
        ref = np.linalg.cholesky(C[k])
        assert np.abs(T[k] - ref).max() <= 1e-12 * np.abs(ref).max()
        assert np.all(np.triu(T[k], 1) == 0)
    e1, v1 = np.linalg.eigh(C[1])
    psd = (v1 * np.where(e1 < e1.max() * 1e-16, 0.0, e1)) @ v1.T
    assert np.abs(T[1] @ T[1].T - psd).max() <= 1e-11 * np.abs(psd).max()
    for F in (64, 66, 94, 130, 200, 384, 390, 418, 450, 520):
        A = rng.standard_normal((2, F, F + 2))
        C = A @ A.transpose(0, 2, 1) + 0.05 * np.eye(F)
        T, info = ctx.factor_batched(ctx.to_device(C))   # (with the reference's jitter)
        T = T.cpu().numpy()
        ref = np.linalg.cholesky(C + 1e-14 * np.einsum("lii->li", C).max(axis=1)[:, None, None] * np.eye(F))
        assert np.all(info.cpu().numpy() == 0)
        assert np.abs(T - ref).max() <= 1e-12 * np.abs(ref).max(), F
        assert np.all(np.triu(T, 1) == 0)


def test_matrix_root_manynull_api(golden):
    from cora_amd.util import nputil

    r = nputil.matrix_root_manynull(golden["root_well_in"], truncate=False)
    assert _rel(r, golden["root_well_out"]) < 1e-13
    rt, npos = nputil.matrix_root_manynull(golden["root_rank3_in"])
    assert npos == 3 and rt.shape == (1, 6, 3)  # leading axis: quirk of the reference's eigen branch
    assert np.abs(rt[0] @ rt[0].T - golden["root_rank3_in"]).max() < 1e-13 * np.abs(golden["root_rank3_in"]).max()
    z = nputil.matrix_root_manynull(np.zeros((5, 5)), truncate=False)
    assert np.array_equal(z, golden["root_zero_out"])


# ------------------------------------------------------------------ K3
@pytest.mark.parametrize("key,cl,seed,nside", [("alm_21cm_F4_l16_seed3", "cla_21cm_F4_l16_zromb1", 3, 8),
                                               ("alm_21cm_F8_l64_seed4", "cla_21cm_F8_l64_zromb3", 4, 32)])
def test_mkfullsky_alms_golden(golden, key, cl, seed, nside):
    """Same seed -> same a_lm as the reference itself (golden captured from cora)."""
    from cora_amd.core import skysim

    a = skysim.mkfullsky(golden[cl], nside, alms=True, rng=np.random.default_rng(seed))
    ref = golden[key]
    assert a.shape == ref.shape and a.dtype == np.complex128
    assert np.abs(a - ref).max() <= 1e-12 * np.abs(ref).max()


def test_mkfullsky_alms_legacy_global_rng(golden):
    from cora_amd.core import skysim

    np.random.seed(1234)
    a = skysim.mkfullsky(golden["cla_21cm_F4_l16_zromb1"], 8, alms=True)
    assert np.abs(a - golden["alm_21cm_F4_l16_legacy1234"]).max() <= 1e-12 * np.abs(a).max()


def test_mkfullsky_foreground_near_singular(golden):
    """cond ~ 1e19 blocks: factor is rounding sensitive: check T T^T = C and
    a_lm to the looser contract; l = 0 (zero block) must give exactly zero."""
    from cora_amd.core import skysim

    C = golden["cla_syn_F8_l64_zromb0"]
    a = skysim.mkfullsky(C, 32, alms=True, rng=np.random.default_rng(5))
    ref = golden["alm_syn_F8_l64_seed5"]
    assert np.all(a[:, 0, 0, :] == 0)
    assert np.abs(a - ref).max() <= 1e-4 * np.abs(ref).std()


def test_draw_shard_consistency(ctx, golden):
    """Frequency-sharded draw (nu0, nnu) equals the matching rows of the full draw."""
    import torch

    C = golden["cla_21cm_F8_l64_zromb3"]
    T, info = ctx.factor_batched(ctx.to_device(C))
    g = ctx.normals_philox(11, 64, 8)
    full = ctx.alm_dev_to_square(ctx.draw_alm(T, info, g, 64, 8), 64, 8).cpu().numpy()
    part = ctx.alm_dev_to_square(ctx.draw_alm(T, info, g, 64, 8, nu0=3, nnu=4), 64, 4).cpu().numpy()
    assert np.array_equal(part, full[3:7])


def test_draw_fused_rng_equals_materialised_stream(ctx, golden):
    """K3 with in-register Philox normals == normals_philox buffer + K3 (same device stream)."""
    C = golden["cla_21cm_F8_l64_zromb3"]
    T, info = ctx.factor_batched(ctx.to_device(C))
    for nu0, nnu in ((0, 8), (2, 5)):
        g = ctx.normals_philox(321, 64, 8)
        a = ctx.alm_dev_to_square(ctx.draw_alm(T, info, g, 64, 8, nu0=nu0, nnu=nnu), 64, nnu).cpu().numpy()
        b = ctx.alm_dev_to_square(ctx.draw_alm_philox(T, info, 321, 64, 8, nu0=nu0, nnu=nnu), 64, nnu).cpu().numpy()
        assert np.abs(a - b).max() <= 1e-13 * np.abs(a).max()
    rng = np.random.default_rng(0)
    for Fodd in (7, 33):  # odd channel counts take the materialised-stream route inside the library
        A = rng.standard_normal((20, Fodd, Fodd + 3))
        Co = A @ A.transpose(0, 2, 1)
        To, io = ctx.factor_batched(ctx.to_device(Co))
        g = ctx.normals_philox(9, 19, Fodd)
        a = ctx.alm_dev_to_square(ctx.draw_alm(To, io, g, 19, Fodd), 19, Fodd).cpu().numpy()
        b = ctx.alm_dev_to_square(ctx.draw_alm_philox(To, io, 9, 19, Fodd), 19, Fodd).cpu().numpy()
        assert np.abs(a - b).max() <= 1e-13 * np.abs(a).max()
    A = rng.standard_normal((40, 70, 75))
    C2 = A @ A.transpose(0, 2, 1)
    T2, info2 = ctx.factor_batched(ctx.to_device(C2))
    g = ctx.normals_philox(5, 39, 70)
    a = ctx.alm_dev_to_square(ctx.draw_alm(T2, info2, g, 39, 70), 39, 70).cpu().numpy()
    b = ctx.alm_dev_to_square(ctx.draw_alm_philox(T2, info2, 5, 39, 70), 39, 70).cpu().numpy()
    assert np.abs(a - b).max() <= 1e-13 * np.abs(a).max()
    # and the draw itself is right: a = T g / sqrt(2) with g in the reference's (nu', m) block order
    gh = g.cpu().numpy()
    l, F = 17, 70
    o = F * l * (l + 1)
    re = gh[o : o + F * (l + 1)].reshape(F, l + 1)
    im = gh[o + F * (l + 1) : o + 2 * F * (l + 1)].reshape(F, l + 1)
    ref = T2[l].cpu().numpy() @ (re + 1j * im) / 2**0.5
    assert np.abs(a[:, 0, l, : l + 1] - ref).max() <= 1e-12 * np.abs(ref).max()


def test_draw_more_than_128_columns(ctx):
    """More than 128 columns (several column groups per l): fused-RNG draw against the materialised stream, for
    triangular and dense (eigen-branch) factors, full and sharded channel ranges, row-sliced factors, and row
    counts that are not multiples of the tiles."""
    import torch

    rng = np.random.default_rng(3)
    for F, lmax in ((144, 21), (256, 140), (200, 33)):
        A = rng.standard_normal((lmax + 1, F, F + 5))
        C = A @ A.transpose(0, 2, 1)
        T, info = ctx.factor_batched(ctx.to_device(C))
        g = ctx.normals_philox(1234 + F, lmax, F)
        for nu0, nnu in ((0, F), (F - 132, 132)):
            a = ctx.alm_dev_to_square(ctx.draw_alm(T, info, g, lmax, F, nu0=nu0, nnu=nnu), lmax, nnu)
            b = ctx.alm_dev_to_square(ctx.draw_alm_philox(T, info, 1234 + F, lmax, F, nu0=nu0, nnu=nnu), lmax, nnu)
            assert (a - b).abs().max().item() <= 1e-13 * a.abs().max().item(), (F, nu0)
            rows = T[:, nu0:nu0 + nnu, :].contiguous()
            c = ctx.alm_dev_to_square(ctx.draw_alm_philox_rows(rows, info, 1234 + F, lmax, F, nu0, nnu), lmax, nnu)
            assert torch.equal(b, c)
        dense = torch.ones_like(info)           # treat the same factors as dense: all k contribute (upper part is 0)
        d = ctx.alm_dev_to_square(ctx.draw_alm_philox(T, dense, 1234 + F, lmax, F), lmax, F)
        a = ctx.alm_dev_to_square(ctx.draw_alm(T, info, g, lmax, F), lmax, F)
        assert (a - d).abs().max().item() <= 1e-13 * a.abs().max().item()


def test_fused_draw_random_shapes(ctx):
    """The persistent fused-RNG draw against the materialised stream over random shapes: channel counts that are not
    multiples of 4 / 16 / 32, channel ranges starting anywhere (aligned and unaligned column groups), lmax below and
    above one 128-m block, triangular and dense factors, row-sliced factors."""
    import torch

    rng = np.random.default_rng(2026)
    for trial in range(14):
        F = int(rng.choice([6, 10, 18, 34, 66, 96, 130, 160, 258]))
        lmax = int(rng.choice([0, 3, 17, 100, 127, 128, 150, 260]))
        if F * lmax > 30000:
            lmax = 30000 // F
        A = rng.standard_normal((lmax + 1, F, F + 3))
        C = A @ A.transpose(0, 2, 1) + 0.05 * np.eye(F)
        T, info = ctx.factor_batched(ctx.to_device(C))
        if trial % 3 == 2:
            info = torch.ones_like(info)                 # dense: every nu' contributes (the upper part is stored zeros)
        seed = 1000 + trial
        g = ctx.normals_philox(seed, lmax, F)
        nu0 = int(rng.integers(0, F))
        nnu = int(rng.integers(1, F - nu0 + 1))
        for (a0, n) in ((0, F), (nu0, nnu)):
            a = ctx.alm_dev_to_square(ctx.draw_alm(T, info, g, lmax, F, nu0=a0, nnu=n), lmax, n)
            b = ctx.alm_dev_to_square(ctx.draw_alm_philox(T, info, seed, lmax, F, nu0=a0, nnu=n), lmax, n)
            assert torch.isfinite(b).all()
            assert (a - b).abs().max().item() <= 1e-13 * a.abs().max().item(), (trial, F, lmax, a0, n)
            rows = T[:, a0:a0 + n, :].contiguous()
            c = ctx.alm_dev_to_square(ctx.draw_alm_philox_rows(rows, info, seed, lmax, F, a0, n), lmax, n)
            assert torch.equal(b, c), (trial, F, lmax, a0, n)


def test_philox_normals_match_stream_oracle(ctx):
    """normals_philox (fast in-kernel log / sqrt / sincos) == numpy restatement of the device stream."""
    from oracle import philox

    for seed, lmax, F in ((7, 48, 8), (2**40 + 12345, 33, 5)):
        g = ctx.normals_philox(seed, lmax, F).cpu().numpy()
        ref = philox.device_normals(seed, lmax, F)
        assert np.abs(g - ref).max() <= 4e-15 * max(1.0, np.abs(ref).max()), np.abs(g - ref).max()


def test_philox_normals_statistics(ctx):
    g = ctx.normals_philox(7, 200, 16).cpu().numpy()
    assert abs(g.mean()) < 5 / np.sqrt(g.size)
    assert abs(g.var() - 1) < 5 * np.sqrt(2 / g.size)
    assert abs((g**3).mean()) < 5 * np.sqrt(15 / g.size)
    assert abs((g**4).mean() - 3) < 5 * np.sqrt(96 / g.size)
    g2 = ctx.normals_philox(7, 200, 16).cpu().numpy()
    g3 = ctx.normals_philox(8, 200, 16).cpu().numpy()
    assert np.array_equal(g, g2) and not np.array_equal(g, g3)
    assert abs(np.corrcoef(g[:-1], g[1:])[0, 1]) < 5 / np.sqrt(g.size)


# ------------------------------------------------------------------ K1
@pytest.mark.parametrize("key,lmax,fkey,zromb,zwidth", [("cla_21cm_F8_l64_zromb0", 64, "f8", 0, None),
                                                        ("cla_21cm_F8_l64_zromb1", 64, "f8", 1, None),
                                                        ("cla_21cm_F8_l64_zromb3", 64, "f8", 3, None),
                                                        ("cla_21cm_F6n_l96_zromb3", 96, "f6", 3, None),
                                                        ("cla_21cm_F6n_l96_zromb2_zw", 96, "f6", 2, 1.0)])
def test_clarray_21cm_golden(golden, key, lmax, fkey, zromb, zwidth):
    from cora_amd.core import skysim
    from cora_amd.signal import corr21cm

    cr = _shared_corr21cm()
    cla = skysim.clarray(cr.angular_powerspectrum, lmax, golden[fkey].copy(), zromb=zromb, zwidth=zwidth)
    ref = golden[key]
    assert cla.shape == ref.shape
    assert np.abs(cla - ref).max() <= 1e-11 * np.abs(ref).max()


_CR = {}


def _shared_corr21cm():
    from cora_amd.signal import corr21cm

    if "cr" not in _CR:
        _CR["cr"] = corr21cm.Corr21cm()
    return _CR["cr"]


def test_21cm_tables_built_on_device(ctx, golden, model21):
    """K0 (row a4): P(k) spline grid + mu^2 / mu^4 + DCT-I along k_par on the GPU (csrc/tables21.hip) against slices
    of the reference's own tables, the full tables of the oracle, and - for a ps_vv callable the library does not
    know - the host-evaluated P(k) route."""
    import time

    from cora_amd.signal import corr21cm

    cr = corr21cm.Corr21cm()
    t0 = time.time()
    dev = cr._tables_on(ctx)
    ctx.sync()
    print("device table build: %.3f s" % (time.time() - t0))
    ix = np.ix_(golden["tab_rows"], golden["tab_cols"])
    for i, nm in enumerate(("dd", "dv", "vv")):
        t = getattr(cr, "_aps_" + nm)
        assert t.shape == (500, 32768)
        assert np.abs(t[ix] - golden["tab_" + nm]).max() <= 1e-13 * np.abs(golden["tab_" + nm]).max(), nm
        ref = model21.tables()[i]
        err = np.abs(t - ref).max() / np.abs(ref).max()
        print("table", nm, "device vs oracle (scipy DCT): %.2e" % err)
        assert err <= 1e-13, (nm, err)
    # a user-supplied power spectrum: evaluated on the host once, everything else on the device
    cr2 = corr21cm.Corr21cm(ps=lambda k: 1.0 / (1.0 + k * k), redshift=1.5)
    assert cr2._ps_spline_plan() is None
    dd = cr2._aps_dd
    kperp = np.logspace(-4, np.log10(40.0), 500)[:, None]
    kpar = np.linspace(0, 20.0, 32768)[None, :]
    import scipy.fftpack

    ref = scipy.fftpack.dct(1.0 / (1.0 + kpar**2 + kperp**2), type=1) * (20.0 / (2 * 32768))
    assert np.abs(dd - ref).max() <= 1e-13 * np.abs(ref).max()
    # replacing ps_vv after construction drops the spline plan as well
    cr.ps_vv = lambda k: k
    assert cr._ps_spline_plan() is None


@pytest.mark.parametrize("n", [4, 16, 106, 1156, 32768])
def test_dct1_rows_vs_scipy(ctx, n):
    """corahip_dct1_rows (prime-factor DFT of length n - 1) == scipy.fftpack.dct(type=1), several factorisations."""
    import scipy.fftpack
    import torch

    rng = np.random.default_rng(n)
    x = rng.standard_normal((5, n)) * np.exp(-np.arange(n) / (0.3 * n))
    got = ctx.dct1_rows(torch.from_numpy(x.copy()).to(ctx.device), 0.25).cpu().numpy()
    ref = scipy.fftpack.dct(x, type=1) * 0.25
    assert np.abs(got - ref).max() <= 1e-13 * np.abs(ref).max()


def test_dct1_rows_rejects_large_prime(ctx):
    import torch
    from cora_amd._lib import CoraHipError

    with pytest.raises(CoraHipError):
        ctx.dct1_rows(torch.zeros((1, 4099 + 1), dtype=torch.float64, device=ctx.device))   # 4099 is prime > 2048


def test_clarray_21cm_many_channels(model21):
    """F = 40 channels (3 tiles of 16: exercises tile mirroring) vs the oracle."""
    from cora_amd.core import skysim
    from oracle import skysim as osk

    cr = _shared_corr21cm()
    f = 600.0 + (np.arange(40) + 0.5) * 1.5625
    cla = skysim.clarray(cr.angular_powerspectrum, 300, f, zromb=1)
    ref = osk.clarray(model21.angular_powerspectrum, 300, f, zromb=1)
    assert np.abs(cla - ref).max() <= 1e-11 * np.abs(ref).max()
    assert np.array_equal(cla, cla.transpose(0, 2, 1))


def test_aps_21cm_kat(golden):
    """The reference's own known-answer test values (tests/test_corr.py:7-32)."""
    from cora_amd.util.cosmology import Cosmology

    cr = _shared_corr21cm()
    aps1 = cr.angular_powerspectrum(np.arange(1000), 800.0, 800.0)
    assert len(aps1) == 1000
    assert np.allclose(aps1.sum(), golden["sig_kat_default"][0], rtol=1e-10)
    assert np.allclose(aps1[[0, 1, 2, 10, 100, 500, 999]], golden["sig_aps_800_800"], rtol=1e-10)
    fa = np.linspace(400.0, 800.0, 64)
    aps2 = cr.angular_powerspectrum(np.arange(1000)[:, None, None], fa[None, :, None], fa[None, None, :])
    assert aps2.shape == (1000, 64, 64)
    sl = aps2[[0, 1, 7, 200, 400, 999]][:, ::9, ::7]
    # off-diagonal entries are ~1e-12 of the diagonal and come from cancelling table values
    assert np.abs(sl - golden["sig_aps2_slices"]).max() <= 1e-11 * np.abs(golden["sig_aps2_slices"]).max()
    # Planck-2013 cosmology reproduces the constants hard-coded in the reference's test
    old = cr.cosmology
    cr.cosmology = Cosmology(omega_b=0.0483, omega_c=0.2589, omega_l=0.6914, H0=67.77)
    try:
        a1 = cr.angular_powerspectrum(np.arange(1000), 800.0, 800.0)
        a2 = cr.angular_powerspectrum(np.arange(1000)[:, None, None], fa[None, :, None], fa[None, None, :])
    finally:
        cr.cosmology = old
    assert np.allclose(a1.sum(), 1.5963772205823096e-09, rtol=1e-7)
    assert np.allclose(a2[400, 40, 40], 8.986790805379046e-13, rtol=1e-7)
    assert np.allclose(a2[200, 10, 40], 1.1939298801340165e-18, rtol=1e-7)


@pytest.mark.parametrize("name,zromb", [("syn", 0), ("syn", 3), ("ups", 0), ("ups", 3)])
def test_clarray_foreground_golden(golden, name, zromb):
    from cora_amd.core import skysim
    from cora_amd.foreground import galaxy, pointsource

    model = galaxy.FullSkySynchrotron() if name == "syn" else pointsource.UnresolvedBackground()
    cla = skysim.clarray(model.angular_powerspectrum, 64, golden["f8"].copy(), zromb=zromb)
    ref = golden["cla_%s_F8_l64_zromb%d" % (name, zromb)]
    assert np.abs(cla - ref).max() <= 1e-13 * np.abs(ref).max()


def test_clarray_generic_callable(golden):
    """A plain Python callable goes through host evaluation + device Romberg reduction."""
    from cora_amd.core import skysim
    from oracle import skysim as osk

    def aps(l, z1, z2):
        return np.exp(-0.5 * (z1 - z2) ** 2) / (1.0 + l) ** 2 * (1 + 0.1 * z1 * z2)

    z = np.linspace(0.5, 2.5, 7)
    for zr in (0, 2):
        a = skysim.clarray(aps, 21, z, zromb=zr)
        b = osk.clarray(aps, 21, z, zromb=zr)
        assert np.abs(a - b).max() <= 1e-14 * np.abs(b).max()


def test_clarray_edge_cases():
    from cora_amd.core import skysim

    aps = lambda l, a, b: l + a + b
    with pytest.raises(ValueError):
        skysim.clarray(aps, 4, np.array([1.0, 2.0]), zromb=1)      # lmax < 5: array_split(.., 0)
    with pytest.raises(IndexError):
        skysim.clarray(aps, 8, np.array([1.0]), zromb=1)           # one channel, no zwidth


# ------------------------------------------------------------------ end to end
@pytest.mark.parametrize("model_name,nside,lmax,F,zromb", [("21cm", 16, 32, 4, 1), ("syn", 32, 64, 8, 0)])
def test_getsky_end_to_end(model21, model_name, nside, lmax, F, zromb):
    """Sky3d.getsky() == oracle clarray + mkfullsky on the same numpy seed."""
    from cora_amd.foreground import galaxy
    from oracle import models
    from oracle import skysim as osk

    if model_name == "21cm":
        m, om = _shared_corr21cm(), model21
    else:
        m, om = galaxy.FullSkySynchrotron(), models.FullSkySynchrotron()
    m.nside, m.lmax, m.oversample = nside, lmax, zromb
    m.frequencies = 500.0 + 20.0 * np.arange(F)
    try:
        sky = m.getsky(rng=np.random.default_rng(42))
    finally:
        m.lmax, m.frequencies = None, None
    cla = osk.clarray(om.angular_powerspectrum, lmax, 500.0 + 20.0 * np.arange(F), zromb=zromb)
    ref = osk.mkfullsky(cla, nside, rng=np.random.default_rng(42))
    assert sky.shape == (F, 12 * nside * nside)
    tol = 1e-10 if model_name == "21cm" else 1e-4  # near-singular foreground blocks: SURVEY 8a8
    assert np.abs(sky - ref).max() <= tol * ref.std()


def test_recovered_cl_device_rng(ctx, golden):
    """Throughput mode (device Philox): recovered power matches C_l (2l+1/2)/(2l+1)
    (complex a_l0 quirk of the reference) within sampling error."""
    from cora_amd import DeviceRNG
    from cora_amd.core import skysim
    from oracle import skysim as osk

    C = golden["cla_21cm_F8_l64_zromb3"]
    lmax = 64
    acc = np.zeros((8, lmax + 1))
    nrep = 40
    rng = DeviceRNG(123)
    for _ in range(nrep):
        a = skysim.mkfullsky(C, 32, alms=True, rng=rng)[:, 0]
        for i in range(8):
            # use only Re(a_l0), as the synthesis does
            a0 = a[i].copy()
            a0[:, 0] = a0[:, 0].real
            acc[i] += osk.sph_ps_from_alm(a0)
    acc /= nrep
    l = np.arange(lmax + 1)
    expect = np.array([C[:, i, i] for i in range(8)]) * (2 * l + 0.5) / (2 * l + 1)
    sigma = expect * np.sqrt(2.0 / ((2 * l + 1) * nrep))
    z = (acc - expect)[:, 2:] / sigma[:, 2:]
    assert np.abs(z).max() < 5.0
    assert abs(z.mean()) < 0.5


# ------------------------------------------------------------------ BASELINE.json configs
def test_config1_single_frequency_21cm(model21):
    """configs[0]: Corr21cm, one frequency, nside=64, lmax=128 (zromb=0: one channel has no width)."""
    from oracle import skysim as osk

    m = _shared_corr21cm()
    m.nside, m.lmax, m.oversample = 64, 128, 0
    m.frequencies = np.array([600.0])
    try:
        sky = m.getsky(rng=np.random.default_rng(1))
    finally:
        m.lmax, m.frequencies, m.oversample = None, None, 3
    cla = osk.clarray(model21.angular_powerspectrum, 128, np.array([600.0]), zromb=0)
    ref = osk.mkfullsky(cla, 64, rng=np.random.default_rng(1))
    assert sky.shape == (1, 12 * 64 * 64)
    assert np.abs(sky - ref).max() <= 1e-10 * ref.std()


def test_config2_synchrotron_full_size():
    """configs[1]: FullSkySynchrotron, 32 channels 400-800 MHz, nside=256, lmax=512, oversample 3.
    C_l vs oracle to 1e-13; maps from host-injected identical a_lm vs the oracle synthesis to 1e-11 rms
    (the factor of the cond~1e19 blocks is rounding sensitive, SURVEY 8a8, so a_lm are compared at 1e-4)."""
    import torch
    from cora_amd import _lib
    from cora_amd.core import skysim
    from cora_amd.foreground import galaxy
    from oracle import models, sht
    from oracle import skysim as osk

    nside, lmax, F = 256, 512, 32
    freq = 400.0 + (np.arange(F) + 0.5) * 12.5
    fg, ofg = galaxy.FullSkySynchrotron(), models.FullSkySynchrotron()
    cla = skysim.clarray(fg.angular_powerspectrum, lmax, freq, zromb=3)
    cref = osk.clarray(ofg.angular_powerspectrum, lmax, freq, zromb=3)
    assert np.abs(cla - cref).max() <= 1e-13 * np.abs(cref).max()
    a = skysim.mkfullsky(cla, nside, alms=True, rng=np.random.default_rng(2))
    aref = osk.mkfullsky(cref, nside, alms=True, rng=np.random.default_rng(2))
    # blocks have cond ~ 7e14 after the 1e-14 jitter: T T^T = C holds to 1e-15 on both sides but T itself
    # (hence T g) moves by ~1e-7..1e-5 with rounding; compare per l against that l's rms
    Tg, _ = _lib.get_context().factor_batched(_lib.get_context().to_device(cref[[1, 100, 512]]))
    for T_l, C_l in zip(Tg.cpu().numpy(), cref[[1, 100, 512]]):
        Cm = C_l + np.eye(F) * C_l.diagonal().max() * 1e-14
        assert np.abs(T_l @ T_l.T - Cm).max() <= 1e-14 * Cm.max()
    for l in range(1, lmax + 1):
        d = np.abs(a[:, 0, l, : l + 1] - aref[:, 0, l, : l + 1]).max()
        assert d <= 1e-4 * np.sqrt((np.abs(aref[:, 0, l, : l + 1]) ** 2).mean()), l
    assert np.all(a[:, 0, 0] == 0)
    # synthesis at full size on identical a_lm, 4 of the 32 channels checked against the C/OpenMP oracle
    ctx = _lib.get_context()
    packed = np.stack([osk.pack_alm(aref[i, 0]) for i in range(F)])
    dev = ctx.alm_packed_to_dev(torch.from_numpy(packed).to(ctx.device), lmax)
    maps = ctx.alm2map(dev, nside, lmax, F).cpu().numpy()
    for i in (0, 7, 18, 31):
        ref = sht.alm2map(packed[i], nside, lmax)
        assert np.abs(maps[i] - ref).max() <= 1e-11 * ref.std(), i


def test_config3_full_size_properties(ctx):
    """configs[2] at FULL size (256 channels, nside=1024, lmax=2048), checked on the device through
    size-independent properties: (1) linearity of the synthesis, (2) Parseval: the pixel variance of every
    channel equals sum_l (2l+1) C^_l / 4pi of its own a_lm (with only Re a_l0 counted) to quadrature accuracy,
    (3) north/south mirror: a_lm with only even l+m gives maps symmetric under z -> -z."""
    import torch

    nside, lmax, F = 1024, 2048, 256
    L = lmax + 1
    nalm = L * (L + 1) // 2
    npix = 12 * nside * nside
    gen = torch.Generator(device=ctx.device)
    gen.manual_seed(5)
    # red spectrum ~ 1/(1+l)^2 so the band limit is well inside the pixelisation
    idx_l = torch.cat([torch.arange(m, L, device=ctx.device) for m in range(L)])
    amp = (1.0 / (1.0 + idx_l.double()) ** 1.0)
    G = F // 4
    alm = torch.randn((nalm, G, 2, 4), generator=gen, device=ctx.device, dtype=torch.float64) * amp[:, None, None, None]
    maps = ctx.alm2map(alm, nside, lmax, F)
    # (2) Parseval per channel
    pw = (alm[:, :, 0, :] ** 2 + alm[:, :, 1, :] ** 2)           # |a_lm|^2  [nalm, G, 4]
    m0 = torch.zeros(nalm, device=ctx.device, dtype=torch.float64)
    m0[:L] = 1.0                                                  # packed index of m = 0 is l
    tot = (2.0 * pw * (1 - m0)[:, None, None] + (alm[:, :, 0, :] ** 2) * m0[:, None, None]).sum(0)  # [G,4]
    var_alm = (tot / (4 * np.pi)).reshape(F)
    mean_sq = (maps**2).mean(dim=1)
    rel = ((mean_sq - var_alm).abs() / var_alm).max().item()
    assert rel < 2e-3, rel  # HEALPix quadrature is not exact; 1e-3 level at lmax = 2 nside
    # (1) linearity on 8 channels
    a8 = alm[:, :2].contiguous()
    b8 = torch.randn(a8.shape, generator=gen, device=ctx.device, dtype=torch.float64) * amp[:, None, None, None]
    ma, mb = ctx.alm2map(a8, nside, lmax, 8).clone(), ctx.alm2map(b8, nside, lmax, 8).clone()
    mc = ctx.alm2map(2.0 * a8 - 3.0 * b8, nside, lmax, 8)
    err = (mc - (2.0 * ma - 3.0 * mb)).abs().max().item() / mc.std().item()
    assert err < 1e-11, err
    # (3) mirror symmetry: keep only even l+m
    par = ((idx_l + torch.cat([torch.full((L - m,), m, device=ctx.device) for m in range(L)])) % 2 == 0).double()
    ms = ctx.alm2map(a8 * par[:, None, None, None], nside, lmax, 8)
    ri = ctx.sht_rings(nside, lmax)
    nring = 4 * nside - 1
    worst = 0.0
    for r in (0, 5, 511, 1023, 1500, 2046):
        s, n = int(ri["start"][r]), int(ri["nphi"][r])
        s2 = int(ri["start"][nring - 1 - r])
        worst = max(worst, (ms[:, s : s + n] - ms[:, s2 : s2 + n]).abs().max().item())
    assert worst < 1e-11 * ms.std().item(), worst
    del maps, alm
    torch.cuda.empty_cache()


def test_frequency_sharded_pipeline_matches_single_gpu():
    """bench.py's N-rank paths, run as 2 and 3 ranks sharing this one GPU over gloo (the GPU boxes allow at most 6
    processes on the card: this process + the launcher + the ranks), give the same per-channel
    map statistics as 1 rank: cfg2 (separable model: l-sharded C_l/factor -> all-gather) and a small 21cm
    case (pair-sharded C_l -> all-to-all -> l-sharded factor -> all-to-all of factor rows).  The RCCL
    calls themselves are exercised with a 1-rank nccl group (--force-dist)."""
    import os
    import re
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

    def run(cmd):
        p = subprocess.run(cmd, cwd=root, capture_output=True, text=True, timeout=600)
        m = re.search(r"CHECKSUM (\w+)", p.stderr)
        assert m, p.stderr[-2000:]
        return m.group(1)

    port = 29631
    for workload in ("cfg2", "tiny"):
        common = ["--workload", workload, "--steps", "1", "--warmup", "0", "--no-cpu-baseline", "--checksum"]
        ref = run([sys.executable, "bench.py"] + common)
        for n in (2, 3):   # 3 does not divide F: the l-shard + all-gather fall-back of the row exchange
            port += 1
            got = run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n),
                       "--master-addr", "127.0.0.1", "--master-port", str(port), "bench.py", "--gpus", str(n),
                       "--dist-backend", "gloo", "--same-device"] + common)
            assert got == ref, (workload, n, got, ref)
        port += 1
        env_port = ["--master-port", str(port)]
        got = run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1",
                   "--master-addr", "127.0.0.1"] + env_port + ["bench.py", "--gpus", "1", "--force-dist"] + common)
        assert got == ref, (workload, "nccl x1", got, ref)


def test_pair_sharded_clarray_and_row_sliced_draw(ctx, golden):
    """The multi-GPU building blocks against their single-GPU forms, in one process: K1 pair shards of 3
    'ranks' assembled by hand == clarray_table21cm; draw from factor row blocks == draw from full factors."""
    import torch
    from cora_amd.core import skysim
    from cora_amd.signal import corr21cm

    cr = corr21cm.Corr21cm()
    F, lmax, zromb = 12, 70, 2
    L = lmax + 1
    freq = np.linspace(500.0, 530.0, F)
    zint = 2**zromb + 1
    zh = abs(freq[1] - freq[0]) / 2
    za = (freq[:, None] + np.linspace(-zh, zh, zint)[None, :]).ravel()
    plan = cr._clarray_plan(cr.angular_powerspectrum)
    p = plan["prepare"](ctx, za)
    w = ctx.to_device(skysim.romberg_weights(zromb))
    larr = np.arange(L, dtype=np.float64)
    lx = ctx.to_device(np.log10(np.where(larr == 0, 1e-10, larr)))
    k1 = [ctx.to_device(p[k]) for k in ("chi", "pfd", "f", "b")]
    tabs = (p["dd"], p["dv"], p["vv"], p["kperpmin"], p["kperpmax"], p["kparmax"])
    C = ctx.clarray_table21cm(*tabs, *k1, F, zint, w, lx)
    W = 3
    lsh = (L + W - 1) // W
    slabs = [ctx.clarray_table21cm_pairs(*tabs, *k1, F, zint, w, lx, r, W, lsh) for r in range(W)]   # [W][npl][lsh] each
    for q in range(W):
        mine = torch.stack([slabs[r][q] for r in range(W)])          # what the all-to-all hands rank q
        nl = min(L, (q + 1) * lsh) - q * lsh
        Cq = ctx.clarray_pairs_finish(mine, F, nl)
        assert torch.equal(Cq, C[q * lsh : q * lsh + nl])
    T, info = ctx.factor_batched(C)
    full = ctx.draw_alm_philox(T, info, 99, lmax, F)
    fsq = ctx.alm_dev_to_square(full, lmax, F)
    for nu0, nnu in ((0, 4), (4, 4), (8, 4), (2, 7)):
        rows = T[:, nu0 : nu0 + nnu, :].contiguous()
        part = ctx.alm_dev_to_square(ctx.draw_alm_philox_rows(rows, info, 99, lmax, F, nu0, nnu), lmax, nnu)
        assert torch.equal(part, fsq[nu0 : nu0 + nnu])


# ------------------------------------------------------------------ n1: analysis (map2alm, sph_ps)
@pytest.mark.parametrize("nside,lmax,nnu", [(8, 16, 3), (16, 47, 8), (64, 128, 5), (32, 40, 17)])
def test_map2alm_quadrature_vs_oracle(ctx, nside, lmax, nnu):
    """K5^T + K4^T (one weighted quadrature pass) against the CPU oracle, through the C ABI."""
    import torch
    from cora_amd.util import hputil
    from oracle import sht

    rng = np.random.default_rng(nside + lmax)
    maps = rng.standard_normal((nnu, 12 * nside * nside))
    w = hputil.ring_weights(nside)
    alm = ctx.map2alm(torch.from_numpy(maps).to(ctx.device), nside, lmax, ctx.to_device(w))
    got = ctx.alm_dev_to_square(alm, lmax, nnu).cpu().numpy()[:, 0]
    for k in range(nnu):
        ref = hputil.unpack_alm(sht.map2alm_adjoint(maps[k], nside, lmax, sht.ring_weights(nside)), lmax)
        assert np.abs(got[k] - ref).max() <= 2e-13 * np.abs(ref).max(), (k, np.abs(got[k] - ref).max())
    # unweighted pass, chunked over channels
    alm_u = ctx.map2alm(torch.from_numpy(maps).to(ctx.device), nside, lmax, None, chunk=8)
    got_u = ctx.alm_dev_to_square(alm_u, lmax, nnu).cpu().numpy()[:, 0]
    ref_u = hputil.unpack_alm(sht.map2alm_adjoint(maps[nnu - 1], nside, lmax, None), lmax)
    assert np.abs(got_u[nnu - 1] - ref_u).max() <= 2e-13 * np.abs(ref_u).max()


def test_map2alm_iterated_matches_oracle_and_round_trips(ctx):
    """healpy.map2alm(use_weights=True, iter=2) semantics: GPU == oracle, and a band-limited sky comes back."""
    import torch
    from cora_amd.util import hputil
    from oracle import sht

    nside, lmax, nnu = 32, 48, 4
    rng = np.random.default_rng(5)
    n = (lmax + 1) * (lmax + 2) // 2
    a = rng.standard_normal((nnu, n)) + 1j * rng.standard_normal((nnu, n))
    a[:, : lmax + 1] = a[:, : lmax + 1].real
    maps = ctx.alm2map(ctx.alm_packed_to_dev(torch.from_numpy(a).to(ctx.device), lmax), nside, lmax, nnu)
    alm = hputil.map2alm_device(maps, nside, lmax)                    # weights + 2 iterations
    got = ctx.alm_dev_to_square(alm, lmax, nnu).cpu().numpy()[:, 0]
    mh = maps.cpu().numpy()
    for k in range(nnu):
        ref = hputil.unpack_alm(sht.map2alm(mh[k], nside, lmax, True, 2), lmax)
        assert np.abs(got[k] - ref).max() <= 1e-11 * np.abs(ref).max()
        assert np.abs(got[k] - hputil.unpack_alm(a[k], lmax)).max() < 1e-4


def test_sphtrans_and_sph_ps_api(ctx):
    """hputil.sphtrans_real / sphtrans_sky / sph_ps shapes and values (cora/util/hputil.py:195-234,460-497,607-619)."""
    from cora_amd.util import hputil
    from oracle import sht

    nside, lmax = 16, 24
    rng = np.random.default_rng(8)
    n = (lmax + 1) * (lmax + 2) // 2
    a = rng.standard_normal((2, n)) + 1j * rng.standard_normal((2, n))
    a[:, : lmax + 1] = a[:, : lmax + 1].real
    m0, m1 = sht.alm2map(a[0], nside, lmax), sht.alm2map(a[1], nside, lmax)
    r = hputil.sphtrans_real(m0, lmax, lside=30)
    assert r.shape == (31, 31) and np.all(r[lmax + 1 :] == 0) and np.all(r[:, lmax + 1 :] == 0)
    assert np.abs(r[: lmax + 1, : lmax + 1] - hputil.unpack_alm(a[0], lmax)).max() < 1e-5   # lmax = 1.5 nside, 2 iterations
    assert hputil.sphtrans_real(m0).shape == (3 * nside, 3 * nside)
    sky = hputil.sphtrans_sky(np.stack([m0, m1]), lmax)
    assert sky.shape == (2, lmax + 1, lmax + 1)
    assert np.abs(sky[0] - r[: lmax + 1, : lmax + 1]).max() < 1e-13
    sky3 = hputil.sphtrans_sky(np.stack([m0, m1])[:, None, :], lmax)
    assert sky3.shape == (2, 1, lmax + 1, lmax + 1) and np.array_equal(sky3[:, 0], sky)
    zero_pol = hputil.sphtrans_sky(np.zeros((2, 3, 12 * nside * nside)), lmax)      # polarised branch (3 components)
    assert zero_pol.shape == (2, 3, lmax + 1, lmax + 1) and not zero_pol.any()
    with pytest.raises(Exception, match="polarisation components"):
        hputil.sphtrans_sky(np.zeros((2, 5, 12 * nside * nside)), lmax)
    al0, al1 = hputil.unpack_alm(a[0], lmax), hputil.unpack_alm(a[1], lmax)
    ll = 2.0 * np.arange(lmax + 1) + 1.0
    auto = (np.abs(al0[:, 0]) ** 2 + 2 * (np.abs(al0[:, 1:]) ** 2).sum(axis=1)) / ll
    cross = ((al0 * al1.conj())[:, 0] + 2 * (al0 * al1.conj())[:, 1:].sum(axis=1).real) / ll
    assert np.abs(hputil.sph_ps(m0, lmax=lmax) - auto).max() < 1e-5 * auto.max()
    assert np.abs(hputil.sph_ps(m0, m1, lmax=lmax) - cross).max() < 1e-5 * auto.max()


def test_map2alm_full_size_adjointness(ctx):
    """At BASELINE cfg-3 geometry (nside 1024, lmax 2048): <S a, x> 4 pi / npix == <a, A x> for random a, x -
    the size-independent property tying the analysis kernels to the synthesis ones."""
    import torch

    nside, lmax, nnu = 1024, 2048, 8
    L = lmax + 1
    nalm = L * (L + 1) // 2
    npix = 12 * nside * nside
    gen = torch.Generator(device=ctx.device).manual_seed(3)
    a = torch.randn((nalm, 2, 2, 4), generator=gen, device=ctx.device, dtype=torch.float64)
    a[:L, :, 1, :] = 0.0                     # imaginary parts of a_l0 do not enter a real map
    x = torch.randn((nnu, npix), generator=gen, device=ctx.device, dtype=torch.float64)
    Sa = ctx.alm2map(a, nside, lmax, nnu)
    Ax = ctx.map2alm(x, nside, lmax, None)
    wgt = torch.full((nalm, 1, 1, 1), 2.0, device=ctx.device, dtype=torch.float64)
    wgt[:L] = 1.0
    lhs = (Sa * x).sum(dim=1) * (4 * np.pi / npix)                      # per channel
    rhs = (wgt * a * Ax).sum(dim=(0, 2)).reshape(-1)[:nnu]               # [G,4] -> channel order
    scale = (Sa.abs() * x.abs()).sum(dim=1) * (4 * np.pi / npix)
    assert ((lhs - rhs).abs() / scale).max().item() < 1e-12
    del a, x, Sa, Ax
    torch.cuda.empty_cache()


def test_map2alm_adjointness_nside2048(ctx):
    """The same property at the cfg-5 geometry (nside 2048; lmax 383 keeps it light): eight ring tiles - the tile reduction's
    path beyond four -, the belt rings through the length-4096 analysis kernel, the caps through the run-time kernel."""
    import torch

    nside, lmax, nnu = 2048, 383, 8
    L = lmax + 1
    nalm = L * (L + 1) // 2
    npix = 12 * nside * nside
    gen = torch.Generator(device=ctx.device).manual_seed(4)
    a = torch.randn((nalm, 2, 2, 4), generator=gen, device=ctx.device, dtype=torch.float64)
    a[:L, :, 1, :] = 0.0
    x = torch.randn((nnu, npix), generator=gen, device=ctx.device, dtype=torch.float64)
    Sa = ctx.alm2map(a, nside, lmax, nnu)
    Ax = ctx.map2alm(x, nside, lmax, None)
    wgt = torch.full((nalm, 1, 1, 1), 2.0, device=ctx.device, dtype=torch.float64)
    wgt[:L] = 1.0
    lhs = (Sa * x).sum(dim=1) * (4 * np.pi / npix)
    rhs = (wgt * a * Ax).sum(dim=(0, 2)).reshape(-1)[:nnu]
    scale = (Sa.abs() * x.abs()).sum(dim=1) * (4 * np.pi / npix)
    assert ((lhs - rhs).abs() / scale).max().item() < 1e-12
    del a, x, Sa, Ax
    torch.cuda.empty_cache()


def test_mkconstrained_vs_oracle(golden):
    """skysim.mkconstrained (cora/core/skysim.py:139-205): constrained channels reproduce their constraint
    maps (up to the l = 0 mode the reference zeroes) and the whole stack matches the CPU oracle."""
    from cora_amd.core import skysim
    from oracle import sht
    from oracle import skysim as osk

    cl = golden["cla_21cm_F8_l64_zromb3"][:33]                 # [33, 8, 8], well conditioned
    nside, lmax = 16, 32
    rng = np.random.default_rng(4)
    n = (lmax + 1) * (lmax + 2) // 2
    cons = []
    for fi in (1, 5):
        a = rng.standard_normal(n) + 1j * rng.standard_normal(n)
        a[: lmax + 1] = a[: lmax + 1].real
        a[0] = 0.0                                              # no monopole: mkconstrained drops l = 0
        cons.append([fi, sht.alm2map(a, nside, lmax)])
    got = skysim.mkconstrained(cl, cons, nside)
    ref = osk.mkconstrained(cl, cons, nside)
    assert got.shape == (8, 12 * nside * nside)
    assert np.abs(got - ref).max() <= 1e-9 * np.abs(ref).max()
    for fi, cm in cons:
        assert np.abs(got[fi] - cm).max() < 1e-3 * np.abs(cm).max()
    with pytest.raises(Exception, match="incorrect shape"):
        skysim.mkconstrained(np.zeros((5, 3, 4)), cons, nside)


def test_makesky_cli_21cm_and_gaussianfg(tmp_path):
    """cora-makesky commands on the GPU path (scripts/makesky.py:313-390): same-seed maps equal the module API."""
    from click.testing import CliRunner

    from cora_amd.foreground import galaxy
    from cora_amd.scripts import makesky
    from cora_amd.signal import corr21cm

    out = str(tmp_path / "m21.h5")
    r = CliRunner().invoke(makesky.cli, ["21cm", "--nside", "16", "--freq", "600", "640", "4", "--freq-mode", "edge",
                                         "--pol", "zero", "--oversample", "1", "--seed", "3", "--filename", out])
    assert r.exit_code == 0, r.output
    f = np.load(out + ".npz")
    assert f["map"].shape == (4, 4, 12 * 16 * 16) and np.all(f["map"][:, 1:] == 0)
    cr = corr21cm.Corr21cm()
    cr.nside = 16
    cr.frequencies = np.array([605.0, 615.0, 625.0, 635.0])
    cr.oversample = 1
    assert np.array_equal(f["map"][:, 0], cr.getsky(rng=np.random.default_rng(3)))
    assert np.array_equal(f["index_map__freq"]["centre"], cr.frequencies) and np.all(f["index_map__freq"]["width"] == 10.0)

    out2 = str(tmp_path / "fg.h5")
    r = CliRunner().invoke(makesky.cli, ["gaussianfg", "--nside", "8", "--freq", "400", "800", "3", "--freq-mode", "edge",
                                         "--pol", "none", "--seed", "5", "--filename", out2])
    assert r.exit_code == 0, r.output
    g = np.load(out2 + ".npz")
    assert g["map"].shape == (3, 1, 768) and np.isfinite(g["map"]).all() and g["map"].std() > 0
    # brighter at low frequency (synchrotron spectral index -2.8)
    assert g["map"][0].std() > g["map"][2].std()
    # --pol full: T from the unpolarised model, Q/U from E/B draws of the polarised one through the spin-2 synthesis
    out3 = str(tmp_path / "fgpol.h5")
    r = CliRunner().invoke(makesky.cli, ["gaussianfg", "--nside", "8", "--freq", "400", "800", "2", "--freq-mode", "edge",
                                         "--pol", "full", "--seed", "5", "--filename", out3])
    assert r.exit_code == 0, r.output
    h = np.load(out3 + ".npz")
    assert h["map"].shape == (2, 4, 768) and np.isfinite(h["map"]).all()
    st = h["map"].std(axis=-1)
    assert np.all(st[:, 1] > 0) and np.all(st[:, 2] > 0) and np.all(st[:, 1:3] < st[:, :1])      # Q, U present, fainter than T
    assert np.all(st[:, 3] < 1e-5 * st[:, 0])                    # V: only the 1e-14 diagonal jitter of mkfullsky
    del galaxy


# ------------------------------------------------------------------ the healpy boundary itself, where healpy exists
def test_healpy_cross_check_when_available(ctx):
    """healpy is absent from this image and from the GPU boxes of the pool (the one boundary no reference
    output pins).  On a box that HAS it this test lights up: the synthesis against ``healpy.alm2map`` - what
    hputil.sphtrans_inv_real calls (cora/util/hputil.py:388-391) - at nside 64 / lmax 128, and the analysis against
    ``healpy.map2alm(use_weights=True, iter=2)`` (cora/util/hputil.py:228-230), whose ring weights come from healpy's
    data files where this library restates them by their defining property."""
    hp = pytest.importorskip("healpy")
    from cora_amd.util import hputil

    nside, lmax = 64, 128
    L = lmax + 1
    rng = np.random.default_rng(64128)
    alm = np.zeros((L, L), dtype=np.complex128)
    for l in range(L):
        alm[l, : l + 1] = (rng.standard_normal(l + 1) + 1j * rng.standard_normal(l + 1)) / (1.0 + l)
    alm[:, 0] = alm[:, 0].real
    got = hputil.sphtrans_inv_real(alm, nside)
    ref = hp.alm2map(hputil.pack_alm(alm), nside, lmax=lmax, pol=False)
    assert np.abs(got - ref).max() <= 1e-11 * ref.std()
    back = hputil.sphtrans_real(ref, lmax=lmax)
    ref_alm = hp.map2alm(ref, lmax=lmax, use_weights=True, iter=2)
    ref2d = hputil.unpack_alm(ref_alm, lmax)
    # (the restated ring weights equal healpy's file weights only approximately: the documented unpinned piece)
    assert np.abs(back - ref2d).max() <= 1e-6 * np.abs(ref2d).max()


# ------------------------------------------------------------------ EoR21cm (cora/signal/corr21cm.py:333-385)
@pytest.fixture(scope="module")
def eor_golden():
    """Outputs of the reference's own EoR21cm (tests/golden/make_golden_eor.py)."""
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "eor_vectors.npz"))


def test_eor21cm_reference_vectors_through_k1(eor_golden):
    """EoR21cm through the device path: the aps on the 150-200 MHz band (other table rows and y columns than any
    400-800 MHz test reaches: chi ~ 6000-6800 Mpc/h) and clarray (K1) at zromb 0 / 1 / 3 and with an explicit
    zwidth on 100-200 MHz against outputs of the reference's own class, <= 1e-12 of the maximum."""
    from cora_amd.core import skysim
    from cora_amd.signal import corr21cm

    g = eor_golden
    eor = corr21cm.EoR21cm()
    aps1 = eor.angular_powerspectrum(np.arange(1000), 180.0, 180.0)
    assert np.abs(aps1 - g["aps_180_180"]).max() <= 1e-12 * np.abs(g["aps_180_180"]).max()
    fa = g["fa"]
    aps2 = eor.angular_powerspectrum(np.arange(1000)[:, None, None], fa[None, :, None], fa[None, None, :])
    got = np.array([aps1.sum(), aps2[400, 10, 10], aps2[200, 3, 10], aps2[0, 5, 6], aps2[999, 15, 0]])
    assert np.abs(got / g["aps2_samples"] - 1.0).max() < 1e-9, got            # (the far off-diagonal samples are 1e-7 of the diagonal)
    assert np.abs(aps2[200] - g["aps2_l200"]).max() <= 1e-12 * np.abs(g["aps2_l200"]).max()
    for zr in (0, 1, 3):
        ref = g["cla_eor_F8_l64_zromb%d" % zr]
        cla = skysim.clarray(eor.angular_powerspectrum, 64, g["f8"].copy(), zromb=zr)
        assert cla.shape == ref.shape and np.abs(cla - ref).max() <= 1e-12 * np.abs(ref).max(), zr
    ref = g["cla_eor_F6_l40_zromb2_zw1"]
    cla = skysim.clarray(eor.angular_powerspectrum, 40, g["f6"].copy(), zromb=2, zwidth=1.0)
    assert np.abs(cla - ref).max() <= 1e-12 * np.abs(ref).max()
    # bias 3 and the Santos et al. T_b are what separates it from Corr21cm on the same band
    c21 = skysim.clarray(_shared_corr21cm().angular_powerspectrum, 64, g["f8"].copy(), zromb=0)
    assert np.abs(c21 - g["cla_eor_F8_l64_zromb0"]).max() > 0.5 * np.abs(c21).max()


def test_makesky_cli_21cm_eor(tmp_path):
    """`cora-makesky 21cm --eor` (cora/scripts/makesky.py:316-334) = EoR21cm through getsky: same-seed maps equal the
    module API, and differ from the intensity-mapping model's."""
    from click.testing import CliRunner

    from cora_amd.scripts import makesky
    from cora_amd.signal import corr21cm

    out = str(tmp_path / "eor.h5")
    args = ["21cm", "--nside", "16", "--freq", "150", "190", "4", "--freq-mode", "edge", "--pol", "none", "--oversample", "1",
            "--seed", "9", "--filename"]
    r = CliRunner().invoke(makesky.cli, args[:1] + ["--eor"] + args[1:] + [out])
    assert r.exit_code == 0, r.output
    f = np.load(out + ".npz")
    assert f["map"].shape == (4, 1, 12 * 16 * 16)
    cr = corr21cm.EoR21cm()
    cr.nside = 16
    cr.frequencies = np.array([155.0, 165.0, 175.0, 185.0])
    cr.oversample = 1
    assert np.array_equal(f["map"][:, 0], cr.getsky(rng=np.random.default_rng(9)))
    out2 = str(tmp_path / "im.h5")
    r = CliRunner().invoke(makesky.cli, args + [out2])
    assert r.exit_code == 0, r.output
    assert f["map"].std() > 3.0 * np.load(out2 + ".npz")["map"].std()


# ------------------------------------------------------------------ full-size pipeline / remaining BASELINE configs
def _alm_power(alm_dev, lmax):
    """C^_l per channel from alm_dev [nalm, G, 2, 4] counting only Re a_l0 (what the synthesis uses): [4G, L]."""
    import torch

    L = lmax + 1
    dev = alm_dev.device
    pw = alm_dev[:, :, 0, :] ** 2 + alm_dev[:, :, 1, :] ** 2          # [nalm, G, 4]
    pw[:L] = alm_dev[:L, :, 0, :] ** 2                                 # m = 0: real part only
    idx_l = torch.cat([torch.arange(m, L, device=dev) for m in range(L)])
    wgt = torch.full((pw.shape[0],), 2.0, device=dev, dtype=torch.float64)
    wgt[:L] = 1.0
    out = torch.zeros((L,) + tuple(pw.shape[1:]), device=dev, dtype=torch.float64)
    out.index_add_(0, idx_l, pw * wgt[:, None, None])
    out = out / (2.0 * torch.arange(L, device=dev, dtype=torch.float64) + 1.0)[:, None, None]
    return out.reshape(L, -1).T


def test_config3_pipeline_full_size_recovered_spectrum(ctx):
    """configs[2] END TO END at full size (Corr21cm, 256 channels 400-800 MHz, nside 1024, lmax 2048, device
    Philox stream): (1) the spectrum of the drawn a_lm matches the integrated C_l(nu,nu) (2l+1/2)/(2l+1) within
    sampling error for every channel, and adjacent channels have the model's cross-correlation; (2) the a_lm
    recovered from the final MAPS by the analysis kernels equal the drawn ones to iteration accuracy - so
    K1 -> K2 -> K3 -> K4 -> K5 is closed on the device at BASELINE size."""
    import torch
    from cora_amd.core import skysim
    from cora_amd.signal import corr21cm
    from cora_amd.util import hputil

    nside, lmax, F = 1024, 2048, 256
    L = lmax + 1
    cr = corr21cm.Corr21cm()
    freq = 400.0 + (np.arange(F) + 0.5) * (400.0 / F)
    C = skysim.clarray_device(cr.angular_powerspectrum, lmax, freq, zromb=3)          # K1  [L, F, F]
    T, info = skysim.factor_device(C)                                                  # K2
    assert int(info.abs().sum().item()) == 0                                           # all Cholesky (cond ~ 4)
    alm = ctx.draw_alm_philox(T, info, 20261003, lmax, F)                              # K3
    ps = _alm_power(alm, lmax)                                                         # [F, L]
    l = torch.arange(L, device=ctx.device, dtype=torch.float64)
    expect = torch.diagonal(C, dim1=1, dim2=2).T * (2 * l + 0.5) / (2 * l + 1)         # [F, L]
    sigma = expect * torch.sqrt(2.0 / (2 * l + 1))
    z = ((ps - expect) / sigma)[:, 2:]
    # (chi^2 with 2l+1 degrees of freedom: the extreme-value bound is applied where it is near Gaussian)
    assert z[:, 30:].abs().max().item() < 6.5 and abs(z.mean().item()) < 0.05, (z[:, 30:].abs().max().item(), z.mean().item())
    assert abs((z**2).mean().item() - 1.0) < 0.05
    # cross-spectrum of channels 100/101 at l in [200, 2048]: correlation coefficient as in the model
    a0, a1 = alm[:, 25, :, 0], alm[:, 25, :, 1]                                        # channels 100, 101
    cross = (a0 * a1).sum(dim=1)
    idx_l = torch.cat([torch.arange(m, L, device=ctx.device) for m in range(L)])
    sel = idx_l >= 200
    r_hat = (cross[sel].sum() / torch.sqrt((a0[sel] ** 2).sum() * (a1[sel] ** 2).sum())).item()
    wl = (2 * l[200:] + 1)
    r_mod = ((wl * C[200:, 100, 101]).sum() / torch.sqrt((wl * C[200:, 100, 100]).sum() * (wl * C[200:, 101, 101]).sum())).item()
    assert abs(r_hat - r_mod) < 5e-3, (r_hat, r_mod)
    del T, C
    # (2) maps -> analysis -> a_lm for 8 channels
    sub = alm[:, 24:26].contiguous()                                                   # channels 96..103
    maps = ctx.alm2map(sub, nside, lmax, 8)                                            # K4 + K5
    rec = hputil.map2alm_device(maps, nside, lmax, use_weights=True, niter=3)
    sub0 = sub.clone()
    sub0[:L, :, 1, :] = 0.0                                                            # Im a_l0 is not in the map
    err = (rec - sub0).abs().max().item() / sub0.abs().max().item()
    assert err < 2e-3, err
    del alm, maps, rec
    torch.cuda.empty_cache()


def test_config4_three_components_frequency_shard(ctx):
    """configs[3]: 21cm (zromb 3) + synchrotron + unresolved point sources (zromb 0) on a 512-channel grid,
    nside 1024, lmax 2048 - the 64-channel shard one of eight ranks synthesises.  The sum of the component maps
    equals the synthesis of the summed a_lm (linearity across components), every component's drawn spectrum
    matches its own C_l, and C_0 = 0 components carry no monopole."""
    import torch
    from cora_amd.core import skysim
    from cora_amd.foreground import galaxy, pointsource
    from cora_amd.signal import corr21cm

    nside, lmax, F, nu0, nnu = 1024, 2048, 512, 192, 64
    L = lmax + 1
    freq = 400.0 + (np.arange(F) + 0.5) * (400.0 / F)
    comps = [(corr21cm.Corr21cm(), 3), (galaxy.FullSkySynchrotron(), 0), (pointsource.CombinedPointSources._UnresolvedBackground(), 0)]
    l = torch.arange(L, device=ctx.device, dtype=torch.float64)
    total_alm = None
    total_map = None
    for k, (model, zromb) in enumerate(comps):
        C = skysim.clarray_device(model.angular_powerspectrum, lmax, freq, zromb=zromb)
        T, info = skysim.factor_device(C)
        alm = ctx.draw_alm_philox(T, info, 77 + k, lmax, F, nu0=nu0, nnu=nnu)
        ps = _alm_power(alm, lmax)                                                     # [64, L]
        expect = torch.diagonal(C, dim1=1, dim2=2).T[nu0:nu0 + nnu] * (2 * l + 0.5) / (2 * l + 1)
        z = ((ps - expect) / (expect * torch.sqrt(2.0 / (2 * l + 1))))[:, 2:]
        assert z[:, 30:].abs().max().item() < 6.5 and abs(z.mean().item()) < 0.1, (k, z[:, 30:].abs().max().item(), z.mean().item())
        if k > 0:
            assert float(ps[:, 0].abs().max().item()) == 0.0                            # C_0 = 0 (gaussianfg.py:108-115)
        m = ctx.alm2map(alm, nside, lmax, nnu)
        total_map = m.clone() if total_map is None else total_map + m
        total_alm = alm.clone() if total_alm is None else total_alm + alm
        del C, T, alm, m
    both = ctx.alm2map(total_alm, nside, lmax, nnu)
    assert (both - total_map).abs().max().item() <= 1e-11 * total_map.std().item()
    # the synchrotron dominates and is red: brighter at the low-frequency end of the shard
    assert total_map[0].std().item() > total_map[-1].std().item()
    del both, total_map, total_alm
    torch.cuda.empty_cache()


def test_config4_skysum_full_size_factors_and_synthesis(ctx):
    """configs[3] through the product object (parallel.SkySum; 512 channels, nside 1024, lmax 2048 on one GPU), both
    forms.  (i) The near-singular F = 512 foreground blocks (cond ~ 1e19): Cholesky branch for every l >= 1
    (info = 0; the all-zero l = 0 block gives the zero root the reference's eigen branch returns) and
    |T T^T - (C_l + jitter)| <= 1e-13 max C_l at six multipoles; (ii) the joint factor reproduces
    sum_c (C_l^(c) + jitter_c) to the same bound; (iii) two channels of the realised maps equal the ORACLE synthesis
    of the a_lm SkySum drew and summed, pixel by pixel; (iv) the joint draw's spectrum matches the diagonal of the
    summed covariance (cora/core/skysim.py:114-121 run once instead of three times)."""
    import torch
    from cora_amd.core import skysim
    from cora_amd.foreground import galaxy, pointsource
    from cora_amd.parallel import SkySum
    from cora_amd.signal import corr21cm
    from oracle import sht

    nside, lmax, F = 1024, 2048, 512
    L = lmax + 1
    freq = 400.0 + (np.arange(F) + 0.5) * (400.0 / F)
    mk = lambda: [(corr21cm.Corr21cm(), 3), (galaxy.FullSkySynchrotron(), 0),      # noqa: E731
                  (pointsource.CombinedPointSources._UnresolvedBackground(), 0)]
    ls = [0, 1, 2, 100, 1000, 2048]
    eye = torch.eye(F, device=ctx.device, dtype=torch.float64)

    def packed(alm, f):
        g, v = divmod(f, 4)
        return alm[:, g, 0, v].cpu().numpy() + 1j * alm[:, g, 1, v].cpu().numpy()

    def check_maps(obj, tag):
        maps = obj.realise(4040, fac)
        for f in (0, F - 1):
            ref = sht.alm2map(packed(obj.alm_buf, f), nside, lmax)
            err = np.abs(maps[f].cpu().numpy() - ref).max() / ref.std()
            print("cfg4 SkySum(%s) channel %d: max|err|/rms = %.2e" % (tag, f, err))
            assert err <= 1e-11, (tag, f, err)

    # ---- separate form
    sky = SkySum(mk(), freq, nside, lmax, mode="separate")
    fac = sky.factors()
    Csum = None
    for k, (model, zromb) in enumerate(mk()):
        C = skysim.clarray_device(model.angular_powerspectrum, lmax, freq, zromb=zromb)[ls]
        jit = C.diagonal(dim1=1, dim2=2).amax(dim=1) * 1e-14
        Cj = C + jit[:, None, None] * eye
        Csum = Cj if Csum is None else Csum + Cj
        T, info, rows = fac[k]
        if k > 0:                                  # the separable foreground components: one factor serves every l
            assert rows and tuple(T.shape) == (L, F, F) and int(info.abs().sum().item()) == 0
            Tl = T[ls]
            res = (Tl @ Tl.transpose(1, 2) - Cj).abs().amax(dim=(1, 2)) / Cj.abs().amax(dim=(1, 2)).clamp_min(1e-300)
            print("cfg4 component %d: |T T^T - C|/max C at l = %s: %s" % (k, ls, ["%.1e" % v for v in res.tolist()]))
            assert res[1:].max().item() <= 1e-13 and float(Tl[0].abs().max().item()) == 0.0
            assert torch.equal(Tl.triu(1), torch.zeros_like(Tl))          # lower triangular: the Cholesky branch
        del C
    check_maps(sky, "separate")
    del sky, fac, T, Tl
    torch.cuda.empty_cache()

    # ---- joint form
    sky = SkySum(mk(), freq, nside, lmax, mode="joint")
    fac = sky.factors()
    assert len(fac) == 1
    T, info, rows = fac[0]
    assert not rows and int(info.abs().sum().item()) == 0                 # every block of the sum is positive definite
    Tl = T[ls]
    res = (Tl @ Tl.transpose(1, 2) - Csum).abs().amax(dim=(1, 2)) / Csum.abs().amax(dim=(1, 2))
    print("cfg4 joint: |T T^T - sum_c (C + jitter)|/max at l = %s: %s" % (ls, ["%.1e" % v for v in res.tolist()]))
    assert res.max().item() <= 1e-13
    check_maps(sky, "joint")
    # spectrum of the joint draw against the diagonal of the summed covariance (m = 0 quirk: (2l + 1/2) / (2l + 1))
    l = torch.arange(L, device=ctx.device, dtype=torch.float64)
    ps = _alm_power(sky.alm_buf, lmax)                                      # [F, L]
    diag = None
    for model, zromb in mk():
        d = torch.diagonal(skysim.clarray_device(model.angular_powerspectrum, lmax, freq, zromb=zromb), dim1=1, dim2=2).T.clone()
        diag = d if diag is None else diag + d
    expect = diag * (2 * l + 0.5) / (2 * l + 1)
    z = ((ps - expect) / (expect * torch.sqrt(2.0 / (2 * l + 1))))[:, 2:]
    assert z[:, 30:].abs().max().item() < 6.5 and abs(z.mean().item()) < 0.1, (z[:, 30:].abs().max().item(), z.mean().item())
    del sky, fac, T, Tl, ps, diag
    torch.cuda.empty_cache()


def test_config5_geometry_synthesis_properties(ctx):
    """configs[4] geometry (nside 2048, lmax 4096; one 8-channel slice of a rank's 128): the largest plan -
    ring FFTs of 8192 pixels (two channels per workgroup), Bluestein length 8192, 8.4 M a_lm per channel.
    Parseval and linearity of the synthesis, and lambda_lm at l = m = 4096 against the closed form."""
    import torch

    nside, lmax, nnu = 2048, 4096, 8
    L = lmax + 1
    nalm = L * (L + 1) // 2
    gen = torch.Generator(device=ctx.device).manual_seed(9)
    idx_l = torch.cat([torch.arange(m, L, device=ctx.device) for m in range(L)])
    amp = 1.0 / (1.0 + idx_l.double())
    a = torch.randn((nalm, 2, 2, 4), generator=gen, device=ctx.device, dtype=torch.float64) * amp[:, None, None, None]
    b = torch.randn((nalm, 2, 2, 4), generator=gen, device=ctx.device, dtype=torch.float64) * amp[:, None, None, None]
    ma = ctx.alm2map(a, nside, lmax, nnu).clone()
    ps = _alm_power(a.clone(), lmax)                                                    # [8, L]
    var_alm = (ps * (2 * torch.arange(L, device=ctx.device, dtype=torch.float64) + 1)).sum(dim=1) / (4 * np.pi)
    rel = (((ma**2).mean(dim=1) - var_alm).abs() / var_alm).max().item()
    assert rel < 2e-3, rel
    mb = ctx.alm2map(b, nside, lmax, nnu).clone()
    mc = ctx.alm2map(2.0 * a - 3.0 * b, nside, lmax, nnu)
    assert (mc - (2.0 * ma - 3.0 * mb)).abs().max().item() < 1e-11 * mc.std().item()
    # lambda_mm(theta) = (-1)^m sqrt((2m+1)!!/(4 pi (2m)!!)) sin^m(theta) at m = lmax, equator ring pair
    lam = ctx.sht_lambda(nside, lmax, lmax, 2 * nside - 1).cpu().numpy()
    import math
    lg = 0.5 * (math.lgamma(2 * lmax + 2) - 2 * math.lgamma(lmax + 1) - (2 * lmax) * math.log(2.0) - math.log(4 * math.pi))
    assert abs(lam[0] - math.exp(lg)) < 1e-9 * math.exp(lg)       # z = 0: sin theta = 1; (-1)^4096 = +1
    del a, b, ma, mb, mc
    torch.cuda.empty_cache()


def test_c_abi_with_ctypes_only_no_torch(tmp_path, golden):
    """The drop-in boundary on its own: tools/abi_ctypes_demo.py drives libcorahip.so with ctypes + numpy in a
    process that never imports torch (the binding INTEGRATION.md shows), and its seeded maps / a_lm equal the
    reference's own a_lm (golden) and the oracle synthesis; the analysis entry point inverts the maps."""
    import os
    import subprocess
    import sys

    from oracle import sht
    from oracle import skysim as osk

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = str(tmp_path / "abi.npz")
    p = subprocess.run([sys.executable, os.path.join(root, "tools", "abi_ctypes_demo.py"), "cla_21cm_F8_l64_zromb3", "32",
                        "4", out], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "ABI_DEMO ok" in p.stdout and p.stdout.strip().endswith("False"), p.stdout + p.stderr
    r = np.load(out)
    ref_alm = golden["alm_21cm_F8_l64_seed4"]                       # the reference's own mkfullsky(alms=True, rng=default_rng(4))
    assert np.abs(r["alm"] - ref_alm).max() <= 1e-12 * np.abs(ref_alm).max()
    for i in (0, 5):
        m = sht.alm2map(osk.pack_alm(ref_alm[i, 0]), 32, 64)
        assert np.abs(r["maps"][i] - m).max() <= 1e-11 * m.std()
        a1 = sht.map2alm_adjoint(r["maps"][i], 32, 64, None)
        got = osk.pack_alm(r["rec"][i, 0])
        assert np.abs(got - a1).max() <= 1e-12 * np.abs(a1).max()


def test_fused_mkfullsky_entry_point(ctx, golden):
    """corahip_mkfullsky (the fused convenience entry) against the five-call chain behind
    skysim.mkfullsky_device, for its three kinds of normals; the PCG64 kind hands back the generator state numpy would
    be left in; a workspace too small for one synthesis pass is worked through in chunks, one too small for anything
    is refused with CORAHIP_ENOMEM."""
    import torch
    from cora_amd import _lib
    from cora_amd.core import skysim
    from cora_amd.util.nputil import DeviceRNG

    C = golden["cla_21cm_F8_l64_zromb3"]
    Cd = ctx.to_device(C)
    F, nside = C.shape[1], 32
    rng = np.random.default_rng(4)
    st = rng.bit_generator.state["state"]
    ref_maps = skysim.mkfullsky_device(C, nside, rng=np.random.default_rng(4))
    maps, after = ctx.mkfullsky_fused(Cd, nside, ("pcg64", st["state"], st["inc"]))
    assert torch.equal(maps, ref_maps)
    g = skysim._host_normals(F, C.shape[0] - 1, rng)                   # advances `rng` as the reference's draws do
    assert after == int(rng.bit_generator.state["state"]["state"])
    alm, _ = ctx.mkfullsky_fused(Cd, nside, ("pcg64", st["state"], st["inc"]), alms=True)
    ref_alm = golden["alm_21cm_F8_l64_seed4"]
    assert np.abs(alm.cpu().numpy() - ref_alm).max() <= 1e-12 * np.abs(ref_alm).max()
    maps_s, _ = ctx.mkfullsky_fused(Cd, nside, ("stream", ctx.to_device(g)))
    assert torch.equal(maps_s, ref_maps)
    maps_p, _ = ctx.mkfullsky_fused(Cd, nside, ("philox", 77), nu0=2, nnu=4)
    assert torch.equal(maps_p, skysim.mkfullsky_device(C, nside, rng=DeviceRNG(77), nu_range=(2, 4)))
    # rng=None of the reference: numpy's legacy global state through the same entry
    np.random.seed(1234)
    alm_l, st_l = ctx.mkfullsky_fused(ctx.to_device(golden["cla_21cm_F4_l16_zromb1"]), 8, ("legacy", np.random.get_state(legacy=False)),
                                      alms=True)
    ref_l = golden["alm_21cm_F4_l16_legacy1234"]
    assert np.abs(alm_l.cpu().numpy() - ref_l).max() <= 1e-12 * np.abs(ref_l).max()
    twin = np.random.RandomState(0)
    twin.set_state(st_l)
    skysim._host_normals(4, 16, None)                                  # (np.random was seeded 1234: the reference's draws)
    assert np.array_equal(twin.random_sample(64), np.random.random_sample(64))
    # chunked synthesis: the minimum the entry accepts is in the error text of a refused call
    with pytest.raises(RuntimeError) as ei:
        ctx.mkfullsky_fused(Cd, nside, ("stream", ctx.to_device(g)), workspace_bytes=1024)
    need_min = int(str(ei.value).split("need at least ")[1].split()[0])
    maps_c, _ = ctx.mkfullsky_fused(Cd, nside, ("stream", ctx.to_device(g)), workspace_bytes=need_min)
    assert torch.equal(maps_c, ref_maps)


def test_pinned_tables_follow_table_changes(ctx):
    """K1 keeps its transposed copy of the 21cm tables between calls while the model has them pinned
    (corahip_clarray_tables_pin); assigning new tables (the setters the reference's load_fft_cache uses,
    cora/signal/corr.py:879-887) must not leave a stale copy behind: C_l of the doubled tables is exactly 2 C_l."""
    from cora_amd.core import skysim
    from cora_amd.signal import corr21cm

    m = corr21cm.Corr21cm()
    freq = 600.0 + 2.0 * np.arange(6)
    C1 = skysim.clarray(m.angular_powerspectrum, 40, freq, zromb=1)
    C1b = skysim.clarray(m.angular_powerspectrum, 40, freq, zromb=1)      # second call: the pinned copy is reused
    assert np.array_equal(C1, C1b)
    dd, dv, vv = m._aps_dd.copy(), m._aps_dv.copy(), m._aps_vv.copy()
    m._aps_dd, m._aps_dv, m._aps_vv = 2.0 * dd, 2.0 * dv, 2.0 * vv
    C2 = skysim.clarray(m.angular_powerspectrum, 40, freq, zromb=1)
    assert np.array_equal(C2, 2.0 * C1)
    other = corr21cm.Corr21cm()                                            # a second model on the same context, then back
    C3 = skysim.clarray(other.angular_powerspectrum, 40, freq, zromb=1)
    assert np.array_equal(C3, C1)
    assert np.array_equal(skysim.clarray(m.angular_powerspectrum, 40, freq, zromb=1), C2)


def test_table_pin_does_not_outlive_the_model(ctx):
    """A model's pin of its tables (K1 keeps a transposed copy of pinned tables) is withdrawn when the model is
    collected or its device tables are dropped: afterwards the SAME device blocks carrying other numbers - what the
    caching allocator hands to the next caller - are read afresh, not taken for the pinned tables."""
    import gc

    import torch
    from cora_amd.core import skysim
    from cora_amd.signal import corr21cm

    freq = 600.0 + 2.0 * np.arange(6)
    for how in ("collected", "tables dropped"):
        m = corr21cm.Corr21cm()
        C1 = skysim.clarray_device(m.angular_powerspectrum, 40, freq, zromb=1)
        p = m._table_plan(lambda za: 1420.40575177 / za - 1.0)["prepare"](ctx, freq)   # the raw arguments K1 was called with
        dd, dv, vv = p["dd"], p["dv"], p["vv"]                                    # (our references keep the blocks alive)
        args = (p["kperpmin"], p["kperpmax"], p["kparmax"], ctx.to_device(p["chi"]), ctx.to_device(p["pfd"]),
                ctx.to_device(p["f"]), ctx.to_device(p["b"]), len(freq), 1, ctx.to_device(np.ones(1)),
                ctx.to_device(np.log10(np.arange(1.0, 6.0))))
        base = ctx.clarray_table21cm(dd, dv, vv, *args)                          # (pinned copy in use)
        if how == "collected":
            del m, p
            gc.collect()
        else:
            m._aps_dd = m._aps_dd * 1.0                                          # a setter: device tables dropped, pin withdrawn
        for t in (dd, dv, vv):
            t.mul_(2.0)                                                          # same addresses, other numbers (x 2: exact)
        torch.cuda.synchronize()
        got = ctx.clarray_table21cm(dd, dv, vv, *args)
        assert torch.equal(got, 2.0 * base), how
        del C1


def test_factor_rows_pack_unpack_kernels(ctx):
    """corahip_factor_rows_pack / _unpack (csrc/shard.hip) against the permutation they implement, including an
    empty l block (a rank with no multipoles), uneven blocks and an odd row length."""
    import torch

    for F, world, counts in ((8, 2, [3, 2]), (12, 4, [2, 0, 3, 1]), (6, 3, [1, 1, 1]), (10, 5, [4, 4, 0, 0, 1])):
        nnu, l_stride, L = F // world, max(max(counts), 1), sum(counts)
        gen = torch.Generator(device=ctx.device).manual_seed(F)
        blocks = [torch.randn((c, F, F), generator=gen, device=ctx.device, dtype=torch.float64) for c in counts]
        sends = [ctx.factor_rows_pack(b, l_stride, world) for b in blocks]            # what every rank would send
        for r, (b, sd) in enumerate(zip(blocks, sends)):
            want = torch.zeros((world, l_stride, nnu, F), device=ctx.device, dtype=torch.float64)
            for q in range(world):
                want[q, : counts[r]] = b[:, q * nnu:(q + 1) * nnu, :]
            assert torch.equal(sd, want), (F, world, r)
        full = torch.cat(blocks, dim=0)                                                 # [L, F, F]
        for q in range(world):                                                          # what rank q receives: slab q of every rank
            recv = torch.stack([sd[q] for sd in sends]).contiguous()
            T_rows = ctx.factor_rows_unpack(recv, counts)
            assert tuple(T_rows.shape) == (L, nnu, F)
            assert torch.equal(T_rows, full[:, q * nnu:(q + 1) * nnu, :]), (F, world, q)


def test_c_abi_sharded_mkfullsky_two_processes_no_torch(tmp_path, golden):
    """The sharded path through the C ABI alone (corahip_shard_plan, corahip_factor_rows_pack / _unpack,
    corahip_draw_alm_philox_rows): tools/abi_shard_demo.py runs mkfullsky on an
    l-distributed C_l (cora/core/skysim.py:97-110,125-134) as 2 and 3 ctypes-only processes that exchange the factor
    row blocks through files - what a caput / mpi4py caller would do with MPI_Alltoall - and their frequency shards
    must equal the single-process realisation of the same seed; that one is checked against the oracle's synthesis
    of its own a_lm and against T g computed in numpy from the device Philox stream's specification."""
    import os
    import subprocess
    import sys

    from oracle import philox
    from oracle import sht
    from oracle import skysim as osk

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    key, nside, seed = "cla_21cm_F8_l64_zromb3", 16, 11
    # F = 8: world 2 and 4 divide it (row-block exchange); L = 65 splits unevenly over both
    for world in (2, 4):
        d = str(tmp_path / ("w%d" % world))
        os.makedirs(d)
        p = subprocess.run([sys.executable, os.path.join(root, "tools", "abi_shard_demo.py"), key, str(nside), str(seed),
                            str(world), "launch", d], capture_output=True, text=True, timeout=600)
        assert p.returncode == 0 and "ABI_SHARD ok" in p.stdout and p.stdout.strip().endswith("False"), p.stdout + p.stderr
        em, ea = (float(v) for v in p.stdout.split("ABI_SHARD ok")[1].split()[:2])
        assert em <= 1e-13 and ea <= 1e-13, (world, em, ea)
    r = np.load(os.path.join(d, "single.npz"))
    C = golden[key]
    L, F, _ = C.shape
    lmax = L - 1
    # the single-process result itself: a_lm = T g with g the specified Philox stream, maps = synthesis of those a_lm
    g = philox.device_normals(seed, lmax, F)
    o = 0
    for l in range(L):
        n = F * (l + 1)
        re, im = g[o:o + n].reshape(F, l + 1), g[o + n:o + 2 * n].reshape(F, l + 1)
        o += 2 * n
        T = osk.matrix_root_manynull(C[l] + np.identity(F) * C[l].diagonal().max() * 1e-14, truncate=False)
        ref = T @ ((re + 1j * im) / 2**0.5)
        assert np.abs(r["alm"][:, 0, l, : l + 1] - ref).max() <= 1e-12 * np.abs(ref).max(), l
    for i in (0, 7):
        m = sht.alm2map(osk.pack_alm(r["alm"][i, 0]), nside, lmax)
        assert np.abs(r["maps"][i] - m).max() <= 1e-11 * m.std()


def test_complex_transform_family(ctx):
    """hputil.sphtrans_inv_complex / sphtrans_complex (cora/util/hputil.py:237-263,435-457): a complex field from
    a_lm with both signs of m equals the oracle synthesis of its real/imaginary projections, and transforms back."""
    from cora_amd.util import hputil
    from oracle import sht
    from oracle import skysim as osk

    nside, lmax = 16, 20
    L = lmax + 1
    rng = np.random.default_rng(12)
    full = np.zeros((L, 2 * L - 1), dtype=np.complex128)
    for l in range(L):
        for m in range(-l, l + 1):
            full[l, m] = rng.standard_normal() + 1j * rng.standard_normal()     # FFT order: negative m at the end
    # the reference's split puts ALL of a_l0 into the "real" part and synthesises only Re(a_l0): the m = 0 modes
    # of the imaginary part of the field are dropped (hputil.py:451-457) - mirrored, so keep a_l0 real here
    full[:, 0] = full[:, 0].real
    z = hputil.sphtrans_inv_complex(full, nside)
    almr = hputil._make_half_alm(full)
    almi = 1.0j * (full[:, :L] - almr)
    ref = sht.alm2map(osk.pack_alm(almr), nside, lmax) + 1j * sht.alm2map(osk.pack_alm(almi), nside, lmax)
    assert np.abs(z - ref).max() <= 1e-11 * np.abs(ref).max()
    # hputil.py:455 builds the imaginary part as 1j * (a - a_real) = -s_lm (s = coefficients of Im f): the
    # reference's inverse returns the CONJUGATE of the field whose forward transform is `full` - mirrored
    back = hputil.sphtrans_complex(np.conj(z), lmax)
    assert back.shape == (L, 2 * L - 1) and np.abs(back - full).max() < 1e-5 * np.abs(full).max()
    back = hputil.sphtrans_complex(z, lmax)
    cen = hputil.sphtrans_complex(z, lmax, centered=True)
    assert np.allclose(cen[:, lmax:], back[:, :L]) and np.allclose(cen[:, :lmax], back[:, L:])
    with pytest.raises(Exception, match="wrong shape"):
        hputil.sphtrans_inv_complex(np.zeros((4, 4), dtype=np.complex128), nside)
    # a real field has a_{l,-m} = (-1)^m conj(a_lm): _make_full_alm / _make_half_alm are inverse there
    half = hputil.unpack_alm(osk.pack_alm(almr), lmax)
    assert np.allclose(hputil._make_half_alm(hputil._make_full_alm(half)), half)


# ------------------------------------------------------------------ n3: xi(r) -> C_l(chi, chi')
def _xi_model(r):
    r = np.asarray(r, dtype=np.float64)
    return np.exp(-r / 60.0) * np.cos(r / 35.0) / (1.0 + (r / 15.0) ** 2)


def test_corr_to_clarray_reference_vectors(ctx):
    """corrfunc.corr_to_clarray (generic callable: host xi, device bin average + Legendre MFMA projection) against
    outputs of the reference's own function (tests/golden/corrfunc_vectors.npz)."""
    import os

    from cora_amd.signal import corrfunc

    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "corrfunc_vectors.npz"))
    assert np.abs(corrfunc.legendre_array(12, g["legendre_l12_mu"]) - g["legendre_l12"]).max() < 1e-14
    xa = g["xarray"]
    for tag, lmax, kw in (("l40_xromb2_q2", 40, dict(xromb=2, q=2)), ("l40_xromb0_q3", 40, dict(xromb=0, q=3)),
                          ("l24_xromb1_xw10", 24, dict(xromb=1, q=2, xwidth=10.0))):
        got = corrfunc.corr_to_clarray(_xi_model, lmax, xa, chunksize=7, **kw)
        ref = g["cl_" + tag]
        assert got.shape == ref.shape and np.abs(got - ref).max() <= 1e-12 * np.abs(ref).max(), tag


def test_corr_to_clarray_spline_tables_on_device(ctx):
    """The device evaluation of spline correlation functions (plain / log / sinh interpolaters, bisection, end-slope
    extrapolation, radial-bin average) equals the host evaluation of the same interpolater through the generic path,
    and the oracle; sizes where the GEMM has several tiles and a ragged K."""
    from cora_amd.signal import corrfunc
    from cora_amd.util import cubicspline as cs
    from oracle import corrfunc as ocf

    r = np.concatenate([[0.0], np.logspace(-1, 3.7, 300)])
    f = _xi_model(r)
    sinh = cs.SinhInterpolater(np.stack([r, f], axis=1), 1.0, 1e-4)
    plain = cs.Interpolater(np.stack([r, f], axis=1))
    logi = cs.LogInterpolater(np.stack([r[1:], np.exp(-r[1:] / 80.0) + 1e-3], axis=1))
    xa = 1400.0 + 12.5 * np.arange(20) + 3.0 * np.sin(np.arange(20))
    for interp, lmax, xromb, q in ((sinh, 150, 2, 2), (plain, 37, 1, 3), (logi, 64, 0, 2)):
        dev = corrfunc.corr_to_clarray(interp, lmax, xa, xromb=xromb, q=q)
        host = ocf.corr_to_clarray(lambda rr: interp.value(np.ravel(rr)).reshape(np.shape(rr)), lmax, xa, xromb=xromb, q=q)
        assert dev.shape == (lmax + 1, 20, 20)
        assert np.abs(dev - host).max() <= 1e-11 * np.abs(host).max(), (type(interp).__name__, np.abs(dev - host).max())
        assert np.array_equal(dev, dev.transpose(0, 2, 1))
    # the interpolaters themselves: array entry points agree with scalar calls, extrapolation on both sides
    pts = np.array([0.0, 0.05, 0.1, 3.3, 4000.0, 9000.0])
    assert np.allclose(sinh.value_sinh_array(pts), [sinh(float(p)) for p in pts], rtol=1e-14, atol=0)


def test_getsky_shard_equals_sky3d_getsky():
    """parallel.getsky_shard (the N-rank pipeline object, here 1 rank) == Sky3d.getsky with the same device seed,
    including the mean-temperature offset (cora/core/maps.py:227-237)."""
    from cora_amd import DeviceRNG
    from cora_amd.parallel import getsky_shard
    from cora_amd.signal import corr21cm

    cr = corr21cm.Corr21cm()
    cr.nside = 16
    cr.frequencies = np.array([500.0, 510.0, 520.0, 530.0, 540.0, 550.0, 560.0, 570.0])
    cr.oversample = 2
    ref = cr.getsky(rng=DeviceRNG(77))
    maps, nu0 = getsky_shard(cr, 77)
    assert nu0 == 0 and np.array_equal(maps.cpu().numpy(), ref)


def test_small_and_ragged_sizes_next_rows(ctx):
    """Edge sizes of the n1 / n3 entry points: tiny lmax (mu nodes not a multiple of the GEMM's K chunk), two
    distances, one channel; nside 1 and 2 analysis with channel counts that are not multiples of 4 or 8."""
    import torch
    from cora_amd.signal import corrfunc
    from cora_amd.util import hputil
    from oracle import corrfunc as ocf
    from oracle import sht

    for lmax, xa, xromb, q in ((3, [100.0, 130.0], 0, 2), (5, [50.0, 60.0, 75.0], 1, 3), (17, [10.0, 20.0], 2, 2)):
        got = corrfunc.corr_to_clarray(_xi_model, lmax, np.array(xa), xromb=xromb, q=q)
        ref = ocf.corr_to_clarray(_xi_model, lmax, np.array(xa), xromb=xromb, q=q)
        assert got.shape == ref.shape and np.abs(got - ref).max() <= 1e-12 * np.abs(ref).max(), (lmax, xromb)
    rng = np.random.default_rng(1)
    for nside, lmax, nnu in ((1, 2, 1), (2, 4, 3), (2, 5, 9), (4, 8, 13)):
        maps = rng.standard_normal((nnu, 12 * nside * nside))
        alm = ctx.map2alm(torch.from_numpy(maps).to(ctx.device), nside, lmax, None)
        got = ctx.alm_dev_to_square(alm, lmax, nnu).cpu().numpy()[:, 0]
        for k in (0, nnu - 1):
            ref = hputil.unpack_alm(sht.map2alm_adjoint(maps[k], nside, lmax, None), lmax)
            assert np.abs(got[k] - ref).max() <= 1e-12 * max(np.abs(ref).max(), 1e-300), (nside, lmax, nnu, k)


# ------------------------------------------------------------------ n4: polarised (spin-2) synthesis
@pytest.mark.parametrize("nside,lmax,nfreq", [(4, 8, 1), (8, 20, 3), (16, 47, 4), (32, 64, 8), (64, 150, 2),
                                              # legendre_pol_kernel<2>, <4> with steady-state stages
                                              (64, 150, 8), (64, 150, 16)])
def test_alm2map_spin2_vs_oracle(ctx, nside, lmax, nfreq):
    """(E, B) -> (Q, U) on the GPU (legendre_pol_kernel + the ring FFT) against the CPU oracle, through the C ABI."""
    import torch
    from oracle import sht

    rng = np.random.default_rng(7 * nside + nfreq)
    n = (lmax + 1) * (lmax + 2) // 2
    nch = 2 * nfreq
    npad = nch if nch % 8 in (0, 6) else (nch + 7) // 8 * 8
    packed = np.zeros((npad, n), dtype=np.complex128)
    packed[:nch] = rng.standard_normal((nch, n)) + 1j * rng.standard_normal((nch, n))
    packed[:, : lmax + 1] = packed[:, : lmax + 1].real
    dev = ctx.alm_packed_to_dev(torch.from_numpy(packed).to(ctx.device), lmax)
    maps = ctx.alm2map_spin2(dev, nside, lmax, npad).cpu().numpy()
    for f in range(nfreq):
        q, u = sht.alm2map_spin2(packed[2 * f], packed[2 * f + 1], nside, lmax)
        assert np.abs(maps[2 * f] - q).max() <= 1e-11 * q.std(), (f, np.abs(maps[2 * f] - q).max() / q.std())
        assert np.abs(maps[2 * f + 1] - u).max() <= 1e-11 * u.std(), f
    assert np.all(maps[nch:] == 0)


def test_sphtrans_inv_pol_api(ctx):
    """hputil.sphtrans_inv_real_pol / sphtrans_inv_sky with 3 and 4 polarisation entries (hputil.py:394-432,500-531)."""
    from cora_amd.util import hputil
    from oracle import sht
    from oracle import skysim as osk

    nside, lmax, nfreq = 8, 16, 3
    L = lmax + 1
    rng = np.random.default_rng(21)
    alm = np.zeros((nfreq, 4, L, L), dtype=np.complex128)
    for l in range(L):
        alm[:, :, l, : l + 1] = rng.standard_normal((nfreq, 4, l + 1)) + 1j * rng.standard_normal((nfreq, 4, l + 1))
    alm[:, :, :, 0] = alm[:, :, :, 0].real
    sky = hputil.sphtrans_inv_sky(alm, nside)
    assert sky.shape == (nfreq, 4, 12 * nside * nside)
    for f in range(nfreq):
        t = sht.alm2map(osk.pack_alm(alm[f, 0]), nside, lmax)
        v = sht.alm2map(osk.pack_alm(alm[f, 3]), nside, lmax)
        q, u = sht.alm2map_spin2(osk.pack_alm(alm[f, 1]), osk.pack_alm(alm[f, 2]), nside, lmax)
        for got, ref in ((sky[f, 0], t), (sky[f, 1], q), (sky[f, 2], u), (sky[f, 3], v)):
            assert np.abs(got - ref).max() <= 1e-11 * ref.std()
    one = hputil.sphtrans_inv_real_pol(alm[1, :3], nside)
    assert one.shape == (3, 12 * nside * nside) and np.abs(one - sky[1, :3]).max() <= 1e-12 * np.abs(one).max()
    with pytest.raises(Exception, match="wrong shape"):
        hputil.sphtrans_inv_real_pol(alm[0, :2], nside)


# ------------------------------------------------------------------ polarised (spin-2) analysis
@pytest.mark.parametrize("nside,lmax,nf,weights", [(4, 8, 1, False), (8, 12, 2, True), (16, 32, 3, True), (32, 64, 5, False)])
def test_map2alm_spin2_quadrature_vs_oracle(ctx, nside, lmax, nf, weights):
    """One (Q, U) -> (E, B) quadrature pass, composed on the device from six scalar passes over ring-scaled maps,
    vs the oracle's direct W / X quadrature."""
    import torch
    from oracle import sht

    rng = np.random.default_rng(7 * nside + nf)
    npix = 12 * nside * nside
    qu = rng.standard_normal((2 * nf, npix))
    w = sht.ring_weights(nside) if weights else None
    dev = ctx.map2alm_spin2(torch.from_numpy(qu).to(ctx.device), nside, lmax, ctx.to_device(w) if weights else None)
    sq = ctx.alm_dev_to_square(dev, lmax, 4 * dev.shape[1]).cpu().numpy()[: 2 * nf, 0]          # [2 nf, l, m]
    for f in range(nf):
        e, b = sht.map2alm_spin2_adjoint(qu[2 * f], qu[2 * f + 1], nside, lmax, w)
        scale = max(np.abs(e).max(), np.abs(b).max())
        for m in range(lmax + 1):
            for l in range(m, lmax + 1):
                i = sht.alm_index(l, m, lmax)
                assert abs(sq[2 * f, l, m] - e[i]) < 2e-12 * scale and abs(sq[2 * f + 1, l, m] - b[i]) < 2e-12 * scale
    assert np.abs(sq[:, :2]).max() == 0.0                                       # l < 2 carries no spin-2 power


def test_sphtrans_real_pol_round_trip_and_api(ctx):
    """hputil.sphtrans_real_pol / sphtrans_complex_pol / the polarised branch of sphtrans_sky: healpy.map2alm(iter=2,
    use_weights) semantics vs the oracle, and recovery of band-limited T, E, B (V) through sphtrans_inv_real_pol."""
    from cora_amd.util import hputil
    from oracle import sht

    nside, lmax = 16, 24
    L = lmax + 1
    rng = np.random.default_rng(3)
    alm = np.zeros((4, L, L), dtype=np.complex128)
    for p in range(4):
        for l in range(2 if p in (1, 2) else 0, L):
            alm[p, l, : l + 1] = (rng.standard_normal(l + 1) + 1j * rng.standard_normal(l + 1)) / (1.0 + l)
            alm[p, l, 0] = alm[p, l, 0].real
    maps = hputil.sphtrans_inv_real_pol(alm, nside)                             # T, Q, U, V
    back = hputil.sphtrans_real_pol(maps, lmax=lmax)
    assert back.shape == (4, L, L)
    assert np.abs(back - alm).max() < 5e-6 * np.abs(alm).max()                  # two Jacobi refinements at lmax = 1.5 nside
    e, b = sht.map2alm_spin2(maps[1], maps[2], nside, lmax, use_weights=True, niter=2)
    t = sht.map2alm(maps[0], nside, lmax, use_weights=True, niter=2)
    for m in range(L):
        for l in range(m, L):
            i = sht.alm_index(l, m, lmax)
            assert abs(back[1, l, m] - e[i]) < 1e-11 and abs(back[2, l, m] - b[i]) < 1e-11 and abs(back[0, l, m] - t[i]) < 1e-11
    three = hputil.sphtrans_real_pol(maps[:3], lmax=lmax, lside=lmax + 3)
    assert three.shape == (3, lmax + 4, lmax + 4) and np.array_equal(three[:, :L, :L], back[:3])
    sky = np.stack([maps, 2.0 * maps])                                          # [freq, pol, npix]
    alm_sky = hputil.sphtrans_sky(sky, lmax=lmax)
    assert alm_sky.shape == (2, 4, L, L)
    assert np.abs(alm_sky[0] - back).max() < 1e-12 and np.abs(alm_sky[1] - 2.0 * back).max() < 1e-11
    cplx = hputil.sphtrans_complex_pol(maps[:3] + 1j * maps[:3][::-1], lmax=lmax)
    assert cplx.shape == (3, L, 2 * L - 1)
    ref = hputil._make_full_alm(back[:3]) + 1j * hputil._make_full_alm(hputil.sphtrans_real_pol(maps[:3][::-1], lmax=lmax))
    assert np.abs(cplx - ref).max() < 1e-12


def test_host_delivery_paths(golden):
    """The numpy-returning surface: mkfullsky through pinned memory, the l-block-wise upload of the host normal stream
    (two staging buffers) and the double-buffered stream of realisations all give the arrays of the plain path."""
    from cora_amd import _lib
    from cora_amd.core import skysim
    from cora_amd.util.nputil import DeviceRNG

    ctx = _lib.get_context()
    C = golden["cla_21cm_F8_l64_zromb3"]
    nside = 128                                                    # 8 x 196608 doubles = 12.6 MB ... below the pinned threshold
    ref = skysim.mkfullsky_device(C, nside, rng=np.random.default_rng(3)).cpu().numpy()
    old = ctx._PINNED_MIN_BYTES
    try:
        type(ctx)._PINNED_MIN_BYTES = 1 << 10                      # force the pinned route
        a = skysim.mkfullsky(C, nside, rng=np.random.default_rng(3))
        assert isinstance(a, np.ndarray) and a.flags.writeable and np.array_equal(a, ref)
        outs = list(skysim.mkfullsky_stream(C, nside, [DeviceRNG(s) for s in (5, 6, 7)]))
        for s, o in zip((5, 6, 7), outs):
            assert np.array_equal(o, skysim.mkfullsky_device(C, nside, rng=DeviceRNG(s)).cpu().numpy())
        outs = list(skysim.mkfullsky_stream(C, nside, [np.random.default_rng(3), None]))
        assert np.array_equal(outs[0], ref) and outs[1].shape == ref.shape
    finally:
        type(ctx)._PINNED_MIN_BYTES = old
    # chunked upload of the host stream: more normals than one 256 MB staging buffer (F = 40, lmax = 1300 -> 68 M)
    F, lmax = 40, 1300
    g_ref = skysim._host_normals(F, lmax, np.random.default_rng(11))
    g_dev = skysim._upload_host_normals(ctx, F, lmax, np.random.default_rng(11)).cpu().numpy()
    assert g_ref.size > (1 << 25) and np.array_equal(g_dev, g_ref)
