"""The device route of skysim.mkconstrained (csrc/constrained.hip) on the GPU against the oracle of
tests/_constrained_oracle.py, whose module docstring derives every tolerance used here (u = 2^-53; none is tuned), and
against the reference's own cv (tests/golden/mkconstrained_vectors.npz).  tests/test_constrained_host.py pins the oracle
to the reference first.  Every test prints its worst error over tolerance."""
import functools

import numpy as np
import pytest

import _constrained_oracle as co
from test_constrained_host import golden_case

pytestmark = pytest.mark.gpu

U = co.U


@pytest.fixture(scope="module")
def gold():
    return co.load_golden()


def _poisoned(ctx, shape, dtype=None):
    import torch

    if dtype is not None:
        return torch.full(shape, -77, dtype=dtype, device=ctx.device)
    return torch.full(shape, float("nan"), dtype=torch.float64, device=ctx.device)


def _eig(ctx, fam, k, max_iter=None):
    import torch

    L, F = fam.shape[0], fam.shape[1]
    out = (_poisoned(ctx, (L, F, k)), _poisoned(ctx, (L, k)), _poisoned(ctx, (L,), torch.int32))
    V, theta, info = ctx.eig_top_batched(ctx.to_device(fam), k, max_iter=max_iter, out=out)
    assert V is out[0] and theta is out[1] and info is out[2]
    return V, theta, info


def _weights(ctx, V, f_ind):
    """W [L, F, k] of the matrices of V through constrained_weights (which keeps l = 0 for itself: one block in front)."""
    import torch

    return ctx.constrained_weights(torch.cat([V[:1], V]), f_ind)[1:].cpu().numpy()


def _check_family(ctx, name, fam, k, max_iter=None):
    """The three assertions of the eigen kernel, in the order that matters (tol_W grows with rho_dev); returns info."""
    L, F = fam.shape[0], fam.shape[1]
    V, theta, info = _eig(ctx, fam, k, max_iter)
    Vh, th, ih = V.cpu().numpy(), theta.cpu().numpy(), info.cpu().numpy()
    assert np.all(np.isfinite(Vh)) and np.all(np.isfinite(th)) and set(ih.tolist()) <= {0, 1}
    f_ind = list(range(F - k, F))[::-1] if F > 2 else list(range(k))
    W = _weights(ctx, V, f_ind)
    worst = [0.0, 0.0, 0.0]
    for l in range(L):
        r = co.rho(fam[l], Vh[l], th[l])
        b_rho = 16 * F * U * co.norm_inf(fam[l])
        worst[0] = max(worst[0], r / b_rho)
        assert r <= b_rho, (name, F, k, l, r, b_rho)
        orth = np.abs(Vh[l].T @ Vh[l] - np.eye(k)).max()
        worst[1] = max(worst[1], orth / (8 * F * U))
        assert orth <= 8 * F * U, (name, F, k, l, orth)
        assert np.all(np.diff(th[l]) >= 0)
        tol, Wref = co.tol_W(fam[l], f_ind, r)
        err = np.abs(W[l] - Wref).max()
        worst[2] = max(worst[2], err / tol)
        assert err <= tol, (name, F, k, l, err, tol)
    print("%s F %d k %d max_iter %s: rho / bound %.3g, orth / bound %.3g, W err / tol %.3g, info %s"
          % (name, F, k, max_iter, worst[0], worst[1], worst[2], ih.tolist()))
    return ih


FS = [1, 2, 3, 15, 16, 17, 18, 34, 64, 258]
FK = [(F, k) for F in FS for k in (1, 2, 3) if k <= F]


@functools.lru_cache(maxsize=None)
def _synch(F):
    return co.synchrotron_family(F)


@functools.lru_cache(maxsize=None)
def _toep(F):
    return co.toeplitz_family(F)


@pytest.mark.parametrize("F,k", FK)
def test_eig_top_synchrotron(ctx, F, k):
    """B A_l for l = 1 .. 5 and B times 7e-20 and 7e+20 (seven matrices): every one takes the iteration."""
    info = _check_family(ctx, "synchrotron", _synch(F), k)
    assert np.all(info == 0)


@pytest.mark.parametrize("F,k", FK)
def test_eig_top_toeplitz(ctx, F, k):
    """exp(-|i - j| / 3): under the default cap (route not asserted) and with max_iter = 1, which reaches the full
    decomposition without waiting wherever the block does not span the space (F > 16)."""
    _check_family(ctx, "toeplitz", _toep(F), k)
    info = _check_family(ctx, "toeplitz", _toep(F), k, max_iter=1)
    assert np.all(info == (1 if F > 16 else 0))


@pytest.mark.parametrize("k", [1, 2, 3])
def test_eig_top_indefinite(ctx, k):
    """Spectrum {-2, 1, 0.6, 0.3 .. 0.01}: the algebraically largest pairs come back, not the largest in magnitude."""
    fam = co.spectrum_family(co.INDEFINITE, 100)
    _check_family(ctx, "indefinite", fam, k)
    _, theta, _ = _eig(ctx, fam, k)
    want = np.sort(co.INDEFINITE)[-k:]
    assert np.all(np.abs(theta.cpu().numpy() - want[None, :]) <= 64 * 48 * U * 2.0)


def test_eig_top_clustered(ctx):
    """{1, 0.999 .. 0.99, 0.5 .. 0.01}, k = 1: thousands of products for the iteration; only correctness is asserted."""
    _check_family(ctx, "clustered", co.spectrum_family(co.CLUSTERED, 200), 1)


def test_eig_top_same_bits_and_limits(ctx):
    import torch

    for fam, k, mi in ((_synch(34), 2, None), (_toep(34), 3, None), (_toep(34), 3, 1)):
        a, b = _eig(ctx, fam, k, mi), _eig(ctx, fam, k, mi)
        assert all(torch.equal(x, y) for x, y in zip(a, b))
    # the upper triangle is not read
    fam = _toep(18).copy()
    ref = _eig(ctx, fam, 2)
    fam[:, np.triu_indices(18, 1)[0], np.triu_indices(18, 1)[1]] = np.nan
    assert all(torch.equal(x, y) for x, y in zip(ref, _eig(ctx, fam, 2)))
    fmax = ctx.eig_top_max_f()
    assert fmax >= 520 and fmax % 16 == 0
    with pytest.raises(ValueError, match="exceed the limit"):
        ctx.eig_top_batched(torch.zeros((1, fmax + 1, fmax + 1), dtype=torch.float64, device=ctx.device), 1)
    # 520 channels and the largest shape the LDS takes (one below a multiple of 16): a matrix of rank 3, so that the
    # iteration is done after two products whatever the size
    for F in (520, fmax - 1):
        x = (np.arange(F) + 0.5) / F
        vec = np.stack([np.ones(F), np.cos(np.pi * x), np.cos(2 * np.pi * x)])
        C = np.einsum("r,ri,rj->ij", np.array([3.0, 2.0, 1.0]), vec, vec)[None] * np.array([1.0, 3.0])[:, None, None]
        info = _check_family(ctx, "rank 3", C, 2)
        assert np.all(info == 0)


# ---- weights -----------------------------------------------------------------------------------------------------------

def test_weights(ctx):
    import torch

    from cora_amd.core import skysim

    fam = _synch(18)
    V, theta, _ = _eig(ctx, fam, 3)
    # l = 0: zero, whatever C_0 / V_0 hold
    Vn = V.clone()
    Vn[0] = float("nan")
    W = ctx.constrained_weights(Vn, [0, 1, 5]).cpu().numpy()
    assert np.all(W[0] == 0) and np.all(np.isfinite(W[1:]))
    corr = fam.copy()
    corr[0] = np.nan
    Wd, info = skysim.constrained_weights_device(corr, [0, 1, 5])
    assert torch.equal(Wd, ctx.constrained_weights(Vn, [0, 1, 5])) and info.cpu().numpy().tolist() == [0] * 7
    # f_ind in any order: the reference's column order
    for f_ind in ([0, 1, 5], [5, 0, 1], [17, 3, 9]):
        Wp = ctx.constrained_weights(V, f_ind).cpu().numpy()
        for l in range(1, 7):
            r = co.rho(fam[l], V[l].cpu().numpy(), theta[l].cpu().numpy())
            tol, Wref = co.tol_W(fam[l], f_ind, r)
            assert np.abs(Wp[l] - Wref).max() <= tol
            assert np.abs(Wp[l][f_ind] - np.eye(3)).max() <= tol + 64 * U
    # duplicates: singular, as the reference's solve
    with pytest.raises(np.linalg.LinAlgError, match="l = 1"):
        ctx.constrained_weights(V, [4, 1, 4])
    with pytest.raises(ValueError, match="f_ind"):
        ctx.constrained_weights(V, [0, 1, 18])
    # a top eigenvector that vanishes exactly at the constrained channel: block diagonal, the large block away from it
    blk = np.zeros((4, 6, 6))
    blk[:, :3, :3] = np.array([[5.0, 1.0, 0.5], [1.0, 4.0, 0.25], [0.5, 0.25, 3.0]])
    blk[:, 3:, 3:] = np.array([[1.0, 0.5, 0.0], [0.5, 0.75, 0.125], [0.0, 0.125, 0.5]])
    blk[2, :3, :3], blk[2, 3:, 3:] = blk[0, 3:, 3:].copy(), blk[0, :3, :3].copy()      # l = 2: the large block holds channel 4
    Vb, _, _ = _eig(ctx, blk, 1)
    assert np.all(Vb.cpu().numpy()[[0, 1, 3], 3:, 0] == 0)
    with pytest.raises(np.linalg.LinAlgError, match="l = 1"):
        ctx.constrained_weights(Vb, [4])
    Vb2 = Vb.clone()
    Vb2[1], Vb2[3] = Vb[2], Vb[2]
    assert np.all(np.isfinite(ctx.constrained_weights(Vb2, [4]).cpu().numpy()))
    Vb2[3] = Vb[3]
    with pytest.raises(np.linalg.LinAlgError, match="l = 3"):
        ctx.constrained_weights(Vb2, [4])


# ---- alm_mix_l ----------------------------------------------------------------------------------------------------------

def _dev_layout(a, G, pad):
    """[n, nalm] complex -> device layout [nalm, G, 2, 4], padding channels = pad."""
    n, nalm = a.shape
    d = np.full((nalm, 4 * G, 2), pad, dtype=np.float64)
    d[:, :n, 0], d[:, :n, 1] = a.real.T, a.imag.T
    return np.ascontiguousarray(d.reshape(nalm, G, 4, 2).transpose(0, 1, 3, 2))


def _from_dev(d, n):
    nalm, G = d.shape[0], d.shape[1]
    x = d.transpose(0, 1, 3, 2).reshape(nalm, 4 * G, 2)
    return np.ascontiguousarray((x[:, :n, 0] + 1j * x[:, :n, 1]).T), x[:, n:, :]


@pytest.mark.parametrize("k,F", [(1, 1), (2, 5), (3, 18), (8, 34)])
@pytest.mark.parametrize("lmax", [0, 5, 32])
def test_alm_mix_l(ctx, lmax, k, F):
    import torch

    rng = np.random.default_rng(1000 * lmax + 10 * k + F)
    nalm = (lmax + 1) * (lmax + 2) // 2
    larr, marr = co.getlm(lmax)
    a = rng.standard_normal((k, nalm)) + 1j * rng.standard_normal((k, nalm))
    W = rng.standard_normal((lmax + 1, F, k)) * 10.0 ** rng.uniform(-3, 3, (lmax + 1, 1, 1))
    W[0] = 0.0
    Gin, Gout = (k + 3) // 4, (F + 3) // 4
    d = ctx.to_device(_dev_layout(a, Gin, np.nan))
    out = ctx.alm_mix_l(d, lmax, ctx.to_device(W), out=_poisoned(ctx, (nalm, Gout, 2, 4)))
    got, padding = _from_dev(out.cpu().numpy(), F)
    Wl = W[larr].astype(co.LD)                                           # [nalm, F, k]
    ref = np.einsum("ifj,ji->fi", Wl, a.real.astype(co.LD)) + 1j * np.einsum("ifj,ji->fi", Wl, a.imag.astype(co.LD))
    for part in ("real", "imag"):
        tol = (k + 1) * U * np.einsum("ifj,ji->fi", np.abs(W[larr]), np.abs(getattr(a, part))) * co.SLACK
        err = np.abs(getattr(got, part).astype(co.LD) - getattr(ref, part))
        assert np.all(err <= tol)
    assert np.all(padding == 0) and np.all(np.isfinite(got.view(np.float64)))
    assert np.all(got[:, larr == 0] == 0)
    assert torch.equal(out, ctx.alm_mix_l(d, lmax, ctx.to_device(W)))
    tolr = (k + 1) * U * np.einsum("ifj,ji->fi", np.abs(W[larr]), np.abs(a.real)) * co.SLACK
    print("alm_mix_l lmax %d k %d F %d: worst err / tol %.3g"
          % (lmax, k, F, float((np.abs(got.real - ref.real)[:, larr > 0] / np.where(tolr > 0, tolr, 1)[:, larr > 0]).max()) if lmax else 0))
    with pytest.raises(ValueError, match="overlaps"):
        big = _poisoned(ctx, (nalm * (Gin + Gout) * 8,))
        ctx.alm_mix_l(big[: nalm * Gin * 8].reshape(nalm, Gin, 2, 4), lmax, ctx.to_device(W), out=big[4: 4 + nalm * Gout * 8].reshape(nalm, Gout, 2, 4))


# ---- end to end -----------------------------------------------------------------------------------------------------------

def _device_cv(ctx, corr, f_ind, calm):
    """(cv [F, nalm] read back through alm_dev_to_square, rho_dev [L]) of the device stages on host inputs."""
    import torch

    from cora_amd.core import skysim

    L, F = corr.shape[0], corr.shape[1]
    lmax, k = L - 1, len(f_ind)
    C = ctx.to_device(corr)
    V, theta, info = ctx.eig_top_batched(C[1:].contiguous(), k)
    rho = np.zeros(L)
    for l in range(1, L):
        rho[l] = co.rho(corr[l], V[l - 1].cpu().numpy(), theta[l - 1].cpu().numpy())
        assert rho[l] <= 16 * F * U * co.norm_inf(corr[l])
    W, info2 = skysim.constrained_weights_device(C, f_ind)
    assert torch.equal(W[1:], ctx.constrained_weights(torch.cat([V[:1], V]), f_ind)[1:]) and torch.equal(info2[1:], info)
    d = ctx.alm_packed_to_dev(ctx.to_device(calm, dtype=np.complex128), lmax)
    sq = ctx.alm_dev_to_square(ctx.alm_mix_l(d, lmax, W), lmax, F).cpu().numpy()[:, 0]          # [F, l, m]
    larr, marr = co.getlm(lmax)
    return sq[:, larr, marr], rho


@pytest.mark.parametrize("case", ["a", "b"])
def test_cv_golden(ctx, gold, case):
    corr, f_ind, calm, cv_ref = golden_case(gold, case)
    cv, rho = _device_cv(ctx, corr, f_ind, calm)
    tol = co.tol_cv(corr, f_ind, calm, rho_dev=rho)
    cv_o, _ = co.mkconstrained_cv(corr, f_ind, calm)
    larr, _ = co.getlm(corr.shape[0] - 1)
    for name, want in (("the reference's cv", cv_ref), ("the oracle's cv", cv_o)):
        err = np.abs(cv - want)
        print("%s: device cv against %s, worst err / tol %.3g" % (case, name, (err[:, larr > 0] / tol[:, larr > 0]).max()))
        assert np.all(err <= tol)
    assert np.all(cv[:, larr == 0] == 0)


def _e2e_case(name, golden):
    from oracle import sht

    nside, lmax = 16, 32
    if name == "21cm":
        corr, f_ind = golden["cla_21cm_F8_l64_zromb3"][:33].copy(), [1, 5]
    else:
        from cora_amd.foreground import galaxy

        syn = galaxy.FullSkySynchrotron()
        nu = np.concatenate(([408.0, 1420.0], np.linspace(400.0, 800.0, 16)))
        B = syn.frequency_covariance(nu[:, None], nu[None, :])
        corr, f_ind = np.asarray(syn.angular_ps(np.arange(lmax + 1.0)))[:, None, None] * B[None], [0, 1]
    rng = np.random.default_rng(4)
    n = (lmax + 1) * (lmax + 2) // 2
    cons = []
    for fi in f_ind:
        a = rng.standard_normal(n) + 1j * rng.standard_normal(n)
        a[: lmax + 1] = a[: lmax + 1].real
        a[0] = 0.0                                              # no monopole: mkconstrained drops l = 0
        cons.append([fi, sht.alm2map(a, nside, lmax)])
    return np.ascontiguousarray(corr, dtype=np.float64), cons, nside, lmax


@pytest.mark.parametrize("name,F", [("21cm", 8), ("synchrotron", 18)])
def test_mkconstrained_device(ctx, golden, name, F):
    """Tensor constraints: a device tensor [F, npix]; the constrained channels reproduce their maps as in
    test_mkconstrained_vs_oracle; the whole stack against oracle.skysim.mkconstrained.

    Bound of the last comparison, per channel f (tests/_constrained_oracle.py, 'Maps'): the a_lm of the two stacks differ by
    at most tol_cv (weights and mixing, with the device's own residuals) plus sum_j |W_ref| |dc_j|, dc the MEASURED
    difference between the device's and the oracle's analysis of the constraint maps; tol_map turns that into pixels.
    The two syntheses themselves round: a Legendre value from a three-term recurrence of up to lmax steps carries about
    4 lmax u, the sum over l and the ring FFT another (lmax + 1 + log2 nphi) u, so each synthesis is within 8 (lmax + 1) u of
    tol_map(|cv|): twice that for the pair."""
    import torch

    from cora_amd.core import skysim
    from cora_amd.util import hputil
    from oracle import sht
    from oracle import skysim as osk

    corr, cons, nside, lmax = _e2e_case(name, golden)
    f_ind = [c[0] for c in cons]
    k = len(f_ind)
    assert corr.shape == (33, F, F)
    dcons = [(fi, ctx.to_device(m)) for fi, m in cons]
    got_d = skysim.mkconstrained(corr, dcons, nside)
    assert isinstance(got_d, torch.Tensor) and got_d.device == ctx.device and tuple(got_d.shape) == (F, 12 * nside * nside)
    assert torch.equal(got_d, skysim.mkconstrained(ctx.to_device(corr), dcons, nside))        # corr as a tensor; same bits
    got = got_d.cpu().numpy()
    for fi, cm in cons:
        assert np.abs(got[fi] - cm).max() < 1e-3 * np.abs(cm).max()
    ref = osk.mkconstrained(corr, cons, nside)
    # the bound
    calm_o = np.stack([sht.map2alm(np.asarray(m, dtype=np.float64), nside, lmax, use_weights=False, niter=3) for _, m in cons])
    dc = hputil.map2alm_device(torch.stack([m for _, m in dcons]), nside, lmax, use_weights=False, niter=3)
    larr, marr = co.getlm(lmax)
    calm_d = ctx.alm_dev_to_square(dc, lmax, k).cpu().numpy()[:, 0][:, larr, marr]
    cv_d, rho = _device_cv(ctx, corr, f_ind, calm_d)
    cv_o, W_ref = co.mkconstrained_cv(corr, f_ind, calm_o)
    da = co.tol_cv(corr, f_ind, calm_d, rho_dev=rho) + np.einsum("ifj,ji->fi", np.abs(W_ref[larr]), np.abs(calm_d - calm_o))
    tol = (co.tol_map(da, lmax) + 2 * 8 * (lmax + 1) * U * co.tol_map(np.abs(cv_o), lmax)) * co.SLACK
    err = np.abs(got - ref).max(axis=1)
    print("mkconstrained %s F %d: device route against the oracle, worst err / tol %.3g (err %.3g of rms %.3g)"
          % (name, F, (err / tol).max(), err.max(), ref.std()))
    assert np.all(err <= tol)
    with pytest.raises(ValueError, match="at most 8 constraints"):
        skysim.mkconstrained(np.zeros((4, 12, 12)), [(i, dcons[0][1]) for i in range(9)], nside)
    with pytest.raises(Exception, match="incorrect shape"):
        skysim.mkconstrained(np.zeros((5, 3, 4)), dcons, nside)


def test_mkconstrained_numpy_route_unchanged(ctx, golden):
    """numpy maps: an ndarray, bit for bit what the host route (per-l eigh, the square cv array) gives."""
    from cora_amd.core import skysim

    corr, cons, nside, lmax = _e2e_case("21cm", golden)
    got = skysim.mkconstrained(corr, cons, nside)
    assert isinstance(got, np.ndarray) and np.array_equal(got, skysim._mkconstrained_host(corr, cons, nside))
    import scipy.linalg as la

    from cora_amd.util import hputil

    # the host route restated from its published steps (eigh per l, solve, the square array, one synthesis)
    L, k = lmax + 1, len(cons)
    f_ind = [c[0] for c in cons]
    import torch

    calm = hputil.map2alm_device(torch.from_numpy(np.stack([c[1] for c in cons])).to(ctx.device), nside, lmax, use_weights=False, niter=3)
    cmap = ctx.alm_dev_to_square(calm, lmax, k).cpu().numpy()[:, 0]
    cv = np.zeros((corr.shape[1], L, L), dtype=np.complex128)
    for l in range(1, L):
        tr = la.eigh(corr[l])[1][:, -k:].T
        cv[:, l, : l + 1] = np.dot(tr.T, la.solve(tr[:, f_ind].T, cmap[:, l, : l + 1]))
    assert np.array_equal(got, hputil._synth(cv, nside))


# ---- getsky_device ------------------------------------------------------------------------------------------------------

def test_getsky_device_stays_on_the_device(ctx, monkeypatch):
    import torch

    import cora_amd
    from cora_amd import _lib
    from test_gpu_galaxy import FREQ, NSIDE, _sky_data
    from cora_amd.foreground import galaxy

    haslam, spectral, faraday = _sky_data()
    gal = galaxy.ConstrainedGalaxy(haslam=haslam, spectral=spectral, faraday=faraday, amp_nside=NSIDE)
    gal.nside, gal.frequencies = NSIDE, FREQ
    npix, F = 12 * NSIDE * NSIDE, FREQ.size + 2
    moved = []
    real_h, real_d = _lib.Context.to_host, _lib.Context.to_device

    def to_host(self, t):
        moved.append(("to_host", tuple(t.shape)))
        return real_h(self, t)

    def to_device(self, a, dtype=np.float64):
        moved.append(("to_device", tuple(np.shape(a))))
        return real_d(self, a, dtype=dtype)

    monkeypatch.setattr(_lib.Context, "to_host", to_host)
    monkeypatch.setattr(_lib.Context, "to_device", to_device)
    one = gal.getsky_device(celestial=False, rng=cora_amd.DeviceRNG(7))
    big = [m for m in moved if len(m[1]) >= 1 and m[1][-1] == npix and int(np.prod(m[1])) > npix]
    print("getsky_device transfers: %r" % (sorted(set(moved)),))
    assert not big, big
    assert not [m for m in moved if m[0] == "to_host" and int(np.prod(m[1])) >= npix]
    monkeypatch.undo()
    assert tuple(one.shape) == (FREQ.size, npix)
    assert torch.equal(one, gal.getsky_device(celestial=False, rng=cora_amd.DeviceRNG(7)))
    dbg = gal.getsky_device(debug=True, celestial=False, rng=cora_amd.DeviceRNG(7))
    assert torch.equal(dbg[0], one) and all(isinstance(x, torch.Tensor) for x in dbg[:5]) and isinstance(dbg[5], float)
    assert tuple(dbg[1].shape) == (F, npix) and tuple(dbg[2].shape) == (F, npix)
