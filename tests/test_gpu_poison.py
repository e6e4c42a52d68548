"""Transforms on POISONED workspaces.  The kernels do not zero-fill their buffers: K4 writes the `inter` cells and K5
reads only m < mcut(ring) of them, the Bluestein buffers are never cleared, K4^T's tile reduction skips what a ring
tile cannot reach (plan tables d_lmin / d_zeros) and the padding channels of the compile-time K5^T kernels are zeroed
at the store.  A call is correct only if every cell one kernel reads was written earlier in the same call.
Context.workspace() is ONE cached buffer every transform reuses, so a break of that contract would read whatever the
previous call left there and pass or fail with the test order.  Here every entry point that takes a workspace runs
on a zeroed workspace (and output buffer), then on the same buffers filled with each of two poisons:

  bytes 0xFF: every f64 is NaN, every int32 is -1;
  bytes 0x7E: every f64 is ~2^1000, finite (a stale read a fmax / compare-select would pass a NaN through).

Criteria (stated per test):
  "exact"  - the poisoned result is finite and bit-identical to the zeroed-workspace one (analysis: K5^T, K4^T and
             the reduction have a fixed summation order);
  "atomic" - finite and max|diff| <= 1e-14 rms: the synthesis calls, whose run-time ring kernel folds aliases with
             LDS atomicAdd (csrc/sht_ringfft.hip), so the sum order of an aliased bin may vary between calls (measured:
             1.2e-15 rms at nside 1024 / lmax 3071, the last bit of the largest pixels; a stale read of either poison
             is NaN or ~2^1000).
Run with -m gpu."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

POISONS = (0xFF, 0x7E)


def _fill(t, byte):
    import torch

    t.view(torch.uint8).fill_(byte)


def _poisoned_runs(ctx, call, ws, outs=(), exact=True, valid=None, label=""):
    """call() -> device tensor, run with ``ws`` and every tensor of ``outs`` zeroed, then filled with each poison;
    ``valid`` selects the compared part of the result (default: all of it).  ``ws`` must be the buffer the call
    uses: the Context's cached workspace is checked to be the same tensor after every call."""
    import torch

    sel = valid or (lambda t: t)
    cached = ctx._workspace

    def run(byte):
        _fill(ws, byte)
        for o in outs:
            _fill(o, byte)
        r = sel(call())
        torch.cuda.synchronize()
        assert ctx._workspace is cached, "the call reallocated the cached workspace: the poison was not seen"
        return r

    ref = run(0).clone()
    assert bool(torch.isfinite(ref).all()), label
    rms = ref.double().pow(2).mean().sqrt().item()
    for byte in POISONS:
        got = run(byte)
        assert bool(torch.isfinite(got).all()), (label, hex(byte), "non-finite output")
        if exact:
            assert torch.equal(got, ref), (label, hex(byte), (got - ref).abs().max().item() / rms)
        else:
            d = (got - ref).abs().max().item()
            assert d <= 1e-14 * rms, (label, hex(byte), d / rms)
    return ref


def _channels(alm_dev, nnu):
    """alm_dev [nalm, G, 2, 4] -> [nnu, nalm, 2]: the valid channels (padding lanes are not part of the result)."""
    nalm = alm_dev.shape[0]
    return alm_dev.permute(1, 3, 0, 2).reshape(-1, nalm, 2)[:nnu]


def _red_alm(ctx, lmax, G, seed):
    import torch

    L = lmax + 1
    nalm = L * (L + 1) // 2
    gen = torch.Generator(device=ctx.device).manual_seed(seed)
    l_of = torch.cat([torch.arange(m, L, device=ctx.device) for m in range(L)])
    a = torch.randn((nalm, G, 2, 4), generator=gen, device=ctx.device, dtype=torch.float64)
    a *= (1.0 / (1.0 + l_of.double()))[:, None, None, None]
    a[:L, :, 1, :] = 0.0
    return a


# (nside, lmax, nnu, max_workspace_bytes as a channel count or None): the K4 shapes <1, 2> with padding (5), <1, 2> (8),
# <4, 2> (32), <8, 1> (64); the chunked workspace (13 channels in chunks of 8, the last one ragged); the aliased
# lmax = 3 nside - 1; the nside-512 classes; nside 2048 with 3 channels (the padded alm slice); two small shapes on the
# run-time ring kernels
SHAPES = [(1024, 2048, 5, None), (1024, 2048, 8, None), (1024, 2048, 32, None), (1024, 2048, 64, None),
          (1024, 2048, 13, 8), (1024, 3071, 8, None), (512, 1024, 12, None), (2048, 2048, 3, None),
          (32, 64, 5, None), (64, 100, 8, None)]


@pytest.mark.parametrize("nside,lmax,nnu,chunk", SHAPES)
def test_alm2map_on_poisoned_workspace(ctx, nside, lmax, nnu, chunk):
    """alm2map (K4 + K5): criterion "atomic" (the run-time ring kernel folds aliases with LDS atomics); the output maps
    are poisoned too, every pixel must be written."""
    import torch

    plan = ctx.sht_plan(nside, lmax)
    G = (nnu + 3) // 4
    alm = _red_alm(ctx, lmax, G, 100 + nnu)
    nalm = (lmax + 1) * (lmax + 2) // 2
    # room for `chunk` channels of `inter` plus their alm slice: corahip_alm2map then goes through chunks of that size
    maxb = ctx.alm2map_workspace_bytes(plan, chunk) + nalm * 16 * 8 * (chunk // 8) if chunk else None
    ws = ctx.workspace(maxb or ctx.alm2map_workspace_bytes(plan, nnu))
    maps = ctx.empty((nnu, 12 * nside * nside))
    _poisoned_runs(ctx, lambda: ctx.alm2map(alm, nside, lmax, nnu, out=maps, max_workspace_bytes=maxb), ws, (maps,),
                   exact=False, label=(nside, lmax, nnu, chunk))
    del alm, maps, ws
    torch.cuda.empty_cache()


@pytest.mark.parametrize("nside,lmax,nnu,chunk", SHAPES)
def test_map2alm_on_poisoned_workspace(ctx, nside, lmax, nnu, chunk):
    """map2alm (K5^T + K4^T + the row reduction): criterion "exact" on the valid channels; the output alm_dev is
    poisoned too (its padding lanes are not compared)."""
    import torch

    plan = ctx.sht_plan(nside, lmax)
    npix = 12 * nside * nside
    nalm = (lmax + 1) * (lmax + 2) // 2
    gen = torch.Generator(device=ctx.device).manual_seed(200 + nnu)
    x = torch.randn((nnu, npix), generator=gen, device=ctx.device, dtype=torch.float64)
    w = ctx.to_device(1.0 + 0.01 * np.cos(np.arange(2 * nside)))
    ws = ctx.workspace(ctx.map2alm_workspace_bytes(plan, chunk or nnu))
    out = ctx.empty((nalm, (nnu + 3) // 4, 2, 4))
    _poisoned_runs(ctx, lambda: ctx.map2alm(x, nside, lmax, w, chunk=chunk, out=out), ws, (out,), exact=True,
                   valid=lambda t: _channels(t, nnu), label=(nside, lmax, nnu, chunk))
    del x, out, ws
    torch.cuda.empty_cache()


@pytest.mark.parametrize("nside,lmax", [(1024, 2048), (32, 64)])
def test_spin2_transforms_on_poisoned_workspace(ctx, nside, lmax):
    """Two (Q, U) pairs: map2alm_spin2 (six scalar passes over ring-scaled maps + the combination; criterion "exact")
    and alm2map_spin2 of the result (criterion "atomic"), workspace and outputs poisoned."""
    import torch

    plan = ctx.sht_plan(nside, lmax)
    nf = 2
    npix = 12 * nside * nside
    nalm = (lmax + 1) * (lmax + 2) // 2
    gen = torch.Generator(device=ctx.device).manual_seed(300 + nside)
    qu = torch.randn((2 * nf, npix), generator=gen, device=ctx.device, dtype=torch.float64)
    gout = (2 * nf + 7) // 8 * 2
    nnu = 4 * gout
    ws = ctx.workspace(max(ctx.map2alm_workspace_bytes(plan, 6 * nf), ctx.alm2map_workspace_bytes(plan, nnu)))
    out = ctx.empty((nalm, gout, 2, 4))
    alm = _poisoned_runs(ctx, lambda: ctx.map2alm_spin2(qu, nside, lmax, None, out=out), ws, (out,), exact=True,
                         valid=lambda t: _channels(t, 2 * nf), label=("map2alm_spin2", nside, lmax))
    # the synthesis of those coefficients (padding channels zero), every (Q, U) channel of the launch compared
    src = torch.zeros((nalm, gout, 2, 4), dtype=torch.float64, device=ctx.device)
    for f in range(2 * nf):
        src[:, f // 4, :, f % 4] = alm[f]
    maps = ctx.empty((nnu, npix))
    _poisoned_runs(ctx, lambda: ctx.alm2map_spin2(src, nside, lmax, nnu, out=maps), ws, (maps,), exact=False,
                   label=("alm2map_spin2", nside, lmax))
    del qu, out, alm, src, maps, ws
    torch.cuda.empty_cache()


def _mk_cl(F, L, seed):
    """C_l blocks [L, F, F]: random positive definite ones, a zero l = 0 block and an indefinite l = 3 block (both
    take the eigen route of the factorisation, where the Jacobi kernel writes a dense T)."""
    rng = np.random.default_rng(seed)
    C = np.empty((L, F, F))
    for l in range(L):
        A = rng.standard_normal((F, F + 3))
        C[l] = A @ A.T / (F * (1.0 + l) ** 2)
    C[0] = 0.0
    C[3][0, 0] = -2.0 * np.abs(C[3]).max()
    return C


@pytest.mark.parametrize("kind", ["philox", "pcg64"])
@pytest.mark.parametrize("F", [8, 96])
def test_mkfullsky_fused_on_poisoned_workspace(ctx, kind, F):
    """corahip_mkfullsky with the caller's workspace poisoned: it holds T, info, the a_lm and the synthesis workspace
    (factor -> draw -> K4 -> K5 in one call).  Criterion "atomic" (synthesis); for PCG64 the generator state after the
    call must not depend on the poison either."""
    import torch

    nside, lmax = 32, 64
    L = lmax + 1
    Cd = ctx.to_device(_mk_cl(F, L, F))
    plan = ctx.sht_plan(nside, lmax)
    code = {"philox": 1, "pcg64": 2}[kind]
    b = ctypes.c_size_t()
    assert ctx.lib.corahip_mkfullsky_workspace_bytes(plan, F, 0, F, code, 0, ctypes.byref(b)) == 0
    ws = torch.empty((int(b.value),), dtype=torch.uint8, device=ctx.device)
    if kind == "philox":
        rng = ("philox", 4321)
    else:
        st = np.random.default_rng(F).bit_generator.state["state"]
        rng = ("pcg64", st["state"], st["inc"])
    states = []

    def call():
        maps, after = ctx.mkfullsky_fused(Cd, nside, rng, workspace=ws)
        states.append(after)
        return maps

    # (mkfullsky_fused takes no output buffer: the maps are a fresh allocation, the workspace is what is poisoned)
    ref = _poisoned_runs(ctx, call, ws, exact=False, label=(kind, F))
    assert len(set(states)) == 1, states
    assert ref.shape == (F, 12 * nside * nside) and float(ref.abs().max()) > 0.0
    del Cd, ws, ref
    torch.cuda.empty_cache()
