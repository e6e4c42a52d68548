#!/usr/bin/env python3
"""Timing of the polarised spectra (hputil.map2alm_sky_device, Context.alm_gather_channels, the Gram call on the
field-major buffer) and of lssutil.laplacian_device; prints one JSON line.

Shapes: nside 512 x 256 channels x 3 planes (T, Q, U), the shape of tools/bench_faraday.py, lmax = 3 nside - 1, for the
analysis, the gather and the Gram call (768 channels); nside 1024 x 128 slices for the Laplacian.  Inputs are torch.randn
on the device.

Method: device events around each call (ctx.timer_begin / timer_end), one warm-up call of every form, then ``--reps``
(>= 5) timed calls; where two forms of the same work exist they alternate in the same loop on the same tensors.  Medians
are reported, minima beside them.

  analysis   map2alm_sky_device for each chunk size of ``--chunks``; peak memory beyond input and output
             (torch.cuda.max_memory_allocated) beside hputil.map2alm_sky_bytes.
  gather     what one full pass of the analysis asks of the gather: T of 256 channels into channels 0 .. 255, E and B out
             of the 512 interleaved (E_f, B_f) channels into 256 .. 511 and 512 .. 767 (three kernel calls).  Bytes moved
             = 16 bytes read and 16 written per channel and (l, m); set against the chip's measured copy rate
             (6.29 TB/s, a float4 copy) and a ``copy_`` of the same number of bytes timed here.  The same placement from
             torch operations, two ways: strided ``copy_`` from views of the source (possible because these index sets are
             regular and 256 is a multiple of 4; no workspace) and the general route for any index set
             (``index_select`` on a channel-major view; full-size temporaries).  Results are compared bit for bit.
             ``Context.alm_gather_channels`` validates a device ``idx`` on the host, one device-to-host copy and
             synchronisation per call; the three calls' copies lie inside the timed interval, so the kernel's own rate is
             slightly above the figure reported here.
  gram       Context.alm_cross_spectra on the 768-channel buffer, symmetric; the MFMA count as tools/bench_spectra.py.
  laplacian  lssutil.laplacian_device, default chunk; peak memory beside lssutil.laplacian_bytes.
Usage: python tools/bench_polspectra.py [--reps 5] [--chunks 16] [--skip-laplacian]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
import torch  # noqa: E402

from cora_amd import _lib  # noqa: E402
from cora_amd.signal import lssutil  # noqa: E402
from cora_amd.util import hputil  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--nside", type=int, default=512)
ap.add_argument("--channels", type=int, default=256)
ap.add_argument("--chunks", type=str, default=str(hputil.SKY_CHUNK), help="comma-separated chunk sizes of the analysis")
ap.add_argument("--lap-nside", type=int, default=1024)
ap.add_argument("--lap-slices", type=int, default=128)
ap.add_argument("--skip-analysis", action="store_true")
ap.add_argument("--skip-laplacian", action="store_true")
a = ap.parse_args()
if a.reps < 5:
    ap.error("--reps must be at least 5")
if a.channels % 4:
    ap.error("--channels must be a multiple of 4 (the strided torch form needs whole groups)")

COPY_BPS, MFMA_TF = 6.29e12, 77.4e12
T, KM = 128, 8                     # tile edge and m rows per chunk of cross_spectra_kernel
ctx = _lib.get_context()
g = torch.Generator(device=ctx.device).manual_seed(1)
F, nside = a.channels, a.nside
lmax = 3 * nside - 1
npix = 12 * nside * nside
nalm = (lmax + 1) * (lmax + 2) // 2


def timed(fns, reps=a.reps):
    """median and min ms of each callable; the callables are run alternately"""
    for fn in fns:
        fn()
    torch.cuda.synchronize()
    t = [[] for _ in fns]
    for _ in range(reps):
        for k, fn in enumerate(fns):
            ctx.timer_begin()
            fn()
            t[k].append(ctx.timer_end())
    return [(float(np.median(x)), float(min(x))) for x in t]


def peak_of(fn):
    """peak device memory of one call beyond what is allocated before it, and its result"""
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated(ctx.device)
    torch.cuda.reset_peak_memory_stats(ctx.device)
    res = fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated(ctx.device) - base, res


def mfma_count(nx, lmax):
    """MFMA instructions of the symmetric cross_spectra_kernel (tools/bench_spectra.py)"""
    blocks = 0
    for ti in range((nx + T - 1) // T):
        for tj in range(ti + 1):
            for wr in (0, 64):
                for wc in (0, 64):
                    if ti == tj and wr < wc:
                        continue
                    nu = sum(1 for u in range(4) if ti * T + wr + 16 * u < nx)
                    nv = sum(1 for v in range(4) if tj * T + wc + 16 * v < nx)
                    blocks += nu * nv
    l = np.arange(lmax + 1)
    return blocks * int((4 * ((l + KM - 1) // KM) + 1).sum())


line = dict(bench="polspectra", reps=a.reps, nside=nside, channels=F, planes=3, lmax=lmax, copy_rate_Bps=COPY_BPS)

# ---- analysis ----------------------------------------------------------------------------------------------------
if not a.skip_analysis:
    maps = torch.randn((F, 3, npix), dtype=torch.float64, device=ctx.device, generator=g)
    for chunk in [int(c) for c in a.chunks.split(",")]:
        peak, alm = peak_of(lambda: hputil.map2alm_sky_device(maps, chunk=chunk))
        peak -= alm.numel() * 8
        del alm
        (ms, ms_min), = timed([lambda: hputil.map2alm_sky_device(maps, chunk=chunk)])
        tag = "analysis_chunk%d" % chunk
        line.update({tag + "_ms": round(ms, 2), tag + "_ms_min": round(ms_min, 2), tag + "_peak_GB": round(peak / 1e9, 3),
                     tag + "_bound_GB": round(hputil.map2alm_sky_bytes(nside, lmax, 3, chunk) / 1e9, 3)})
        torch.cuda.empty_cache()
    line.update(input_GB=round(maps.numel() * 8 / 1e9, 3), output_GB=round(nalm * (3 * F // 4) * 64 / 1e9, 3))
    del maps
    torch.cuda.empty_cache()

# ---- gather ------------------------------------------------------------------------------------------------------
src_t = torch.randn((nalm, F // 4, 2, 4), dtype=torch.float64, device=ctx.device, generator=g)
src_eb = torch.randn((nalm, 2 * F // 4, 2, 4), dtype=torch.float64, device=ctx.device, generator=g)
dst_k = torch.zeros((nalm, 3 * F // 4, 2, 4), dtype=torch.float64, device=ctx.device)
dst_v, dst_i = torch.zeros_like(dst_k), torch.zeros_like(dst_k)
ar = torch.arange(F, dtype=torch.int32, device=ctx.device)
idx_t, idx_e, idx_b = ar.contiguous(), (2 * ar).contiguous(), (2 * ar + 1).contiguous()
G4 = F // 4


def gather_kernel():
    ctx.alm_gather_channels(src_t, F, idx_t, dst_k, 3 * F, 0)
    ctx.alm_gather_channels(src_eb, 2 * F, idx_e, dst_k, 3 * F, F)
    ctx.alm_gather_channels(src_eb, 2 * F, idx_b, dst_k, 3 * F, 2 * F)


def gather_views():
    """strided copies: channel 2 f + eb of the source = [g', gg, comp, k, eb] with f = 4 g' + 2 gg + k"""
    dst_v[:, :G4].copy_(src_t)
    v = src_eb.view(nalm, G4, 2, 2, 2, 2)                       # [nalm, g', gg, comp, k, eb]
    for eb in (0, 1):
        dst_v[:, (1 + eb) * G4:(2 + eb) * G4].view(nalm, G4, 2, 2, 2).copy_(v[..., eb].permute(0, 1, 3, 2, 4))


def gather_index():
    """the general route: channel-major views, index_select, back"""
    def channels(x):                                            # [nalm, G, 2, 4] -> [nalm, 2, 4 G]
        return x.permute(0, 2, 1, 3).reshape(nalm, 2, -1)

    parts = [channels(src_t).index_select(2, idx_t), channels(src_eb).index_select(2, idx_e), channels(src_eb).index_select(2, idx_b)]
    dst_i.copy_(torch.cat(parts, dim=2).view(nalm, 2, 3 * G4, 4).permute(0, 2, 1, 3))


pk, _ = peak_of(gather_kernel)
pv, _ = peak_of(gather_views)
pi, _ = peak_of(gather_index)
same = bool(torch.equal(dst_k, dst_v) and torch.equal(dst_k, dst_i))
moved = 2 * 3 * F * nalm * 16                                    # bytes read + bytes written
same_size = torch.empty_like(dst_k)
(k, k_min), (v, v_min), (i, i_min), (c, c_min) = timed([gather_kernel, gather_views, gather_index, lambda: same_size.copy_(dst_k)])
line.update(gather_bytes=moved, gather_ms=round(k, 3), gather_ms_min=round(k_min, 3), gather_TBps=round(moved / k / 1e9, 3),
            gather_frac_copy_rate=round(moved / (k * 1e-3) / COPY_BPS, 3), copy_same_bytes_ms=round(c, 3),
            copy_same_bytes_TBps=round(moved / c / 1e9, 3), gather_torch_views_ms=round(v, 3), gather_torch_views_ms_min=round(v_min, 3),
            gather_torch_index_ms=round(i, 3), gather_torch_index_ms_min=round(i_min, 3), gather_workspace_bytes=pk,
            gather_torch_views_workspace_bytes=pv, gather_torch_index_workspace_GB=round(pi / 1e9, 3), gather_results_equal=same)
del src_t, src_eb, dst_v, dst_i, same_size
torch.cuda.empty_cache()

# ---- the Gram call at 3 F channels -----------------------------------------------------------------------------------
n = 3 * F
out = ctx.empty((lmax + 1, n, n))
(s, s_min), = timed([lambda: ctx.alm_cross_spectra(dst_k, n, lmax, out=out)])
fl = mfma_count(n, lmax) * 2048
line.update(gram_channels=n, gram_ms=round(s, 3), gram_ms_min=round(s_min, 3), gram_flops=fl, gram_TF=round(fl / s / 1e9, 2),
            gram_frac_mfma=round(fl / MFMA_TF * 1e3 / s, 3), gram_symmetric=bool(torch.equal(out, out.transpose(1, 2))))
del out, dst_k
torch.cuda.empty_cache()

# ---- laplacian -----------------------------------------------------------------------------------------------------
if not a.skip_laplacian:
    ns, nl = a.lap_nside, a.lap_slices
    lm = 3 * ns - 1
    maps = torch.randn((nl, 12 * ns * ns), dtype=torch.float64, device=ctx.device, generator=g)
    x = 1000.0 + 5.0 * np.arange(nl)
    res = ctx.empty((nl, 12 * ns * ns))
    peak, _ = peak_of(lambda: lssutil.laplacian_device(maps, x, out=res))
    (ms, ms_min), = timed([lambda: lssutil.laplacian_device(maps, x, out=res)])
    line.update(laplacian_nside=ns, laplacian_slices=nl, laplacian_lmax=lm, laplacian_ms=round(ms, 2), laplacian_ms_min=round(ms_min, 2),
                laplacian_peak_GB=round(peak / 1e9, 3), laplacian_bound_GB=round(lssutil.laplacian_bytes(ns, lm) / 1e9, 3),
                laplacian_finite=bool(torch.isfinite(res).all()))
print(json.dumps(line))
