#!/usr/bin/env python3
"""Timing of the polarised-galaxy path (csrc/faraday.hip, cora_amd.foreground.galaxy) on one GPU at the reference's
native size, nside 512 x nphi 1000 x 256 channels; prints one JSON line.

  (i)  faraday_mix alone (weighting, depth -> frequency product, saturation, product with the intensity: one kernel)
       against the same steps as torch operations on the same tensors: the weights from torch.exp, torch.matmul on
       complex128, tanh / abs, the four planes.  The two are timed alternately in one loop.  If the torch form does not
       fit in device memory at the size asked for, the comparison is repeated at ``--small-nside`` and the full size is
       timed for the kernel alone.
  (ii) the whole drawn polarised_galaxy_device call (draw and synthesis of 2 nphi maps in chunks, pack, inverse FFT,
       variance, mix, rotation), with a DeviceRNG.

Method: buffers filled with torch.randn on the device; one warm-up call per item, then ``--reps`` (>= 5) timed calls
with device events around the call (ctx.timer_begin / timer_end); the median is reported, the minimum beside it.

Models the figures are set against (arithmetic, not measurements): the flops of the product, 8 npix nphi nfreq, at
77.4 TF (the FP64 MFMA rate of profiles/mfma_f64_probe_r01.txt), and the bytes of y read once, 16 npix nphi, at
6.3 TB/s (the copy rate measured on an MI355X).
Usage: python tools/bench_faraday.py [--nside 512] [--maxphi 500] [--nfreq 256] [--reps 5] [--pipeline-reps 3]
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
from cora_amd.foreground import galaxy  # noqa: E402
from cora_amd.util.nputil import DeviceRNG  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--nside", type=int, default=512)
ap.add_argument("--small-nside", type=int, default=128)
ap.add_argument("--maxphi", type=float, default=500.0)
ap.add_argument("--nfreq", type=int, default=256)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--pipeline-reps", type=int, default=3, help="0 skips the whole drawn call")
a = ap.parse_args()
if a.reps < 5:
    ap.error("--reps must be at least 5")

HBM, MFMA_TF = 6.3e12, 77.4e12
ctx = _lib.get_context()
phifreq, pcfreq = galaxy.faraday_depth_grid(1.0, a.maxphi)
nphi, nfreq = len(phifreq), a.nfreq
freq = 400.0 + 400.0 / nfreq * np.arange(nfreq)
A = np.ascontiguousarray((galaxy.faraday_transfer(phifreq[:, None], freq[None, :], freq[1] - freq[0])).T)
Ad = torch.from_numpy(A).to(ctx.device)
phid = ctx.to_device(phifreq)
gen = torch.Generator(device=ctx.device).manual_seed(1)


def timed(fns, reps):
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


def mix_case(nside, with_torch):
    npix = 12 * nside * nside
    y = torch.view_as_complex(torch.randn((npix, nphi, 2), dtype=torch.float64, device=ctx.device, generator=gen))
    sigma = torch.exp(torch.rand(npix, dtype=torch.float64, device=ctx.device, generator=gen) * 5.0 - 1.0)   # 0.37 .. 55
    T = torch.rand((nfreq, npix), dtype=torch.float64, device=ctx.device, generator=gen) * 20.0 + 5.0
    out = torch.empty((nfreq, 4, npix), dtype=torch.float64, device=ctx.device)
    scale = 0.35

    def fused():
        ctx.faraday_mix(y, phid, sigma, Ad, scale, intensity=T, out=out)

    def composed():
        w = torch.exp(-0.25 * (phid[None, :] / sigma[:, None]) ** 2)
        w /= w.sum(dim=1, keepdim=True)
        z = torch.matmul(y * w, Ad.T) * scale
        m = z.abs()
        P = (z * (torch.tanh(m) / m)).T
        res = torch.empty((nfreq, 4, npix), dtype=torch.float64, device=ctx.device)
        res[:, 0] = T
        res[:, 1] = P.real * T
        res[:, 2] = P.imag * T
        res[:, 3] = 0.0
        return res

    flops, ybytes = 8.0 * npix * nphi * nfreq, 16.0 * npix * nphi
    r = dict(nside=nside, npix=npix, flops=flops, y_bytes=ybytes)
    fns = [fused]
    if with_torch:
        try:
            ref = composed()
            fused()
            r["max_abs_difference"] = float((ref[:, 1:3] - out[:, 1:3]).abs().max())
            del ref
            fns.append(composed)
        except torch.cuda.OutOfMemoryError:
            torch.cuda.empty_cache()
            r["torch_form"] = "did not fit in device memory"
    res = timed(fns, a.reps)
    ms, ms_min = res[0]
    r.update(faraday_mix_ms=round(ms, 3), faraday_mix_ms_min=round(ms_min, 3),
             faraday_mix_tflops=round(flops / (ms * 1e-3) / 1e12, 2), frac_mfma_peak=round(flops / MFMA_TF * 1e3 / ms, 3),
             y_read_Bps=round(ybytes / (ms * 1e-3), -9), frac_hbm_y_read=round(ybytes / HBM * 1e3 / ms, 3))
    if len(res) > 1:
        r.update(torch_ms=round(res[1][0], 3), torch_ms_min=round(res[1][1], 3), fused_speedup=round(res[1][0] / ms, 3))
    return r


line = dict(bench="faraday", nphi=nphi, nfreq=nfreq, reps=a.reps, hbm_model_Bps=HBM, mfma_model_flops=MFMA_TF)
full = mix_case(a.nside, True)
line["mix"] = full
torch.cuda.empty_cache()
if "torch_ms" not in full and a.small_nside < a.nside:
    line["mix_small"] = mix_case(a.small_nside, True)
    torch.cuda.empty_cache()

if a.pipeline_reps > 0:
    npix = 12 * a.nside * a.nside
    sigma = np.exp(np.random.default_rng(2).uniform(-1.0, 4.0, npix))
    T = torch.rand((nfreq, npix), dtype=torch.float64, device=ctx.device, generator=gen) * 20.0 + 5.0
    rng = DeviceRNG(11)
    (ms, ms_min), = timed([lambda: galaxy.polarised_galaxy_device(T, sigma, freq, a.nside, rng=rng, maxphi=a.maxphi)],
                          a.pipeline_reps)
    line["polarised_galaxy_device"] = dict(nside=a.nside, ms=round(ms, 1), ms_min=round(ms_min, 1), reps=a.pipeline_reps)
print(json.dumps(line))
