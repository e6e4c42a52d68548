#!/usr/bin/env python3
"""Timing of the LSS chain kernels (csrc/lsschain.hip) on device tensors at nside 1024, n = 128; prints one JSON line.

Method: buffers filled with torch.randn on the device; per item one warm-up call, then ``--reps`` (>= 5) timed calls
with ctx.timer_begin / timer_end (device events around the call); the median is reported, the minimum beside it.
Where two forms are compared they are timed alternately in the same loop on the same tensors.

  (i)   slice_mix with a dense random K, and torch.matmul(K, f) on the same tensors
  (ii)  fingers_of_god with chi = linspace(1800, 2400, n), sigmaP = 1.93: exact, and with band_cut = 1e-18
  (iii) linear_dynamics (one fused launch) against the same expression from diff2_device plus torch operations
  (iv)  biased_field with b2 (moments + bias kernel), lognormal_transform axis=1 (two moment passes + transform), and
        their kernels alone (diff2, bias_field, lognormal, slice_moments) from the library's stage profile

Models the figures are set against (arithmetic, not measurements):
  streaming kernels: the bytes the kernel must move (each input element read once, each output element written
                     once) at 6.3 TB/s, the copy rate measured on an MI355X;
  slice_mix:         the MFMA flops it issues (2 x 16 x 16 x 4 per instruction; with ranges, only those inside them)
                     at 77.4 TF (profiles/mfma_f64_probe_r01.txt), and its bytes (f once, out once) at 6.3 TB/s.
Usage: python tools/bench_lss_chain.py [--nside 1024] [--n 128] [--reps 7]
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
from cora_amd.signal import lss, lssutil  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--nside", type=int, default=1024)
ap.add_argument("--n", type=int, default=128)
ap.add_argument("--reps", type=int, default=7)
a = ap.parse_args()
if a.reps < 5:
    ap.error("--reps must be at least 5")

HBM, MFMA_TF = 6.3e12, 77.4e12
ctx = _lib.get_context()
n, npix = a.n, 12 * a.nside * a.nside
N = n * npix
g = torch.Generator(device=ctx.device).manual_seed(1)


def randn(*shape):
    return torch.randn(shape, dtype=torch.float64, device=ctx.device, generator=g)


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


def mix_flops(ranges):
    """MFMA flops slice_mix issues for ranges [nb, 2] (or None: dense), per column tile of 16"""
    nb = (n + 15) // 16
    n4 = (n + 3) // 4 * 4
    steps = nb * n4 // 4 if ranges is None else int(sum(max(0, min(n4, (hi + 3) // 4 * 4) - lo // 4 * 4) // 4 for lo, hi in ranges))
    return steps * 2 * 16 * 16 * 4 * ((npix + 15) // 16)


def ms_at(bytes_, rate=HBM):
    return bytes_ / rate * 1e3


line = dict(bench="lss_chain", nside=a.nside, n=n, elements=N, reps=a.reps, hbm_model_Bps=HBM, mfma_model_flops=MFMA_TF)
f = randn(n, npix)
out = torch.empty_like(f)

# (i) dense slice_mix against torch.matmul
K = randn(n, n)
rd = ctx.to_device(ctx.slice_mix_ranges(K.cpu().numpy())[1], dtype=np.int32)
(mix, mix_min), (mm, mm_min) = timed([lambda: ctx.slice_mix(K, f, out=out, ranges=rd), lambda: torch.matmul(K, f, out=out)])
fl, by = mix_flops(None), 2 * N * 8
line.update(slice_mix_ms=round(mix, 3), slice_mix_ms_min=round(mix_min, 3), torch_matmul_ms=round(mm, 3),
            torch_matmul_ms_min=round(mm_min, 3), slice_mix_over_matmul=round(mix / mm, 3), slice_mix_flops=fl,
            slice_mix_bytes=by, slice_mix_mfma_floor_ms=round(fl / MFMA_TF * 1e3, 3), slice_mix_hbm_floor_ms=round(ms_at(by), 3),
            slice_mix_frac_mfma=round(fl / MFMA_TF * 1e3 / mix, 3), slice_mix_frac_hbm=round(ms_at(by) / mix, 3),
            slice_mix_workspace_bytes=0)

# (ii) Fingers of God, exact and with band_cut
chi = np.linspace(1800.0, 2400.0, n)
(fog, fog_min), (fogb, fogb_min) = timed([lambda: lss.fingers_of_god_device(f, chi, 1.93),
                                         lambda: lss.fingers_of_god_device(f, chi, 1.93, band_cut=1e-18)])
Kf = lssutil.exponential_FoG_kernel(chi, 1.93, 1.0)
r_exact, r_band = ctx.slice_mix_ranges(Kf)[1], ctx.slice_mix_ranges(Kf, 1e-18)[1]
line.update(fog_exact_ms=round(fog, 3), fog_exact_ms_min=round(fog_min, 3), fog_band_ms=round(fogb, 3),
            fog_band_ms_min=round(fogb_min, 3), fog_band_speedup=round(fog / fogb, 3),
            fog_exact_flops=mix_flops(r_exact), fog_band_flops=mix_flops(r_band),
            fog_band_mfma_floor_ms=round(mix_flops(r_band) / MFMA_TF * 1e3, 3), fog_hbm_floor_ms=round(ms_at(by), 3))

# (iii) linear dynamics, fused against diff2_device + torch operations
phi, delta = f, randn(n, npix)
bias = randn(n, npix)
D, fr = np.linspace(0.8, 0.6, n), np.linspace(0.8, 0.95, n)
Dd, td = ctx.to_device(D)[:, None], ctx.to_device(-(D * fr))[:, None]


def unfused():
    v = lssutil.diff2_device(phi, chi, out=out)
    v *= td
    res = bias + Dd * delta
    res += v
    return res


(lin, lin_min), (unf, unf_min) = timed([lambda: lss.linear_dynamics_device(phi, delta, bias, chi, D, fr, out=out), unfused])
line.update(linear_dynamics_ms=round(lin, 3), linear_dynamics_ms_min=round(lin_min, 3), linear_unfused_ms=round(unf, 3),
            linear_unfused_ms_min=round(unf_min, 3), linear_fused_speedup=round(unf / lin, 3),
            linear_dynamics_bytes=4 * N * 8, linear_dynamics_floor_ms=round(ms_at(4 * N * 8), 3),
            linear_dynamics_frac_hbm=round(ms_at(4 * N * 8) / lin, 3))
del bias

# (iv) bias with b2, lognormal transform: whole calls, then the kernels alone from the stage profile
b1, b2 = np.full(n, 1.3), np.full(n, -0.2)
delta *= 0.5
(bf, bf_min), (ln, ln_min) = timed([lambda: lss.biased_field_device(delta, D, b1, b2, out=out),
                                   lambda: lssutil.lognormal_transform_device(delta, out=out, axis=1)])
line.update(biased_field_b2_ms=round(bf, 3), biased_field_b2_bytes=3 * N * 8, biased_field_b2_floor_ms=round(ms_at(3 * N * 8), 3),
            lognormal_transform_ms=round(ln, 3), lognormal_transform_bytes=4 * N * 8,
            lognormal_transform_floor_ms=round(ms_at(4 * N * 8), 3))

ctx.profile_enable(True)
stages = {"slice_diff2": (lambda: lssutil.diff2_device(phi, chi, out=out), 2 * N * 8),
          "bias_field": (lambda: ctx.bias_field(delta, D * b1, D**2 * b2, np.full(n, 0.25), out=out), 2 * N * 8),
          "lognormal": (lambda: ctx.lognormal(delta, np.full(n, 0.125), out=out), 2 * N * 8),
          "slice_moments": (lambda: ctx.slice_moments(delta), N * 8)}
for name, (fn, nbytes) in stages.items():
    fn()
    ctx.sync()
    ctx.profile_reset()
    ts = []
    for _ in range(a.reps):
        fn()
        ctx.sync()
        ts.append(ctx.profile_get(name)[0])
        ctx.profile_reset()
    ms = float(np.median(ts))
    line.update({name + "_ms": round(ms, 3), name + "_bytes": nbytes, name + "_floor_ms": round(ms_at(nbytes), 3),
                 name + "_Bps": round(nbytes / (ms * 1e-3), -9), name + "_frac_hbm": round(ms_at(nbytes) / ms, 3)})
ctx.profile_enable(False)
print(json.dumps(line))
