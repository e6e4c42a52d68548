#!/usr/bin/env python3
"""Timing of the Zel'dovich displacement field (cora_amd.signal.lss.zeldovich_displacement_device: iterated analysis,
derivative synthesis, radial gradient; csrc/sht_der1.hip) at nside 1024, 128 slices, lmax 2048 on device tensors;
prints one JSON line.  ``phi`` is synthesised on the device from a steep (l^-3) random spectrum.

Besides the total, the library's stage timers (``Context.profile_get``) give the split into the analysis passes
(the quadrature passes and the syntheses of the refinements), the derivative synthesis (the three scalar syntheses per
field) and the three new kernels.  For those the bytes they must move are set against the 6 TB/s streaming figure
tools/bench_lss.py uses:
  der1_prep       reads 16 B, writes 48 B per coefficient and field (the a2 operand re-reads its neighbour from cache);
  der1_combine    reads 24 B, writes 16 B per pixel and field;
  radial_gradient reads 8 B (each element once; 24 B if nothing were reused), writes 8 B per element.
Usage: python tools/bench_lss_displacement.py [--nside 1024] [--nchi 128] [--lmax 2048] [--reps 3]
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
ap.add_argument("--nchi", type=int, default=128)
ap.add_argument("--lmax", type=int, default=2048)
ap.add_argument("--reps", type=int, default=3)
a = ap.parse_args()

ctx = _lib.get_context()
nside, nchi, lmax = a.nside, a.nchi, a.lmax
npix = 12 * nside * nside
nalm = (lmax + 1) * (lmax + 2) // 2

# phi: l^-3 spectrum, drawn on the device in the alm_dev layout [nalm, G, 2, 4] (the imaginary parts of m = 0 are ignored)
l_of = np.concatenate([np.arange(m, lmax + 1) for m in range(lmax + 1)]).astype(np.float64)
amp = ctx.to_device(np.maximum(l_of, 1.0) ** -1.5)
g = torch.Generator(device=ctx.device).manual_seed(11)
phi = ctx.empty((nchi, npix))
for c0 in range(0, nchi, 16):
    n = min(16, nchi - c0)
    alm = torch.randn((nalm, (n + 3) // 4, 2, 4), dtype=torch.float64, device=ctx.device, generator=g)
    alm *= amp[:, None, None, None]
    phi[c0:c0 + n] = ctx.alm2map(alm, nside, lmax, n)
    del alm
chi = 1000.0 + 5.0 * np.arange(nchi)
D = np.linspace(0.9, 0.5, nchi)
f = np.linspace(0.8, 0.95, nchi)
psi = ctx.empty((3, nchi, npix))

lss.zeldovich_displacement_device(phi, chi, D, f, lmax=lmax, out=psi)          # warm-up (plans, workspaces)
torch.cuda.synchronize()
times = []
for _ in range(a.reps):
    torch.cuda.synchronize()
    ctx.timer_begin()
    lss.zeldovich_displacement_device(phi, chi, D, f, lmax=lmax, out=psi)
    times.append(ctx.timer_end())
ms = float(np.median(times))

# one more call under the stage timers
ctx.profile_enable(True)
ctx.profile_reset()
lss.zeldovich_displacement_device(phi, chi, D, f, lmax=lmax, out=psi)
ctx.sync()
names = ["ringana", "legendre_adj", "legendre", "ringfft", "der1_prep", "der1_combine", "radial_gradient"]
prof = {}
for nm in names:
    try:
        prof[nm] = ctx.profile_get(nm)
    except _lib.CoraHipError:
        prof[nm] = (0.0, 0)
ctx.profile_enable(False)

# the synthesis stages ran for the refinements of the analysis (3 passes over nchi channels) and for the derivative
# synthesis (1 pass over 3 nchi channels): equal channel counts, split in proportion
syn = prof["legendre"][0] + prof["ringfft"][0]
ana = prof["ringana"][0] + prof["legendre_adj"][0]
bytes_prep = 64 * nalm * nchi
bytes_comb = 40 * npix * nchi
bytes_rad = 16 * npix * nchi


def frac(nbytes, t_ms):
    return round(nbytes / 6.0e12 * 1e3 / t_ms, 3) if t_ms > 0 else None


line = dict(bench="zeldovich_displacement", nside=nside, nchi=nchi, lmax=lmax, niter=3, ms=round(ms, 2),
            ms_min=round(min(times), 2), finite=bool(torch.isfinite(psi).all()),
            analysis_quadrature_ms=round(ana, 2), synthesis_ms=round(syn, 2),
            analysis_passes_ms=round(ana + syn / 2, 2), der1_synthesis_ms=round(syn / 2, 2),
            der1_prep_ms=round(prof["der1_prep"][0], 3), der1_combine_ms=round(prof["der1_combine"][0], 3),
            radial_gradient_ms=round(prof["radial_gradient"][0], 3),
            der1_prep_bytes=bytes_prep, der1_combine_bytes=bytes_comb, radial_gradient_bytes=bytes_rad,
            der1_prep_frac_6TBs=frac(bytes_prep, prof["der1_prep"][0]),
            der1_combine_frac_6TBs=frac(bytes_comb, prof["der1_combine"][0]),
            radial_gradient_frac_6TBs=frac(bytes_rad, prof["radial_gradient"][0]),
            stage_launches={k: v[1] for k, v in prof.items()},
            temp_bytes_bound=lssutil.gradient_bytes(nside, lmax))
print(json.dumps(line))
