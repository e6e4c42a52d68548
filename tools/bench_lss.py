#!/usr/bin/env python3
"""Timing of the Zel'dovich SPH assignment (cora_amd.signal.lss.za_density_sph_device, csrc/pmesh.hip) at nside 1024,
nchi 128 (1.61e9 particles) on device tensors; prints one JSON line.

Models (not measurements) the figure is set against, per call with N = nchi npix particles:
  streaming floor: reads of psi (3 fields), delta_b, delta_m (40 N bytes) + read and write of out (16 N bytes) at
                   6 TB/s;
  atomic-only:     27 f64 adds per particle (216 N bytes) at the 1.3 TB/s measured for f32 global atomics.
The kernel adds into an LDS tile first; ``flush_atomic_bytes_max`` bounds its global adds from the tile (one per tile
cell; only non-zero cells are added), deposits that leave the tile add on top of that.
The host oracle (tests/_za_oracle.py, numpy) is timed per slice at nside 256 and scaled by the pixel count.
Usage: python tools/bench_lss.py [--nside 1024] [--nchi 128] [--reps 5]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import torch  # noqa: E402

from cora_amd import _lib  # noqa: E402
from cora_amd.signal import lss  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--nside", type=int, default=1024)
ap.add_argument("--nchi", type=int, default=128)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--no-oracle", action="store_true")
a = ap.parse_args()

ctx = _lib.get_context()
nside, nchi = a.nside, a.nchi
npix = 12 * nside * nside
N = nchi * npix
res = np.sqrt(4 * np.pi / npix)
g = torch.Generator(device=ctx.device).manual_seed(1)
psi = torch.randn((3, nchi, npix), dtype=torch.float64, device=ctx.device, generator=g)
psi[0] *= 2.0
psi[1] *= res
psi[2] *= 2 * res
db = 0.4 * torch.randn((nchi, npix), dtype=torch.float64, device=ctx.device, generator=g)
dm = 0.8 * torch.randn((nchi, npix), dtype=torch.float64, device=ctx.device, generator=g)
chi = ctx.to_device(1000.0 + 5.0 * np.arange(nchi))
out = torch.zeros((nchi, npix), dtype=torch.float64, device=ctx.device)

lss.za_density_sph_device(psi, db, dm, chi, out)              # warm-up
torch.cuda.synchronize()
times = []
for _ in range(a.reps):
    out.zero_()
    torch.cuda.synchronize()
    ctx.timer_begin()
    lss.za_density_sph_device(psi, db, dm, chi, out)
    times.append(ctx.timer_end())
mass = float((out + 1).sum()) / float((1 + db).sum()) - 1.0
ms = float(np.median(times))

nbf = (nside + 15) // 16
bytes_moved = 56 * N
floor_ms = bytes_moved / 6.0e12 * 1e3
line = dict(bench="za_density_sph", nside=nside, nchi=nchi, particles=N, ms=round(ms, 3),
            ms_min=round(min(times), 3), bytes_moved=bytes_moved, floor_ms_model=round(floor_ms, 2),
            frac_of_floor=round(floor_ms / ms, 3), atomic_only_ms_model=round(216 * N / 1.3e12 * 1e3, 1),
            flush_atomic_bytes_max=nbf * nbf * 12 * ((nchi + 7) // 8) * 14 * 24 * 24 * 8,
            mass_rel_err=mass)
if not a.no_oracle:
    import _za_oracle as zo
    from cora_amd.util import hputil

    ns = 256
    npx = 12 * ns * ns
    rng = np.random.default_rng(0)
    r = np.sqrt(4 * np.pi / npx)
    ch = 1000.0 + 5.0 * np.arange(4)
    ang = np.array(hputil.pix2ang(ns, np.arange(npx)))
    p = np.stack([rng.normal(0, 2, npx), rng.normal(0, r, npx), rng.normal(0, 2 * r, npx)])
    t0 = time.perf_counter()
    t = zo.slice_terms(p, rng.normal(0, 0.4, npx), rng.normal(0, 0.8, npx), ch[1], ch, ns, r / 2, 2.5, ang)
    zo.scatter(*t, 4, npx)
    host = (time.perf_counter() - t0) * 1e3
    line.update(oracle_ms_per_slice_nside256=round(host, 1),
                oracle_ms_per_slice_scaled=round(host * npix / npx, 0))
print(json.dumps(line))
