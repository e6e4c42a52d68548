#!/usr/bin/env python3
"""Timing of the correlated shot noise step (corahip_normal_rows_pcg64) at nside 1024 x 128 slices; prints one JSON line.

Method: per form one warm-up call, then ``--reps`` (>= 5) timed calls with ctx.timer_begin / timer_end (device events
around the call, which includes the read-back of the raw-draw count both forms make); the two device forms are timed
alternately in the same loop on the same field; the median is reported, the minimum beside it.

  (a) the fused call: ``normal_rows_pcg64(..., accumulate=True)`` - the normals leave the generator's emit pass scaled and
      added to the field.  Traffic: the field read and written once, 16 B per voxel; no workspace beyond the block tables.
  (b) the composition available before the entry point existed: ``normals_pcg64`` into a buffer of nchi x npix doubles,
      then ``field.addcmul_(buffer, std[:, None])``.  Traffic: 8 B (the buffer written) + 24 B (buffer and field read,
      field written) per voxel, and the buffer itself as workspace.
  (c) numpy on the host: ``rng.normal(scale=std[0], size=npix)`` for one slice (wall clock, median of 3), times nchi;
      the upload of the result is not included.

The fused call cuts its rows into sessions of 2^28 values; at this size that is 7 sessions.  ``--check`` (default on)
draws the same 128 slices with numpy on the host, one slice at a time, and compares the first and the last 4096 values of
every slice, bit for bit, with the fused call on a zeroed field, and the generator states afterwards.

After the timing one call of each form runs under the library's stage profile: the seek, count, scan and emit passes of
the generator are reported per form (``fused_zig_emit_ms`` ...).

Usage: python tools/bench_shotnoise.py [--nside 1024] [--n 128] [--reps 5] [--no-check]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
import torch  # noqa: E402

from cora_amd import _lib  # noqa: E402
from cora_amd.signal import lss  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--nside", type=int, default=1024)
ap.add_argument("--n", type=int, default=128)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--no-check", dest="check", action="store_false")
a = ap.parse_args()
if a.reps < 5:
    ap.error("--reps must be at least 5")

ctx = _lib.get_context()
n, npix = a.n, 12 * a.nside * a.nside
N = n * npix
chi = np.linspace(1800.0, 2400.0, n)
std = lss.shot_noise_std(a.nside, chi, 1e-3)
std_d = ctx.to_device(std)
seed = 20261020
st = np.random.default_rng(seed).bit_generator.state["state"]
s0, inc = int(st["state"]), int(st["inc"])

field = torch.zeros((n, npix), dtype=torch.float64, device=ctx.device)


def fused():
    return ctx.normal_rows_pcg64(s0, inc, std_d, npix, field, accumulate=True)


buf = torch.empty((N,), dtype=torch.float64, device=ctx.device)


def composed():
    ctx.normals_pcg64(s0, inc, N, out=buf)
    field.addcmul_(buf.view(n, npix), std_d[:, None])


line = dict(bench="shotnoise", nside=a.nside, n=n, elements=N, reps=a.reps)

if a.check:
    # the cut into sessions against numpy: first and last 4096 values of every slice, and the state afterwards
    rng = np.random.default_rng(seed)
    n_raw = fused()
    torch.cuda.synchronize()
    head, tail = field[:, :4096].cpu().numpy(), field[:, -4096:].cpu().numpy()
    ok = True
    for r in range(n):
        ref = rng.normal(scale=std[r], size=npix)
        ok = ok and np.array_equal(head[r].view(np.uint64), ref[:4096].view(np.uint64)) \
            and np.array_equal(tail[r].view(np.uint64), ref[-4096:].view(np.uint64))
    state_ok = _lib.pcg64_advance(s0, inc, n_raw) == int(rng.bit_generator.state["state"]["state"])
    line.update(sessions=-(-n // max(1, (1 << 28) // npix)), cut_equals_numpy=bool(ok), state_equals_numpy=bool(state_ok),
                raw_draws_per_normal=round(n_raw / N, 6))
    field.zero_()

t = [[], []]
for fn in (fused, composed):
    fn()
torch.cuda.synchronize()
for _ in range(a.reps):
    for k, fn in enumerate((fused, composed)):
        ctx.timer_begin()
        fn()
        t[k].append(ctx.timer_end())
fa, fb = float(np.median(t[0])), float(np.median(t[1]))

host = []
hr = np.random.default_rng(seed)
for _ in range(3):
    t0 = time.perf_counter()
    hr.normal(scale=std[0], size=npix)
    host.append(time.perf_counter() - t0)
fc = float(np.median(host)) * n * 1e3

line.update(fused_ms=round(fa, 3), fused_ms_min=round(min(t[0]), 3), composed_ms=round(fb, 3), composed_ms_min=round(min(t[1]), 3),
            fused_over_composed=round(fa / fb, 4), numpy_host_ms=round(fc, 1), numpy_over_fused=round(fc / fa, 1),
            fused_bytes=16 * N, composed_bytes=32 * N, composed_workspace_bytes=8 * N, host_upload_bytes=8 * N,
            fused_GBps=round(16 * N / fa / 1e6, 1), composed_GBps=round(32 * N / fb / 1e6, 1))

# the library's stage profile of one call of each form (device events around each stage)
ctx.profile_enable(True)
for tag, fn in (("fused", fused), ("composed", composed)):
    ctx.profile_reset()
    fn()
    torch.cuda.synchronize()
    for stage in ("zig_seek", "zig_count", "zig_scan", "zig_emit"):
        line["%s_%s_ms" % (tag, stage)] = round(ctx.profile_get(stage)[0], 3)
ctx.profile_enable(False)
print(json.dumps(line))
