#!/usr/bin/env python3
"""Timing of the LOFAR synchrotron path (csrc/lofar.hip, cora_amd.foreground.lofar) on one GPU; prints one JSON line.

Per shape (x_num = y_num = numz = n, nfreq channels; default 256 x 256 x 256 at 256 channels and 128 x 128 x 128 at 64):
  (i)   ``powerlaw_los`` (the fused call, affine maps folded in) against the same expression as torch operations on the
        same tensors, as the reference writes it: the two rescaled fields once, then per channel one ``[x, y, z]``
        temporary ``A * freq[i] ** beta`` and its sum over z (lofar.py:63-71).  exp per second = nfreq n^3 / time;
        workspace bytes = what each form allocates besides its output (the fused call: none; the torch form: the peak
        of the allocator above the level before the call, minus the output);
  (ii)  ``field_moments`` of one field;
  (iii) the whole ``LofarGDSE.getfield_device(seed=1)`` call (two draws with their FFTs, the moments, the sum).

Method: one warm-up call per item, then ``--reps`` (>= 5) timed calls with device events around the call
(ctx.timer_begin / timer_end); the fused and the torch form alternate in one loop; median, minimum and maximum are
reported.  No ratio is fixed in advance: the torch form on the same tensors is the baseline.
Usage: python tools/bench_lofar.py [--shapes 256:256,128:64] [--reps 5]
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
from cora_amd.foreground import lofar  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--shapes", default="256:256,128:64", help="comma-separated n:nfreq")
ap.add_argument("--reps", type=int, default=5)
a = ap.parse_args()
if a.reps < 5:
    ap.error("--reps must be at least 5")

ctx = _lib.get_context()


def timed(fns, reps):
    """(median, min, max) ms of each callable; the callables are run alternately"""
    for fn in fns:
        fn()
    torch.cuda.synchronize()
    t = [[] for _ in fns]
    for _ in range(reps):
        for k, fn in enumerate(fns):
            ctx.timer_begin()
            fn()
            t[k].append(ctx.timer_end())
    return [(float(np.median(x)), float(min(x)), float(max(x))) for x in t]


def ms3(r):
    return dict(ms=round(r[0], 3), ms_min=round(r[1], 3), ms_max=round(r[2], 3))


line = dict(bench="lofar", reps=a.reps, shapes=[])
gen = torch.Generator(device=ctx.device).manual_seed(1)
for spec in a.shapes.split(","):
    n, F = (int(v) for v in spec.split(":"))
    A = torch.randn((n, n, n), dtype=torch.float64, device=ctx.device, generator=gen)
    B = torch.randn((n, n, n), dtype=torch.float64, device=ctx.device, generator=gen)
    freq = (400.0 + 400.0 / F * (np.arange(F) + 0.5)) / 325.0
    x = ctx.to_device(np.log(freq))
    fr = ctx.to_device(freq)
    a0, sa, b0, sb = 20.0 / n, 0.4 / n**0.5, -2.55, 0.1
    out = ctx.empty((F, n * n))
    out_t = ctx.empty((F, n, n))

    def fused():
        ctx.powerlaw_los(A, B, x, a0=a0, sa=sa, b0=b0, sb=sb, out=out, beta_absmax=8.0)

    def torch_form():
        As = a0 + A * sa
        Bs = b0 + B * sb
        for i in range(F):
            out_t[i] = (As * fr[i] ** Bs).sum(dim=2)

    fused()
    torch_form()
    diff = float(((out.reshape(F, n, n) - out_t).abs() / out_t.abs()).max().item())
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    torch_form()
    torch.cuda.synchronize()
    work_torch = int(torch.cuda.max_memory_allocated() - base)
    torch.cuda.reset_peak_memory_stats()
    fused()
    torch.cuda.synchronize()
    work_fused = int(torch.cuda.max_memory_allocated() - base)
    r = timed([fused, torch_form], a.reps)
    nexp = float(F) * n**3
    rm, = timed([lambda: ctx.field_moments(A)], a.reps)

    m = lofar.LofarGDSE()
    m.x_num = m.y_num = n
    m.nu_num = F
    rw, = timed([lambda: m.getfield_device(seed=1)], a.reps)
    line["shapes"].append(dict(
        n=n, nfreq=F, exps=nexp, max_rel_difference=diff,
        powerlaw_los=dict(ms3(r[0]), exp_per_s=round(nexp / (r[0][0] * 1e-3), -8), workspace_bytes=work_fused),
        torch=dict(ms3(r[1]), exp_per_s=round(nexp / (r[1][0] * 1e-3), -8), workspace_bytes=work_torch),
        torch_over_kernel=round(r[1][0] / r[0][0], 3),
        field_moments=ms3(rm), getfield_device_seed1=ms3(rw)))
    del A, B, out, out_t
    torch.cuda.empty_cache()

print(json.dumps(line))
