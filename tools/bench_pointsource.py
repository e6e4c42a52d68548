#!/usr/bin/env python3
"""Timing of the point-source path (csrc/pointsource.hip, cora_amd.foreground.pointsource) on one GPU at full size:
nside 1024 x 256 channels, DiMatteo with the default flux_min = 1e-4 (about 2.0e7 sources); prints one JSON line.

  (i)   the steps of ``PointSourceModel.getsky`` one by one: population (one launch), torch.sort(stable=True) on pixel
        with the gathers that reorder flux and index, paint (offsets + one-lane-per-pixel kernel), and
        ``polarise_rotate``;
  (ii)  the paint and the rotation against the same steps as torch operations on the same inputs: for the paint,
        ``flux[:, None] * exp(index[:, None] * x[None, :])`` over chunks of ``--chunk`` sources added with
        ``index_add_`` (the full [N, F] array is 41 GB and is what the paint avoids; float64 ``index_add_`` uses
        atomics, so its sums are not reproducible), then the unit conversion; for the rotation, complex tensor
        arithmetic channel by channel, as the reference does.  Fused and torch forms are timed alternately in one loop;
  (iii) the synthetic component of ``CombinedPointSources`` (about 7.4e4 sources) at the same map size, written as a
        whole map and accumulated onto an existing one.

Method: one warm-up call per item, then ``--reps`` (>= 5) timed calls with device events around the call
(ctx.timer_begin / timer_end); median, minimum and maximum are reported.

Models the figures are set against (arithmetic, not measurements): the bytes the paint writes, 8 F npix, at 6.3 TB/s
(the copy rate measured on an MI355X), and its exp evaluations, N F.
Usage: python tools/bench_pointsource.py [--nside 1024] [--nfreq 256] [--flux-min 1e-4] [--reps 5] [--chunk 262144]
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
from cora_amd.foreground import pointsource, poisson  # noqa: E402
from cora_amd.util import constants  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--nside", type=int, default=1024)
ap.add_argument("--nfreq", type=int, default=256)
ap.add_argument("--flux-min", type=float, default=1e-4)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--chunk", type=int, default=262144)
ap.add_argument("--no-torch", action="store_true", help="skip the torch forms")
a = ap.parse_args()
if a.reps < 5:
    ap.error("--reps must be at least 5")

HBM = 6.3e12
ctx = _lib.get_context()
nside, F = a.nside, a.nfreq
npix = 12 * nside * nside
freq = 400.0 + 400.0 / F * (np.arange(F) + 0.5)


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


def spline_of(model):
    area = 4 * np.pi
    flux_max = model._flux_max(area)
    t = np.log(flux_max / model.flux_min)
    rate = model._log_rate(area)
    data, y2 = poisson.inverse_cdf(t, rate).data()
    return poisson.expected_events(t, rate), data[:, 0].copy(), data[:, 1].copy(), y2


def paint_inputs(model):
    x = np.log(freq / model.spectral_pivot)
    den = 2 * constants.k_B * freq**2 * 1e12 * (4 * np.pi / npix)
    return x, den, constants.c**2


line = dict(bench="pointsource", nside=nside, npix=npix, nfreq=F, reps=a.reps, hbm_model_Bps=HBM)

# ---- (i), (ii): the full population --------------------------------------------------------------------------------------
m = pointsource.DiMatteo()
m.nside, m.frequencies, m.flux_min = nside, freq, a.flux_min
av, xs, ys, y2 = spline_of(m)
N = int(round(av))
line.update(expected_sources=av, sources=N)
x, den, c2 = paint_inputs(m)
state = {}


def population():
    state["pop"] = ctx.pointsource_population(11, N, xs, ys, y2, m.flux_min, m.spectral_mean, m.spectral_width, npix)


def sort():
    pix, flux, index = state["pop"]
    spix, order = torch.sort(pix, stable=True)
    state["sorted"] = (spix, flux[order].contiguous(), index[order].contiguous())


out = ctx.empty((F, npix))


def paint():
    spix, flux, index = state["sorted"]
    ctx.pointsource_paint(spix, flux, index, x, den, c2, npix, out=out)


(r_pop,) = timed([population], a.reps)
(r_sort,) = timed([sort], a.reps)
xd = ctx.to_device(x)
convd = ctx.to_device(1e-26 * c2 / den)


def paint_torch():
    pix, flux, index = state["pop"]
    res = torch.zeros((F, npix), dtype=torch.float64, device=ctx.device)
    for s in range(0, N, a.chunk):
        e = min(N, s + a.chunk)
        sr = flux[s:e, None] * torch.exp(index[s:e, None] * xd[None, :])
        res.index_add_(1, pix[s:e], sr.T)
    res *= convd[:, None]
    return res


fns = [paint]
paint_line = dict(bytes_written=8.0 * F * npix, exp_evaluations=float(N) * F)
if not a.no_torch:
    try:
        ref = paint_torch()
        paint()
        paint_line["max_rel_difference"] = float(((ref - out).abs().max() / ref.abs().max()).item())
        del ref
        fns.append(paint_torch)
    except torch.cuda.OutOfMemoryError:
        torch.cuda.empty_cache()
        paint_line["torch_form"] = "did not fit in device memory"
res = timed(fns, a.reps)
paint_line.update(ms3(res[0]))
sec = res[0][0] * 1e-3
paint_line.update(written_Bps=round(8.0 * F * npix / sec, -9), frac_hbm_written=round(8.0 * F * npix / HBM / sec, 3),
                  exp_per_s=round(float(N) * F / sec, -6))
if len(res) > 1:
    paint_line.update(torch=ms3(res[1]), torch_over_paint=round(res[1][0] / res[0][0], 3), chunk=a.chunk)
line.update(population=ms3(r_pop), sort=ms3(r_sort), paint=paint_line)
state.clear()
torch.cuda.empty_cache()

# ---- polarise_rotate ---------------------------------------------------------------------------------------------------
rng = np.random.default_rng(3)
q, u = (ctx.to_device(0.03 * rng.standard_normal(npix)) for _ in range(2))
rm = ctx.to_device(rng.uniform(-300.0, 300.0, npix))
wv = 1e-6 * constants.c / freq
rot_line = dict(bytes_moved=8.0 * F * npix * 5)
try:
    cube = ctx.empty((F, 4, npix))

    def rotate():
        ctx.polarise_rotate(out, q, u, wv=wv, rm=rm, out=cube)

    def rotate_torch():
        res = torch.zeros((F, 4, npix), dtype=torch.float64, device=ctx.device)
        res[:, 0] = out
        for f in range(F):
            far = torch.exp(torch.complex(torch.zeros_like(rm), -2.0 * wv[f] * rm))
            qu = torch.complex(out[f] * q, out[f] * u) * far
            res[f, 1] = qu.real
            res[f, 2] = qu.imag
        return res

    fns = [rotate]
    if not a.no_torch:
        try:
            ref = rotate_torch()
            rotate()
            rot_line["max_abs_difference"] = max(float((ref[f] - cube[f]).abs().max().item()) for f in range(F))
            del ref
            fns.append(rotate_torch)
        except torch.cuda.OutOfMemoryError:
            torch.cuda.empty_cache()
            rot_line["torch_form"] = "did not fit in device memory"
    res = timed(fns, a.reps)
    rot_line.update(ms3(res[0]))
    rot_line.update(moved_Bps=round(rot_line["bytes_moved"] / (res[0][0] * 1e-3), -9),
                    frac_hbm=round(rot_line["bytes_moved"] / HBM / (res[0][0] * 1e-3), 3))
    if len(res) > 1:
        rot_line.update(torch=ms3(res[1]), torch_over_kernel=round(res[1][0] / res[0][0], 3))
    del cube
except torch.cuda.OutOfMemoryError:
    rot_line["polarise_rotate"] = "the [F, 4, npix] cube did not fit in device memory"
line["polarise_rotate"] = rot_line
torch.cuda.empty_cache()

# ---- (iii): the synthetic component of CombinedPointSources ------------------------------------------------------------------
mc = pointsource.CombinedPointSources._RandomResolved()
mc.nside, mc.frequencies = nside, freq
avc, xsc, ysc, y2c = spline_of(mc)
Nc = int(round(avc))
xc, denc, _ = paint_inputs(mc)


def combined(accumulate):
    def run():
        pix, flux, index = ctx.pointsource_population(12, Nc, xsc, ysc, y2c, mc.flux_min, mc.spectral_mean, mc.spectral_width, npix)
        spix, order = torch.sort(pix, stable=True)
        ctx.pointsource_paint(spix, flux[order].contiguous(), index[order].contiguous(), xc, denc, c2, npix, out=out,
                              accumulate=accumulate)
    return run


r_w, r_a = timed([combined(False), combined(True)], a.reps)
line["combined_random_resolved"] = dict(sources=Nc, whole_map=ms3(r_w), accumulate=ms3(r_a))
print(json.dumps(line))
