#!/usr/bin/env python3
"""Timing of the exact curved-sky C_l (csrc/fullsky.hip, RedshiftCorrelation.angular_powerspectrum_full) on one GPU;
prints one JSON line.

  (i)   ``sphbessel_radial`` on one chunk of the wavenumber grid of the flagship shape (``--lmax`` x ``--channels`` channels
        x ``2^zromb + 1`` sub-samples, ``--nk`` wavenumbers from the upper end of the grid, where every lane stays on the
        upward recurrence, and from the lower end, where the downward passes run): recurrence steps per second =
        (lmax + 1) F nsub nk / time;
  (ii)  ``cl_gram`` on that table, in TF (2 (lmax + 1) F^2 nk flops: the full square, although only the tiles on and
        above the diagonal are multiplied) and as a share of 77.4 TF (the FP64 MFMA rate of
        profiles/mfma_f64_probe_r01.txt), beside ``torch.bmm`` on the same operands (g folded into one of them first);
  (iii) the whole ``clarray(Corr21cm().angular_powerspectrum_full, lmax, freqs, zromb)`` on the device;
  (iv)  the ratio full / flat-sky of ``Corr21cm`` at l = 2, 10, 100, 1000 on the diagonal at ``--nu`` MHz.

Method: one warm-up call per item, then ``--reps`` (>= 5) timed calls with device events around the call
(ctx.timer_begin / timer_end); median, minimum and maximum are reported.  Nothing is asserted.
Usage: python tools/bench_fullsky_aps.py [--lmax 2048] [--channels 256] [--zromb 3] [--nk 2048] [--reps 5]
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
from cora_amd.core import skysim  # noqa: E402
from cora_amd.signal import corr21cm  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--lmax", type=int, default=2048)
ap.add_argument("--channels", type=int, default=256)
ap.add_argument("--zromb", type=int, default=3)
ap.add_argument("--nk", type=int, default=2048, help="wavenumbers of the kernel timings (one chunk)")
ap.add_argument("--nu", type=float, default=600.0, help="frequency (MHz) of the full / flat-sky ratios")
ap.add_argument("--band", default="400:800", help="band of the whole-clarray timing, MHz")
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--skip-clarray", action="store_true")
a = ap.parse_args()
if a.reps < 5:
    ap.error("--reps must be at least 5")

MFMA_TF = 77.4e12
ctx = _lib.get_context()


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    t = []
    for _ in range(reps):
        ctx.timer_begin()
        fn()
        t.append(ctx.timer_end())
    return dict(ms=round(float(np.median(t)), 3), ms_min=round(min(t), 3), ms_max=round(max(t), 3))


cr = corr21cm.Corr21cm()
lo, hi = (float(v) for v in a.band.split(":"))
F, lmax = a.channels, a.lmax
freqs = lo + (hi - lo) / F * (np.arange(F) + 0.5)
zint = 2 ** a.zromb + 1 if a.zromb else 1
half = (freqs[1] - freqs[0]) / 2.0
za = (freqs[:, None] + np.linspace(-half, half, zint)[None, :]).ravel() if a.zromb else freqs.copy()
p = cr._clarray_plan(cr.angular_powerspectrum_full)["prepare"](za, zint, skysim.romberg_weights(a.zromb))
nk_all = int(p["k"].size)
line = dict(bench="fullsky_aps", reps=a.reps, lmax=lmax, channels=F, zromb=a.zromb, nsub=zint, grid_wavenumbers=nk_all,
            kmax=float(p["k"][-1]), chi_max=float(p["chi"].max()))

nk = min(a.nk, nk_all)
chi, cb, cf = (ctx.to_device(p[n]) for n in ("chi", "cb", "cf"))
steps = float(lmax + 1) * F * zint * nk
for tag, sl in (("upper_end", slice(nk_all - nk, nk_all)), ("lower_end", slice(0, nk))):
    k = ctx.to_device(p["k"][sl])
    r = timed(lambda: ctx.sphbessel_radial(k, chi, cb, cf, lmax), a.reps)
    line["radial_" + tag] = dict(r, nk=nk, x_min=float(p["k"][sl][0] * p["chi"].min()),
                                 steps_per_s=float("%.4g" % (steps / (r["ms"] * 1e-3))))

A = ctx.sphbessel_radial(k, chi, cb, cf, lmax)
g = ctx.to_device(p["g"][:nk])
out = ctx.empty((lmax + 1, F, F))
flop = 2.0 * (lmax + 1) * F * F * nk
r = timed(lambda: ctx.cl_gram(A, g, out=out), a.reps)
line["cl_gram"] = dict(r, nk=nk, tf=round(flop / (r["ms"] * 1e-3) / 1e12, 2),
                       share_of_mfma_rate=round(flop / (r["ms"] * 1e-3) / MFMA_TF, 3))
out_t = ctx.empty((lmax + 1, F, F))


def bmm():
    torch.bmm(A * g, A.transpose(1, 2), out=out_t)


r = timed(bmm, a.reps)
line["torch_bmm"] = dict(r, tf=round(flop / (r["ms"] * 1e-3) / 1e12, 2), share_of_mfma_rate=round(flop / (r["ms"] * 1e-3) / MFMA_TF, 3))
line["gram_max_rel_difference"] = float(((out - out_t).abs().max() / out_t.abs().max()).item())
del A, out, out_t
torch.cuda.empty_cache()

if not a.skip_clarray:
    r = timed(lambda: skysim.clarray_device(cr.angular_powerspectrum_full, lmax, freqs, zromb=a.zromb), max(a.reps, 5))
    line["clarray"] = dict(r, chunk=ctx.clarray_fullsky_chunk(lmax, F, nk_all), recurrence_steps=float(lmax + 1) * F * zint * nk_all,
                           gram_flop=2.0 * (lmax + 1) * F * F * nk_all)

ls = [l for l in (2, 10, 100, 1000) if l <= max(lmax, 1000)]
full = cr.angular_powerspectrum_full(np.array(ls), a.nu, a.nu)
flat = cr.angular_powerspectrum(np.array(ls, dtype=np.float64), a.nu, a.nu)
line["full_over_flat"] = {str(l): float("%.6g" % (x / y)) for l, x, y in zip(ls, full, flat)}
line["full_diag"] = {str(l): float(x) for l, x in zip(ls, full)}
print(json.dumps(line))
