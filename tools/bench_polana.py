#!/usr/bin/env python3
"""Timing of the spin-2 analysis both ways: the composition of six scalar passes (Context.map2alm_spin2,
csrc/sht_polana.hip) and the one-pass kernel (Context.map2alm_spin2_native, csrc/sht_polana_native.hip); prints one JSON
line.

  pass   one quadrature pass of ``--fields`` (Q, U) pairs at nside 1024, lmax 2048 (the analysis line of
         tools/bench_pol.py): totals from device events, the stages from the library's stage timers in a profiled call of
         each route (``alm_reduce`` / ``alm_reduce_pol`` are the tile reductions INSIDE ``legendre_adj`` /
         ``legendre_adj_pol``), peak temporaries beyond input and output, the largest difference of the two results, and
         the Legendre rate of the native kernel counted as 2 x the scalar flops per channel (8 nside nalm), beside that of
         the scalar kernel in the composed route, both as fractions of the FP64 MFMA rate.
  sky    hputil.map2alm_sky_device at nside 512 x 256 channels x 3 planes, default chunk, under both settings of
         hputil.spin2_method; peaks beside hputil.map2alm_sky_bytes of each.

Method: device events around each call (ctx.timer_begin / timer_end), one warm-up call of each form, then ``--reps``
(>= 5) timed calls, the two forms alternating in the same loop on the same tensors; medians, minima beside them.
Usage: python tools/bench_polana.py [--reps 5] [--fields 8] [--skip-sky] [--skip-pass]
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
from cora_amd.util import hputil  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--nside", type=int, default=1024)
ap.add_argument("--lmax", type=int, default=2048)
ap.add_argument("--fields", type=int, default=8)
ap.add_argument("--sky-nside", type=int, default=512)
ap.add_argument("--sky-channels", type=int, default=256)
ap.add_argument("--skip-pass", action="store_true")
ap.add_argument("--skip-sky", action="store_true")
a = ap.parse_args()
if a.reps < 5:
    ap.error("--reps must be at least 5")

MFMA_TF = 77.4e12                  # measured FP64 MFMA rate of the chip (profiles/mfma_f64_probe_r01.txt)
ctx = _lib.get_context()
g = torch.Generator(device=ctx.device).manual_seed(1)


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
    ctx._workspace = None          # the cached workspace is a temporary of the route that sized it
    torch.cuda.empty_cache()
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated(ctx.device)
    torch.cuda.reset_peak_memory_stats(ctx.device)
    res = fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated(ctx.device) - base, res


def stages(fn, names):
    ctx.profile_reset()
    ctx.profile_enable(True)
    fn()
    torch.cuda.synchronize()
    st = {k: round(ctx.profile_get(k)[0], 3) for k in names}
    ctx.profile_enable(False)
    return st


line = dict(bench="polana", reps=a.reps, mfma_rate_TF=MFMA_TF / 1e12)

# ---- one quadrature pass -------------------------------------------------------------------------------------------
if not a.skip_pass:
    nside, lmax, nf = a.nside, a.lmax, a.fields
    nalm = (lmax + 1) * (lmax + 2) // 2
    qu = torch.randn((2 * nf, 12 * nside * nside), dtype=torch.float64, device=ctx.device, generator=g)
    composed = lambda: ctx.map2alm_spin2(qu, nside, lmax)
    native = lambda: ctx.map2alm_spin2_native(qu, nside, lmax)
    pc, rc = peak_of(composed)
    pn, rn = peak_of(native)
    out_bytes = rn.numel() * 8
    diff = float((rn - rc).abs().max() / rc.abs().max())
    del rc, rn
    (c, c_min), (n, n_min) = timed([composed, native])
    sc = stages(composed, ("spin2_scale", "ringana", "legendre_adj", "alm_reduce", "spin2_combine"))
    sn = stages(native, ("ringana", "legendre_adj_pol", "alm_reduce_pol"))
    unit = 8.0 * nside * nalm                                       # scalar Legendre flops per channel
    kc = (sc["legendre_adj"] - sc["alm_reduce"]) * 1e-3             # the MFMA kernels alone
    kn = (sn["legendre_adj_pol"] - sn["alm_reduce_pol"]) * 1e-3
    line.update(pass_nside=nside, pass_lmax=lmax, pass_fields_QU=nf,
                composed_ms=round(c, 3), composed_ms_min=round(c_min, 3), native_ms=round(n, 3), native_ms_min=round(n_min, 3),
                pass_speedup=round(c / n, 3), composed_stages_ms=sc, native_stages_ms=sn,
                ringana_ratio=round(sc["ringana"] / sn["ringana"], 3),
                legendre_ratio=round(sc["legendre_adj"] / sn["legendre_adj_pol"], 3),
                composed_peak_GB=round((pc - out_bytes) / 1e9, 3), native_peak_GB=round((pn - out_bytes) / 1e9, 3),
                input_GB=round(qu.numel() * 8 / 1e9, 3), native_minus_composed_rel=diff,
                legendre_adj_TF=round(unit * 6 * nf / kc / 1e12, 2),
                legendre_adj_frac_mfma=round(unit * 6 * nf / kc / MFMA_TF, 3),
                legendre_adj_pol_TF=round(2 * unit * 2 * nf / kn / 1e12, 2),
                legendre_adj_pol_frac_mfma=round(2 * unit * 2 * nf / kn / MFMA_TF, 3))
    del qu
    torch.cuda.empty_cache()

# ---- the polarised sky ---------------------------------------------------------------------------------------------
if not a.skip_sky:
    nside, F = a.sky_nside, a.sky_channels
    lmax = 3 * nside - 1
    maps = torch.randn((F, 3, 12 * nside * nside), dtype=torch.float64, device=ctx.device, generator=g)
    def sky(m):
        with hputil.spin2_method(m):
            return hputil.map2alm_sky_device(maps)

    def bound(m):
        with hputil.spin2_method(m):
            return hputil.map2alm_sky_bytes(nside, lmax, 3)

    forms = {m: (lambda m=m: sky(m)) for m in ("composed", "native")}
    for m, fn in forms.items():
        peak, alm = peak_of(fn)
        line.update({"sky_%s_peak_GB" % m: round((peak - alm.numel() * 8) / 1e9, 3),
                     "sky_%s_bound_GB" % m: round(bound(m) / 1e9, 3)})
        del alm
    (c, c_min), (n, n_min) = timed([forms["composed"], forms["native"]])
    line.update(sky_nside=nside, sky_channels=F, sky_planes=3, sky_lmax=lmax, sky_chunk=hputil.SKY_CHUNK,
                sky_composed_ms=round(c, 2), sky_composed_ms_min=round(c_min, 2), sky_native_ms=round(n, 2),
                sky_native_ms_min=round(n_min, 2), sky_speedup=round(c / n, 3))
print(json.dumps(line))
