#!/usr/bin/env python3
"""Timing of the all-pairs spectrum kernel (csrc/spectra.hip, Context.alm_cross_spectra) on a_lm in the device layout;
prints one JSON line.

Cases: cfg 3 (256 channels, lmax 2048), symmetric and with a second operand; 128 slices at nside 1024 (lmax 3071),
symmetric.  The a_lm are torch.randn on the device.

Method: per case one warm-up call of each form, then ``--reps`` (>= 5) timed calls with ctx.timer_begin / timer_end
(device events around the call), the forms alternating in the same loop on the same tensors; medians are reported,
minima beside them.

Baseline: the torch route on the same a_lm - ``alm_dev_to_square`` (the layout change the host route needs, kept on the
device here) plus one batched complex product ``bmm(X c_m, X^H).real / (2l+1)`` over l.  Its result is compared with
the kernel's (``*_max_diff``: largest difference over the largest value).

Models the figures are set against (arithmetic, not measurements):
  MFMA floor: the v_mfma_f64_16x16x4_f64 the kernel issues (2048 flop each; counted as executed: the symmetric case
              skips the tiles above the diagonal, 16 x 16 blocks beyond the channel count are not multiplied, the m
              rows of the last chunk of an l are padded to a multiple of 2) at 77.4 TF (profiles/mfma_f64_probe_r01.txt);
  HBM floor:  every operand element read once and every output element written once at 6.3 TB/s.
Usage: python tools/bench_spectra.py [--reps 7] [--skip-lss] [--channels 256 --lmax 2048]
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

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--channels", type=int, default=256)
ap.add_argument("--lmax", type=int, default=2048)
ap.add_argument("--slices", type=int, default=128)
ap.add_argument("--nside", type=int, default=1024)
ap.add_argument("--skip-lss", action="store_true")
a = ap.parse_args()
if a.reps < 5:
    ap.error("--reps must be at least 5")

HBM, MFMA_TF = 6.3e12, 77.4e12
T, KM = 128, 8                     # tile edge and m rows per chunk of cross_spectra_kernel
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


def mfma_count(nx, ny, lmax, sym):
    """MFMA instructions cross_spectra_kernel issues: per l and 64 x 64 wave block the 16 x 16 blocks inside the
    operands, times 4 steps per chunk of 8 m (m = 1 .. l) + 1 step for m = 0"""
    blocks = 0
    for ti in range((nx + T - 1) // T):
        for tj in range((ny + T - 1) // T):
            if sym and tj > ti:
                continue
            for wr in (0, 64):
                for wc in (0, 64):
                    if sym and ti == tj and wr < wc:
                        continue
                    nu = sum(1 for u in range(4) if ti * T + wr + 16 * u < nx)
                    nv = sum(1 for v in range(4) if tj * T + wc + 16 * v < ny)
                    blocks += nu * nv
    l = np.arange(lmax + 1)
    steps = int((4 * ((l + KM - 1) // KM) + 1).sum())
    return blocks * steps


def randn_alm(n, lmax):
    nalm = (lmax + 1) * (lmax + 2) // 2
    return torch.randn((nalm, (n + 3) // 4, 2, 4), dtype=torch.float64, device=ctx.device, generator=g)


def torch_route(alm_a, nx, alm_b, ny, lmax, cm, inv):
    X = ctx.alm_dev_to_square(alm_a, lmax, nx)[:, 0].permute(1, 0, 2)              # [l, channel, m]
    Y = X if alm_b is None else ctx.alm_dev_to_square(alm_b, lmax, ny)[:, 0].permute(1, 0, 2)
    return torch.bmm(X * cm, Y.conj().transpose(1, 2)).real * inv


def case(tag, nx, ny, lmax, two):
    alm_a = randn_alm(nx, lmax)
    alm_b = randn_alm(ny, lmax) if two else None
    out = ctx.empty((lmax + 1, nx, ny))
    cm = torch.full((lmax + 1,), 2.0, dtype=torch.float64, device=ctx.device)
    cm[0] = 1.0
    inv = (1.0 / (2.0 * torch.arange(lmax + 1, dtype=torch.float64, device=ctx.device) + 1.0))[:, None, None]
    ref = torch_route(alm_a, nx, alm_b, ny, lmax, cm, inv)
    got = ctx.alm_cross_spectra(alm_a, nx, lmax, alm_b=alm_b, ny=ny if two else None, out=out)
    diff = float((got - ref).abs().max() / ref.abs().max())
    del ref
    (k, k_min), (t, t_min) = timed([lambda: ctx.alm_cross_spectra(alm_a, nx, lmax, alm_b=alm_b, ny=ny if two else None, out=out),
                                    lambda: torch_route(alm_a, nx, alm_b, ny, lmax, cm, inv)])
    fl = mfma_count(nx, ny, lmax, not two) * 2048
    by = (alm_a.numel() + (alm_b.numel() if two else 0) + out.numel()) * 8
    return {tag + "_ms": round(k, 3), tag + "_ms_min": round(k_min, 3), tag + "_torch_ms": round(t, 3),
            tag + "_torch_ms_min": round(t_min, 3), tag + "_over_torch": round(k / t, 4), tag + "_max_diff": diff,
            tag + "_flops": fl, tag + "_bytes": by, tag + "_mfma_floor_ms": round(fl / MFMA_TF * 1e3, 3),
            tag + "_hbm_floor_ms": round(by / HBM * 1e3, 3), tag + "_frac_mfma": round(fl / MFMA_TF * 1e3 / k, 3),
            tag + "_frac_hbm": round(by / HBM * 1e3 / k, 3)}


line = dict(bench="spectra", reps=a.reps, channels=a.channels, lmax=a.lmax, hbm_model_Bps=HBM, mfma_model_flops=MFMA_TF)
line.update(case("sym", a.channels, a.channels, a.lmax, False))
torch.cuda.empty_cache()
line.update(case("two", a.channels, a.channels, a.lmax, True))
torch.cuda.empty_cache()
if not a.skip_lss:
    line.update(lss_slices=a.slices, lss_nside=a.nside, lss_lmax=3 * a.nside - 1)
    line.update(case("lss", a.slices, a.slices, 3 * a.nside - 1, False))
print(json.dumps(line))
