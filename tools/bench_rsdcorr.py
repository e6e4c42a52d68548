#!/usr/bin/env python3
"""Timing of the redshift-space correlation kernels (csrc/pk2xi.hip: jl_romb; csrc/rsdcorr.hip: xi_rsd) and of
``Corr21cm.gen_cache()``.  Device events, median of 5 runs after a warm-up, the two forms of a comparison alternating.

  jl_romb    the three orders over 2^16 + 1 wavenumbers at 512 separations against three sinc_romb calls on the same input
             (all the library had for that work): Bessel evaluations per second against sinc_romb's sines per second.
  gen_cache  the default table of the 21cm model (1000 separations, three orders): wall time, the host evaluation of the
             spectrum included, and the device run of the plan alone (``_MultipolePlan.run`` between events: the
             uploads of the wavenumber grids and of the samples of the spectrum are inside it, as in bench_pk2xi.py).
  xi_rsd     2^26 points on the 1000-knot table, 3 and 6 tables, 1 and 65 536 coefficient rows, against the same
             expression composed from torch operations on the same tensors (searchsorted and gathers); the fraction of
             the HBM copy rate (a device-to-device copy of the same 24 B per point, measured here).

Prints one JSON line (and the results so far on stderr after each part).  ``--points`` sets log2 of the number of points (default 26)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def alternating_ms(fa, fb, runs=5):
    """Median device times (ms) of fa() and fb(), run alternately: one warm-up each, then `runs` event pairs each."""
    import torch

    fa(), fb()
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(runs):
        for fn, ts in ((fa, ta), (fb, tb)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1))
    return float(np.median(ta)), float(np.median(tb))


def torch_xi_rsd(kx, ky, ky2, pi, sigma, coef):
    """xi_rsd composed from torch operations: the expressions of cubicspline.Interpolater._eval and corr.py:274-348."""
    import torch

    nfun, nk = ky.shape
    n, ncoef = pi.numel(), coef.shape[0]
    if ncoef > 1:                       # point i reads row i % ncoef: the rows broadcast along the last axis of this view
        pi, sigma = pi.view(n // ncoef, ncoef), sigma.view(n // ncoef, ncoef)
    r = torch.sqrt(pi * pi + sigma * sigma)
    mu = pi / (r + 1e-100)
    hi = torch.searchsorted(kx, r, right=True).clamp_(1, nk - 1)
    lo = hi - 1
    xl, xh = kx[lo], kx[hi]
    h = xh - xl
    a, b = (xh - r) / h, (r - xl) / h
    below, above = r < kx[0], r >= kx[-1]
    h0, h1 = kx[1] - kx[0], kx[-1] - kx[-2]
    s = []
    for f in range(nfun):
        y, y2 = ky[f], ky2[f]
        v = a * y[lo] + b * y[hi] + ((a**3 - a) * y2[lo] + (b**3 - b) * y2[hi]) * (h * h / 6.0)
        v = torch.where(below, ((y[1] - y[0]) / h0 - h0 * y2[1] / 6.0) * (r - kx[0]) + y[0], v)
        v = torch.where(above, ((y[-1] - y[-2]) / h1 + h1 * y2[-2] / 6.0) * (r - kx[-1]) + y[-1], v)
        s.append(v)
    c = coef if ncoef > 1 else coef.expand(n, 4)
    dd0, dv0, dv2 = (s[3], s[4], s[5]) if nfun == 6 else (s[0], s[0], s[1])
    mu2 = mu * mu
    p2 = (3.0 * mu2 - 1.0) / 2.0
    p4 = (35.0 * mu2 * mu2 - 30.0 * mu2 + 3.0) / 8.0
    return (((dd0 * c[:, 0] + 2.0 / 3.0 * dv0 * c[:, 1] + 1.0 / 5.0 * s[0] * c[:, 2])
            - (4.0 / 3.0 * dv2 * c[:, 1] + 4.0 / 7.0 * s[1] * c[:, 2]) * p2 + 8.0 / 35.0 * s[2] * c[:, 2] * p4) * c[:, 3]).reshape(n)


def main():
    import torch

    from cora_amd import _lib
    from cora_amd.signal import corr21cm, corrfunc

    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=26)
    args = ap.parse_args()
    ctx = _lib.get_context()
    d = ctx.to_device
    res = {}

    # jl_romb against three sinc_romb calls
    c21 = corr21cm.Corr21cm()
    plan = corrfunc._MultipolePlan(np.logspace(-3, 4, 1000))
    pd = np.reshape(c21.ps_vv(plan.kdirect[np.newaxis, :]), -1)
    ka, g = d(plan.kdirect), d(pd * plan.kdirect**3 / (2 * np.pi**2))
    r = d(np.logspace(-3, 1, 512))
    out3, out1 = ctx.empty((1, 3, 512)), ctx.empty((512,))
    g2 = g.unsqueeze(0).contiguous()

    def three_sinc():
        for _ in range(3):
            ctx.sinc_romb(g, ka, plan.dlk, r, out=out1)

    t_jl, t_sinc = alternating_ms(lambda: ctx.jl_romb(g2, ka, plan.dlk, r, out=out3), three_sinc)
    n_eval = 512.0 * plan.kdirect.size
    res["jl_romb_ms"], res["three_sinc_romb_ms"] = t_jl, t_sinc
    res["jl_evaluations_per_s"] = 3 * n_eval / (t_jl * 1e-3)
    res["sinc_romb_sines_per_s"] = 3 * n_eval / (t_sinc * 1e-3)
    res["jl_romb_l0_equals_sinc_romb"] = bool(torch.equal(out3[0, 0], out1))
    _progress(res)

    # gen_cache of the 21cm model
    t0 = time.time()
    c21.gen_cache()
    torch.cuda.synchronize()
    res["gen_cache_first_wall_s"] = time.time() - t0
    t0 = time.time()
    c21.gen_cache()
    torch.cuda.synchronize()
    res["gen_cache_wall_s"] = time.time() - t0
    pf = np.reshape(c21.ps_vv(plan.kfine), -1)
    dev, _ = alternating_ms(lambda: plan.run([(pd, pf)], [(0, 2, 4)]), lambda: None)
    res["gen_cache_device_ms"] = dev
    res["gen_cache_levels"] = [plan.n * 2**ii for ii in range(plan.richardson_n)]
    _progress(res)

    # xi_rsd against torch operations
    n = 1 << args.points
    rng = np.random.default_rng(1)
    tab = c21._xi_knots
    kx = d(tab[0])
    ext = np.stack([tab[1][0] * 1.1, tab[1][0] * 0.9, tab[1][1] * 1.05])
    from cora_amd.util import cubicspline

    ext2 = np.stack([cubicspline.Interpolater(tab[0], e)._y2 for e in ext])
    tables = {3: (d(tab[1]), d(tab[2])), 6: (d(np.concatenate([tab[1], ext])), d(np.concatenate([tab[2], ext2])))}
    gen = torch.Generator(device=ctx.device).manual_seed(3)
    rr = 10.0 ** (torch.rand(n, generator=gen, device=ctx.device, dtype=torch.float64) * 7.5 - 3.25)
    th = torch.rand(n, generator=gen, device=ctx.device, dtype=torch.float64) * np.pi
    pi, sigma = rr * torch.cos(th), rr * torch.sin(th)
    del rr, th
    out = ctx.empty((n,))
    src = ctx.empty((3 * n,))
    dst = ctx.empty((3 * n,))                       # 12 B read + 12 B written per point: the traffic of xi_rsd
    t_copy, _ = alternating_ms(lambda: dst[: 3 * n // 2].copy_(src[: 3 * n // 2]), lambda: None)
    res["points"], res["copy_24B_per_point_ms"] = n, t_copy
    for nfun in (3, 6):
        for ncoef in (1, 65536):
            coef = d(rng.uniform(0.5, 2.0, (ncoef, 4)))
            ky, ky2 = tables[nfun]
            t_dev, t_torch = alternating_ms(lambda: ctx.xi_rsd(kx, ky, ky2, pi, sigma, coef, out=out),
                                            lambda: torch_xi_rsd(kx, ky, ky2, pi, sigma, coef))
            ref = torch_xi_rsd(kx, ky, ky2, pi, sigma, coef)
            key = "xi_rsd_nfun%d_ncoef%d" % (nfun, ncoef)
            res[key + "_ms"], res[key + "_torch_ms"] = t_dev, t_torch
            res[key + "_GBps"] = 24.0 * n / (t_dev * 1e-3) / 1e9
            res[key + "_fraction_of_copy_rate"] = t_copy / t_dev
            res[key + "_max_diff_over_max"] = float((out - ref).abs().max() / ref.abs().max())
            del ref
    print(json.dumps(res))


def _progress(res):
    print(json.dumps(res), file=sys.stderr, flush=True)


if __name__ == "__main__":
    main()
