#!/usr/bin/env python3
"""Timing of P(k) -> xi(r) (csrc/pk2xi.hip, corrfunc.ps_to_corr) at the defaults of lss.calculate_correlations: 2001
direct separations over 2^16 + 1 wavenumbers, nine FFTLog levels of 14000 x 2^ii points.  Device events, median of 5
runs after a warm-up; the same work in numpy (the reference's expressions, scipy's loggamma for the FFTLog kernel) on the
host cores of the same box.  Prints one JSON line."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DEFAULTS = dict(minlogr=-1, maxlogr=5, switchlogr=1, samples_per_decade=1000, pad_low=4, pad_high=6, richardson_n=9)
HOST_DIRECT_NR = 251          # separations of the host direct integral (the figure is scaled to all of them)


def pk(k):
    return k * np.exp(-8.0 * k)


def device_ms(fn, runs=5):
    """Median device time of fn() in ms: one warm-up, then `runs` event pairs on the current stream."""
    import torch

    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return float(np.median(ts))


def host_direct(ka, g, dlk, r):
    """_corr_direct of the reference, a block of separations at a time."""
    import scipy.integrate as si

    out = np.empty(r.size)
    for a in range(0, r.size, 64):
        out[a : a + 64] = si.romb(g[None, :] * np.sinc(ka[None, :] * r[a : a + 64, None] / np.pi)) * dlk
    return out


def host_fftlog(plan, pfine):
    """_corr_hankl_richardson of the reference with hankl.P2xi written out in numpy."""
    import scipy.special as ss

    from cora_amd.signal import corrfunc

    est = []
    for ii in range(plan.richardson_n):
        u, step = 2**ii, plan.umax >> ii
        k = plan.kfine[::step]
        N = k.size
        eta = 2 * np.pi * np.arange(N // 2 + 1) / (N * np.log(k[1] / k[0]))
        U = np.exp(1j * (eta * np.log(2.0) + 2 * ss.loggamma((1.5 + 1j * eta) / 2).imag))
        g = np.fft.irfft(np.fft.rfft(pfine[::step] * k**1.5) * U, N)[::-1]
        est.append((g[(u - 1) :: u] * (2 * np.pi) ** -1.5 * plan.r0**-1.5)[plan.mask])
    return corrfunc.richardson(est, 2.0)


def main():
    import torch

    from cora_amd import _lib
    from cora_amd.signal import corrfunc

    ctx = _lib.get_context()
    t0 = time.time()
    plan = corrfunc._CorrPlan(**DEFAULTS)
    t_plan = time.time() - t0
    t0 = time.time()
    pd, pf = pk(plan.kdirect), pk(plan.kfine)
    t_ps = time.time() - t0
    res = {"separations_direct": int(plan.rlow.size), "separations_fftlog": int(plan.rhigh.size),
           "levels": [plan.n * 2**ii for ii in range(plan.richardson_n)], "splits": plan.splits,
           "host_plan_s": t_plan, "host_psfunc_s": t_ps}

    # the whole default-size call: device part (uploads of the samples included), and wall time with the host evaluation
    res["ps_to_corr_device_ms"] = device_ms(lambda: plan.run(pd, pf))
    t0 = time.time()
    r, xi = corrfunc.ps_to_corr(pk, **DEFAULTS)
    res["ps_to_corr_wall_s"] = time.time() - t0

    # each kernel at its default size
    d = ctx.to_device
    ka, g, rl = d(plan.kdirect), d(pd * plan.kdirect**3 / (2 * np.pi**2)), d(plan.rlow)
    out = ctx.empty((plan.rlow.size,))
    ms = device_ms(lambda: ctx.sinc_romb(g, ka, plan.dlk, rl, out=out))
    nsin = float(plan.rlow.size) * plan.kdirect.size
    res["sinc_romb_ms"], res["sines_per_s"] = ms, nsin / (ms * 1e-3)
    N = plan.n * plan.umax
    L = N * float(np.log(plan.kfine[1] / plan.kfine[0]))
    U = ctx.empty((N // 2 + 1,), dtype=torch.complex128)
    res["fftlog_phase_ms"] = device_ms(lambda: ctx.fftlog_phase(0.5, L, N, out=U))
    data = torch.complex(d(pf * plan.kfine**1.5), torch.zeros(N, dtype=torch.float64, device=ctx.device))
    res["logconv_ms"] = device_ms(lambda: ctx.logconv(data, U, plan.splits[-1]))      # (in place, over and over: timing only)
    res["logconv_N"] = N

    # the same on the host cores
    t0 = time.time()
    sub = plan.rlow[:: max(1, plan.rlow.size // HOST_DIRECT_NR)]          # (the same stride below)
    hd = host_direct(plan.kdirect, pd * plan.kdirect**3 / (2 * np.pi**2), plan.dlk, sub)
    res["host_direct_s"] = (time.time() - t0) * plan.rlow.size / sub.size
    t0 = time.time()
    hf = host_fftlog(plan, pf)
    res["host_fftlog_s"] = time.time() - t0
    res["host_total_s"] = res["host_direct_s"] + res["host_fftlog_s"]
    res["speedup_device_part"] = res["host_total_s"] / (res["ps_to_corr_device_ms"] * 1e-3)
    env = 2 / (2 * np.pi**2 * np.maximum(r, 1e-30) * (64.0 + r * r) ** 1.5)      # the envelope of the analytic xi of pk
    nl = plan.rlow.size
    stride = max(1, nl // HOST_DIRECT_NR)
    res["max_dev_minus_host_over_envelope_direct"] = float((np.abs(xi[:nl:stride] - hd) / env[:nl:stride])[1:].max())
    below = plan.rhigh < 1e3
    res["max_dev_minus_host_over_envelope_fftlog_r_below_1e3"] = float((np.abs(xi[nl:] - hf) / env[nl:])[below].max())
    res["finite"] = bool(np.isfinite(xi).all())
    print(json.dumps(res))


if __name__ == "__main__":
    main()
