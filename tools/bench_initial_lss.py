#!/usr/bin/env python3
"""Timing of the initial-LSS step (csrc/corrfunc.hip: xi_multi_average, cl_blocks; signal/lss.py) at the project's LSS
size: nside 1024 (lmax 3071), 128 slices, leg_q 4 (12 284 nodes), xromb 2 (5 radial points).

(a) kernel A/B at 64, 602 and 2925 knots (the last the most the LDS kernel takes): one ``xi_multi_average`` of three
    tables against three ``xi_table_average`` calls, on ``--ab-nodes`` of the 12 284 nodes, the two forms alternating;
    both kernels evaluate the F (F + 1) / 2 pairs (i, j >= i) per node and function, and are counted so;
(b) the full step at 6002 knots (``calculate_correlations`` at its defaults): the xi kernel, the projection, the assembly,
    the factorisation of the 256-channel blocks, the draw plus synthesis; device memory in use; the host route's rate.

Device events, median of 5 runs after a warm-up.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MFMA_F64_TF = 77.4           # the FP64 MFMA rate of profiles/mfma_f64_probe_r01.txt


def ps(k):
    x = np.asarray(k, dtype=np.float64) / 0.02
    return 2e4 * x / (1.0 + x * x) ** 2


def ms_of(fn):
    import torch

    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def device_ms(fn, runs=5):
    """Median device time of fn() in ms: one warm-up, then `runs` event pairs on the current stream."""
    import torch

    fn()
    torch.cuda.synchronize()
    return float(np.median([ms_of(fn) for _ in range(runs)]))


def device_ms_ab(fa, fb, runs=5):
    """Medians of two forms, alternating, after one warm-up of each."""
    import torch

    fa()
    fb()
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(runs):
        ta.append(ms_of(fa))
        tb.append(ms_of(fb))
    return float(np.median(ta)), float(np.median(tb))


def in_use():
    import torch

    free, total = torch.cuda.mem_get_info()
    return int(total - free)


def main():
    import scipy.special as ss
    import torch

    from cora_amd import _lib
    from cora_amd.core import skysim
    from cora_amd.signal import corrfunc, lss
    from cora_amd.util import constants, cubicspline
    from cora_amd.util.cosmology import Cosmology

    ap = argparse.ArgumentParser()
    ap.add_argument("--nside", type=int, default=1024)
    ap.add_argument("--slices", type=int, default=128)
    ap.add_argument("--ab-nodes", type=int, default=384)
    ap.add_argument("--no-draw", action="store_true", help="stop after the factorisation")
    args = ap.parse_args()

    ctx = _lib.get_context()
    d = ctx.to_device
    nside, F, leg_q, xromb = args.nside, args.slices, 4, 2
    lmax = 3 * nside - 1
    freq = np.linspace(800.0, 400.0, F, endpoint=False)
    chi = np.asarray(Cosmology().comoving_distance(constants.nu21 / freq - 1.0), dtype=np.float64)
    M = leg_q * lmax
    mu, w, wsum = ss.roots_legendre(M, mu=True)
    xa, xw, xint = corrfunc._radial_nodes(chi, xromb, None)
    npair = F * (F + 1) // 2
    res = {"nside": nside, "lmax": lmax, "slices": F, "nodes": M, "xint": xint}

    t0 = time.time()
    corrs = lss.calculate_correlations(ps, ksmooth=0.02)
    res["calculate_correlations_wall_s"] = time.time() - t0
    cs = [corrs["corr0"], corrs["corr2"], corrs["corr4"]]
    kind, kx, ky, ky2, x_t, f_t = corrfunc.joint_spline_tables(cs)
    res["knots"] = int(kx.size)

    # (a) the three functions resampled on 1 + (nk - 1) separations: the most the LDS kernel takes, where it runs one
    # workgroup per CU, and the small tables at which its table fill is short and several workgroups share a CU
    nk_max = min(2925, ctx.xi_table_max_knots())
    ma = args.ab_nodes
    mu_a = d(mu[:: max(1, M // ma)][:ma])
    ma = mu_a.numel()
    xa_d, xw_d = d(xa), d(xw)
    out_m = ctx.empty((ma, 3, npair))
    out_t = ctx.empty((ma, F, F))
    evals_ab = 3.0 * ma * npair * xint * xint        # both kernels evaluate the pairs (i, j >= i) only
    res["ab"] = []
    for nk_a in (64, 602, nk_max):
        r_a = np.concatenate([[0.0], np.logspace(-1, 5, nk_a - 1)])
        small = [cubicspline.SinhInterpolater(np.column_stack([r_a, c(r_a)]), x_t=r_a[1], f_t=c.f_t) for c in cs]
        _, kxa, kya, ky2a, x_ta, f_ta = corrfunc.joint_spline_tables(small)
        kxa_d, kya_d, ky2a_d = d(kxa), d(kya), d(ky2a)
        rows_a = [(kya_d[f].contiguous(), ky2a_d[f].contiguous()) for f in range(3)]

        def fused():
            ctx.xi_multi_average(kxa_d, kya_d, ky2a_d, 2, x_ta, f_ta, mu_a, xa_d, xw_d, F, xint, out=out_m)

        def three_calls():
            for f in range(3):
                ctx.xi_table_average(kxa_d, rows_a[f][0], rows_a[f][1], 2, x_ta, f_ta[f], mu_a, xa_d, xw_d, F, xint, out=out_t)

        t_m, t_t = device_ms_ab(fused, three_calls)
        res["ab"].append({"knots": nk_a, "nodes": ma, "xi_multi_ms": t_m, "three_xi_table_ms": t_t,
                          "ratio_multi_over_three": t_m / t_t, "xi_multi_spline_evals_per_s": evals_ab / (t_m * 1e-3),
                          "xi_table_spline_evals_per_s": evals_ab / (t_t * 1e-3)})
    # the same fused kernel on the 6002-knot tables and the same nodes: what the larger table costs
    kx_d, ky_d, ky2_d = d(kx), d(ky), d(ky2)
    t_big = device_ms(lambda: ctx.xi_multi_average(kx_d, ky_d, ky2_d, 2, x_t, f_t, mu_a, xa_d, xw_d, F, xint, out=out_m))
    res["xi_multi_ms_at_%d_knots_ab_nodes" % kx.size] = t_big
    del out_m, out_t
    print(json.dumps(res), file=sys.stderr, flush=True)        # (stages so far, should a later one fail)

    # (b) the full step
    torch.cuda.synchronize()
    base = in_use()
    rows = (M + 15) // 16 * 16
    mu_p, wt_p = np.zeros(rows), np.zeros(rows)
    mu_p[:M], wt_p[:M] = mu, w * 4.0 * np.pi / wsum
    mu_d, wt_d = d(mu_p), d(wt_p)
    xi = ctx.empty((rows, 3, npair))
    t_xi = device_ms(lambda: ctx.xi_multi_average(kx_d, ky_d, ky2_d, 2, x_t, f_t, mu_d[:M], xa_d, xw_d, F, xint, nm_rows=rows, out=xi))
    evals = 3.0 * M * npair * xint * xint
    packed = ctx.empty((lmax + 1, 3 * npair))
    t_pr = device_ms(lambda: ctx.legendre_project(mu_d, wt_d, lmax, xi.reshape(rows, 3 * npair), out=packed))
    flop = 2.0 * (lmax + 1) * rows * 3 * npair
    ext = ctx.empty((lmax + 1, 2 * F, 2 * F))
    t_as = device_ms(lambda: ctx.cl_blocks(packed.reshape(lmax + 1, 3, npair), F, out=ext))
    torch.cuda.synchronize()
    res["full"] = {"xi_multi_ms": t_xi, "spline_evals": evals, "spline_evals_per_s": evals / (t_xi * 1e-3),
                   "projection_ms": t_pr, "projection_TF": flop / (t_pr * 1e-3) / 1e12,
                   "projection_share_of_mfma_rate": flop / (t_pr * 1e-3) / 1e12 / MFMA_F64_TF,
                   "assembly_ms": t_as, "assembly_GBps": (packed.numel() + ext.numel()) * 8 / (t_as * 1e-3) / 1e9,
                   "bytes_in_use_xi_packed_ext": in_use() - base,
                   "bytes_xi": xi.numel() * 8, "bytes_packed": packed.numel() * 8, "bytes_ext": ext.numel() * 8}
    del xi, packed
    torch.cuda.empty_cache()
    print(json.dumps(res["full"]), file=sys.stderr, flush=True)
    factors = None

    def factor():
        nonlocal factors
        factors = skysim.factor_device(ext)

    res["full"]["factor_ms"] = device_ms(factor)
    res["full"]["blocks_not_cholesky"] = int((factors[1] != 0).sum())
    print(json.dumps(res["full"]), file=sys.stderr, flush=True)
    if not args.no_draw:
        def draw():
            return skysim.mkfullsky_device(None, nside, rng=np.random.default_rng(1), factors=factors)

        draw()
        torch.cuda.synchronize()
        t0 = time.time()
        sky = draw()
        torch.cuda.synchronize()
        res["full"]["draw_and_synthesis_wall_s"] = time.time() - t0
        res["full"]["finite"] = bool(torch.isfinite(sky[::37, ::1001]).all())
        res["full"]["bytes_in_use_after_draw"] = in_use() - base
        del sky
    res["full"]["torch_max_memory_allocated"] = int(torch.cuda.max_memory_allocated())

    # the host route: SinhInterpolater on the 6002-knot table, one core
    rr = np.random.default_rng(0).uniform(0.0, 6000.0, 2_000_000)
    t0 = time.time()
    cs[0](rr)
    dt = time.time() - t0
    res["host"] = {"evals_per_s": rr.size / dt, "xi_stage_s_extrapolated_three_functions_full_square": 3.0 * M * (F * xint) ** 2 / (rr.size / dt)}
    res["full"]["xi_speedup_over_host_route"] = res["host"]["xi_stage_s_extrapolated_three_functions_full_square"] / (t_xi * 1e-3)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
