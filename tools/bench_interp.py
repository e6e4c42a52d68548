#!/usr/bin/env python3
"""Timing of the HEALPix bilinear-interpolation kernels (csrc/hpinterp.hip) at working size on device tensors; prints
one JSON line per part.

  rotate   hputil.rotate_map_device at nside 1024 x 256 channels, against its torch composition on the same tensors:
           four gather-multiply-adds ``maps[:, pix_k] * w_k`` with pix, w already on the device
           (``torch_gather_only_ms``), the angles of the rotated pixel centres (torch, from device-resident centre
           vectors) and their weights (Context.healpix_interp_weights) timed apart
           (``device_angles_and_weights_ms``), and both together (``torch_ms``); no host work is timed; reported as a fraction of the HBM rate for its minimum traffic, one read and one
           write of the cube, 2 nmap npix 8 bytes.  ``workspace_saved_bytes``: what the composition holds beyond the
           cube and the result (pix, w, angles, and two [nmap, npix] temporaries).
  val      hputil.get_interp_val_device on 1e7 random directions x 256 maps, against the same composition.
  grid     lss.za_density_grid_device at nside 1024 x 128 slices, against za_density_sph_device on the same inputs and
           against a torch composition (new positions in torch, weights from Context.healpix_interp_weights,
           torch.bucketize, eight ``index_add_``).  Model it is set against: 8 f64 atomic adds per particle (64 N
           bytes) at the 1.3 TB/s chip-wide rate of global float atomics, and the streaming floor of its reads (psi,
           delta_bias: 32 N bytes) plus the read and write of out (16 N bytes) at the HBM rate.

Every figure is the median of ``--reps`` runs after one warm-up, timed with device events, with the min and max beside
it; the torch compositions run ``--torch-reps`` times.  No pass / fail threshold.
Usage: python tools/bench_interp.py [--only rotate,val,grid] [--nside 1024] [--nmap 256] [--nchi 128] [--reps 5]
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
from cora_amd.signal import lss  # noqa: E402
from cora_amd.util import hputil  # noqa: E402

HBM = 6.3e12          # bytes / s: the rate tools/bench_lss_chain.py sets its streaming floors against

ap = argparse.ArgumentParser()
ap.add_argument("--only", default="rotate,val,grid")
ap.add_argument("--nside", type=int, default=1024)
ap.add_argument("--nmap", type=int, default=256)
ap.add_argument("--nchi", type=int, default=128)
ap.add_argument("--ndir", type=int, default=10_000_000)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--torch-reps", type=int, default=2)
a = ap.parse_args()

ctx = _lib.get_context()
dev = ctx.device
nside = a.nside
npix = 12 * nside * nside
gen = torch.Generator(device=dev).manual_seed(1)


def timed(fn, reps):
    fn()                                                       # warm-up
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return dict(ms=round(float(np.median(ms)), 3), ms_min=round(min(ms), 3), ms_max=round(max(ms), 3))


def gather_torch(maps, pix, w, out):
    """out = sum_k maps[:, pix_k] * w_k with two [nmap, n] temporaries"""
    torch.index_select(maps, 1, pix[0], out=out)
    out.mul_(w[0])
    for k in range(1, 4):
        out.add_(torch.index_select(maps, 1, pix[k]).mul_(w[k]))
    return out


def rel(a_, b_):
    return float((a_ - b_).abs().max() / b_.abs().max())


def rotated_angles(vdev, Rdev):
    """(theta, phi) of R n_p from the pixel-centre vectors, all on the device"""
    r = Rdev @ vdev
    th = torch.atan2(torch.sqrt(r[0] * r[0] + r[1] * r[1]), r[2])
    ph = torch.atan2(r[1], r[0])
    return th, torch.where(ph < 0, ph + 2 * np.pi, ph)


if "rotate" in a.only:
    nmap = a.nmap
    maps = torch.randn((nmap, npix), dtype=torch.float64, device=dev, generator=gen)
    out = torch.empty_like(maps)
    R = hputil.coord_matrix("G", "C")
    t = timed(lambda: hputil.rotate_map_device(maps, R, out=out), a.reps)
    ref = torch.empty_like(maps)
    # nothing of the composition runs on the host inside a timed region: the pixel-centre vectors and R are device
    # tensors made once, here
    vdev = torch.stack([ctx.to_device(c) for c in hputil.pix2vec(nside, np.arange(npix))])
    Rdev = ctx.to_device(R)
    torch.cuda.synchronize()
    held = {}

    def geometry():
        th, ph = rotated_angles(vdev, Rdev)
        held["pix"], held["w"] = ctx.healpix_interp_weights(nside, th, ph)

    tg = timed(geometry, a.torch_reps)
    tgather = timed(lambda: gather_torch(maps, held["pix"], held["w"], ref), a.torch_reps)

    def compose():
        geometry()
        gather_torch(maps, held["pix"], held["w"], ref)

    tt = timed(compose, a.torch_reps)
    traffic = 2 * nmap * npix * 8
    print(json.dumps(dict(bench="rotate_map_device", nside=nside, nmap=nmap, **t, min_traffic_bytes=traffic,
                          frac_of_hbm=round(traffic / HBM * 1e3 / t["ms"], 3), torch_gather_only_ms=tgather["ms"],
                          torch_gather_only_ms_min=tgather["ms_min"], device_angles_and_weights_ms=tg["ms"],
                          torch_ms=tt["ms"], torch_ms_min=tt["ms_min"],
                          speedup_over_torch=round(tt["ms"] / t["ms"], 2),
                          speedup_over_gather_only=round(tgather["ms"] / t["ms"], 2), max_rel_diff=rel(out, ref),
                          workspace_saved_bytes=2 * nmap * npix * 8 + npix * (4 * 8 + 4 * 8 + 5 * 8))), flush=True)
    del maps, out, ref, vdev, held
    torch.cuda.empty_cache()

if "val" in a.only:
    nmap, n = a.nmap, a.ndir
    maps = torch.randn((nmap, npix), dtype=torch.float64, device=dev, generator=gen)
    th = torch.acos(2 * torch.rand(n, dtype=torch.float64, device=dev, generator=gen) - 1)
    ph = 2 * np.pi * torch.rand(n, dtype=torch.float64, device=dev, generator=gen)
    holder = {}

    def run():
        holder["out"] = hputil.get_interp_val_device(maps, th, ph)

    t = timed(run, a.reps)
    ref = torch.empty((nmap, n), dtype=torch.float64, device=dev)

    def compose():
        pix, w = ctx.healpix_interp_weights(nside, th, ph)
        gather_torch(maps, pix, w, ref)

    tt = timed(compose, a.torch_reps)
    print(json.dumps(dict(bench="get_interp_val_device", nside=nside, nmap=nmap, ndir=n, **t,
                          samples_per_s=round(nmap * n / t["ms"] * 1e3), torch_ms=tt["ms"], torch_ms_min=tt["ms_min"],
                          speedup_over_torch=round(tt["ms"] / t["ms"], 2), max_rel_diff=rel(holder["out"], ref))),
          flush=True)
    del maps, ref, holder
    torch.cuda.empty_cache()

if "grid" in a.only:
    nchi = a.nchi
    N = nchi * npix
    res = np.sqrt(4 * np.pi / npix)
    psi = torch.randn((3, nchi, npix), dtype=torch.float64, device=dev, generator=gen)
    psi[0] *= 2.0
    psi[1] *= res
    psi[2] *= 2 * res
    db = 0.4 * torch.randn((nchi, npix), dtype=torch.float64, device=dev, generator=gen)
    dm = 0.8 * torch.randn((nchi, npix), dtype=torch.float64, device=dev, generator=gen)
    chi_h = 1000.0 + 5.0 * np.arange(nchi)
    chi = ctx.to_device(chi_h)
    out = torch.zeros((nchi, npix), dtype=torch.float64, device=dev)

    def grid():
        out.zero_()
        lss.za_density_grid_device(psi, db, dm, chi, out)

    def sph():
        out.zero_()
        lss.za_density_sph_device(psi, db, dm, chi, out)

    zero = timed(out.zero_, a.reps)["ms"]
    ts = timed(sph, a.reps)
    t = timed(grid, a.reps)
    mass = float((out + 1).sum()) / float((1 + db).sum()) - 1.0
    line = dict(bench="za_density_grid_device", nside=nside, nchi=nchi, particles=N, ms=round(t["ms"] - zero, 3),
                ms_min=round(t["ms_min"] - zero, 3), ms_max=round(t["ms_max"] - zero, 3), zero_fill_ms=zero,
                sph_ms=round(ts["ms"] - zero, 3), sph_over_grid=round((ts["ms"] - zero) / (t["ms"] - zero), 2),
                atomic_only_ms_model=round(64 * N / 1.3e12 * 1e3, 1), stream_floor_ms_model=round(48 * N / HBM * 1e3, 1),
                mass_rel_change=mass)     # shares beyond the two radial ends are dropped
    got = out.clone()
    del dm
    torch.cuda.empty_cache()
    thp, php = (ctx.to_device(c) for c in hputil.pix2ang(nside, np.arange(npix)))
    ext = ctx.to_device(np.r_[2 * chi_h[0] - chi_h[1], chi_h, 2 * chi_h[-1] - chi_h[-2]])

    def compose():
        out.zero_()
        flat = out.view(-1)
        for ii in range(nchi):                                  # slice by slice, as the reference loops
            th, ph = thp + psi[1, ii], php + psi[2, ii]
            wrap = (th > np.pi) | (th < 0)
            th = torch.where(wrap, np.pi - torch.remainder(th, np.pi), th)
            ph = torch.remainder(torch.where(wrap, ph + np.pi, ph), 2 * np.pi)
            pix, w = ctx.healpix_interp_weights(nside, th, ph)
            x = chi_h[ii] + psi[0, ii]
            ind = torch.bucketize(x, ext, right=True)
            c0, c1 = ext[(ind - 1) % (nchi + 2)], ext[ind % (nchi + 2)]
            rho = 1 + db[ii]
            for rb, rw in ((ind - 2, ((c1 - x) / (c1 - c0)).abs()), (ind - 1, ((x - c0) / (c1 - c0)).abs())):
                ok = (rb >= 0) & (rb < nchi)
                rw = torch.where(ok, rw, torch.zeros_like(rw))
                row = torch.where(ok, rb, torch.zeros_like(rb)) * npix
                for k in range(4):
                    flat.index_add_(0, row + pix[k], (rho * w[k]) * rw)
        out.sub_(1.0)

    tt = timed(compose, max(1, a.torch_reps - 1))
    line.update(torch_ms=tt["ms"], speedup_over_torch=round(tt["ms"] / line["ms"], 2),
                max_diff_vs_torch=float((got - out).abs().max()))
    print(json.dumps(line), flush=True)
