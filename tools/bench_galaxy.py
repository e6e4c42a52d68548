#!/usr/bin/env python3
"""Timing of the constrained-galaxy path (csrc/galaxy.hip, cora_amd.foreground.galaxy) on one GPU at nside 512 x 256
channels; prints one JSON line.

  (i)   ``galaxy_combine`` against the same expression as torch operations on the same tensors (the dozen full-cube
        passes of galaxy.py:181-198), and its bytes moved (2 F npix + 3 npix doubles read, F npix written) over time as
        a fraction of the HBM copy rate, which this tool measures in the same run (a device-to-device copy of a buffer
        of the cube's size: bytes read + written over time);
  (ii)  ``healpix_block_variance`` (512 -> 16) against the torch route: a gather by the NESTED permutation, ``var`` over
        the children, a gather back (the reference's two reordered copies);
  (iii) one batched ``smoothing_device`` of three maps;
  (iv)  the stages of one ``ConstrainedGalaxy.getsky_device`` call, timed one by one on the host clock with a device
        synchronisation after each: clarray, mkfullsky, smoothing, mkconstrained, the variance chain, combine, rotation.
        ``mkconstrained`` is timed on both routes with the same inputs, run alternately ``--reps`` times (median reported):
        ``mkconstrained_host`` (numpy maps: download, per-l ``eigh`` on the host, the square ``cv`` array, upload) and
        ``mkconstrained_device`` (tensor maps: ``eig_top_batched``, ``constrained_weights``, ``alm_mix_l``); the share of l
        that take the full decomposition is reported for the synchrotron C_l and for a 21cm ``clarray`` of the same shape.

Method: one warm-up call per item, then ``--reps`` (>= 5) timed calls with device events around the call
(ctx.timer_begin / timer_end); the fused and the torch form alternate in one loop; median, minimum and maximum are
reported.  No ratio is fixed in advance: the torch form on the same tensors is the baseline.
Usage: python tools/bench_galaxy.py [--nside 512] [--nfreq 256] [--reps 5]
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

from cora_amd import DeviceRNG, _lib  # noqa: E402
from cora_amd.core import skysim  # noqa: E402
from cora_amd.foreground import galaxy  # noqa: E402
from cora_amd.util import hputil  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--nside", type=int, default=512)
ap.add_argument("--nfreq", type=int, default=256)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--no-getsky", action="store_true", help="skip the stage breakdown (iv)")
a = ap.parse_args()
if a.reps < 5:
    ap.error("--reps must be at least 5")

ctx = _lib.get_context()
nside, F = a.nside, a.nfreq
npix = 12 * nside * nside


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


line = dict(bench="galaxy", nside=nside, npix=npix, nfreq=F, reps=a.reps)
rng = np.random.default_rng(1)
gen = torch.Generator(device=ctx.device).manual_seed(1)

# ---- (i) combine ---------------------------------------------------------------------------------------------------------
efreq = np.concatenate(([408.0, 1420.0], 400.0 + 400.0 / F * (np.arange(F) + 0.5)))
fg = torch.randn((F + 2, npix), dtype=torch.float64, device=ctx.device, generator=gen) * 6.0
fgs = torch.randn((F + 2, npix), dtype=torch.float64, device=ctx.device, generator=gen) * 3.0
haslam = ctx.to_device(rng.uniform(10.0, 60.0, npix))
sc = ctx.to_device(rng.uniform(-3.5, -2.0, npix))
am = ctx.to_device(rng.uniform(0.5, 8.0, npix))
mv = 1.3
out = ctx.empty((F, npix))
ratio = ctx.to_device(efreq / 408.0)


def combine():
    ctx.galaxy_combine(fg, fgs, haslam, sc, am, mv, efreq, skip=2, out=out)


def combine_torch():
    fgt = (am / mv) * (fg - fgs)
    fgsmooth = haslam[None, :] * (ratio[:, None] ** sc)
    fgt /= fgsmooth
    fgt = torch.where(fgt < 0, torch.tanh(fgt), fgt)
    fgt += 1
    fgt *= fgsmooth
    return fgt[2:]


def copy():
    out.copy_(fg[2:])


moved = 8.0 * (3 * F * npix + 3 * npix)
r_copy, = timed([copy], a.reps)
copy_rate = 2 * 8.0 * F * npix / (r_copy[0] * 1e-3)
comb = dict(bytes_moved=moved)
fns = [combine]
try:
    ref = combine_torch()
    combine()
    comb["max_rel_difference"] = float(((ref - out).abs() / ref.abs().clamp_min(1e-300)).max().item())
    del ref
    fns.append(combine_torch)
except torch.cuda.OutOfMemoryError:
    torch.cuda.empty_cache()
    comb["torch_form"] = "did not fit in device memory"
res = timed(fns, a.reps)
comb.update(ms3(res[0]))
comb.update(moved_Bps=round(moved / (res[0][0] * 1e-3), -9), frac_of_copy_rate=round(moved / (res[0][0] * 1e-3) / copy_rate, 3))
if len(res) > 1:
    comb.update(torch=ms3(res[1]), torch_over_kernel=round(res[1][0] / res[0][0], 3))
line.update(hbm_copy=dict(ms3(r_copy), Bps=round(copy_rate, -9)), combine=comb)
del fgs, out
torch.cuda.empty_cache()

# ---- (ii) block variance ---------------------------------------------------------------------------------------------------
nvar = 16
one = fg[:1].contiguous()
to_nest = ctx.to_device(hputil.nest2ring(nside, np.arange(npix)), dtype=np.int64)
to_ring = ctx.to_device(hputil.ring2nest(nvar, np.arange(12 * nvar * nvar)), dtype=np.int64)


def blockvar():
    return ctx.healpix_block_variance(one, nvar)


def blockvar_torch():
    return one[:, to_nest].reshape(1, -1, (nside // nvar) ** 2).var(dim=2, unbiased=False)[:, to_ring]


if nside >= nvar and nside <= 64 * nvar:
    diff = float((blockvar() - blockvar_torch()).abs().max().item())
    r_k, r_t = timed([blockvar, blockvar_torch], a.reps)
    line["block_variance"] = dict(ms3(r_k), nside_out=nvar, max_abs_difference=diff, torch=ms3(r_t),
                                  torch_over_kernel=round(r_t[0] / r_k[0], 3))

# ---- (iii) batched smoothing ---------------------------------------------------------------------------------------------
lmax = 3 * nside - 1
beams = np.stack([hputil.gauss_beam(np.radians(w), lmax) for w in (1.0, 5.8, 0.5 * np.sqrt(8 * np.log(2)))])
three = fg[[0, 1, 0]]
r_s, = timed([lambda: hputil.smoothing_device(three, fl=beams)], a.reps)
line["smoothing_3_maps"] = ms3(r_s)
del fg, three
torch.cuda.empty_cache()

# ---- (iv) the stages of one getsky_device call ------------------------------------------------------------------------------
if not a.no_getsky:
    stages = {}

    def stage(name, fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = fn()
        torch.cuda.synchronize()
        stages[name] = round(stages.get(name, 0.0) + (time.perf_counter() - t0) * 1e3, 3)
        return res

    hmap = rng.uniform(10.0, 60.0, 12 * 64 * 64)
    gal = stage("init_amp_map", lambda: galaxy.ConstrainedGalaxy(haslam=hmap, spectral=np.full(hmap.size, -2.8), amp_nside=nside))
    gal.nside, gal.frequencies = nside, efreq[2:]
    init_ms = stages.pop("init_amp_map")
    syn = galaxy.FullSkySynchrotron()                                 # (the SHT plans exist: (iii) made them)
    cla = stage("clarray", lambda: skysim.clarray(syn.angular_powerspectrum, lmax, efreq, zromb=0))
    fg = stage("mkfullsky", lambda: skysim.mkfullsky_device(cla, nside, rng=DeviceRNG(1)))
    sm = stage("smoothing", lambda: hputil.smoothing_device(fg[[0, 1, 0]], fl=beams))
    sub = stage("download", lambda: ctx.to_host(sm[:2]))
    # mkconstrained: the host route (numpy maps: per-l eigh, the square cv array) and the device route (tensor maps:
    # eig_top_batched, constrained_weights, alm_mix_l) on the same inputs, run alternately; the median of each
    cla_d = ctx.to_device(cla)
    t_h, t_d = [], []
    for rep in range(a.reps):
        for name, ts, fn in (("mkconstrained_host", t_h, lambda: skysim.mkconstrained(cla, [(0, sub[0])], nside)),
                             ("mkconstrained_device", t_d, lambda: skysim.mkconstrained(cla_d, [(0, sm[0])], nside))):
            before = stages.get(name, 0.0)
            res = stage(name, fn)
            ts.append(stages[name] - before)
            if name == "mkconstrained_host":
                fgs_h = res
            else:
                fgs_d = res
            print("mkconstrained rep %d %s %.1f ms" % (rep, name, ts[-1]), file=sys.stderr, flush=True)
    stages["mkconstrained_host"] = round(float(np.median(t_h)), 3)
    stages["mkconstrained_device"] = round(float(np.median(t_d)), 3)
    mk = dict(host_ms=ms3((np.median(t_h), min(t_h), max(t_h))), device_ms=ms3((np.median(t_d), min(t_d), max(t_d))),
              host_over_device=round(float(np.median(t_h) / np.median(t_d)), 2),
              max_abs_difference_over_rms=float(np.abs(fgs_d.cpu().numpy() - fgs_h).max() / fgs_h.std()))
    # the share of l that take the full decomposition: the synchrotron C_l of this run, and a 21cm clarray of the same shape
    mk["fallback_share_synchrotron"] = float((skysim.constrained_weights_device(cla_d, [0])[1][1:] != 0).double().mean())
    try:
        from cora_amd.signal import corr21cm

        c21 = skysim.clarray_device(corr21cm.Corr21cm().angular_powerspectrum, lmax, efreq[2:].copy(), zromb=0)
        i21 = skysim.constrained_weights_device(c21, [0])[1]
        mk["fallback_share_21cm"] = float((i21[1:] != 0).double().mean())
        del c21
    except Exception as e:      # (the 21cm tables need their data file)
        mk["fallback_share_21cm"] = "not measured: %s" % type(e).__name__
    line["mkconstrained"] = mk
    del fgs_d, cla_d
    fgs = stage("upload", lambda: ctx.to_device(fgs_h))
    hs, scs, ams = stage("ud_grade", lambda: tuple(hputil.ud_grade(ctx.to_device(m) if isinstance(m, np.ndarray) else m, nside)
                                                   for m in (gal._haslam, gal._sp_ind["md"], gal._amp_map)))
    vm = stage("variance_chain", lambda: hputil.smoothing_device(galaxy.map_variance(sm[2:3], 16).sqrt(), sigma=np.radians(2.0)))
    mvv = float(vm.mean())
    fgt = stage("combine", lambda: ctx.galaxy_combine(fg, fgs, hs, scs, ams, mvv, efreq, skip=2))
    del fg, fgs
    stage("rotation", lambda: hputil.rotate_map_device(fgt, hputil.coord_matrix("C", "G")))
    del fgt
    # totals of the two routes: the host route has the download, the host stage and the upload, the device route its stage
    dev_ms = stages.pop("mkconstrained_device")
    total = sum(stages.values())
    total_dev = total - stages["download"] - stages["mkconstrained_host"] - stages["upload"] + dev_ms
    line["getsky_stages_ms"] = dict(stages, mkconstrained_device=dev_ms, total=round(total, 3), total_device_route=round(total_dev, 3),
                                    init_amp_map=init_ms,
                                    mkconstrained_host_fraction=round(stages["mkconstrained_host"] / total, 3),
                                    mkconstrained_device_fraction=round(dev_ms / total_dev, 3))
print(json.dumps(line))
