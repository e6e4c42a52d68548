"""The flat-sky line-FFT engine (cora_amd/csrc/flatsky.hip, flatsky_ct.hip, fft_ct.h, tile_walk.h) through ctx.fft_c2c,
ctx.rfftn and ctx.irfftn, held per line and per element to the derived bounds of tests/_linefft_oracle.py on every route:
both ends of the range of each of the 14 Bluestein convolution lengths, both sides of every inner-extent threshold, the
lengths the generic kernel takes by design, and - one length per kernel template - tile counts above the grid cap of the
launch, so that the persistent loop and its prefetch run, and for the strided kernels the XCD pairing of tile_walk.h
(on and off; the contiguous kernels never pair).  tests/test_linefft_host.py shows that the same bounds reject seven
deliberate defects, and that every case below sees every input family.  Run with -m gpu.

Every case: a whole tile, a single line (strided: one outer index; the narrowest strided axis is 2) and a ragged shape
of at least 24 lines, one more than whole items.  Neighbouring lines cycle through four families - impulse, noise scaled
by 2^-300 .. 2^+300, tone, noise - so any four lines in a row hold all of them, every item of two or more lines holds
lines of different families, and every scaled line sits between an impulse and a tone of scale 1 (a tile of 16 lines
holds 2^+300, 2^-300, 2^+150 and 2^-150); the 24 lines bring all six impulse positions, three tones and six exponents.  Every output
against numpy.fft or a closed form, 64 outputs of two lines against the longdouble DFT under the bare bound; output
finite; a sentinel behind the transformed block untouched; a second call returns the same bits.  The table, and the
persistent-loop entries, run a second time in a child process each with CORAHIP_FLAT_GENERIC=1 (generic radix-4 stages
and power-of-two Bluestein at every length; 14 s and 11 s, most of it the host side of the checks), and the bits of the
two runs must differ exactly where the table says a compile-time kernel takes the case.

What these tests do not hold sharply: the Bluestein bound of the compile-time kernels is 2500 - 9900 EPS sqrt(n) ||x||_2,
about 1000 times the observed error, because the error of the device-made filter (flat_blu_filter_kernel) is only certain
in the 2-norm.  A relative error of 1e-13 in a twiddle or a filter value inside lineblu_*_ct or flat_blu_filter_kernel
would pass; gross faults (chirp index, filter wrap, pad, cross-line leak) do not.  The shared passes of fft_ct.h are held
sharply through the scheduled routes (85 - 118 EPS ||x||_1).  Comparing filt_ct itself with the longdouble filter would
close this, but needs a way to read the plan out of the library.

Observed on the MI355X (worst err / bound per route family; the constants are derived in the oracle, none was fitted):

  cases of the table, by the route the table names     default process              CORAHIP_FLAT_GENERIC=1
                                                       numpy / closed  longdouble   numpy / closed  longdouble
  strided c2c, scheduled (linec2c_ct)                  0.058           0.045        0.091           0.086
  strided c2c, scheduled (linec2c_h2_ct)               0.039           0.037        0.087           0.032
  strided c2c, Bluestein (lineblu_c2c_ct)              0.00080         0.00070      0.016           0.014
  strided c2c, generic                                 0.11            0.43         the same bits
  contiguous c2c, generic                              0.090           0.065        the same bits
  even real, scheduled (liner2c_ct / linec2r_ct)       0.080           0.079        0.057           0.048
  even real, Bluestein (lineblu_r2c_ct / _c2r_ct)      0.0014          0.00031      0.0077          0.0027
  even real, generic; odd real                         0.086; 0.034    0.067; 0.024 the same bits
  persistent loop: linec2c_ct / _h2_ct                 0.034 / 0.039   0.033 / 0.034   0.059 / 0.087   0.035 / 0.077
  persistent loop: lineblu_c2c_ct<256 .. 4096>         0.00095 .. 0.00009              0.0099 .. 0.0028
  persistent loop: real scheduled / real Bluestein     0.064 / 0.00055 0.016 / 0.00027 0.0054 / 0.0047
  persistent loop: linefft_kernel strided / contiguous 0.080 / 0.080   0.035 / 0.034   the same bits

The Cooley-Tukey bounds are worst-case sums along the longest path, which random roundings stay 10 - 30 times below
(0.43: n = 2, where the bound is one rounding).  The generic kernel's Bluestein filter is made in longdouble on the host
and its bound is 25 - 57 times smaller than that of the compile-time kernels.  The route check agreed with the table for
all 167 cases and the ten persistent-loop entries.
"""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":
    sys.path.insert(0, sys.argv[1])
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _linefft_oracle as lo

pytestmark = pytest.mark.gpu

FORCED_GENERIC = os.environ.get("CORAHIP_FLAT_GENERIC") is not None
SENTINEL = 0xA5


# ---------------------------------------------------------------------------------------------------------------------
# the case table: (transform, n, inner, route the default process is expected to take)
#   transform "c2c": fft_c2c along an axis of length n with ``inner`` elements behind it (1: the contiguous axis);
#   "real": rfftn and irfftn (naxes = 1) of real length n on the last axis.
#   route "sched" / "h2" / "blu:P" are the compile-time kernels of flatsky_ct.hip, "generic" is linefft_kernel.
# Read off launch_linefft, flat_c2c_ct, flat_r2c_ct, flat_c2r_ct, flat_blu_c2c_ct, flat_blu_real_ct, flat_blu_length.
# ---------------------------------------------------------------------------------------------------------------------
BLU_EDGES = {256: (17, 127), 320: (129, 160), 384: (161, 192), 512: (193, 255), 640: (257, 320), 768: (321, 383),
             1024: (385, 511), 1280: (513, 640), 1536: (641, 767), 2048: (769, 1023), 2560: (1025, 1280),
             3072: (1281, 1536), 3584: (1537, 1792), 4096: (1793, 2047)}
# lines per item of the scheduled strided kernels (flat_c2c_ct) and of the scheduled real kernels (flat_r2c_ct / flat_c2r_ct)
C2C_NCH = {256: 16, 512: 16, 384: 16, 768: 8}
REAL_NCH = {256: 16, 512: 16, 1024: 8, 2048: 4, 192: 16, 384: 16, 768: 8, 1536: 4}

CASES = []
for _P, (_lo, _hi) in BLU_EDGES.items():
    for _n in (_lo, _hi):                                        # the smallest n of P, and the largest (n = P / 2: no pad)
        for _inner in sorted({lo.BLU_NCH[_P], 2, lo.BLU_NCH[_P] + 1}):
            CASES.append(("c2c", _n, _inner, "blu:%d" % _P))
CASES += [("c2c", 384, 15, "blu:768"), ("c2c", 768, 7, "blu:1536")]       # scheduled lengths below their thresholds
for _n in (256, 512, 384):
    CASES += [("c2c", _n, 16, "sched"), ("c2c", _n, 17, "sched")]
CASES += [("c2c", 1024, 8, "sched"), ("c2c", 1024, 15, "sched"), ("c2c", 1024, 16, "h2"), ("c2c", 1024, 17, "h2"),
          ("c2c", 768, 8, "sched"), ("c2c", 768, 9, "sched")]
# powers of two below their thresholds have no Bluestein plan: generic
CASES += [("c2c", 256, 15, "generic"), ("c2c", 512, 15, "generic"), ("c2c", 1024, 7, "generic")]
for _n in (1, 2, 3, 16, 32, 64, 128, 2048, 4096, 2049, 4095):
    _T = max(1, min(16, 4096 // lo.pow2_length(_n, (_n & (_n - 1)) != 0)))
    for _inner in sorted({max(_T, 2), 2, _T + 1}):
        CASES.append(("c2c", _n, _inner, "generic"))
CASES += [("c2c", 255, 1, "generic"), ("c2c", 256, 1, "generic"), ("c2c", 4096, 1, "generic")]
for _P, (_lo, _hi) in BLU_EDGES.items():
    CASES += [("real", 2 * _lo, 1, "blu:%d" % _P), ("real", 2 * _hi, 1, "blu:%d" % _P)]
CASES += [("real", 2 * _h, 1, "sched") for _h in (192, 256, 384, 512, 768, 1024, 1536, 2048)]
CASES += [("real", 2 * _h, 1, "generic") for _h in (8, 16, 32, 64, 128)]
CASES += [("real", _n, 1, "generic") for _n in (3, 17, 255, 4095)]


def case_id(case):
    return "%s-n%d-i%d-%s" % (case[0], case[1], case[2], case[3].replace(":", ""))


def generic_lines(P, mode3_h=0):
    """Lines per tile of linefft_kernel (launch_linefft: 4096 LDS elements, at most 16 lines; mode 3 prefetches h + 1 bins)."""
    T = max(1, min(16, 4096 // P))
    while mode3_h and T > 1 and T * (mode3_h + 1) > 4096:
        T -= 1
    return T


def generic_route(n, mode3=False):
    blu = (n & (n - 1)) != 0
    P = lo.pow2_length(n, blu)
    return lo.Route("blu" if blu else "r4", n, P if blu else 0, ct=False, nch=generic_lines(P, n if mode3 else 0))


def route_of(case, c2r=False, forced=FORCED_GENERIC):
    """The Route (bound constants, lines per item) of a case in THIS process."""
    tr, n, inner, label = case
    m = n if tr == "c2c" else (n // 2 if n % 2 == 0 else n)          # the complex length
    if forced or label == "generic":
        return generic_route(m, mode3=c2r and tr == "real" and n % 2 == 0)
    if label.startswith("blu:"):
        P = int(label[4:])
        assert lo.blu_length(m) == P, (case, lo.blu_length(m))
        return lo.Route("blu", m, P, ct=True, nch=lo.BLU_NCH[P])
    if tr == "real":
        nch = REAL_NCH[m]
        return lo.Route("sched", m, nch=nch, mo=-(-nch * m // 512))
    if label == "h2":
        return lo.Route("h2", 1024, nch=16)
    return lo.Route("sched", n, nch=8 if n == 1024 else C2C_NCH[n])


def table_route(case):
    """Lines per item of the route the TABLE names (the shapes are the same in both processes)."""
    return route_of(case, forced=False)


def first_stride(route):
    """Q0 of the first pass of a route (0: none): the impulses at Q0 - 1 and Q0 sit on both sides of its digit boundary."""
    N = route.P if route.kind == "blu" and route.ct else (512 if route.kind == "h2" else (route.n if route.kind == "sched" else 0))
    return N // lo.SCH[N][0] if N in lo.SCH else 0


# ---------------------------------------------------------------------------------------------------------------------
# running one transform with a sentinel behind the block and a second call
# ---------------------------------------------------------------------------------------------------------------------
def _bits_equal(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def _guarded(ctx, shape, dtype):
    """(big, block): a tensor of shape[0] + 1 leading rows filled with the sentinel, and its leading block."""
    import torch

    big = torch.empty((shape[0] + 1,) + tuple(shape[1:]), dtype=dtype, device=ctx.device)
    big.view(torch.uint8).fill_(SENTINEL)
    return big, big[: shape[0]]


def _tail_intact(big, rows):
    import torch

    return bool((big[rows:].contiguous().view(torch.uint8) == SENTINEL).all().item())


def run_c2c(ctx, arr, axis, inverse):
    """fft_c2c on the leading block of a sentinel-filled tensor, twice -> (result, sentinel intact, same bits)."""
    import torch

    big, blk = _guarded(ctx, arr.shape, torch.complex128)
    src = torch.from_numpy(arr)
    blk.copy_(src)
    ctx.fft_c2c(blk, axis, inverse=inverse)
    got = blk.cpu().numpy()
    ok = _tail_intact(big, arr.shape[0])
    blk.copy_(src)
    ctx.fft_c2c(blk, axis, inverse=inverse)
    return got, ok and _tail_intact(big, arr.shape[0]), _bits_equal(got, blk.cpu().numpy())


def run_real(ctx, arr, n, c2r):
    """ctx.rfftn / ctx.irfftn (naxes = 1) of the leading block of a sentinel-filled input, then the same library call
    into the leading block of a sentinel-filled output -> (result, sentinels intact, same bits)."""
    import torch

    from cora_amd import _lib

    nl = arr.shape[0]
    bigin, blk = _guarded(ctx, arr.shape, torch.complex128 if c2r else torch.float64)
    blk.copy_(torch.from_numpy(arr))
    if c2r:
        got = ctx.irfftn(blk.clone(), naxes=1, last=n).cpu().numpy()
        bigout, out = _guarded(ctx, (nl, n), torch.float64)
        _lib._check(ctx.lib.corahip_irfftn(ctx.h, ctx._c128(blk), 2, ctx._dims((nl, n)), 1, ctx._f64(out)))
    else:
        got = ctx.rfftn(blk, naxes=1).cpu().numpy()
        bigout, out = _guarded(ctx, (nl, n // 2 + 1), torch.complex128)
        _lib._check(ctx.lib.corahip_rfftn(ctx.h, ctx._f64(blk), 2, ctx._dims((nl, n)), 1, ctx._c128(out)))
    again = out.cpu().numpy()
    return got, _tail_intact(bigin, nl) and _tail_intact(bigout, nl), _bits_equal(got, again)


def _ld_lines(plan):
    """Two lines for the longdouble DFT: the first noise line (the first line where there is none) and the last line of
    the last tile."""
    first = next((l for l, p in enumerate(plan) if p[0] in ("noise", "scaled")), 0)
    return sorted({first, len(plan) - 1})


def run_shape(ctx, case, shape, kinds, seed, rec, offset=0, rot=0):
    """One shape of a case: c2c shape = (nouter, inner) lines of n along a strided (inner > 1) or contiguous axis; real
    shape = (nlines,).  offset, rot: where the line plan starts (lo.line_plan)."""
    tr, n, _, _ = case
    for kind in kinds:
        c2r = kind == "c2r"
        route = route_of(case, c2r)
        q0 = first_stride(route)
        if tr == "c2c":
            nouter, inner = shape
            nlines = nouter * inner
            x, plan, exact = lo.make_lines(kind, n, nlines, seed, q0=q0, offset=offset, rot=rot)
            if inner > 1:
                arr = np.ascontiguousarray(x.reshape(nouter, inner, n).transpose(0, 2, 1))
                got, sent, same = run_c2c(ctx, arr, 1, kind == "inv")
                got = np.ascontiguousarray(got.transpose(0, 2, 1)).reshape(nlines, n)
            else:
                got, sent, same = run_c2c(ctx, x, 1, kind == "inv")
        else:
            (nlines,) = shape
            x, plan, exact = lo.make_lines(kind, n, nlines, seed, q0=q0 if c2r else 2 * q0, offset=offset, rot=rot)
            got, sent, same = run_real(ctx, np.ascontiguousarray(x), n, c2r)
        a, b, msgs = lo.check_lines(kind, route, n, x, exact, got, _ld_lines(plan), seed)
        tag = "%s %s %s" % (case_id(case), shape, kind)
        rec["np"] = max(rec["np"], a)
        rec["ld"] = max(rec["ld"], b)
        rec["msgs"] += ["%s: %s" % (tag, m) for m in msgs]
        if not sent:
            rec["msgs"].append("%s: sentinel behind the block overwritten" % tag)
        if not same:
            rec["msgs"].append("%s: second call returned other bits" % tag)
        rec["hash"].update(np.ascontiguousarray(got).view(np.uint8))
        seed += 1


MIN_LINES = 24       # six groups of the four families: every impulse position, tone and six scale exponents


def shapes_of(case):
    """[(shape, offset, rot)]: a whole tile, a single line (a noise line; strided: one outer index) and a ragged shape of
    at least MIN_LINES lines and one line more than whole items (strided: inner is the case's own, the outer count grows).
    The plan of the first shape starts one family later than that of the last, so that items of two lines pair the
    families both ways."""
    tr, n, inner, _ = case
    nch = table_route(case).nch
    if tr == "c2c" and inner > 1:
        return [((1, inner), 1, 0), ((max(3, -(-MIN_LINES // inner)), inner), 0, 1)]
    big = -(-MIN_LINES // nch) * nch + 1
    if tr == "real":
        return [((nch,), 1, 0), ((1,), 3, 0), ((big,), 0, 1)]
    return [((nch, 1), 1, 0), ((1, 1), 3, 0), ((big, 1), 0, 1)]


def items_of(case, shape):
    """Item (tile) index of every line of a shape, in the order of the line plan."""
    nch = table_route(case).nch
    if len(shape) == 2 and shape[1] > 1:
        nouter, inner = shape
        chunks = -(-inner // nch)
        return [o * chunks + i // nch for o in range(nouter) for i in range(inner)]
    return [l // nch for l in range(shape[0])]


def run_case(ctx, case):
    rec = {"np": 0.0, "ld": 0.0, "msgs": [], "hash": hashlib.sha1()}
    kinds = ("fwd", "inv") if case[0] == "c2c" else ("r2c", "c2r")
    seed = 1000 * case[1] + 10 * case[2]
    for s, offset, rot in shapes_of(case):
        run_shape(ctx, case, s, kinds, seed, rec, offset, rot)
        seed += 2
    rec["digest"] = rec.pop("hash").hexdigest()
    return rec


# ---------------------------------------------------------------------------------------------------------------------
# persistent-loop shapes: tile counts above the grid cap of the launch, one length per kernel template
# ---------------------------------------------------------------------------------------------------------------------
def fpc(i):
    return i + (i >> 4)          # fft_ct.h, padding 1: one spare slot per 16 elements


def ct_cap(num_cu, nch, bs, T, wg_cap=None):
    """ct_launch_geom: min(floor(160 KiB / LDS bytes), 2048 / T) workgroups per CU, at least one."""
    per_cu = min((160 * 1024) // (16 * nch * bs), 2048 // T if wg_cap is None else wg_cap)
    return num_cu * max(1, per_cu)


def generic_cap(num_cu, T, P, extra=0):
    """launch_linefft: two workgroups per CU where two tiles (with the twiddle table) fit the 160 KiB, else one."""
    shm = 16 * (T * P + (P // 4 if P <= 4096 else 0) + extra)
    return num_cu * (2 if 2 * shm <= 160 * 1024 else 1)


# (name, case, cap(num_cu) in the default process): the shortest length of each template
PERSISTENT = [
    ("linec2c_ct", ("c2c", 256, 16, "sched"), lambda cu: ct_cap(cu, 16, fpc(256) + 1, 256)),
    ("linec2c_h2_ct", ("c2c", 1024, 16, "h2"), lambda cu: ct_cap(cu, 16, fpc(512) + 1, 512, wg_cap=1)),
    ("lineblu_c2c_ct<256>", ("c2c", 17, 16, "blu:256"), lambda cu: ct_cap(cu, 16, fpc(256) + 1, 512)),
    ("lineblu_c2c_ct<640>", ("c2c", 257, 8, "blu:640"), lambda cu: ct_cap(cu, 8, fpc(640) + 1, 512)),
    ("lineblu_c2c_ct<1280>", ("c2c", 513, 4, "blu:1280"), lambda cu: ct_cap(cu, 4, fpc(1280) + 1, 512)),
    ("lineblu_c2c_ct<4096>", ("c2c", 1793, 2, "blu:4096"), lambda cu: ct_cap(cu, 2, fpc(4096) + 1, 512)),
    ("linec2r_ct / liner2c_ct", ("real", 384, 1, "sched"), lambda cu: max(ct_cap(cu, 16, fpc(192) + 2, 256), ct_cap(cu, 16, fpc(192) + 2, 512))),
    ("lineblu_c2r_ct / lineblu_r2c_ct", ("real", 34, 1, "blu:256"), lambda cu: ct_cap(cu, 16, fpc(256) + 1, 512)),
    ("linefft_kernel strided", ("c2c", 16, 16, "generic"), lambda cu: generic_cap(cu, 16, 16)),
    ("linefft_kernel contiguous", ("c2c", 16, 1, "generic"), lambda cu: generic_cap(cu, 16, 16)),
]


def pairs_xcds(entry):
    """tile_walk::pair_xcds is called by the strided kernels only (linec2c_ct, linec2c_h2_ct, lineblu_c2c_ct, and
    linefft_kernel where inner != 1): the contiguous kernels walk their items in launch order."""
    return entry[1][0] == "c2c" and entry[1][2] > 1


def persistent_tiles(cap):
    """Twice the cap plus 5 (a ragged last trip), a multiple of 64 above the cap (strided kernels: pairing on), and one
    tile more (off).  The contiguous kernels get the same counts: for them they are three trips of the plain loop."""
    paired = (cap // 64 + 1) * 64
    return [2 * cap + 5, paired, paired + 1]


def persistent_shape(case, tiles):
    tr, n, inner, _ = case
    nch = table_route(case).nch
    if tr == "c2c" and inner > 1:
        chunks = next((d for d in (3, 5, 7, 11, 2) if tiles % d == 0), 1)
        return (tiles // chunks, chunks * nch - (1 if chunks > 1 else 0))       # the last chunk of an outer index is short
    nlines = (tiles - 1) * nch + 1                                              # the last item holds one line
    return (nlines,) if tr == "real" else (nlines, 1)


def run_persistent(ctx, entry, num_cu):
    name, case, capf = entry
    cap = capf(num_cu)
    rec = {"np": 0.0, "ld": 0.0, "msgs": [], "hash": hashlib.sha1(), "cap": cap, "tiles": persistent_tiles(cap)}
    kinds = ("fwd", "inv") if case[0] == "c2c" else ("r2c", "c2r")
    for i, tiles in enumerate(rec["tiles"]):
        assert tiles > cap, (name, tiles, cap)                 # a changed launch rule fails here, not silently
        shape = persistent_shape(case, tiles)
        nch = table_route(case).nch
        ntiles = shape[0] * (-(-shape[1] // nch)) if len(shape) == 2 and shape[1] > 1 else -(-shape[0] // nch)
        assert ntiles == tiles, (name, shape, ntiles, tiles)
        # both kinds at every count: the sign is a template parameter of the strided kernels
        run_shape(ctx, case, shape, kinds, 77 + 2 * i, rec)
    rec["digest"] = rec.pop("hash").hexdigest()
    return rec


def _num_cu(ctx):
    import torch

    return int(torch.cuda.get_device_properties(ctx.device).multi_processor_count)


# ---------------------------------------------------------------------------------------------------------------------
# tests
# ---------------------------------------------------------------------------------------------------------------------
_DEFAULT = {}        # case id -> record of this (default) process: the route check compares their digests with the child's


def _family(case):
    tr, n, inner, label = case
    where = "contiguous c2c" if (tr == "c2c" and inner == 1) else ("strided c2c" if tr == "c2c" else ("odd real" if n % 2 else "even real"))
    kind = "generic" if label == "generic" else ("Bluestein" if label.startswith("blu") else "scheduled" + (" (h2)" if label == "h2" else ""))
    return "%s, %s" % (where, kind)


def _record(ctx, key):
    if key not in _DEFAULT:
        by_id = {case_id(c): c for c in CASES}
        if key in by_id:
            _DEFAULT[key] = run_case(ctx, by_id[key])
        else:
            _DEFAULT[key] = run_persistent(ctx, next(e for e in PERSISTENT if "persistent " + e[0] == key), _num_cu(ctx))
    return _DEFAULT[key]


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_line_transform_is_under_its_bound(ctx, case):
    """Whole tile, single line and ragged tile of one case of the table, forward and inverse (rfftn and irfftn)."""
    rec = _record(ctx, case_id(case))
    print("%s [%s, %r]: worst err / bound %.3g (numpy, closed forms), %.3g (longdouble DFT)"
          % (case_id(case), _family(case), route_of(case), rec["np"], rec["ld"]))
    assert not rec["msgs"], "\n".join(rec["msgs"][:20])


@pytest.mark.parametrize("entry", PERSISTENT, ids=lambda e: e[0].replace(" / ", "+").replace("<", "-").replace(">", "").replace(" ", "_"))
def test_persistent_loop_and_xcd_pairing(ctx, entry):
    """Tile counts of twice the grid cap plus 5, a multiple of 64 above the cap and that count plus one.  For the strided
    kernels the second count switches tile_walk::pair_xcds on (the cap itself must then be a multiple of 64) and the
    third switches it off; the contiguous kernels never pair."""
    cap = entry[2](_num_cu(ctx))
    if pairs_xcds(entry):
        assert cap % 64 == 0, "the grid of %s (%d workgroups) is no multiple of 64: pairing never switches on" % (entry[0], cap)
    rec = _record(ctx, "persistent " + entry[0])
    print("%s: cap %d, tiles %s: worst err / bound %.3g (numpy, closed forms), %.3g (longdouble DFT)"
          % (entry[0], rec["cap"], rec["tiles"], rec["np"], rec["ld"]))
    assert rec["tiles"][1] % 64 == 0 and rec["tiles"][2] % 64 == 1 and min(rec["tiles"]) > rec["cap"]
    assert not rec["msgs"], "\n".join(rec["msgs"][:20])


def _summary(records):
    fam = {}
    for c in CASES:
        r = records.get(case_id(c))
        if r is not None:
            f = fam.setdefault(_family(c), [0.0, 0.0])
            f[0], f[1] = max(f[0], r["np"]), max(f[1], r["ld"])
    lines = ["  %-34s %-10.2g %.2g" % (k, v[0], v[1]) for k, v in sorted(fam.items())]
    for e in PERSISTENT:
        r = records.get("persistent " + e[0])
        if r is not None:
            lines.append("  %-34s %-10.2g %.2g" % ("persistent " + e[0], r["np"], r["ld"]))
    return "\n".join(lines)


def _child_and_route_check(ctx, tmp_path, part, keys, labels):
    assert not FORCED_GENERIC, "this test compares the default dispatch with the forced-generic one"
    out = tmp_path / "generic.json"
    env = dict(os.environ)
    env["CORAHIP_FLAT_GENERIC"] = "1"
    # (observed: 14 s for the table, 11 s for the persistent entries, most of it on the host; the limit is for a hang)
    p = subprocess.run([sys.executable, os.path.abspath(__file__), ROOT, str(out), part], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-2000:])
    child = json.loads(out.read_text())
    print("forced generic, worst err / bound (numpy and closed forms, longdouble DFT):\n" + _summary(child))
    bad = [m for r in child.values() for m in r["msgs"]]
    assert not bad, "\n".join(bad[:20])
    assert sorted(child) == sorted(keys)
    wrong = []
    for key, label in zip(keys, labels):
        same = _record(ctx, key)["digest"] == child[key]["digest"]
        if same != (label == "generic"):
            wrong.append("%s: table says %s, but the bits %s those of the generic kernel" % (key, label, "equal" if same else "differ from"))
    print("default process, worst err / bound (numpy and closed forms, longdouble DFT):\n" + _summary({k: _DEFAULT[k] for k in keys}))
    assert not wrong, "\n".join(wrong)


def test_forced_generic_process_and_route_table(ctx, tmp_path):
    """The same table in one fresh child process with CORAHIP_FLAT_GENERIC=1 (read once per process), held to the bounds
    of the generic routes; then the route check: where the table names a compile-time kernel the default output differs
    in bits from the generic one, where it names the generic kernel the bits are equal."""
    _child_and_route_check(ctx, tmp_path, "table", [case_id(c) for c in CASES], [c[3] for c in CASES])


def test_forced_generic_process_persistent_entries(ctx, tmp_path):
    """The persistent-loop shapes on the generic kernel, in a child process of their own, and their route check."""
    _child_and_route_check(ctx, tmp_path, "persistent", ["persistent " + e[0] for e in PERSISTENT], [e[1][3] for e in PERSISTENT])


if __name__ == "__main__":
    from cora_amd import _lib

    assert FORCED_GENERIC
    _ctx = _lib.get_context()
    if sys.argv[3] == "table":
        _out = {case_id(c): run_case(_ctx, c) for c in CASES}
    else:
        _cu = _num_cu(_ctx)
        _out = {"persistent " + _e[0]: run_persistent(_ctx, _e, _cu) for _e in PERSISTENT}
    with open(sys.argv[2], "w") as f:
        json.dump(_out, f)
