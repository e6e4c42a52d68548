"""Every entry point outside the SHT on POISONED outputs, workspaces and library scratch (harness: tests/_poison.py).

Each case is one call at the smallest shape that has a tail (no extent a kernel tiles over is a multiple of the tile),
run with every fresh ``torch.empty`` allocation, the cached workspace and the scratch slots of the context (csrc/common.h)
filled with byte 0, then 0xFF, then 0x7E.  It passes if the poisoned results are finite and equal to the byte-0 one:
"exact" unless the case says otherwise ("atomic": the call ends in the run-time ring kernel; "global-atomics": float atomics
on global memory, the run-to-run bound of test_gpu_interp.py::test_grid_matches_golden).  The numerical tests of the
modules hold the values themselves; this file holds that they do not depend on what the memory held before.

Where a case names scratch slots, those are the slots the call is documented to use; they must hold bytes after the call.
A module fixture makes the context hold one slot (10) before the first case, so no run is without poisoned scratch.  For
the calls that work wholly in place (logconv, fft_c2c, spec_mul_real, faraday_pack, faraday_rotate, and the accumulating
forms: normal_rows_pcg64 and pointsource_paint with accumulate, za_density_sph / _grid) nothing is allocated and the data
is ``inout``: the scratch of the context - for those that take no slot of their own, that foreign slot alone - is ALL that
is poisoned (``_run(..., inplace=True)``).  Every other case must also have poisoned at least one allocation.
Each case prints what was poisoned: ``label: byte -> (allocations, allocation bytes, scratch bytes)``.  Run with -m gpu."""
import numpy as np
import pytest

import _corrfunc_oracle as co
import _poison
from test_gpu_poison import _channels, _mk_cl

pytestmark = pytest.mark.gpu

_KEEP = {}


@pytest.fixture(scope="module", autouse=True)
def _a_slot_is_held(ctx):
    """One scratch slot (10, 64 KB) exists before the first case, so that a case run on its own poisons scratch too."""
    import torch

    ctx.complex_variance(torch.ones(3, dtype=torch.complex128, device=ctx.device))


def _run(ctx, label, call, inplace=False, **kw):
    """``inplace``: the call works wholly in place (nothing allocated; poisoned: the scratch of the context alone)."""
    ref, report = _poison.poisoned_runs(ctx, call, label=label, **kw)
    print("%s: %s" % (label, ", ".join("0x%02X -> %r" % (b, report[b]) for b in sorted(report))))
    for b, (nalloc, nbytes, sbytes) in report.items():
        assert sbytes > 0 and (nalloc == 0) == (nbytes == 0), (label, hex(b), report[b])
        assert nalloc > 0 or inplace, (label, hex(b), "no allocation was poisoned", report[b])
    return ref


def _rng(seed):
    return np.random.default_rng(seed)


def _randn(ctx, shape, seed, complex_=False):
    r = _rng(seed)
    a = r.standard_normal(shape)
    if complex_:
        import torch

        return torch.from_numpy(a + 1j * r.standard_normal(shape)).to(ctx.device)
    return ctx.to_device(a)


def _alm_dev(ctx, lmax, nnu, seed):
    """alm_dev [nalm, ceil(nnu / 4), 2, 4] with defined (zero) padding lanes and real m = 0 entries."""
    L = lmax + 1
    nalm = L * (L + 1) // 2
    G = (nnu + 3) // 4
    a = _rng(seed).standard_normal((nalm, G, 2, 4))
    a[:L, :, 1, :] = 0.0
    lane = np.arange(4 * G).reshape(G, 4)
    a *= (lane < nnu)[None, :, None, :]
    return ctx.to_device(a)


# ---------------------------------------------------------------- K1 ----------------------------------------------------
def _model(ctx):
    """The package's 21cm model with its device tables built once, and the raw K1 arguments at F = 5, lmax 20, zromb 1."""
    if "m21" not in _KEEP:
        from cora_amd.signal import corr21cm

        m = corr21cm.Corr21cm()
        freq = 600.0 + 2.0 * np.arange(5)
        zint = 3
        half = 1.0
        za = (freq[:, None] + np.linspace(-half, half, zint)[None, :]).flatten()
        p = m._table_plan(lambda x: 1420.40575177 / x - 1.0)["prepare"](ctx, za)
        d = ctx.to_device
        from cora_amd.core import skysim

        larr = np.arange(21.0)
        args = (p["kperpmin"], p["kperpmax"], p["kparmax"], d(p["chi"]), d(p["pfd"]), d(p["f"]), d(p["b"]), 5, zint,
                d(skysim.romberg_weights(1)), d(np.log10(np.where(larr == 0.0, 1e-10, larr))))
        _KEEP["m21"] = (m, freq, (p["dd"], p["dv"], p["vv"]), args)
    return _KEEP["m21"]


def test_k1_clarray_21cm_with_pinned_tables(ctx, model21):
    """skysim.clarray_device of the 21cm model (its tables pinned: K1 keeps the transposed copy in slot 0 between calls
    and the hook marks that copy invalid); the byte-0 result is the oracle model's C_l to the parity tests' 1e-11."""
    from cora_amd.core import skysim
    from oracle import skysim as osk

    m, freq, _, _ = _model(ctx)
    ref = _run(ctx, "clarray pinned", lambda: skysim.clarray_device(m.angular_powerspectrum, 20, freq, zromb=1), slots=(0, 1, 2))
    want = osk.clarray(model21.angular_powerspectrum, 20, freq, zromb=1)
    assert np.abs(ref[0].cpu().numpy() - want).max() <= 1e-11 * np.abs(want).max()


def test_k1_clarray_21cm_without_pin(ctx):
    m, freq, tabs, args = _model(ctx)
    ctx.unpin_tables(0)
    try:
        _run(ctx, "clarray unpinned", lambda: ctx.clarray_table21cm(*tabs, *args), slots=(0, 1, 2))
    finally:
        m._tables_on(ctx)                                            # the model's pin, as the model makes it


def test_k1_pair_shards_of_two_ranks(ctx):
    import torch

    _, _, tabs, args = _model(ctx)
    nl, W, lb = 21, 2, 11

    def call():
        slabs = [ctx.clarray_table21cm_pairs(*tabs, *args, r, W, lb, nblocks=W) for r in range(W)]
        parts = [ctx.clarray_pairs_finish(torch.stack([slabs[r][q] for r in range(W)]), 5, min(nl, (q + 1) * lb) - q * lb)
                 for q in range(W)]
        return torch.cat(parts)

    ref = _run(ctx, "pair shards W=2", call, slots=(0, 2))
    assert torch.equal(ref[0], ctx.clarray_table21cm(*tabs, *args))


def test_k1_separable_romb_reduce_aps_points(ctx):
    import _clarray_oracle as clo

    r = _rng(11)
    F, zint, nl = 5, 3, 7
    w = ctx.to_device(clo.make_case(F + zint, F=1, zint=zint, chan=[300.0], half=0.1, log10l=clo.log10l_range(1))["w"])
    al, bcov = ctx.to_device(r.standard_normal(nl)), ctx.to_device(r.standard_normal((F * zint, F * zint)))
    X = ctx.to_device(r.standard_normal((nl, F, zint, F, zint)))
    _run(ctx, "clarray_separable", lambda: ctx.clarray_separable(al, bcov, F, zint, w))
    _run(ctx, "romb_reduce", lambda: ctx.romb_reduce(X, nl, F, zint, w))
    c = clo.case("interior_z3")
    pts = [ctx.to_device(v) for v in clo.make_points(c, 401, 5)]
    d = ctx.to_device
    tabs = (d(c["dd"]), d(c["dv"]), d(c["vv"]))
    _run(ctx, "aps_table21cm_points",
         lambda: ctx.aps_table21cm_points(*tabs, c["kperpmin"], c["kperpmax"], c["kparmax"], *pts))


@pytest.mark.parametrize("n", [106, 1156])
def test_k0_dct1_rows(ctx, n):
    """In place on ``data`` (inout); the prime-factor passes run in the cached workspace of the context."""
    x = _rng(n).standard_normal((5, n)) * np.exp(-np.arange(n) / (0.3 * n))
    data = ctx.to_device(x)
    ctx.workspace(1 << 16)
    _run(ctx, "dct1_rows n=%d" % n, lambda: ctx.dct1_rows(data, 0.25), inout=(data,))


def test_k0_device_build_of_the_21cm_tables(ctx):
    """The device build (spline P(k) grid, mu^2 / mu^4, DCT-I along k_par) at 5 x 1156 instead of 500 x 32768."""
    from cora_amd.signal import corr21cm

    cr = corr21cm.Corr21cm()
    cr.nkperp, cr.nkpar = 5, 1156

    def call():
        cr._drop_dev_tables()
        cr._build_tables(ctx)
        return cr._dev_tables[ctx.device.index]

    ref = _run(ctx, "21cm table build", call)
    assert tuple(ref[0].shape) == (5, 1156)
    cr._drop_dev_tables()


# ---------------------------------------------------------------- K2 ----------------------------------------------------
@pytest.mark.parametrize("F", [5, 33, 70])
def test_k2_factor_batched(ctx, F):
    """Positive definite blocks, the zero l = 0 block and the indefinite l = 3 block (eigen route: its per-call list and
    scratch are poisoned by the hook); T and info are fresh allocations."""
    Cd = ctx.to_device(_mk_cl(F, 6, F))
    ref = _run(ctx, "factor_batched F=%d" % F, lambda: ctx.factor_batched(Cd))
    info = ref[1].cpu().numpy()
    assert info[0] != 0 and info[3] != 0 and not info[[1, 2, 4, 5]].any()


def test_k2_cooperative_route(ctx, monkeypatch):
    """F = 384, every matrix through the cooperative kernel (CORAHIP_K2_COOP=2, as
    test_k2_cooperative_kernel_matches_one_workgroup_form forces it): barrier words and panel exchange in slot 8."""
    import torch

    F, nl = 384, 3
    G = ((F + 31) // 32 + 3) // 4
    assert (nl + 7) // 8 * 8 * G <= torch.cuda.get_device_properties(ctx.device).multi_processor_count
    r = _rng(384)
    A = r.standard_normal((nl, F, F + 3))
    Cd = ctx.to_device(A @ A.transpose(0, 2, 1) / F)
    monkeypatch.setenv("CORAHIP_K2_COOP", "2")
    ref = _run(ctx, "factor_batched cooperative", lambda: ctx.factor_batched(Cd), slots=(8,))
    assert not ref[1].any()


def test_k2_matrix_root_manynull(ctx):
    from cora_amd.util import nputil

    r = _rng(9)
    A = r.standard_normal((7, 3))
    M = A @ A.T                                                      # rank 3 of 7: the eigen route

    def call():
        root, npos = nputil.matrix_root_manynull(M.copy())
        return np.ascontiguousarray(root), npos

    ref = _run(ctx, "matrix_root_manynull", call)
    assert int(ref[1]) == 3


# ------------------------------------------------------- K3 and generators ----------------------------------------------
def _factors(ctx, F, lmax):
    key = ("T", F, lmax)
    if key not in _KEEP:
        _KEEP[key] = ctx.factor_batched(ctx.to_device(_mk_cl(F, lmax + 1, 7 * F + lmax)))
    return _KEEP[key]


@pytest.mark.parametrize("F,lmax,nu0,nnu", [(34, 40, 0, 34), (7, 33, 2, 5), (136, 130, 0, 136)])
def test_k3_draw_alm_and_philox(ctx, F, lmax, nu0, nnu):
    """(34, 40): one column group; (7, 33, channels 2 .. 6): odd F, whose Philox stream is materialised in slot 1; (136, 130):
    two column groups and two m blocks.  Compared: the valid channels (test_gpu_poison.py:68, _channels: the padding
    lanes of alm_dev are not part of the result)."""
    T, info = _factors(ctx, F, lmax)
    g = ctx.normals_philox(77, lmax, F)
    _run(ctx, "draw_alm F=%d" % F, lambda: _channels(ctx.draw_alm(T, info, g, lmax, F, nu0, nnu), nnu), slots=(3,))
    _run(ctx, "draw_alm_philox F=%d" % F, lambda: _channels(ctx.draw_alm_philox(T, info, 77, lmax, F, nu0, nnu), nnu),
         slots=(1, 3) if F % 2 else (3,))


def test_k3_row_blocks_of_a_folded_shard(ctx):
    """F = 64, the folded pair of 8-channel chunks (8 .. 15, 48 .. 55): draw_alm_rows on the first, the chunk set on both."""
    import torch

    F, lmax = 64, 40
    T, info = _factors(ctx, F, lmax)
    g = ctx.normals_philox(78, lmax, F)
    rows8 = T[:, 8:16].contiguous()
    rows16 = torch.cat([T[:, 8:16], T[:, 48:56]], dim=1).contiguous()
    # (test_gpu_poison.py:68: valid channels only)
    _run(ctx, "draw_alm_rows", lambda: _channels(ctx.draw_alm_rows(rows8, info, g, lmax, F, 8, 8), 8))
    _run(ctx, "draw_alm_philox_chunks",
         lambda: _channels(ctx.draw_alm_philox_chunks(rows16, info, 78, lmax, F, [(8, 8), (48, 8)]), 16))


def _pcg(seed):
    st = np.random.default_rng(seed).bit_generator.state["state"]
    return st["state"], st["inc"]


def _words(v):
    return [(int(v) >> s) & 0xFFFFFFFF for s in (96, 64, 32, 0)]


def _mt_words(state):
    return [np.asarray(state["state"]["key"], dtype=np.int64), int(state["state"]["pos"]), int(state["has_gauss"]),
            float(state["gauss"])]


N_NORMALS = 100003            # several generator blocks of either generator and a ragged last one


def test_generators_whole_stream(ctx):
    st, inc = _pcg(3)
    ref = _run(ctx, "normals_pcg64", lambda: ctx.normals_pcg64(st, inc, N_NORMALS), slots=(6,))
    want = np.random.Generator(np.random.PCG64(3)).standard_normal(4096)
    assert np.array_equal(ref[0][:4096].cpu().numpy(), want)
    leg = np.random.RandomState(5).get_state(legacy=False)

    def legacy():
        g, after = ctx.normals_legacy(leg, N_NORMALS)
        return g, _mt_words(after)

    ref = _run(ctx, "normals_legacy", legacy, slots=(6, 9))
    assert np.array_equal(ref[0][:4096].cpu().numpy(), np.random.RandomState(5).standard_normal(4096))


def test_generators_scaled_rows(ctx):
    st, inc = _pcg(4)
    scale = np.array([0.5, 2.0, 1e-3])
    off = np.array([2 * 33337 + 6, 1, 33337 + 5], dtype=np.int64)         # rows out of order, gaps between them
    size = 3 * 33337 + 11

    def write():
        out = ctx.empty((size,))                                      # poisoned; the gaps are not the call's to write
        nraw = ctx.normal_rows_pcg64(st, inc, scale, 33333, out, row_off=off)
        return [out[o:o + 33333] for o in off.tolist()], nraw         # every row whole, tails included

    _run(ctx, "normal_rows_pcg64 write", write, slots=(6,))

    def dense():
        out = ctx.empty((3, 33333))                                   # write mode: every element of out is written
        return out, ctx.normal_rows_pcg64(st, inc, scale, 33333, out)

    _run(ctx, "normal_rows_pcg64 write, dense", dense, slots=(6,))
    acc = _randn(ctx, (3, 33333), 41)
    _run(ctx, "normal_rows_pcg64 add", lambda: (acc, ctx.normal_rows_pcg64(st, inc, scale, 33333, acc, accumulate=True)),
         inplace=True, inout=(acc,), slots=(6,))


@pytest.mark.parametrize("kind", ["pcg64", "legacy"])
def test_k3_draw_alm_numpy_with_a_1kb_ring(ctx, kind):
    """numpy's own stream generated range by range through a 1 KB ring (slot 7; generator tables in slot 6, the MT19937
    position lists in slot 9); the generator state after the draw must not depend on the poison either."""
    F, lmax = 34, 40
    T, info = _factors(ctx, F, lmax)
    if kind == "pcg64":
        rng, slots, words = ("pcg64",) + _pcg(6), (6, 7), _words
    else:
        rng, slots, words = ("legacy", np.random.RandomState(6).get_state(legacy=False)), (6, 7, 9), _mt_words

    def call():
        alm, after = ctx.draw_alm_numpy(T, info, rng, lmax, F, ring_bytes=1024)
        return _channels(alm, F), words(after)                       # (test_gpu_poison.py:68: valid channels only)

    _run(ctx, "draw_alm_numpy " + kind, call, slots=slots)


def test_alm_layout_conversions(ctx):
    """nnu = 5: one full group and one with three padding lanes.  alm_packed_to_dev must write those lanes as zeros
    (compared); alm_dev_to_square writes every (l, m), also m > l."""
    import torch

    lmax, nnu = 9, 5
    nalm = (lmax + 1) * (lmax + 2) // 2
    packed = _randn(ctx, (nnu, nalm), 51, complex_=True)
    ref = _run(ctx, "alm_packed_to_dev", lambda: ctx.alm_packed_to_dev(packed, lmax))
    assert not ref[0][:, 1, :, 1:].any() and bool(ref[0][:, 1, :, 0].any())
    alm = ref[0]
    ref = _run(ctx, "alm_dev_to_square", lambda: ctx.alm_dev_to_square(alm, lmax, nnu))
    sq = ref[0][:, 0].abs()                                          # [nnu, l, m] (dev_to_square_kernel): m > l is zero
    low = torch.tril(torch.ones(sq.shape[1:], dtype=torch.bool, device=sq.device))
    assert bool(sq[:, low].all()) and not bool(sq[:, ~low].any())


def test_shared_slots_across_uses(ctx):
    """No hook: slot 1 serves the K1 pair results and the Philox stream of an odd-F draw (draw_philox materialises it
    there), slot 6 both numpy generators.  The draw's 2 F nalm doubles cover all of K1's npairs x nl pair results."""
    import torch

    _, _, tabs, args = _model(ctx)
    first = ctx.clarray_table21cm(*tabs, *args).clone()
    F, lmax = 7, 33
    T, info = _factors(ctx, F, lmax)
    k1_doubles, draw_doubles = (5 * 6 // 2) * 21, 2 * F * (lmax + 1) * (lmax + 2) // 2
    assert draw_doubles >= k1_doubles
    ctx.draw_alm_philox(T, info, 5, lmax, F)
    ctx.sync()
    assert ctx.debug_poison_scratch(-1)[1] >= 8 * draw_doubles        # (sizes only: byte < 0 fills nothing)
    assert torch.equal(ctx.clarray_table21cm(*tabs, *args), first)
    st, inc = _pcg(8)
    g0 = ctx.normals_pcg64(st, inc, N_NORMALS)[0].clone()
    ctx.normals_legacy(np.random.RandomState(8).get_state(legacy=False), N_NORMALS)
    assert torch.equal(ctx.normals_pcg64(st, inc, N_NORMALS)[0], g0)


# ------------------------------------------------------- xi -> C_l, P(k) -> xi -------------------------------------------
def test_xi_averages(ctx):
    """65 knots, F = 5; xi_multi_average with 3 functions keeps its spline records in slot 12 and writes the rows past nm
    as zeros (compared)."""
    d = ctx.to_device
    xs, ys, y2 = co.table(0, "max", 65)
    mu, xa, xw = co.bin_average_case(0, 5, 3)
    dev = [d(v) for v in (xs, ys, y2, mu, xa, xw)]
    _run(ctx, "xi_table_average",
         lambda: ctx.xi_table_average(dev[0], dev[1], dev[2], 0, co.X_T, co.F_T, dev[3], dev[4], dev[5], 5, 3))
    ky, ky2 = d(np.stack([ys, 0.5 * ys, -2.0 * ys])), d(np.stack([y2, 0.5 * y2, -2.0 * y2]))
    f_t = np.array([co.F_T, 0.5 * co.F_T, 2.0 * co.F_T])
    ref = _run(ctx, "xi_multi_average",
               lambda: ctx.xi_multi_average(dev[0], ky, ky2, 0, co.X_T, f_t, dev[3], dev[4], dev[5], 5, 3,
                                            nm_rows=len(mu) + 3), slots=(12,))
    assert not ref[0][len(mu):].any() and bool(ref[0][:len(mu)].any())


@pytest.mark.parametrize("nm,slots", [(21, (4, 5)), (32, (4,))])
def test_legendre_project(ctx, nm, slots):
    """nm = 21: Kp = 32, the operand is copied to slot 5 and padded with zero rows; nm = 32: xi is the operand itself."""
    mu, wt, xi = co.projection_case(10, 5, nm)
    xi = np.ascontiguousarray(xi)
    d = ctx.to_device
    mud, wtd, xid = d(mu), d(wt), d(xi)
    _run(ctx, "legendre_project nm=%d" % nm, lambda: ctx.legendre_project(mud, wtd, 9, xid), slots=slots)


def test_cl_blocks(ctx):
    F, L = 5, 7
    npair = F * (F + 1) // 2
    one, three = _randn(ctx, (L, npair), 61), _randn(ctx, (L, 3, npair), 62)
    _run(ctx, "cl_blocks 1", lambda: ctx.cl_blocks(one, F))
    _run(ctx, "cl_blocks 3", lambda: ctx.cl_blocks(three, F))


def test_pk2xi_kernels(ctx):
    import torch

    n = (1 << 5) + 1
    ka = np.logspace(-3, 1, n)
    dlk = np.log(ka[1] / ka[0])
    g = ctx.to_device(ka ** 4 * np.exp(-8.0 * ka))
    kad, r = ctx.to_device(ka), ctx.to_device(np.concatenate([[0.0], np.logspace(-1, 3, 256)]))
    _run(ctx, "sinc_romb", lambda: ctx.sinc_romb(g, kad, dlk, r))
    _run(ctx, "fftlog_phase", lambda: ctx.fftlog_phase(0.5, 700 * 0.05, 700))
    for N, split in ((105, (105, 1)), (105, (3, 35)), (700, None)):
        u = ctx.fftlog_phase(0.5, N * 0.05, N)
        data = torch.complex(ctx.to_device(_rng(N).standard_normal(N)), torch.zeros(N, dtype=torch.float64, device=ctx.device))
        _run(ctx, "logconv N=%d split=%r" % (N, split), lambda: ctx.logconv(data, u, split=split), inplace=True, inout=(data,))


def test_ps_to_corr_device_end_to_end(ctx):
    import _pk2xi_oracle as po
    from cora_amd.signal import corrfunc
    from test_gpu_pk2xi import E2E

    _run(ctx, "ps_to_corr_device", lambda: corrfunc.ps_to_corr_device(po.pk_pair, **E2E))


# ---------------------------------------------------------------- flat sky ----------------------------------------------
def test_flatsky_fft_c2c_every_axis(ctx):
    data = _randn(ctx, (5, 7, 9), 71, complex_=True)
    for axis in range(3):
        for inverse in (False, True):
            _run(ctx, "fft_c2c axis %d inverse %r" % (axis, inverse), lambda: ctx.fft_c2c(data, axis, inverse), inplace=True, inout=(data,))


@pytest.mark.parametrize("shape", [(5, 7, 9), (30, 20, 14), (128, 128)])
def test_flatsky_rfftn_irfftn(ctx, shape):
    """irfftn overwrites its spectrum (inout)."""
    import torch

    arr = _randn(ctx, shape, 72)
    ref = _run(ctx, "rfftn %r" % (shape,), lambda: ctx.rfftn(arr))
    spec = ref[0].clone()
    back = _run(ctx, "irfftn %r" % (shape,), lambda: ctx.irfftn(spec, last=shape[-1]), inout=(spec,))
    assert tuple(back[0].shape) == tuple(shape) and torch.equal(spec, ref[0])


def test_flatsky_random_fields_and_pointwise(ctx):
    import torch

    kw = ctx.to_device(np.abs(_rng(73).standard_normal((5, 7, 5))))
    _run(ctx, "randomfield_draw", lambda: ctx.randomfield_draw(kw, 9))
    _run(ctx, "randomfield_irfftn", lambda: ctx.randomfield_irfftn(kw, 9, last=9))
    _run(ctx, "randomfield_irfftn even", lambda: ctx.randomfield_irfftn(kw, 9))
    fw, nrm = _randn(ctx, (3, 2), 74), _randn(ctx, (2, 5, 7), 75)
    aff = _randn(ctx, (5, 7), 76, complex_=True)
    _run(ctx, "fg_mix", lambda: ctx.fg_mix(fw, nrm, aff))
    spec, wt = _randn(ctx, (5, 7, 5), 77, complex_=True), _randn(ctx, (5, 7, 5), 78)
    _run(ctx, "spec_mul_real", lambda: ctx.spec_mul_real(spec, wt), inplace=True, inout=(spec,))
    cube, vf = _randn(ctx, (7, 9, 11), 79), _randn(ctx, (7, 9, 11), 80)
    a, b, c = (_randn(ctx, (7,), s) for s in (81, 82, 83))
    _run(ctx, "cube_affine", lambda: ctx.cube_affine(cube, vf, a, b, c))
    _run(ctx, "cube_affine density", lambda: ctx.cube_affine(cube, None, a, b, c))
    # the shapes of test_raytrace_kernel_edges_and_affine: lines of sight that leave the box (exact zeros there)
    d = ctx.to_device
    zc = d(np.array([0.0, 0.3, 5.999, 6.0, 6.0000001, -1e-12, 3.5]))
    scale = d(np.array([1.0, 0.7, 1.3, 2.0, 1.0, 1.0, 2.5]))
    tx, ty = d(np.linspace(-0.5, 0.5, 6)), d(np.linspace(-0.5, 0.5, 5))
    ref = _run(ctx, "raytrace_slices", lambda: ctx.raytrace_slices(cube, zc, scale, tx, ty, 1.0, 1.0))
    assert not ref[0][4].any() and not ref[0][5].any() and bool(ref[0][3].any())


# ---------------------------------------------------------------- spectra -----------------------------------------------
@pytest.mark.parametrize("nx,ny", [(5, None), (130, 3), (6, 129)])
def test_alm_cross_spectra(ctx, nx, ny):
    lmax = 5                                                         # the smallest lmax of LMAXES with a tail in m
    a = _alm_dev(ctx, lmax, nx, 90 + nx)
    b = None if ny is None else _alm_dev(ctx, lmax, ny, 190 + ny)
    _run(ctx, "alm_cross_spectra %r" % ((nx, ny),), lambda: ctx.alm_cross_spectra(a, nx, lmax, b, ny))
    for lm in (0, 1):
        a = _alm_dev(ctx, lm, nx, 95 + lm)
        b = None if ny is None else _alm_dev(ctx, lm, ny, 195 + lm)
        _run(ctx, "alm_cross_spectra lmax %d %r" % (lm, (nx, ny)), lambda: ctx.alm_cross_spectra(a, nx, lm, b, ny))


# ---------------------------------------------------------------- LSS ---------------------------------------------------
def _za_fields(ctx, nside, nchi, seed):
    from test_gpu_lss import _fields

    return [ctx.to_device(a) for a in _fields(nside, nchi, seed, pix_shift=1.5)]


def test_lss_neighbours_and_densities(ctx):
    from cora_amd.signal import lss

    _run(ctx, "healpix_neighbours", lambda: ctx.healpix_neighbours(4))
    psi, db, dm, chi = _za_fields(ctx, 8, 3, 31)
    out = _randn(ctx, (3, 768), 32) * 0.1
    # both add into out (inout) with float atomics on global memory: the run-to-run bound of
    # test_gpu_interp.py::test_grid_matches_golden
    _run(ctx, "za_density_sph", lambda: lss.za_density_sph_device(psi, db, dm, chi, out), inplace=True, inout=(out,),
         criterion="global-atomics")
    _run(ctx, "za_density_grid", lambda: lss.za_density_grid_device(psi, db, dm, chi, out), inplace=True, inout=(out,),
         criterion="global-atomics")


def test_lss_gradients_and_displacement(ctx):
    from cora_amd.signal import lss
    from cora_amd.util import hputil

    f = _randn(ctx, (5, 1001), 33)
    x = np.array([800.0, 807.0, 816.5, 824.0, 833.0])
    _run(ctx, "radial_gradient", lambda: ctx.radial_gradient(f, x, scale=np.arange(1.0, 6.0)))
    nside, lmax, nf = 16, 20, 3
    alm = _alm_dev(ctx, lmax, nf, 34)
    # ends in the run-time ring kernel: "atomic"
    _run(ctx, "alm2map_der1", lambda: hputil.alm2map_der1_device(alm, nside, lmax, nf), criterion="atomic")
    phi = ctx.alm2map(alm, nside, lmax, nf).clone()
    chi = np.array([800.0, 808.0, 817.0])
    _run(ctx, "zeldovich_displacement",
         lambda: lss.zeldovich_displacement_device(phi, chi, np.array([1.0, 0.9, 0.8]), f=np.array([0.5, 0.6, 0.7]), lmax=lmax),
         criterion="atomic")


@pytest.mark.parametrize("n", [5, 33])
def test_lss_slice_mix(ctx, n):
    """ncol = 1001; a dense kernel and a banded one (blocks of 16 rows skip the slices outside their band)."""
    r = _rng(n)
    f = _randn(ctx, (n, 1001), 35 + n)
    dense = r.standard_normal((n, n))
    band = np.where(np.abs(np.subtract.outer(np.arange(n), np.arange(n))) <= 2, dense, 0.0)
    _run(ctx, "slice_mix dense n=%d" % n, lambda: ctx.slice_mix(dense, f))
    _run(ctx, "slice_mix banded n=%d" % n, lambda: ctx.slice_mix(band, f))
    _run(ctx, "slice_mix no ranges n=%d" % n, lambda: ctx.slice_mix(band, f, skip=False))


def test_lss_chain_pointwise(ctx):
    from cora_amd.signal import lss

    n, ncol = 5, 1001
    f, g, h = (_randn(ctx, (n, ncol), s) for s in (36, 37, 38))
    x = np.array([800.0, 807.0, 816.5, 824.0, 833.0])
    s, t = np.arange(1.0, 6.0), np.linspace(-1.0, 1.0, 5)
    _run(ctx, "slice_diff2", lambda: ctx.slice_diff2(f, x))
    _run(ctx, "slice_diff2 fused", lambda: ctx.slice_diff2(f, x, g=g, h=h, s=s, t=t))
    _run(ctx, "slice_diff2 no f", lambda: ctx.slice_diff2(None, None, g=g, h=h, s=s))
    _run(ctx, "slice_moments", lambda: ctx.slice_moments(f, c=np.linspace(-0.5, 0.5, n)))
    wide = _randn(ctx, (n, 4, ncol), 39)
    _run(ctx, "slice_moments strided", lambda: ctx.slice_moments(wide[:, 1]))
    _run(ctx, "bias_field", lambda: ctx.bias_field(f, s, c2=t, m2=np.full(n, 0.9)))
    _run(ctx, "bias_field linear", lambda: ctx.bias_field(f, s))
    _run(ctx, "lognormal", lambda: ctx.lognormal(f, np.full(n, 0.5), prefactor=2.0, row_scale=s))
    _run(ctx, "lognormal no transform", lambda: ctx.lognormal(f, None, row_scale=s))
    chi = np.array([800.0, 807.0, 816.5, 824.0, 833.0])
    _run(ctx, "fingers_of_god", lambda: lss.fingers_of_god_device(f, chi, 3.0, D=np.linspace(1.0, 0.8, n)))
    _run(ctx, "fingers_of_god banded", lambda: lss.fingers_of_god_device(f, chi, 0.2, band_cut=1e-8))


# ---------------------------------------------------------------- interpolation -----------------------------------------
def test_healpix_interpolation(ctx):
    """nside 4, 1001 directions including both poles, 3 maps."""
    r = _rng(40)
    theta = np.arccos(r.uniform(-1.0, 1.0, 1001))
    phi = r.uniform(0.0, 2.0 * np.pi, 1001)
    theta[:4] = (0.0, np.pi, 0.0, np.pi)
    phi[:4] = (0.0, 0.0, 5.0, 1.0)
    th, ph = ctx.to_device(theta), ctx.to_device(phi)
    maps = _randn(ctx, (3, 192), 41)
    _run(ctx, "healpix_interp_weights", lambda: ctx.healpix_interp_weights(4, th, ph))
    _run(ctx, "healpix_interp_val", lambda: ctx.healpix_interp_val(maps, th, ph))
    c, s = np.cos(0.3), np.sin(0.3)
    R = np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]]) @ np.array([[1.0, 0.0, 0.0], [0.0, c, -s], [0.0, s, c]])
    _run(ctx, "healpix_rotate_maps", lambda: ctx.healpix_rotate_maps(maps, R))


# ---------------------------------------------------------------- Faraday -----------------------------------------------
@pytest.mark.parametrize("count", [1, 257, 70001])
def test_faraday_complex_variance(ctx, count):
    y = _randn(ctx, (count,), 42, complex_=True)
    _run(ctx, "complex_variance %d" % count, lambda: ctx.complex_variance(y), slots=(10,))


def test_faraday_pack_and_mix(ctx):
    """faraday_pack writes columns k0 .. k0 + R / 2 - 1 of y and leaves the others (inout); faraday_mix at the smallest
    shape of test_gpu_faraday.py, both output forms."""
    import torch
    from test_gpu_faraday import SHAPES, _grid

    R, npix, nphi = 5, 48 * 3 + 1, 8
    maps = _randn(ctx, (2 * R, npix), 43)
    y = _randn(ctx, (npix, nphi), 44, complex_=True)
    _run(ctx, "faraday_pack", lambda: ctx.faraday_pack(maps, y, 2), inplace=True, inout=(y,))
    ncol, nphi, nfreq = min(SHAPES, key=lambda s: s[0] * s[1] * s[2])
    r = _rng(45)
    yy = _randn(ctx, (ncol, nphi), 46, complex_=True)
    A = torch.from_numpy(np.exp(1j * r.uniform(0, 2 * np.pi, (nfreq, nphi)))).to(ctx.device)
    phi, sigma = _grid(nphi), r.uniform(0.5, 3.0, ncol)
    inten = ctx.to_device(r.uniform(1.0, 2.0, (nfreq, ncol)))
    _run(ctx, "faraday_mix", lambda: ctx.faraday_mix(yy, phi, sigma, A, 0.3))
    _run(ctx, "faraday_mix intensity", lambda: ctx.faraday_mix(yy, phi, sigma, A, 0.3, intensity=inten))


# ---------------------------------------------------------------- point sources -----------------------------------------
def test_pointsource_population(ctx):
    from test_gpu_pointsource import _spline

    m, xs, ys, y2 = _spline()
    _run(ctx, "pointsource_population",
         lambda: ctx.pointsource_population(12, 1001, xs, ys, y2, m.flux_min, m.spectral_mean, m.spectral_width, 192,
                                            interval=True))


@pytest.mark.parametrize("n", [0, 37])
def test_pointsource_paint(ctx, n):
    """nside 4, F = 3, the sources on five pixels: without accumulate EVERY pixel is written (per-pixel offsets in slot
    11); with accumulate ``out`` is added to (inout)."""
    r = _rng(47 + n)
    npix = 192
    pix = np.sort(r.choice(np.array([0, 7, 100, 190, 191]), n)).astype(np.int64)
    flux, beta, gamma = r.uniform(0.1, 5.0, n), r.normal(-0.7, 0.2, n), r.normal(0.0, 0.05, n)
    polw = r.uniform(-0.1, 0.1, (n, 2))
    x, den = np.log(np.array([0.9, 1.0, 1.1])), np.array([1.2, 1.0, 0.8])
    import torch

    pd = torch.from_numpy(pix).to(ctx.device)
    _run(ctx, "pointsource_paint n=%d" % n, lambda: ctx.pointsource_paint(pd, flux, beta, x, den, 2.0, npix, gamma=gamma),
         slots=(11,))
    _run(ctx, "pointsource_paint pol n=%d" % n,
         lambda: ctx.pointsource_paint(pd, flux, beta, x, den, 2.0, npix, gamma=gamma, polw=polw, npol=4), slots=(11,))
    acc = _randn(ctx, (3, npix), 48)
    _run(ctx, "pointsource_paint accumulate n=%d" % n,
         lambda: ctx.pointsource_paint(pd, flux, beta, x, den, 2.0, npix, out=acc, accumulate=True), inplace=True, inout=(acc,), slots=(11,))


def test_pointsource_polarisation_and_grading(ctx):
    r = _rng(49)
    F, npix = 3, 192
    inten = _randn(ctx, (F, npix), 50)
    q, u, rm = r.uniform(-0.1, 0.1, npix), r.uniform(-0.1, 0.1, npix), r.normal(0, 30.0, npix)
    wv = np.array([0.5, 0.45, 0.4])
    _run(ctx, "polarise_rotate", lambda: ctx.polarise_rotate(inten, q, u, wv=wv, rm=rm))
    _run(ctx, "polarise_rotate no rm", lambda: ctx.polarise_rotate(inten, q, u))
    pol = _randn(ctx, (F, 4, npix), 52)
    _run(ctx, "faraday_rotate", lambda: ctx.faraday_rotate(pol, rm, wv), inplace=True, inout=(pol,))
    _run(ctx, "healpix_ud_grade up", lambda: ctx.healpix_ud_grade(inten, 8))
    _run(ctx, "healpix_ud_grade down", lambda: ctx.healpix_ud_grade(inten, 2))


# ---------------------------------------------------------------- galaxy and constrained --------------------------------
def test_galaxy_kernels(ctx):
    r = _rng(53)
    npix = 192
    maps = _randn(ctx, (3, npix), 54)
    _run(ctx, "healpix_reorder r2n", lambda: ctx.healpix_reorder(maps, True))
    _run(ctx, "healpix_reorder n2r", lambda: ctx.healpix_reorder(maps, False))
    _run(ctx, "healpix_block_variance", lambda: ctx.healpix_block_variance(maps, 2))
    _run(ctx, "healpix_block_variance same nside", lambda: ctx.healpix_block_variance(maps, 4))
    lmax, nnu = 9, 5
    alm = _alm_dev(ctx, lmax, nnu, 55)
    fl = r.uniform(0.5, 1.5, (nnu, lmax + 1))
    _run(ctx, "alm_scale_l", lambda: ctx.alm_scale_l(alm, lmax, fl))
    _run(ctx, "alm_scale_l one row", lambda: ctx.alm_scale_l(alm, lmax, fl[0]))
    nchan = 5
    fg, fgs = _randn(ctx, (nchan, npix), 56), _randn(ctx, (nchan, npix), 57)
    haslam, sc, am = r.uniform(10.0, 50.0, npix), r.normal(-2.8, 0.1, npix), r.uniform(0.5, 2.0, npix)
    efreq = np.array([408.0, 1420.0, 600.0, 650.0, 700.0])
    _run(ctx, "galaxy_combine", lambda: ctx.galaxy_combine(fg, fgs, haslam, sc, am, 1.7, efreq))


def test_constrained_kernels(ctx):
    """eig_top_batched by the block iteration (MFMA) and, with max_iter = 1, by the full Jacobi decomposition, whose
    per-call list and scratch the hook poisons; constrained_weights; alm_mix_l at (k 3, F 18, lmax 5), whose padding lanes
    are zero (compared)."""
    import torch

    F, L, k = 18, 6, 3
    C = ctx.to_device(_mk_cl(F, L, 58)[:, :, :] + 0.0)
    C[0] = torch.eye(F, dtype=torch.float64, device=ctx.device) * torch.arange(1.0, F + 1.0, device=ctx.device, dtype=torch.float64)
    C[3] = C[2] * 2.0
    ref = _run(ctx, "eig_top_batched", lambda: ctx.eig_top_batched(C, k))
    jac = _run(ctx, "eig_top_batched max_iter=1", lambda: ctx.eig_top_batched(C, k, max_iter=1))
    print("eig_top routes: default %r, max_iter = 1 %r" % (ref[2].tolist(), jac[2].tolist()))
    assert not ref[2].all() and bool(jac[2].any())                   # both routes ran
    V = ref[0]
    W = _run(ctx, "constrained_weights", lambda: ctx.constrained_weights(V, np.array([2, 9, 17])))[0]
    assert not W[0].any()
    alm = _alm_dev(ctx, 5, k, 59)
    mixed = _run(ctx, "alm_mix_l", lambda: ctx.alm_mix_l(alm, 5, W))[0]
    assert tuple(mixed.shape) == (21, 5, 2, 4) and not mixed[:, 4, :, 2:].any()


# ---------------------------------------------------------------- sharding ----------------------------------------------
def test_factor_rows_pack_unpack(ctx):
    """world 2, F = 8: the l rows past n_local of every slab are zeros (compared)."""
    F, world, counts = 8, 2, [3, 2]
    T = _randn(ctx, (3, F, F), 60)
    ref = _run(ctx, "factor_rows_pack", lambda: ctx.factor_rows_pack(T, 4, world))
    assert not ref[0][:, 3:].any()
    recv = _randn(ctx, (world, 3, F // world, F), 61)
    _run(ctx, "factor_rows_unpack", lambda: ctx.factor_rows_unpack(recv, counts))
