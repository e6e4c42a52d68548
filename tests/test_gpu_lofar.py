"""The LOFAR synchrotron model on the GPU (csrc/lofar.hip, cora_amd.foreground.lofar) against tests/_lofar_oracle.py: the
line-of-sight kernel and the field moments against their longdouble values within the bounds derived there (printed as
err / bound), the channel-subset invariance of the kernel bit for bit, the class against the reference's own maps
(tests/golden/lofar_vectors.npz) and against the oracle on the device's own fields, and both entry points on poisoned
outputs and scratch."""
import functools

import numpy as np
import pytest

import _lofar_oracle as lo
import _poison

pytestmark = pytest.mark.gpu

LD, U = lo.LD, lo.U

# (nfreq, ncol, nz), beta is A
KERNEL_CASES = [((1, 1, 1), False), ((3, 7, 6), False), ((3, 7, 6), True), ((5, 63, 10), False), ((5, 65, 10), False),
                ((5, 65, 10), True), ((70, 31, 33), False), ((3, 70, 1000), False), ((2, 5, 4), False)]
SCALES = dict(a0=0.3, sa=1.0, b0=-2.55, sb=0.3)


@functools.lru_cache(maxsize=None)
def kernel_inputs(shape, alias):
    """(A, beta, x) for a kernel case: normal fields (so that a = 0.3 + A is negative for a third of them), x of both
    signs; the (2, 5, 4) case has x = 0 in its first channel."""
    nfreq, ncol, nz = shape
    rng = np.random.default_rng(1000 * nfreq + 10 * ncol + nz)
    A = rng.standard_normal((ncol, nz))
    beta = A if alias else rng.standard_normal((ncol, nz))
    x = np.array([0.0, 0.5]) if shape == (2, 5, 4) else (np.array([-0.9]) if nfreq == 1 else np.linspace(-0.9, 0.7, nfreq))
    return A, beta, x


@functools.lru_cache(maxsize=None)
def kernel_reference(shape, alias):
    A, beta, x = kernel_inputs(shape, alias)
    return lo.los(A, beta, x, **SCALES)


def _device_fields(ctx, A, beta):
    dA = ctx.to_device(A)
    return dA, (dA if beta is A else ctx.to_device(beta))


@pytest.mark.parametrize("shape,alias", KERNEL_CASES)
def test_powerlaw_los_against_oracle(ctx, shape, alias):
    import torch

    A, beta, x = kernel_inputs(shape, alias)
    ref, bound = kernel_reference(shape, alias)
    dA, dB = _device_fields(ctx, A, beta)
    out = torch.full((shape[0], shape[1]), float("nan"), dtype=torch.float64, device=ctx.device)
    got = ctx.powerlaw_los(dA, dB, x, out=out, **SCALES)
    assert got is out and torch.equal(dA.cpu(), torch.from_numpy(A))            # the raw field is not rewritten
    got = got.cpu().numpy()
    assert np.isfinite(got).all()
    err = np.abs(got.astype(LD) - ref)
    print("powerlaw_los %r%s: max err / bound %.3g" % (shape, " (beta is A)" if alias else "", lo.worst(err, bound)))
    assert (0.3 + A).min() < 0 or shape == (1, 1, 1)
    assert np.all(err <= bound)
    if shape == (2, 5, 4):
        # x = 0: exp gives 1 exactly and the fma adds a_z unrounded, so the channel is the ordered sum of the scaled A
        a = 0.3 + 1.0 * A
        s = np.zeros(shape[1])
        for z in range(shape[2]):
            s = s + a[:, z]
        assert np.array_equal(got[0], s)
    # the same bits from call to call
    assert np.array_equal(ctx.powerlaw_los(dA, dB, x, **SCALES).cpu().numpy(), got)


@pytest.mark.parametrize("shape,subsets", [((5, 65, 10), ([2], [0, 2, 4])), ((70, 31, 33), ([2], [0, 2, 4], [33, 69]))])
def test_channel_subset_invariance(ctx, shape, subsets):
    A, beta, x = kernel_inputs(shape, False)
    dA, dB = _device_fields(ctx, A, beta)
    full = ctx.powerlaw_los(dA, dB, x, **SCALES).cpu().numpy()
    for sub in subsets:
        part = ctx.powerlaw_los(dA, dB, x[sub], **SCALES).cpu().numpy()
        assert part.shape == (len(sub), shape[1]) and np.array_equal(part, full[sub]), sub


MOMENT_CASES = [((7, 6), 0.0), ((65, 10), 0.0), ((70, 1000), 0.0), ((70, 1000), 64.0)]


@pytest.mark.parametrize("shape,offset", MOMENT_CASES)
def test_field_moments_against_oracle(ctx, shape, offset):
    rng = np.random.default_rng(shape[0] + shape[1])
    f = offset + rng.standard_normal(shape)
    cond = lo.moments_condition(f)
    print("field_moments %r offset %g: conditions of the bound (<= 1) %s" % (shape, offset, ", ".join("%.3g" % c for c in cond)))
    assert max(cond) <= 1.0
    want, rel = lo.moments(f)
    d = ctx.to_device(f)
    got = ctx.field_moments(d)
    r = [abs(LD(got[i]) - want[i]) / (rel * want[i]) for i in (0, 1)]
    print("field_moments %r offset %g: err / bound  column sums %.3g  elements %.3g" % (shape, offset, r[0], r[1]))
    assert max(r) <= 1.0
    assert got[2] == float(want[2]) == np.abs(f).max()
    assert ctx.field_moments(d) == got
    assert ctx.field_moments(d.reshape(shape[0], 1, shape[1]))[1:] == got[1:]


def _model(par, correlated=None):
    from cora_amd.foreground import lofar

    m = lofar.LofarGDSE()
    for k in ("nu_num", "x_num", "y_num", "x_width", "y_width", "nu_lower", "nu_upper"):
        setattr(m, k, par[k])
    m.correlated = par["correlated"] if correlated is None else correlated
    return m


def _scale_rel(A):
    # a device standard deviation ((n + 3) u), the division by it and the product or quotient before it
    return (A.size + 3) * U + 2 * U


@pytest.fixture(scope="module")
def gold():
    return lo.load_golden()


@pytest.mark.parametrize("tag", lo.CASES)
def test_class_matches_reference_maps(ctx, gold, tag):
    """seed=None: numpy's global stream, as the reference draws.  The device FFT differs from numpy's in rounding, by up to
    the project's field tolerance (1e-13 max|field|): the bound is that perturbation carried through the two rescalings
    and the sum (_lofar_oracle.propagate, from the golden's own fields) plus the kernel's bound."""
    par, A, beta, Tb = lo.golden_case(gold, tag)
    attrs = lo.golden_attrs(gold)
    m = _model(par)
    np.random.seed(7)
    got = m.getfield()
    assert got.shape == Tb.shape and got.dtype == np.float64
    _, x, sc = lo.model(A, beta, par, attrs)
    _, kbound = lo.los(A, beta, x, *sc)
    prop = lo.propagate(A, beta, x, sc, eps_a=lo.FIELD_TOL * np.abs(A).max(), eps_b=lo.FIELD_TOL * np.abs(beta).max(),
                        rel_sa=_scale_rel(A), rel_sb=_scale_rel(A), rel_x=2 * U)
    bound = (prop + kbound).reshape(Tb.shape)
    err = np.abs(got.astype(LD) - Tb)
    print("LofarGDSE %s against the reference's map: max err / bound %.3g (max |diff| / max |Tb| = %.3g)"
          % (tag, lo.worst(err, bound), float(err.max() / np.abs(Tb).max())))
    assert np.all(err <= bound)


def test_class_integer_seed(ctx, gold):
    par, _, _, _ = lo.golden_case(gold, "c5_12_9")
    attrs = lo.golden_attrs(gold)
    m = _model(par, correlated=False)
    a = m.getfield(seed=3)
    assert a.shape == (5, 12, 9) and np.isfinite(a).all() and np.array_equal(m.getfield(seed=3), a)
    assert not np.array_equal(m.getfield(seed=4), a)
    mc = _model(par, correlated=True)
    c = mc.getfield(seed=3)
    assert np.array_equal(mc.getfield(seed=3), c) and not np.array_equal(c, a)
    for mod, tb in ((m, a), (mc, c)):
        dA, dB, numz = mod._fields_device(3)
        assert numz == 10 and tuple(dA.shape) == (12, 9, 10) and (dB is dA) == mod.correlated
        A = dA.cpu().numpy()
        B = A if dB is dA else dB.cpu().numpy()
        assert mod.correlated or not np.array_equal(A, B)
        assert np.array_equal(mod._los_device(dA, dB, numz).cpu().numpy(), tb)
        ref, x, sc = lo.model(A, B, dict(par, correlated=mod.correlated), attrs)
        _, kbound = lo.los(A, B, x, *sc)
        prop = lo.propagate(A, B, x, sc, rel_sa=_scale_rel(A), rel_sb=_scale_rel(A), rel_x=2 * U)
        bound = (prop + kbound).reshape(tb.shape)
        err = np.abs(tb.astype(LD) - ref)
        print("LofarGDSE seed=3 correlated=%s against the oracle on the device's fields: max err / bound %.3g"
              % (mod.correlated, lo.worst(err, bound)))
        assert np.all(err <= bound)


def test_default_shape(ctx):
    from cora_amd.foreground import lofar

    np.random.seed(1)
    tb = lofar.LofarGDSE().getfield()
    assert tb.shape == (128, 128, 128) and np.isfinite(tb).all() and tb.min() > 0


def test_argument_errors(ctx):
    import torch

    from cora_amd import _lib

    A, beta, x = kernel_inputs((5, 65, 10), False)
    dA, dB = _device_fields(ctx, A, beta)
    with pytest.raises(ValueError, match="must stay below 512"):
        ctx.powerlaw_los(dA, dB, x * 1000.0, **SCALES)
    with pytest.raises(ValueError, match="must stay below 512"):
        ctx.powerlaw_los(dA, dB, x, a0=0.3, sa=1.0, b0=0.0, sb=1e4)
    with pytest.raises(ValueError, match="expected"):
        ctx.powerlaw_los(dA, dB[:64], x)
    with pytest.raises(ValueError, match="out overlaps"):
        ctx.powerlaw_los(dA, dB, x[:2], out=dA.reshape(-1)[:130].reshape(2, 65))
    with pytest.raises(ValueError, match="float64"):
        ctx.field_moments(dA.float())
    # the C entry points refuse before any launch
    lib, h = ctx.lib, ctx.h
    out = ctx.empty((5, 65))
    dx = ctx.to_device(x)
    p = lambda t: _lib.c_void_p(t.data_ptr())  # noqa: E731
    for nfreq, ncol, nz in ((0, 65, 10), (5, 0, 10), (5, 65, 0)):
        assert lib.corahip_powerlaw_los(h, p(dA), p(dB), p(dx), 0.0, 1.0, 0.0, 1.0, nfreq, ncol, nz, p(out)) == -1
    assert lib.corahip_powerlaw_los(h, p(dA), p(dB), p(dx), 0.0, 1.0, 0.0, 1.0, 2, 65, 10, p(dB)) == -1
    assert lib.corahip_powerlaw_los(h, p(dA), p(dB), p(dx), 0.0, 1.0, 0.0, 1.0, 5, 65, 10, p(dx)) == -1
    assert lib.corahip_field_moments(h, p(dA), 0, 10, p(out)) == -1
    assert lib.corahip_field_moments(h, p(dA), 65, 10, p(dA)) == -1
    torch.cuda.synchronize()


def _report(label, report):
    print("%s: %s" % (label, ", ".join("0x%02X -> %r" % (b, report[b]) for b in sorted(report))))


def test_poison_powerlaw_los(ctx):
    rng = np.random.default_rng(9)
    A, B = ctx.to_device(rng.standard_normal((70, 37))), ctx.to_device(rng.standard_normal((70, 37)))
    x = ctx.to_device(np.linspace(-0.9, 0.7, 37))
    _, report = _poison.poisoned_runs(ctx, lambda: ctx.powerlaw_los(A, B, x, beta_absmax=8.0, **SCALES), criterion="exact",
                                      label="powerlaw_los")
    _report("powerlaw_los", report)
    assert all(nalloc > 0 for nalloc, _, _ in report.values())


def test_poison_field_moments(ctx):
    f = ctx.to_device(np.random.default_rng(10).standard_normal((70, 37)))
    _, report = _poison.poisoned_runs(ctx, lambda: ctx.field_moments(f), criterion="exact", slots=(10,), label="field_moments")
    _report("field_moments", report)
    assert all(nalloc > 0 and sbytes > 0 for nalloc, _, sbytes in report.values())
