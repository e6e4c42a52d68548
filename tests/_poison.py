"""Poison harness for the entry points outside the SHT (the cases: test_gpu_poison_modules.py; self-test on the host:
test_poison_harness_host.py).

Outputs and Python-side workspaces of the front end come from ``torch.empty``, and the library keeps grow-only scratch
slots in the context that are never cleared.  A kernel that skips part of an output, or reads a workspace or scratch cell
before it has written it, sees whatever was there: in a test process very often zero, and zero is usually the right
answer for exactly those cells.  Here a call runs three times - with every such byte 0, then 0xFF (every f64 a NaN,
every int32 -1), then 0x7E (every f64 ~2^1000, finite: what a fmax / compare-select would let through where it drops
a NaN) - and passes only if the poisoned results are finite and equal to the byte-0 one.  The criteria are those of
test_gpu_poison.py plus the run-to-run bound of test_gpu_interp.py::test_grid_matches_golden; no other tolerance."""
import contextlib

from test_gpu_poison import POISONS

CRITERIA = ("exact", "atomic", "global-atomics")


class PoisonStats:
    """What one ``poisoned_allocations`` block filled: ``allocations`` tensors of ``bytes`` bytes in all (the cached
    workspace of the context, if there is one, counts as one of them)."""

    def __init__(self):
        self.allocations = 0
        self.bytes = 0


def _fill_storage(torch, empty, t, byte):
    """Every byte of the storage behind ``t`` <- byte (any dtype, any strides); returns the bytes filled."""
    st = t.untyped_storage()
    n = int(st.nbytes())
    if n:
        empty(0, dtype=torch.uint8, device=t.device).set_(st, 0, (n,)).fill_(byte)
    return n


@contextlib.contextmanager
def poisoned_allocations(ctx, byte):
    """For the duration of the block ``torch.empty``, ``torch.empty_like``, ``torch.empty_strided`` and
    ``Tensor.new_empty`` return tensors filled with ``byte`` when they are on ``ctx.device`` or in pinned host memory
    (other devices pass through untouched), and the cached workspace of the context is filled once at entry.  Yields the
    PoisonStats of the block.  The four names are restored on exit, also when the block raises."""
    import torch

    dev = torch.device(ctx.device)
    stats = PoisonStats()
    orig = {"empty": torch.empty, "empty_like": torch.empty_like, "empty_strided": torch.empty_strided}
    orig_new_empty = torch.Tensor.new_empty

    def poison(t):
        if isinstance(t, torch.Tensor) and t.layout == torch.strided:
            pinned = t.device.type == "cpu" and dev.type != "cpu" and t.is_pinned()
            if t.device == dev or pinned:
                n = _fill_storage(torch, orig["empty"], t, byte)
                if n:
                    stats.allocations += 1
                    stats.bytes += n
        return t

    def wrap(fn):
        def poisoned(*args, **kwargs):
            return poison(fn(*args, **kwargs))

        poisoned.__name__ = getattr(fn, "__name__", "empty")
        return poisoned

    ws = getattr(ctx, "_workspace", None)
    try:
        for name, fn in orig.items():
            setattr(torch, name, wrap(fn))
        torch.Tensor.new_empty = wrap(orig_new_empty)
        if ws is not None:
            poison(ws)
        yield stats
    finally:
        for name, fn in orig.items():
            setattr(torch, name, fn)
        torch.Tensor.new_empty = orig_new_empty


def _flat(torch, r):
    """The result of a call as a list of tensors: tensors as they are, numbers and host arrays as CPU tensors."""
    if isinstance(r, torch.Tensor):
        return [r]
    if isinstance(r, (tuple, list)):
        return [t for x in r for t in _flat(torch, x)]
    return [torch.as_tensor(r)]


def _mag(t):
    return t.abs().double() if (t.is_complex() or t.is_floating_point()) else t.double().abs()


def _compare(torch, got, ref, criterion, tag):
    assert len(got) == len(ref), tag
    for i, (g, r) in enumerate(zip(got, ref)):
        assert g.shape == r.shape and g.dtype == r.dtype, (tag, i, g.shape, r.shape)
        assert bool(torch.isfinite(g).all()), (tag, i, "non-finite output")
        if criterion == "exact" or not (g.is_floating_point() or g.is_complex()) or g.numel() == 0:
            assert torch.equal(g, r), (tag, i, "differs from the byte-0 run",
                                       float(_mag(g - r).max()) if g.numel() and g.dtype != torch.bool else None)
            continue
        d = float(_mag(g - r).max())
        if criterion == "atomic":
            rms = float(_mag(r).pow(2).mean().sqrt())
            assert d <= 1e-14 * rms, (tag, i, d, rms)
        else:
            bound = 1e-13 * float(_mag(r + 1).max())
            assert d <= bound, (tag, i, d, bound)


def poisoned_runs(ctx, call, *, inout=(), valid=None, criterion="exact", scratch=True, slots=(), label):
    """``call()`` -> a tensor or a (nested) tuple of tensors and numbers, run with every fresh allocation, the cached
    workspace and (``scratch``) the library's scratch slots filled with byte 0, then with each of POISONS.

    inout : tensors the call legitimately reads and then modifies (accumulate targets, in-place data); they are restored
        from a copy taken here before every run, not poisoned.
    valid : maps the result to its compared part (default: all of it).
    criterion : "exact" - finite and ``torch.equal`` to the byte-0 run; "atomic" - finite and max|diff| <= 1e-14 rms (calls
        that end in the run-time ring kernel, as in test_gpu_poison.py); "global-atomics" - finite and max|diff| <= 1e-13
        max|ref + 1| (the run-to-run bound of test_gpu_interp.py::test_grid_matches_golden).
    slots : scratch slots the call is documented to use (csrc/common.h); they must hold bytes after the byte-0 run.

    Every run must have poisoned at least one allocation or one non-empty scratch slot (asserted).  Returns ``(reference
    result as a list of tensors, report)``; report = per byte ``(allocations, allocation bytes, scratch bytes)``."""
    import torch

    assert criterion in CRITERIA, criterion
    sel = valid or (lambda r: r)
    saved = [t.clone() for t in inout]
    on_gpu = torch.device(ctx.device).type == "cuda"
    report = {}

    def run(byte):
        for t, s in zip(inout, saved):
            t.copy_(s)
        if scratch:
            ctx.debug_poison_scratch(byte)
        with poisoned_allocations(ctx, byte) as st:
            r = _flat(torch, sel(call()))
            if on_gpu:
                torch.cuda.synchronize()
        r = [t.detach().clone() for t in r]
        # (read with the fill switched off: the slots as the call left them, those it grew were filled when they were made)
        sizes = ctx.debug_poison_scratch(-1) if scratch else []
        report[byte] = (st.allocations, st.bytes, sum(sizes))
        assert st.allocations > 0 or any(sizes), (label, hex(byte), "vacuous: no allocation and no scratch slot was poisoned")
        return r, sizes

    try:
        ref, sizes = run(0)
        _compare(torch, ref, ref, criterion, (label, "0x0"))
        for s in slots:
            assert scratch and sizes[s] > 0, (label, "scratch slot %d is empty after the call" % s, sizes)
        failures = []                                     # every poison is run: a report names each one that shows
        for byte in POISONS:
            got, _ = run(byte)
            try:
                _compare(torch, got, ref, criterion, (label, hex(byte)))
            except AssertionError as e:
                failures.append(str(e))
        assert not failures, "; ".join(failures)
    finally:
        if scratch:
            ctx.debug_poison_scratch(-1)
        for t, s in zip(inout, saved):
            t.copy_(s)
    return ref, report
