"""The poison harness (tests/_poison.py) on CPU tensors, the device filter pointed at ``cpu``: it must reject a function
that leaves part of a ``torch.empty`` buffer unwritten, also where the stale value only passes a max (the reason for the
finite poison 0x7E), accept a correct one, refuse a vacuous case, and leave ``torch`` as it found it.  The library hook
behind ``Context.debug_poison_scratch`` is checked for its declaration (header, binding, documents); no GPU needed."""
import os
import re
import types

import pytest

import _poison

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cpu_ctx(workspace=None):
    import torch

    return types.SimpleNamespace(device=torch.device("cpu"), _workspace=workspace)


def _names():
    import torch

    return torch.empty, torch.empty_like, torch.empty_strided, torch.Tensor.new_empty


def _x():
    import torch

    return torch.arange(1.0, 9.0, dtype=torch.float64)


def _ragged_tail():
    """Allocates 9, writes 8: the last element is whatever the allocator handed back."""
    import torch

    t = torch.empty(9, dtype=torch.float64)
    t[:8] = _x()
    return t


def _stale_through_max():
    """Reads the unwritten element through a NaN-dropping max: a NaN poison passes, a huge finite one does not."""
    import torch

    t = torch.empty(9, dtype=torch.float64)
    t[:8] = _x()
    return torch.fmax(t, torch.zeros(9, dtype=torch.float64)).max().reshape(1)


def _correct():
    import torch

    t = torch.empty(9, dtype=torch.float64)
    t[:8] = _x()
    t[8] = 0.0
    u = torch.empty_like(t).copy_(t) + t.new_empty((9,)).zero_() + torch.empty_strided((9,), (1,), dtype=torch.float64).fill_(1.0)
    return u, float(u.sum())


def test_poisons_are_those_of_the_sht_poison_tests():
    import test_gpu_poison

    assert _poison.POISONS is test_gpu_poison.POISONS and _poison.POISONS == (0xFF, 0x7E)


def test_ragged_tail_is_rejected_under_both_poisons():
    import torch

    ctx = _cpu_ctx()
    for byte in _poison.POISONS:
        with _poison.poisoned_allocations(ctx, byte) as st:
            t = _ragged_tail()
        assert st.allocations == 1 and st.bytes == 72
        assert t.view(torch.uint8)[64:].tolist() == [byte] * 8 and torch.equal(t[:8], _x())
        zero = torch.zeros(9, dtype=torch.float64)
        zero[:8] = _x()
        assert not torch.equal(t, zero)
    with pytest.raises(AssertionError, match="0xff"):
        _poison.poisoned_runs(ctx, _ragged_tail, scratch=False, label="ragged")


def test_stale_read_through_a_max_needs_the_finite_poison():
    import torch

    ctx = _cpu_ctx()
    with _poison.poisoned_allocations(ctx, 0) as st:
        ref = _stale_through_max()
    with _poison.poisoned_allocations(ctx, 0xFF):
        nan_run = _stale_through_max()
    with _poison.poisoned_allocations(ctx, 0x7E):
        big_run = _stale_through_max()
    assert st.allocations == 1
    assert torch.equal(nan_run, ref)                  # the NaN is dropped by the max: 0xFF alone would pass this bug
    assert bool(torch.isfinite(big_run).all()) and not torch.equal(big_run, ref)
    with pytest.raises(AssertionError, match="0x7e"):
        _poison.poisoned_runs(ctx, _stale_through_max, scratch=False, label="max")


def test_correct_function_passes_and_is_counted():
    import torch

    ws = torch.zeros(16, dtype=torch.uint8)
    ctx = _cpu_ctx(ws)
    ref, report = _poison.poisoned_runs(ctx, _correct, scratch=False, label="correct")
    assert float(ref[0].sum()) == 36.0 + 9.0 and float(ref[1]) == 45.0
    # four allocations of 72 bytes + the cached workspace, for byte 0 and both poisons; no scratch on the host
    assert report == {b: (5, 4 * 72 + 16, 0) for b in (0,) + _poison.POISONS}
    assert ws.tolist() == [_poison.POISONS[-1]] * 16


def test_inout_tensors_are_restored_not_poisoned():
    import torch

    acc = torch.ones(4, dtype=torch.float64)

    def call():
        acc.add_(torch.empty(4, dtype=torch.float64).fill_(2.0))
        return acc

    ref, _ = _poison.poisoned_runs(_cpu_ctx(), call, inout=(acc,), scratch=False, label="inout")
    assert ref[0].tolist() == [3.0] * 4 and acc.tolist() == [1.0] * 4
    with pytest.raises(AssertionError):                # the same call without the restore accumulates from run to run
        _poison.poisoned_runs(_cpu_ctx(), call, scratch=False, label="no restore")


def test_valid_selects_the_compared_part_and_other_devices_pass_through():
    import torch

    ref, _ = _poison.poisoned_runs(_cpu_ctx(), _ragged_tail, valid=lambda t: t[:8], scratch=False, label="valid")
    assert torch.equal(ref[0], _x())
    other = types.SimpleNamespace(device=torch.device("meta"), _workspace=None)
    with _poison.poisoned_allocations(other, 0xFF) as st:
        t = torch.empty(3, dtype=torch.float64).fill_(1.0)
    assert st.allocations == 0 and t.tolist() == [1.0] * 3


def test_vacuous_case_is_refused():
    import torch

    x = torch.ones(3, dtype=torch.float64)
    with pytest.raises(AssertionError, match="vacuous"):
        _poison.poisoned_runs(_cpu_ctx(), lambda: x * 2.0, scratch=False, label="nothing poisoned")
    with pytest.raises(AssertionError):
        _poison.poisoned_runs(_cpu_ctx(), _correct, criterion="close enough", scratch=False, label="unknown criterion")


def test_tolerant_criteria_are_the_two_of_the_project():
    import torch

    ref = [torch.tensor([1.0, -2.0, 3.0], dtype=torch.float64)]
    rms = float(ref[0].pow(2).mean().sqrt())
    for crit, ok, bad in (("atomic", 0.9e-14 * rms, 1.2e-14 * rms), ("global-atomics", 0.9e-13 * 4.0, 1.2e-13 * 4.0)):
        _poison._compare(torch, [ref[0] + torch.tensor([0.0, 0.0, ok])], ref, crit, crit)
        with pytest.raises(AssertionError):
            _poison._compare(torch, [ref[0] + torch.tensor([0.0, 0.0, bad])], ref, crit, crit)
        with pytest.raises(AssertionError, match="non-finite"):
            _poison._compare(torch, [ref[0] * float("inf")], ref, crit, crit)
    with pytest.raises(AssertionError):
        _poison._compare(torch, [ref[0] + torch.tensor([0.0, 0.0, 4e-16])], ref, "exact", "exact")


def test_patches_are_gone_after_the_block_also_on_an_exception():
    before = _names()
    ctx = _cpu_ctx()
    with _poison.poisoned_allocations(ctx, 0xFF):
        assert all(a is not b for a, b in zip(_names(), before))
    assert all(a is b for a, b in zip(_names(), before))
    with pytest.raises(RuntimeError, match="inside"):
        with _poison.poisoned_allocations(ctx, 0x7E):
            raise RuntimeError("inside")
    assert all(a is b for a, b in zip(_names(), before))
    with pytest.raises(AssertionError):
        _poison.poisoned_runs(ctx, _ragged_tail, scratch=False, label="ragged")
    assert all(a is b for a, b in zip(_names(), before))


def test_debug_hook_is_declared_bound_and_documented():
    from cora_amd import _lib

    header = open(os.path.join(ROOT, "include", "corahip.h")).read()
    assert "int corahip_debug_poison_scratch(corahip_ctx *ctx, int byte, size_t *slot_bytes);" in header
    assert "#define CORAHIP_DEBUG_NSCRATCH %d\n" % _lib.DEBUG_NSCRATCH in header
    common = open(os.path.join(ROOT, "cora_amd", "csrc", "common.h")).read()
    assert "#define CORAHIP_NSCRATCH %d\n" % _lib.DEBUG_NSCRATCH in common
    # the slot map the per-case slot assertions pin names every slot
    # ("N description," entries up to the line that classes the slots: each slot has a description of its own)
    slot_map = common.split("// slots:")[1].split("//  written whole")[0].replace("\n", " ").replace("//", " ")
    entries = re.findall(r"(?:^|,)\s*(\d+)\s+([A-Za-z][^,]*)", slot_map)
    assert [int(n) for n, _ in entries] == list(range(_lib.DEBUG_NSCRATCH)), entries
    assert all(len(text.strip()) >= 5 for _, text in entries), entries
    assert "corahip_debug_poison_scratch" in _lib.SIGNATURES and hasattr(_lib.Context, "debug_poison_scratch")
    lib = _lib.load()
    assert hasattr(lib, "corahip_debug_poison_scratch")
    assert lib.corahip_debug_poison_scratch(None, 0, None) == -1          # CORAHIP_EINVAL: no context
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "corahip_debug_poison_scratch" in doc and "test-only" in doc.split("corahip_debug_poison_scratch")[1][:400]
