"""tests/poison.py on the CPU (devices=("cpu",)): what the wrappers fill, that they pass their arguments through, that the
originals come back, nesting and the counter -- and the completeness of the GPU table: every module of ebfi_amd that calls one
of the replaced allocators is named by a case of tests/test_gpu_poisoned_alloc.py or listed in EXEMPT with its reason."""
import ast
import os

import pytest
import torch

import poison
from poison import poisoned_allocations

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PACKAGE = os.path.join(ROOT, "ebfi-be_amd", "ebfi_amd")

# modules that allocate and have no case of the GPU table: why not
EXEMPT = {
}


def _originals():
    return [getattr(owner, name) for owner, name in poison.ALLOCATORS]


def _all_bytes_ff(t):
    return bool((torch.empty(0, dtype=torch.uint8).set_(t.untyped_storage(), 0, (t.untyped_storage().nbytes(),), (1,)) == 0xFF).all())


def _five(dtype):
    """One result of each of the five allocators."""
    base = torch.zeros(3, 5, dtype=dtype)
    return [torch.empty(3, 5, dtype=dtype), torch.empty_like(base), torch.empty_strided((3, 5), (5, 1), dtype=dtype),
            base.new_empty((2, 7)), base.new_empty_strided((2, 7), (7, 1))]


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16, torch.float32, torch.float64])
def test_float_results_are_all_nan(dtype):
    with poisoned_allocations(devices=("cpu",)):
        got = _five(dtype)
    for t in got:
        assert t.dtype == dtype and torch.isnan(t).all()
        assert _all_bytes_ff(t)


@pytest.mark.parametrize("dtype,value", [(torch.int32, -1), (torch.int64, -1), (torch.int16, -1), (torch.int8, -1), (torch.uint8, 255)])
def test_integer_results_are_all_ones_bits(dtype, value):
    with poisoned_allocations(devices=("cpu",)):
        got = _five(dtype)
    for t in got:
        assert t.dtype == dtype and bool((t == value).all())


def test_non_contiguous_and_memory_format_results_are_filled_completely():
    view = torch.zeros(4, 6, 5)[:, ::2].transpose(0, 2)                  # neither contiguous nor dense
    assert not view.is_contiguous()
    with poisoned_allocations(devices=("cpu",)):
        like = torch.empty_like(view)                                    # preserve_format: the strides follow the view's order
        chan = torch.empty(2, 3, 4, 5, memory_format=torch.channels_last)
        like_cl = torch.empty_like(torch.zeros(2, 3, 4, 5), memory_format=torch.channels_last)
        gaps = torch.empty_strided((3, 4), (10, 2))                      # elements 2 apart, rows 10 apart: the gaps too
    assert like.shape == view.shape and torch.isnan(like).all()
    assert chan.is_contiguous(memory_format=torch.channels_last) and torch.isnan(chan).all()
    assert like_cl.is_contiguous(memory_format=torch.channels_last) and torch.isnan(like_cl).all()
    assert gaps.stride() == (10, 2) and torch.isnan(gaps).all() and _all_bytes_ff(gaps)


def test_arguments_pass_through_unchanged():
    base = torch.zeros(2, 2)
    with poisoned_allocations(devices=("cpu",)):
        a = torch.empty((2, 3), dtype=torch.float64, device="cpu", requires_grad=True)
        b = torch.empty(4, dtype=torch.int32, pin_memory=False)
        c = torch.empty_like(base, dtype=torch.float16, memory_format=torch.contiguous_format)
        d = base.new_empty((5,), dtype=torch.int64, device="cpu")
        e = base.new_empty_strided((2, 2), (1, 2), dtype=torch.float64)
        f = torch.empty(0)                                               # nothing to fill
        out = torch.zeros(3)
        g = torch.empty(3, out=out)
    assert a.dtype == torch.float64 and a.requires_grad and a.shape == (2, 3) and a.device.type == "cpu"
    assert b.dtype == torch.int32 and not b.is_pinned() and bool((b == -1).all())
    assert c.dtype == torch.float16 and c.shape == base.shape and c.is_contiguous()
    assert d.dtype == torch.int64 and d.shape == (5,) and bool((d == -1).all())
    assert e.dtype == torch.float64 and e.stride() == (1, 2) and torch.isnan(e).all()
    assert f.numel() == 0
    assert g is out


def test_other_devices_are_left_alone():
    with poisoned_allocations(devices=("cuda",)) as seen:                # the default: a CPU tensor is not the patch's business
        t = torch.empty(64, dtype=torch.uint8)
        m = torch.empty(8, device="meta")
    assert seen.allocations == 0 and seen.bytes == 0
    assert t.shape == (64,) and m.device.type == "meta"
    with poisoned_allocations(devices=("cpu:0",)) as seen:               # a full device name matches that device only
        torch.empty(8)
    assert seen.allocations == 0


def test_originals_are_back_after_a_normal_exit_and_after_an_exception():
    before = _originals()
    own = ["new_empty" in vars(torch.Tensor), "new_empty_strided" in vars(torch.Tensor)]
    with poisoned_allocations(devices=("cpu",)):
        assert all(a is not b for a, b in zip(_originals(), before))
    assert all(a is b for a, b in zip(_originals(), before))
    with pytest.raises(KeyError):
        with poisoned_allocations(devices=("cpu",)):
            assert torch.isnan(torch.empty(3)).all()
            raise KeyError("inside")
    assert all(a is b for a, b in zip(_originals(), before))
    assert own == ["new_empty" in vars(torch.Tensor), "new_empty_strided" in vars(torch.Tensor)]
    x = torch.zeros(2).new_empty(3)                                      # and they work
    assert x.shape == (3,)


def test_blocks_nest():
    before = _originals()
    with poisoned_allocations(devices=("cpu",)) as outer:
        torch.empty(4)
        mid = _originals()
        with poisoned_allocations(devices=("cpu",)) as inner:
            t = torch.empty(2, dtype=torch.float64)
            assert torch.isnan(t).all()
        assert all(a is b for a, b in zip(_originals(), mid))            # the inner block restores the outer one's wrappers
        u = torch.empty(1)
        assert torch.isnan(u).all()
    assert all(a is b for a, b in zip(_originals(), before))
    assert (inner.allocations, inner.bytes) == (1, 16)
    assert (outer.allocations, outer.bytes) == (3, 16 + 16 + 4)          # the inner block's allocation went through both


def test_the_counter_counts():
    with poisoned_allocations(devices=("cpu",)) as seen:
        assert (seen.allocations, seen.bytes) == (0, 0)
        torch.empty(10, dtype=torch.float32)
        assert (seen.allocations, seen.bytes) == (1, 40)
        torch.zeros(3).new_empty((4, 4), dtype=torch.float16)
        torch.empty(0)                                                   # empty: nothing poisoned, nothing counted
        torch.zeros(5)                                                   # not an uninitialised allocation
        assert (seen.allocations, seen.bytes) == (2, 72)
    assert "allocations=2" in repr(seen)


# ------------------------------------------------------------------------------------------------------ the table is complete
def _allocating_modules():
    """{module: [line numbers]} of the calls `<anything>.<allocator>(...)` in ebfi_amd/*.py -- torch.empty, x.new_empty,
    torch.empty_like, c16.empty (which reaches torch.empty) ..."""
    found = {}
    for name in sorted(os.listdir(PACKAGE)):
        if not name.endswith(".py"):
            continue
        with open(os.path.join(PACKAGE, name)) as f:
            tree = ast.parse(f.read(), name)
        lines = [node.lineno for node in ast.walk(tree)
                 if isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute) and node.func.attr in poison.ALLOCATOR_NAMES]
        if lines:
            found[name[:-3]] = lines
    return found


def test_the_source_scan_sees_the_allocations():
    found = _allocating_modules()
    assert len(found) >= 20 and sum(len(v) for v in found.values()) >= 150, {k: len(v) for k, v in found.items()}
    for module in ("conv", "fused", "loss", "fold3d", "c16", "norm", "metrics", "iwe", "esim", "telemetry"):
        assert module in found, module


def test_every_allocating_module_has_a_poisoned_case_or_an_exemption():
    import test_gpu_poisoned_alloc as T                                  # (imports nothing of the device code at module level)
    covered = {}
    for cid, modules, run in T.CASES:
        assert isinstance(cid, str) and callable(run) and modules and all(isinstance(m, str) for m in modules), cid
        for m in modules:
            covered.setdefault(m, []).append(cid)
    for m in covered:
        assert os.path.exists(os.path.join(PACKAGE, m + ".py")), "%s (cases %s) is no module of ebfi_amd" % (m, covered[m][:3])
    found = _allocating_modules()
    missing = sorted(m for m in found if m not in covered and m not in EXEMPT)
    assert not missing, "modules that allocate (lines %s) with neither a poisoned case nor an exemption: %s" % (
        {m: found[m] for m in missing}, missing)
    for m, reason in EXEMPT.items():
        assert m in found and m not in covered, "stale exemption: %s" % m
        assert isinstance(reason, str) and len(reason.split()) >= 3 and "\n" not in reason, m
