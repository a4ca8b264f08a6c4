"""Poisoned allocations: run a check with every new buffer holding 0xFF bytes instead of whatever the allocator left there.

The native ops take their outputs and workspaces from torch.empty, torch.empty_like, torch.empty_strided, Tensor.new_empty
and Tensor.new_empty_strided (ebfi_amd.c16.empty reaches torch.empty).  In a fresh process that memory is nearly always
zero, so a kernel that adds up a partial nobody wrote still gets the right sum; in a long run the caching allocator hands
back recycled blocks.  Inside `poisoned_allocations()` each of those five allocators is replaced by a wrapper that calls the
original with the arguments unchanged and then sets every byte of the result's storage to 0xFF: NaN read as fp16, bf16, fp32
or fp64, -1 read as int32 or int64, 255 read as uint8.  Allocations made in C++ inside ATen are not touched; the package's
wrappers allocate in Python.

    with poisoned_allocations() as seen:
        run_the_comparison()
    assert seen.allocations > 0

A plain helper: nothing is patched outside the `with` block, and the originals come back on exit and on an exception.
"""
import contextlib

import torch

# (owner, attribute): the Python-level allocators that hand out uninitialised memory
ALLOCATORS = (
    (torch, "empty"),
    (torch, "empty_like"),
    (torch, "empty_strided"),
    (torch.Tensor, "new_empty"),
    (torch.Tensor, "new_empty_strided"),
)
# the names a call site spells: torch.<name>(...) or <tensor>.<name>(...)   (tests/test_poison_host.py reads the package by them)
ALLOCATOR_NAMES = frozenset(name for _, name in ALLOCATORS)
FILL = 0xFF             # every byte of a poisoned allocation (0x00: whether a finding depends on what the buffer held)
_EMPTY = torch.empty    # the allocator itself, for the byte view below (inside a block torch.empty is the wrapper)


class PoisonCount:
    """What one `poisoned_allocations()` block poisoned so far."""

    def __init__(self):
        self.allocations = 0
        self.bytes = 0

    def __repr__(self):
        return "PoisonCount(allocations=%d, bytes=%d)" % (self.allocations, self.bytes)


def _on(t, devices):
    return t.device.type in devices or str(t.device) in devices


def _poison(t, devices, count):
    """The allocation is fresh, so the storage is this tensor's alone: fill all of it (every element of a strided or
    channels-last result, and the gaps of an empty_strided one) through a byte view of the storage."""
    if not isinstance(t, torch.Tensor) or not _on(t, devices):
        return
    storage = t.untyped_storage()
    nbytes = storage.nbytes()
    if nbytes == 0:
        return
    _EMPTY(0, dtype=torch.uint8, device=t.device).set_(storage, 0, (nbytes,), (1,)).fill_(FILL)
    count.allocations += 1
    count.bytes += nbytes


def _wrapper(original, devices, count):
    def poisoned(*args, **kwargs):
        out = original(*args, **kwargs)
        _poison(out, devices, count)
        return out

    poisoned.__name__ = getattr(original, "__name__", "empty")
    poisoned.__wrapped__ = original
    return poisoned


@contextlib.contextmanager
def poisoned_allocations(devices=("cuda",)):
    """Replace the five allocators for the length of the block; yields the block's PoisonCount.  `devices` holds device
    types ("cuda", "cpu") or full names ("cuda:0").  Blocks nest: the inner one wraps the outer one's wrappers, both
    count, and each restores what it found."""
    devices = tuple(devices)
    count = PoisonCount()
    # (Tensor inherits its two from the C base class: there the wrapper is a new entry, taken out again on exit)
    saved = [(owner, name, getattr(owner, name), name in vars(owner)) for owner, name in ALLOCATORS]
    try:
        for owner, name, original, _ in saved:
            setattr(owner, name, _wrapper(original, devices, count))
        yield count
    finally:
        for owner, name, original, own in saved:
            if own:
                setattr(owner, name, original)
            else:
                delattr(owner, name)
