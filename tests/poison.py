"""Poisoned allocations: run an op on scratch and output memory that holds something other than the zeros a fresh process hands out.

`poisoned_allocations(pattern)` patches the four uninitialised allocators (`torch.empty`, `torch.empty_like`,
`torch.empty_strided`, `Tensor.new_empty`) for the duration of a `with` block: the real allocator runs, then the new
tensor's whole storage is filled with the pattern, and `(nbytes, dtype)` is recorded.  An op whose result changes with the
pattern read a word before anything wrote it, or returned an element no kernel wrote.

`guarded(nbytes)` is for direct C-ABI calls: a scratch of exactly the size a `*_scratch_bytes` entry states, with canary
bytes behind it, and a check that they are intact afterwards.

Never use either inside hipGraph capture (the fills are launches of their own); `poisoned_allocations` refuses to.
docs/SCRATCH_CONTRACTS.md says which entries may be run this way and why."""
from __future__ import annotations

import contextlib
import math

import torch

PATTERNS = ("zero", "ones", "garbage")
GARBAGE_BYTE = 0xA5
CANARY_BYTE = 0xC3
# "garbage" for float dtypes: large, finite, and exactly representable nowhere near any test's data
GARBAGE_FLOAT = {torch.float16: 6.0e4, torch.bfloat16: 1.0e30, torch.float32: 1.0e30, torch.float64: 1.0e30}


def _storage_bytes(t):
    """the tensor's whole storage as a flat uint8 tensor (a fresh torch.empty owns its storage alone)"""
    st = t.untyped_storage()
    return torch.zeros(0, dtype=torch.uint8, device=t.device).set_(st, 0, (st.nbytes(),))    # (torch.empty is patched)


def fill_pattern(t, pattern):
    """fill `t` (every byte of its storage) with `pattern`; returns `t`"""
    if pattern not in PATTERNS:
        raise ValueError(f"unknown poison pattern {pattern!r}")
    if t.untyped_storage().nbytes() == 0:
        return t
    with torch.no_grad():
        if pattern == "zero":
            _storage_bytes(t).zero_()
        elif pattern == "ones":
            _storage_bytes(t).fill_(0xFF)
        elif t.dtype in GARBAGE_FLOAT:
            _storage_bytes(t).view(t.dtype).fill_(GARBAGE_FLOAT[t.dtype])
        elif t.dtype == torch.bool:
            _storage_bytes(t).fill_(1)                      # any other byte is not a valid bool
        else:
            _storage_bytes(t).fill_(GARBAGE_BYTE)
    return t


class AllocationRecord(list):
    """[(nbytes, dtype), ...] of every allocation the block poisoned"""

    def has(self, nbytes=None, shape=None, dtype=None):
        """is there a buffer of `nbytes` bytes (or of `shape` elements of `dtype`)?"""
        if shape is not None:
            nbytes = math.prod(shape) * torch.zeros(0, dtype=dtype).element_size()
        return any(n == nbytes and (dtype is None or d == dtype) for n, d in self)


@contextlib.contextmanager
def poisoned_allocations(pattern, devices=("cuda",)):
    """patch the uninitialised allocators; tensors on a device type in `devices` are filled with `pattern` and recorded"""
    if pattern not in PATTERNS:
        raise ValueError(f"unknown poison pattern {pattern!r}")
    record = AllocationRecord()

    def wrap(real):
        def alloc(*args, **kwargs):
            t = real(*args, **kwargs)
            if isinstance(t, torch.Tensor) and t.device.type in devices:
                if t.device.type == "cuda" and torch.cuda.is_current_stream_capturing():
                    raise RuntimeError("poisoned_allocations must not be used inside graph capture")
                fill_pattern(t, pattern)
                record.append((t.numel() * t.element_size(), t.dtype))
            return t
        alloc.__wrapped__ = real
        return alloc

    own_new_empty = "new_empty" in torch.Tensor.__dict__
    saved = (torch.empty, torch.empty_like, torch.empty_strided, torch.Tensor.new_empty)
    torch.empty, torch.empty_like, torch.empty_strided = wrap(saved[0]), wrap(saved[1]), wrap(saved[2])
    torch.Tensor.new_empty = wrap(saved[3])
    try:
        yield record
    finally:
        torch.empty, torch.empty_like, torch.empty_strided = saved[:3]
        if own_new_empty:
            torch.Tensor.new_empty = saved[3]
        else:
            del torch.Tensor.new_empty                      # inherited from the base class again


def guarded(nbytes, guard=256, pattern="ones", device="cuda:0"):
    """(scratch, check): `scratch` is a uint8 tensor of exactly `nbytes` bytes filled with `pattern`; `guard` canary bytes
    lie directly behind it, and `check()` asserts that none of them changed."""
    whole = torch.zeros(int(nbytes) + int(guard), dtype=torch.uint8, device=device)
    scratch, canary = whole[:int(nbytes)], whole[int(nbytes):]
    if nbytes:
        if pattern == "zero":
            scratch.zero_()
        else:
            scratch.fill_(0xFF if pattern == "ones" else GARBAGE_BYTE)
    canary.fill_(CANARY_BYTE)

    def check():
        hit = (canary != CANARY_BYTE).nonzero()
        assert hit.numel() == 0, f"canary behind a {nbytes}-byte scratch overwritten at +{int(hit[0])} ({hit.numel()} bytes)"

    check.whole = whole                                     # keeps the canary alive with the check
    return scratch, check
