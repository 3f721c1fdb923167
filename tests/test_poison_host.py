"""CPU test of tests/poison.py itself: a read of uninitialised memory must show, a full overwrite must not, the record must
list what was touched, and the patches must be gone afterwards."""
import math

import pytest
import torch

from tests import poison
from tests.poison import PATTERNS, guarded, poisoned_allocations

CPU = ("cpu",)


def _reads_before_writing(n):
    buf = torch.empty(n, dtype=torch.float32)
    return float(buf.sum())


def _overwrites(n):
    buf = torch.empty(n, dtype=torch.float32)
    buf.copy_(torch.arange(n, dtype=torch.float32))
    return float(buf.sum())


def _run(fn, pattern):
    with poisoned_allocations(pattern, devices=CPU) as rec:
        return fn(37), rec


def test_a_read_before_write_differs_across_patterns_and_an_overwrite_does_not():
    got = {p: _run(_reads_before_writing, p)[0] for p in PATTERNS}
    assert got["zero"] == 0.0
    assert math.isnan(got["ones"])                              # every byte 0xFF is a NaN
    assert math.isfinite(got["garbage"]) and got["garbage"] > 1e30
    full = {p: _run(_overwrites, p)[0] for p in PATTERNS}
    assert full["zero"] == full["ones"] == full["garbage"] == 37 * 36 / 2


def test_the_record_lists_the_buffer():
    _, rec = _run(_overwrites, "ones")
    assert (37 * 4, torch.float32) in rec
    assert rec.has(nbytes=148) and rec.has(shape=(37,), dtype=torch.float32)
    assert not rec.has(nbytes=149) and not rec.has(shape=(37,), dtype=torch.float64)


def test_all_four_allocators_are_patched_and_fill_every_dtype_as_documented():
    with poisoned_allocations("ones", devices=CPU) as rec:
        a = torch.empty(3, 5, dtype=torch.int32)
        b = torch.empty_like(a, dtype=torch.float64)
        c = torch.empty_strided((4, 3), (1, 4), dtype=torch.int64)        # non-contiguous: the whole storage is filled
        d = a.new_empty((7,), dtype=torch.uint8)
        e = torch.empty(0)
    assert (a == -1).all() and b.isnan().all() and (c == -1).all() and (d == 255).all() and e.numel() == 0
    assert list(rec) == [(60, torch.int32), (120, torch.float64), (96, torch.int64), (7, torch.uint8), (0, torch.float32)]
    with poisoned_allocations("garbage", devices=CPU):
        i = torch.empty(5, dtype=torch.int32)
        h = torch.empty(5, dtype=torch.float16)
        f = torch.empty(5)
        m = torch.empty(5, dtype=torch.bool)
    assert (i == -0x5A5A5A5B).all()                                       # 0xA5A5A5A5 as int32
    assert (h == 6.0e4).all() and (f == 1.0e30).all() and m.all()
    with poisoned_allocations("zero", devices=CPU):
        assert (torch.empty(9, dtype=torch.float32) == 0).all()


def test_only_the_named_device_types_are_touched():
    with poisoned_allocations("ones") as rec:                             # default: device tensors only
        torch.empty(8)
    assert rec == []


def test_the_patches_are_gone_after_the_block_also_when_the_body_raises():
    before = (torch.empty, torch.empty_like, torch.empty_strided, torch.Tensor.new_empty, "new_empty" in torch.Tensor.__dict__)
    with poisoned_allocations("ones", devices=CPU):
        assert torch.empty is not before[0] and torch.Tensor.new_empty is not before[3]
    after = (torch.empty, torch.empty_like, torch.empty_strided, torch.Tensor.new_empty, "new_empty" in torch.Tensor.__dict__)
    assert after == before
    with pytest.raises(ZeroDivisionError):
        with poisoned_allocations("garbage", devices=CPU):
            torch.empty(2)
            1 / 0
    after = (torch.empty, torch.empty_like, torch.empty_strided, torch.Tensor.new_empty, "new_empty" in torch.Tensor.__dict__)
    assert after == before
    with pytest.raises(ValueError):
        with poisoned_allocations("noise"):
            pass
    assert torch.empty is before[0]


def test_guarded_scratch_has_the_stated_size_and_notices_a_byte_written_behind_it():
    scratch, check = guarded(100, guard=32, device="cpu")
    assert scratch.numel() == 100 and scratch.dtype == torch.uint8 and (scratch == 0xFF).all()
    scratch.fill_(7)                                                      # writes inside the stated size are fine
    check()
    check.whole[100] = 0                                                  # the first byte past the stated size
    with pytest.raises(AssertionError, match=r"\+0 "):
        check()
    scratch, check = guarded(0, device="cpu", pattern="garbage")
    assert scratch.numel() == 0
    check()
    assert (guarded(5, pattern="garbage", device="cpu")[0] == poison.GARBAGE_BYTE).all()
