"""-m gpu: every entry that writes a packed weight image (include/vit_ops.h vit_split_weight, vit_split_weight_block, vit_split_weight_pair,
vit_split_weights_many, vit_split_conv_weight_pair) against the torch restatement of the bytes (tests/weight_image_cases.py), in every
arithmetic mode and both layouts.  The entries are called raw (vit_ops.load()) on buffers pre-filled with 0xA5, so a padding row or a k group
that a kernel leaves unwritten shows.  Shapes: smaller than a tile, ragged in both directions over several tiles, exact tiles."""
import ctypes as ct
import functools

import numpy as np
import pytest
import torch

from tests import weight_image_cases as wic

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SHAPES = [(8, 8), (72, 136), (128, 64), (200, 72)]
CONV_SHAPES = [(24, 40, 3), (8, 8, 3), (32, 136, 1)]
VIT_EINVAL = -1


@functools.lru_cache(maxsize=None)
def _weight(rows, cols):
    w = wic.ramp_matrix(rows, cols, seed=1000 * rows + cols)
    return w, wic.word_of(w)


@functools.lru_cache(maxsize=None)
def _expected(rows, cols, transposed, block, mode):
    w, word = _weight(rows, cols)
    return wic.expected_image(w.t().contiguous() if transposed else w, block, mode, word)


def _lib(mode):
    from styl3r_amd import vit_ops
    lib = vit_ops.load()
    assert lib.vit_x6_set_products(wic.PRODUCTS[mode]) == 0            # (conftest puts 6 back after every test)
    return lib, vit_ops._stream(DEV)


def _buffer(lib, rows, cols, transposed, block):
    n = lib.vit_split_weight_block_bytes(rows, cols, 1 if transposed else 0) if block else lib.vit_split_weight_bytes(rows, cols)
    R, Kc = (cols, rows) if transposed else (rows, cols)
    assert n == wic.padded_rows(R, block) * Kc * 6 + wic.WORD_BYTES
    return torch.full((n,), 0xA5, dtype=torch.uint8, device=DEV)


def _announce(lib, mode, word_dev):
    if mode == "f16x3":
        assert lib.vit_x6_set_operand_amax(ct.c_void_p(word_dev.data_ptr()), None) == 0


def _assert_image(buf, expected, block, mode, word, what):
    torch.cuda.synchronize()
    body = buf[:-wic.WORD_BYTES].cpu()
    assert body.numel() == expected.numel(), what
    assert torch.equal(wic.compared(body, block, mode), wic.compared(expected, block, mode)), what
    if mode == "f16x3":
        assert torch.equal(wic.word_slots(buf[-wic.WORD_BYTES:]), wic.word_slots(word)), (what, "tail")


@pytest.mark.parametrize("rows,cols", SHAPES)
@pytest.mark.parametrize("mode", wic.MODES)
def test_single_image_entries_write_the_restated_bytes(mode, rows, cols):
    lib, stream = _lib(mode)
    w, word = _weight(rows, cols)
    wd, word_dev = w.to(DEV), word.to(DEV)
    for block in (False, True):
        for transposed in (False, True):
            buf = _buffer(lib, rows, cols, transposed, block)
            _announce(lib, mode, word_dev)
            entry = lib.vit_split_weight_block if block else lib.vit_split_weight
            assert entry(wd.data_ptr(), buf.data_ptr(), rows, cols, 1 if transposed else 0, stream) == 0
            _assert_image(buf, _expected(rows, cols, transposed, block, mode), block, mode, word, (mode, rows, cols, block, transposed))


@pytest.mark.parametrize("rows,cols", SHAPES)
@pytest.mark.parametrize("mode", wic.MODES)
def test_pair_entry_writes_the_restated_bytes(mode, rows, cols):
    lib, stream = _lib(mode)
    w, word = _weight(rows, cols)
    wd, word_dev = w.to(DEV), word.to(DEV)
    for block_f in (False, True):
        for block_t in (False, True):
            bf, bt = _buffer(lib, rows, cols, False, block_f), _buffer(lib, rows, cols, True, block_t)
            _announce(lib, mode, word_dev)
            assert lib.vit_split_weight_pair(wd.data_ptr(), bf.data_ptr(), bt.data_ptr(), rows, cols, int(block_f), int(block_t), stream) == 0
            _assert_image(bf, _expected(rows, cols, False, block_f, mode), block_f, mode, word, (mode, rows, cols, "fwd", block_f, block_t))
            _assert_image(bt, _expected(rows, cols, True, block_t, mode), block_t, mode, word, (mode, rows, cols, "t", block_f, block_t))


@pytest.mark.parametrize("mode", wic.MODES)
def test_job_table_entry_writes_the_restated_bytes(mode):
    """one table: all four kinds (row / block, forward / transposed) of two weights"""
    lib, stream = _lib(mode)
    job = np.dtype([("w", "u8"), ("packed", "u8"), ("amax", "u8"), ("tail", "u8"), ("rows", "i4"), ("cols", "i4"), ("kind", "i4"),
                    ("first_block", "u4"), ("nbx", "u4"), ("reserved", "u4")])     # VitSplitJob
    keep, rows_of_table, first = [], [], 0
    for rows, cols in [(72, 136), (200, 72)]:
        w, word = _weight(rows, cols)
        wd, word_dev = w.to(DEV), word.to(DEV)
        for kind in range(4):
            transposed, block = bool(kind & 1), bool(kind & 2)
            buf = _buffer(lib, rows, cols, transposed, block)
            R, Kc = (cols, rows) if transposed else (rows, cols)
            nbx, nby = (Kc + 63) // 64, (R + 63) // 64
            rows_of_table.append((wd.data_ptr(), buf.data_ptr(), word_dev.data_ptr() if mode == "f16x3" else 0,
                                  buf.data_ptr() + buf.numel() - wic.WORD_BYTES, rows, cols, kind, first, nbx, 0))
            first += nbx * nby
            keep.append((wd, word_dev, buf, word, (rows, cols, transposed, block)))
    host = np.array(rows_of_table, dtype=job)
    table = torch.from_numpy(host.view(np.uint8).reshape(-1).copy()).to(DEV)
    assert lib.vit_split_weights_many(table.data_ptr(), len(keep), first, stream) == 0
    for _, _, buf, word, (rows, cols, transposed, block) in keep:
        _assert_image(buf, _expected(rows, cols, transposed, block, mode), block, mode, word, (mode, rows, cols, transposed, block))


def _conv_weight(Co, Ci, k):
    g = torch.Generator().manual_seed(Co * 100 + Ci + k)
    w = torch.randn(Co, Ci, k, k, generator=g) * torch.logspace(-6, 3, Ci)[None, :, None, None]
    fwd = w.permute(0, 2, 3, 1).reshape(Co, k * k * Ci).contiguous()                   # column = tap * Ci + ci
    dx = w.flip(2, 3).permute(1, 2, 3, 0).reshape(Ci, k * k * Co).contiguous()         # spatially flipped, channel-transposed
    return w, fwd, dx, wic.word_of(w)


@pytest.mark.parametrize("Co,Ci,k,with_dx", [(*s, True) for s in CONV_SHAPES] + [(16, 24, 3, False)])
@pytest.mark.parametrize("mode", ["f16x3", "bf16x6"])
def test_conv_pair_entry_writes_the_restated_bytes(mode, Co, Ci, k, with_dx):
    lib, stream = _lib(mode)
    w, fwd, dx, word = _conv_weight(Co, Ci, k)
    wd, word_dev = w.to(DEV), word.to(DEV)
    bf = _buffer(lib, Co, k * k * Ci, False, False)
    bd = _buffer(lib, Ci, k * k * Co, False, False) if with_dx else None
    _announce(lib, mode, word_dev)
    assert lib.vit_split_conv_weight_pair(wd.data_ptr(), bf.data_ptr(), bd.data_ptr() if with_dx else None, Co, Ci, k, stream) == 0
    _assert_image(bf, wic.expected_image(fwd, False, mode, word), False, mode, word, (mode, Co, Ci, k, "fwd"))
    if with_dx:
        _assert_image(bd, wic.expected_image(dx, False, mode, word), False, mode, word, (mode, Co, Ci, k, "dx"))


@pytest.mark.parametrize("transposed", [False, True])
def test_split_weight_computes_its_own_scale_when_none_is_announced(transposed):
    """f16x3 without an announced word: vit_split_weight folds max|w| into the image's own tail word and scales by it"""
    lib, stream = _lib("f16x3")
    rows, cols = 72, 136
    w, _ = _weight(rows, cols)
    wd = w.to(DEV)
    buf = _buffer(lib, rows, cols, transposed, False)
    assert lib.vit_split_weight(wd.data_ptr(), buf.data_ptr(), rows, cols, 1 if transposed else 0, stream) == 0
    torch.cuda.synchronize()
    tail = wic.word_slots(buf[-wic.WORD_BYTES:])
    assert int(tail.max()) == int(w.abs().max().view(torch.int32))
    expected = wic.expected_image(w.t().contiguous() if transposed else w, False, "f16x3", buf[-wic.WORD_BYTES:])
    assert torch.equal(wic.compared(buf[:-wic.WORD_BYTES], False, "f16x3"), wic.compared(expected, False, "f16x3"))


def test_entries_that_need_an_announced_word_refuse_without_one():
    lib, stream = _lib("f16x3")
    rows, cols = 72, 136
    wd = _weight(rows, cols)[0].to(DEV)
    a, b = _buffer(lib, rows, cols, False, True), _buffer(lib, rows, cols, True, True)
    assert lib.vit_split_weight_block(wd.data_ptr(), a.data_ptr(), rows, cols, 0, stream) == VIT_EINVAL
    assert lib.vit_split_weight_pair(wd.data_ptr(), a.data_ptr(), b.data_ptr(), rows, cols, 1, 1, stream) == VIT_EINVAL
    Co, Ci, k = CONV_SHAPES[0]
    wc = _conv_weight(Co, Ci, k)[0].to(DEV)
    c = _buffer(lib, Co, k * k * Ci, False, False)
    assert lib.vit_split_conv_weight_pair(wc.data_ptr(), c.data_ptr(), None, Co, Ci, k, stream) == VIT_EINVAL
    torch.cuda.synchronize()
    assert bool((a == 0xA5).all()) and bool((c == 0xA5).all())          # nothing was launched
