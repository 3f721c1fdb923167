"""No GPU: the torch restatement of the packed weight images (tests/weight_image_cases.py) is self-consistent -- what `expected_image` packs,
`unpack_image` reads back, the pieces sum to the value they were split from, and the block layout's padding rows are zero."""
import pytest
import torch

from tests import weight_image_cases as wic


@pytest.mark.parametrize("block", [False, True])
@pytest.mark.parametrize("mode", wic.MODES)
@pytest.mark.parametrize("rows,cols", [(8, 8), (72, 136), (128, 64)])
def test_pieces_sum_back_to_the_values(rows, cols, mode, block):
    v = wic.ramp_matrix(rows, cols, seed=rows + cols)
    word = wic.word_of(v) if mode == "f16x3" else None
    body = wic.expected_image(v, block, mode, word)
    Rp = wic.padded_rows(rows, block)
    assert body.dtype == torch.uint8 and body.numel() == Rp * cols * 6
    planes = wic.unpack_image(body, rows, cols, block, mode, word)
    assert len(planes) == (2 if mode == "f16x3" else 3)
    vd = v.double()
    err = (sum(planes)[:rows] - vd).abs()
    if mode == "f16x3":           # elements below 2^-17 |max| lose bits to fp16's range: an absolute error, below any sum's rounding
        keep = vd.abs() >= 2.0 ** -17 * float(vd.abs().max())
        assert bool(keep.any()) and bool((err[keep] <= 2.0 ** -21 * vd.abs()[keep]).all())
        assert bool((err[~keep] <= 2.0 ** -38 * float(vd.abs().max())).all())
    else:
        assert bool((err <= 2.0 ** -25 * vd.abs()).all())
    for p in planes:
        assert not bool(p[rows:].any())                  # padding rows (block layout only)
    # slot 2 is outside the expectation in f16x3, inside it otherwise
    assert wic.compared(body, block, mode).shape[1] == len(planes)


def test_block_layout_places_row_r_of_group_g_where_the_ring_kernels_read_it():
    """one element set in an otherwise zero matrix lands at [r / 64][k / 8][piece 0][r % 64][k % 8] (block) and [r][k / 8][piece 0][k % 8] (row)"""
    R, K, r, k = 72, 24, 70, 13
    v = torch.zeros(R, K)
    v[r, k] = 1.0
    one = torch.tensor([1.0]).bfloat16().view(torch.int16)
    row = wic.expected_image(v, False, "bf16x6").view(torch.int16)
    blk = wic.expected_image(v, True, "bf16x6").view(torch.int16)
    at_row = ((r * (K // 8) + k // 8) * 3 + 0) * 8 + k % 8
    at_blk = ((((r // 64) * (K // 8) + k // 8) * 3 + 0) * 64 + r % 64) * 8 + k % 8
    assert row[at_row] == one and int((row != 0).sum()) == 1
    assert blk[at_blk] == one and int((blk != 0).sum()) == 1


def test_f16_scale_rule():
    bits = lambda x: int(torch.tensor([x]).view(torch.int32))
    assert wic.f16_scale_of(bits(1.0)) == 2.0 ** 14 and wic.f16_scale_of(bits(1.99)) == 2.0 ** 14 and wic.f16_scale_of(bits(3000.0)) == 2.0 ** 3
    assert wic.f16_scale_of(0) == 1.0 and wic.f16_scale_of(bits(float("inf"))) == 1.0 and wic.f16_scale_of(bits(1e-40)) == 1.0
    assert wic.f16_scale_of(bits(2e-38)) == 2.0 ** 100 and wic.f16_scale_of(bits(3e38)) == 2.0 ** -100
