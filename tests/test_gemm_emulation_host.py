"""No GPU: the host emulation of the split-arithmetic products (tests/gemm_emulation.py), the 2-D row metric (tests/gpu_utils.worst_row_rel_2d)
and the inputs of tests/test_gpu_gemm_ranges.py.

  * the pieces keep what csrc/vit_common.h promises: f16x3 an element at or above 2^-17 of the tensor's |max| to 2^-22, a smaller one to 2^-39 of
    the |max|; bf16 2^-25 (the figure of test_split_weight_is_exact_to_2pow26)
  * every generated case meets the conditions the GPU bar rests on -- emulated worst-row error of the full-scale rows <= 2^-20 (bf16x3, whose
    operands are good to 2^-16: 2^-14, see FULL_SCALE_CAP), of every reduced block at its own scale <= OWN_SCALE_BAR = 2e-4, and NO row on
    either floor of the metric -- so the GPU test cannot go vacuous
  * sensitivity: deliberately wrong emulations on the same inputs.  Flushed fp16 subnormals and a power-of-two scale 2^3 too small PASS the
    whole-tensor bar of the existing tests (2 x bf16x6 + 3e-7 on max |a - e| / max |e|) on every layout and EXCEED the per-row bar, computed from
    the true emulation, on a reduced block: the gap is real and the row metric closes it.  A stale |max| word (the tensor's without its 30 x
    outlier) overflows the outlier's fp16 pieces to Inf; measured here: the Inf reaches the whole-tensor metric too (NaN), so that mutant is
    caught by both metrics -- it cannot hide, and the row metric names the row."""
import numpy as np
import pytest
import torch

from tests import gemm_emulation as ge
from tests.gpu_utils import CANCEL_FLOOR, RANGE_FLOOR, row_scales, worst_row_rel_2d
from tests.weight_image_cases import piece_planes, ramp_matrix, word_of

LINEAR = [(s, l, c) for s in ge.LINEAR_SHAPES for l, c in ge.LAYOUTS]
CONV = [(s, l, c) for s in ge.CONV_SHAPES for l, c in ge.LAYOUTS if (l, c) != ("L5", 15)]
_ids = lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v)


def test_f16_pieces_keep_22_bits_down_to_2pow17_below_the_maximum_and_2pow39_of_it_below():
    v = ramp_matrix(96, 80, 3)                                   # nine decades: fp16 subnormals of the scaled value included
    h, l = piece_planes(v, "f16x3", word_of(v))
    err = (h + l - v.double()).abs()
    amax = float(v.abs().max())
    big = v.abs().double() >= 2.0 ** -17 * amax
    assert big.any() and (~big).any()
    assert float((err[big] / v.abs().double()[big]).max()) <= 2.0 ** -22
    assert float(err[~big].max()) <= 2.0 ** -39 * amax
    assert float(err[~big].max()) > 0                           # (the small elements really are where fp16 rounds)


@pytest.mark.parametrize("mode", ["bf16x6", "bf16x3"])
def test_bf16_pieces_are_exact_to_2pow25(mode):
    v = ramp_matrix(96, 80, 4)
    p = piece_planes(v, mode)
    assert len(p) == 3
    assert float(((p[0] + p[1] + p[2] - v.double()).abs() / v.abs().double().clamp_min(1e-300)).max()) <= 2.0 ** -25
    assert float(((p[0] - v.double()).abs() / v.abs().double().clamp_min(1e-300)).max()) <= 2.0 ** -8


def test_emulation_orders_the_modes_and_the_yardstick_is_float32():
    rng = np.random.default_rng(1)
    a = rng.standard_normal((40, 128)).astype(np.float32); b = rng.standard_normal((24, 128)).astype(np.float32)
    ref = ge.exact(a, b)
    e = {m: ge.whole_tensor_rel(ge.emulate(a, b, m), ref) for m in ge.MODES}
    assert e["bf16x6"] <= 2.0 ** -24 and e["bf16x6"] < e["f16x3"] <= 2.0 ** -21 < e["bf16x3"] <= 2.0 ** -15, e
    y = ge.yardstick(a, b)
    assert np.array_equal(y, y.astype(np.float32).astype(np.float64)) and 0 < ge.whole_tensor_rel(y, ref) <= 1e-6


def test_row_metric_judges_each_row_at_its_own_scale_with_the_two_floors():
    e = np.array([[4.0, -2.0], [2.0 ** -18, 2.0 ** -19], [0.0, 0.0], [2.0 ** -30, 0.0]])
    a = e.copy(); a[1, 1] += 2.0 ** -28                         # 2^-10 of row 1, 2^-30 of the tensor
    assert worst_row_rel_2d(a, e) == (2.0 ** -10, 1)
    assert worst_row_rel_2d(a, e, rows=np.array([0, 2, 3])) == (0.0, 0)
    scale, floored = row_scales(e)
    assert list(floored) == [False, False, True, True] and scale[2] == scale[3] == RANGE_FLOOR * 4.0
    a = e.copy(); a[3, 1] = 2.0 ** -26                          # a row below RANGE_FLOOR x the maximum is judged against that
    assert worst_row_rel_2d(a, e) == (2.0 ** -26 / (RANGE_FLOOR * 4.0), 3)
    trm = np.array([[6.0, 6.0], [1.0, 1.0], [8.0, 8.0], [0.0, 0.0]])       # row 1: a cancellation (|e| = 2^-18 of terms of 1)
    scale, floored = row_scales(e, trm)
    assert scale[1] == CANCEL_FLOOR and scale[2] == 8.0 * CANCEL_FLOOR and list(floored) == [False, True, True, True]
    for bad in (np.nan, np.inf):
        a = e.copy(); a[0, 0] = bad
        assert worst_row_rel_2d(a, e) == (np.inf, 0)


def _conditions(judged, tensor):
    """the three conditions on every judged tensor of a case; tensor(name, how, mode) evaluates it"""
    out = {}
    for name, groups in judged.items():
        ref, trm = tensor(name, "exact", None), tensor(name, "terms", None)
        assert not row_scales(ref, trm)[1].any(), (name, "rows judged on a floor", np.nonzero(row_scales(ref, trm)[1])[0])
        for mode in ge.MODES:
            errs = ge.group_errors(tensor(name, "emulate", mode), ref, trm, groups)
            out[name, mode] = errs
            for g, (e, row) in errs.items():
                cap = ge.FULL_SCALE_CAP[mode] if g == "full" else max(ge.OWN_SCALE_BAR if mode == "f16x3" else 0.0, ge.FULL_SCALE_CAP[mode])
                assert e <= cap, (name, mode, g, row, e, cap)
    return out


@pytest.mark.parametrize("shape,layout,c", LINEAR, ids=_ids)
def test_linear_cases_meet_the_caps_and_keep_every_row_off_the_floors(shape, layout, c):
    case = ge.linear_case(layout, *shape, c=c)
    errs = _conditions(case["judged"], lambda name, how, mode: ge.linear_tensor(case, name, how, mode))
    if layout != "L5":          # the reduced blocks really cost f16x3 something: the own-scale bar is not idle
        (name,) = case["judged"]
        assert errs[name, "f16x3"]["small"][0] > 16 * errs[name, "f16x3"]["full"][0]


@pytest.mark.parametrize("shape,layout,c", CONV, ids=_ids)
def test_convolution_cases_meet_the_caps_and_keep_every_row_off_the_floors(shape, layout, c):
    case = ge.conv_case(layout, *shape, c=c)
    _conditions(case["judged"], lambda name, how, mode: ge.conv_tensor(case, name, how, mode))


@pytest.mark.parametrize("shape", ge.LINEAR_SHAPES[:3], ids=_ids)
@pytest.mark.parametrize("layout", ["L1", "L2", "L3", "L4"])
def test_wrong_splits_pass_the_whole_tensor_bar_and_fail_the_row_bar(shape, layout):
    case = ge.linear_case(layout, *shape)
    (name, groups), = case["judged"].items()
    ref, trm = ge.linear_tensor(case, name, "exact"), ge.linear_tensor(case, name, "terms")
    true = ge.group_errors(ge.linear_tensor(case, name, "emulate", "f16x3"), ref, trm, groups)
    yard = ge.group_errors(ge.linear_tensor(case, name, "yardstick"), ref, trm, groups)
    bars = {g: ge.bar(true[g][0], yard[g][0]) for g in groups}
    old_bar = 2.0 * ge.whole_tensor_rel(ge.linear_tensor(case, name, "emulate", "bf16x6"), ref) + 3e-7
    assert ge.whole_tensor_rel(ge.linear_tensor(case, name, "emulate", "f16x3"), ref) <= old_bar
    assert all(true[g][0] <= bars[g] for g in groups)
    seen = {}
    for mutant in ge.MUTANTS:
        got = ge.linear_tensor(case, name, "emulate", "f16x3", mutant)
        seen[mutant] = (ge.whole_tensor_rel(got, ref), ge.group_errors(got, ref, trm, groups))
    for mutant in ("flush", "scale"):
        whole, rows = seen[mutant]
        assert whole <= old_bar, (mutant, whole, old_bar)                                   # invisible to the whole-tensor metric ...
        assert rows["small"][0] > bars["small"], (mutant, rows, bars)                       # ... and caught on the deepest block
        assert rows["full"][0] <= bars["full"]                                              # (the full-scale rows do not feel it)
    # a flush shows ~1000 x on the 2^-12 block (its low pieces are subnormal, its high ones are not); the scale error only 8 x there
    assert seen["flush"][1]["2^-12"][0] > 100 * true["2^-12"][0] and seen["flush"][1]["2^-12"][0] > bars["2^-12"]
    assert seen["flush"][1]["small"][0] > 3 * true["small"][0]
    whole, rows = seen["stale"]
    assert rows["full"][0] == np.inf and rows["full"][1] == case["outlier"]                 # the outlier's pieces overflowed: the row metric names it
    assert not whole <= old_bar                                                             # (NaN: this one no metric misses)
    assert rows["small"][0] <= bars["small"] and rows["2^-12"][0] <= bars["2^-12"]          # the larger scale only helps the reduced blocks
