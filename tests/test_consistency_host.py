"""CPU tests (-m "not gpu") of the multi-view consistency scores: the float64 restatement (metrics.warp_consistency_expression, which is the
CPU route of metrics.warp_consistency) on a scene where the warp is an exact shift, against the independent per-pixel loop of
tests/consistency_inputs.py, its edge cases, the averaging of compute_consistency, and the C boundary of gsr_warp_consistency (the header,
_lib and the library agree; bad arguments are refused before any launch, so no device is needed)."""
import ctypes as C
import math
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from styl3r_amd import _lib, metrics
from tests.consistency_inputs import ALL_PAIRS, DEPTH_TOL, MARGIN, loop_reference, random_scene, shift_scene, summation_bound

ROOT = Path(__file__).resolve().parents[1]


def run(scene, **kw):
    return metrics.warp_consistency(scene["images"], scene["depth"], scene["c2w"], scene["K"], scene["pairs"], return_warped=True, **kw)


@pytest.mark.parametrize("k", [0, 3, -5])
def test_exact_shift(k):
    sc = shift_scene(k)
    before = metrics.CALLS["consistency_expression"]
    res = run(sc)
    assert metrics.CALLS["consistency_expression"] == before + 1               # CPU tensors take the expression
    src, dst = sc["images"][0, 0].numpy(), sc["images"][0, 1].numpy()
    cols = np.array([0 <= x + k <= 15 for x in range(16)])
    want_mask = np.broadcast_to(cols, (16, 16))
    assert res.mask.dtype == torch.bool and np.array_equal(res.mask[0].numpy(), want_mask)
    assert res.count.dtype == torch.int32 and int(res.count[0]) == 16 * (16 - abs(k))
    assert float(res.valid[0]) == (16 - abs(k)) / 16
    want = np.zeros_like(src)
    xs = np.arange(16)[cols]
    want[:, :, xs] = src[:, :, xs + k]
    assert res.warped.dtype == torch.float32 and np.array_equal(res.warped[0, 0].numpy(), want)          # bit for bit
    # multiples of 1/256 below 1: every square and the whole sum are exact in float64
    sse = float((((want.astype(np.float64) - dst) ** 2) * want_mask).sum())
    assert float(res.sse[0, 0]) == sse
    assert float(res.rmse[0, 0]) == math.sqrt(sse / (3.0 * 16 * (16 - abs(k))))


def test_occlusion_masks_exactly_the_pixels_that_land_on_the_nearer_block():
    k, block = 3, (5, 9, 6, 11)                                                # rows 5..8, columns 6..10 of the src depth are at 0.5
    res = run(shift_scene(k, occluder=block))
    # the shift is whole pixels: ax = ay = 0, the weight is 1 on the tap the pixel lands on, so D is that tap's depth -- except in the last
    # column, where x0 is held at W - 2 with ax = 1 and the landing tap is the right one.  Either way D = depth_src[y, x + k].
    want = np.zeros((16, 16), dtype=bool)
    for y in range(16):
        for x in range(16):
            lx = x + k
            want[y, x] = 0 <= lx <= 15 and not (block[0] <= y < block[1] and block[2] <= lx < block[3])
    assert np.array_equal(res.mask[0].numpy(), want)
    assert int(res.count[0]) == 16 * 13 - 4 * 5
    assert not res.warped[0, 0][:, ~torch.from_numpy(want)].any()              # 0 at invalid pixels


def test_expression_against_the_per_pixel_loop():
    H, W = 8, 12
    sc = random_scene(11, 2, H, W)
    ref = loop_reference(sc["images"], sc["depth"], sc["c2w"], sc["K"], sc["pairs"])
    res = run(sc)
    assert np.array_equal(res.mask.numpy(), ref["mask"]) and np.array_equal(res.count.numpy(), ref["count"])
    assert np.array_equal(res.warped.numpy(), ref["warped"])
    err = np.abs(res.sse.numpy() - ref["sse"])
    print("sse", ref["sse"], "difference", err.max(), "bound", summation_bound(H, W) * ref["sse"].max())
    assert (err <= summation_bound(H, W) * ref["sse"]).all()
    assert 0 < ref["count"][0] < H * W and ref["count"][3] == 0                 # something is seen by both, something is not; views facing apart


def test_nothing_visible_gives_nan_and_no_exception():
    sc = random_scene(11, 1, 8, 12, pairs=((0, 2),))
    res = run(sc)
    assert int(res.count[0]) == 0 and math.isnan(float(res.rmse[0, 0])) and float(res.valid[0]) == 0 and not res.mask.any()
    assert float(res.sse[0, 0]) == 0 and not res.warped.any()
    out = metrics.compute_consistency(sc["images"][:, [0, 2]], sc["depth"][[0, 2]], sc["c2w"][[0, 2]], sc["K"][[0, 2]], gaps=(1, 7))
    assert all(math.isnan(v) for v in out[0].values()) and set(out[0]) == {"short_rmse", "long_rmse", "short_valid", "long_valid"}
    bad = random_scene(11, 1, 8, 12, pairs=((0, 5), (-1, 1)), check=False)      # pairs that name no view: no valid pixel, nothing read
    res = run(bad)
    assert not res.mask.any() and res.count.tolist() == [0, 0]


@pytest.mark.parametrize("value", [0.0, -2.0, float("nan"), float("inf"), float("-inf")])
def test_invalid_depth_masks_its_pixel_as_dst_and_as_a_tap(value):
    sc = shift_scene(0)
    sc["depth"][1, 4, 7] = value                                               # dst: exactly that pixel
    res = run(sc)
    want = np.ones((16, 16), dtype=bool)
    want[4, 7] = False
    assert np.array_equal(res.mask[0].numpy(), want)
    sc = shift_scene(0)
    sc["depth"][0, 4, 7] = value                                               # src: every pixel with (4, 7) among its four taps, whatever its weight
    res = run(sc)
    want = np.ones((16, 16), dtype=bool)
    want[3:5, 6:8] = False
    assert np.array_equal(res.mask[0].numpy(), want)


def test_pairs_and_averaging():
    assert metrics.SHORT_RANGE_GAP == 1 and metrics.LONG_RANGE_GAP == 7
    p = metrics.consistency_pairs(10, 7)
    assert p.dtype == torch.int64 and p.tolist() == [[0, 7], [1, 8], [2, 9]]
    assert metrics.consistency_pairs(3, 7).shape == (0, 2) and metrics.consistency_pairs(4, 1).tolist() == [[0, 1], [1, 2], [2, 3]]
    # four frames: 0, 1 and 3 see each other, frame 2 faces away -> the pairs with it have count 0 and are left out of every mean
    sc = random_scene(11, 2, 8, 12, check=False)
    order = [0, 1, 2, 0]
    img, dep, c2w, K = sc["images"][:, order], sc["depth"][order], sc["c2w"][order], sc["K"][order]
    out = metrics.compute_consistency(img, dep, c2w, K, gaps=(1, 3))
    assert isinstance(out, list) and len(out) == 2
    short = metrics.warp_consistency(img, dep, c2w, K, torch.tensor([[0, 1], [1, 2], [2, 3]]))
    long = metrics.warp_consistency(img, dep, c2w, K, torch.tensor([[0, 3]]))
    assert short.count.tolist()[1:] == [0, 0] and int(short.count[0]) > 0 and int(long.count[0]) > 0
    for s in range(2):
        assert out[s]["short_rmse"] == pytest.approx(float(short.rmse[s, 0]), rel=1e-15)
        assert out[s]["short_valid"] == pytest.approx(float(short.valid[0]), rel=1e-15)
        assert out[s]["long_rmse"] == pytest.approx(float(long.rmse[s, 0]), rel=1e-15)
        assert out[s]["long_valid"] == pytest.approx(float(long.valid[0]), rel=1e-15)
    one = metrics.compute_consistency(img[0], dep, c2w, K, gaps=(1, 3))          # (V,3,H,W): one set
    assert len(one) == 1 and one[0] == out[0]
    same = metrics.compute_consistency(img[:, [0, 0, 0]], dep[[0, 0, 0]], c2w[[0, 0, 0]], K[[0, 0, 0]], gaps=(1, 2))
    assert same[0]["short_rmse"] == 0 and same[0]["long_rmse"] == 0 and same[0]["short_valid"] > 0.5   # a frame against itself (border pixels sit on the bounds)


def test_lpips_keys_use_the_masked_images_and_the_same_averaging():
    sc = random_scene(11, 2, 32, 32, check=False)
    order = [0, 1, 0, 1, 0]
    img, dep, c2w, K = sc["images"][:, order], sc["depth"][order], sc["c2w"][order], sc["K"][order]
    module = metrics.get_lpips("cpu")
    out = metrics.compute_consistency(img, dep, c2w, K, gaps=(1, 3), lpips=module, lpips_batch=64)      # one batch: all 2 x 6 images
    assert set(out[0]) == {"short_rmse", "long_rmse", "short_valid", "long_valid", "short_lpips", "long_lpips"}
    pairs = torch.cat([metrics.consistency_pairs(5, 1), metrics.consistency_pairs(5, 3)])
    res = metrics.warp_consistency(img, dep, c2w, K, pairs, return_warped=True)
    assert (res.count > 0).all()
    m = res.mask[None, :, None].float()
    by_hand = metrics.compute_lpips((res.warped * m).reshape(12, 3, 32, 32), (img[:, pairs[:, 1]] * m).reshape(12, 3, 32, 32), module).reshape(2, 6)
    for s in range(2):
        assert out[s]["short_lpips"] == pytest.approx(float(by_hand[s, :4].double().mean()), rel=1e-6, abs=1e-9)
        assert out[s]["long_lpips"] == pytest.approx(float(by_hand[s, 4:].double().mean()), rel=1e-6, abs=1e-9)
    assert out[0]["short_lpips"] != out[1]["short_lpips"]


def test_refusals():
    sc = random_scene(11, 1, 8, 12, check=False)
    img, dep, c2w, K, pairs = sc["images"], sc["depth"], sc["c2w"], sc["K"], sc["pairs"]
    call = metrics.warp_consistency
    with pytest.raises(ValueError, match="height and width >= 2"):
        call(img[..., :1, :], dep[:, :1], c2w, K, pairs)
    with pytest.raises(ValueError, match="height and width >= 2"):
        call(img[..., :1], dep[..., :1], c2w, K, pairs)
    with pytest.raises(ValueError, match="images are"):
        call(img[:, :, :2], dep, c2w, K, pairs)
    with pytest.raises(ValueError, match="depth is"):
        call(img, dep[:2], c2w, K, pairs)
    with pytest.raises(ValueError, match="cameras are"):
        call(img, dep, c2w[:, :3], K, pairs)
    with pytest.raises(ValueError, match="cameras are"):
        call(img, dep, c2w, K[:2], pairs)
    with pytest.raises(ValueError, match="pairs are"):
        call(img, dep, c2w, K, pairs.double())
    with pytest.raises(ValueError, match="pairs are"):
        call(img, dep, c2w, K, pairs.reshape(-1))
    with pytest.raises(ValueError, match="floating-point"):
        call((img * 255).to(torch.uint8), dep, c2w, K, pairs)
    with pytest.raises(ValueError, match="depth_tol"):
        call(img, dep, c2w, K, pairs, depth_tol=-0.1)
    with pytest.raises(ValueError, match="gaps"):
        metrics.compute_consistency(img, dep, c2w, K, gaps=(1,))
    assert call(img.double(), dep.double(), c2w.float(), K.float(), pairs.int()).count.shape == (5,)       # other dtypes: the expression


@pytest.mark.parametrize("hw", [(2, 2), (7, 31), (8, 32), (9, 33), (9, 31), (7, 33)])
def test_builder_keeps_every_pixel_off_the_thresholds(hw):
    """the condition under which a device's mask must equal the expression's: verified here, on the CPU, for the scenes the GPU tests use"""
    sc = random_scene(5, 1, *hw)
    distinct = [p for p, (i, j) in enumerate(ALL_PAIRS) if i != j]
    print(hw, "margins", sc["margin"], "counts", sc["ref_count"])
    assert (sc["margin"][distinct] > MARGIN).all()
    assert sc["ref_count"][3] == 0 and sc["ref_count"][4] == 0                  # the views that face apart
    if hw != (2, 2):
        assert 0 < sc["ref_count"][0] < hw[0] * hw[1] and 0 < sc["ref_count"][1] < hw[0] * hw[1]
    res = metrics.warp_consistency_expression(sc["images"], sc["depth"], sc["c2w"], sc["K"], sc["pairs"], depth_tol=DEPTH_TOL)
    assert np.array_equal(res.count.numpy(), sc["ref_count"])


@pytest.fixture(scope="module")
def lib():
    _lib.build_library()
    return _lib.load()


def test_the_library_exports_the_two_symbols(lib):
    header = (ROOT / "include/gsr.h").read_text()
    for name in ("gsr_warp_consistency_scratch_bytes", "gsr_warp_consistency"):
        assert name in _lib.EXPORTS and re.search(rf"\b{name}\s*\(", header) and hasattr(lib, name), name
    assert "gsr_consistency.hip" in _lib._SOURCES and (ROOT / "styl3r_amd/csrc/gsr_consistency.hip").is_file()
    for name in ("MAX_SETS", "TILE_W", "TILE_H"):
        assert f"#define GSR_CONSISTENCY_{name} {getattr(_lib, 'GSR_CONSISTENCY_' + name)}\n" in header
    cap, tw, th = _lib.GSR_CONSISTENCY_MAX_SETS, _lib.GSR_CONSISTENCY_TILE_W, _lib.GSR_CONSISTENCY_TILE_H
    assert lib.gsr_warp_consistency_scratch_bytes(110, 5, 256, 256) == 110 * (256 // tw) * (256 // th) * 6 * 8   # count + 5 float64 sums per tile
    assert lib.gsr_warp_consistency_scratch_bytes(1, 1, 2, 2) == 16
    assert lib.gsr_warp_consistency_scratch_bytes(2, cap, th + 1, tw + 1) ==2 * 4 * (cap + 1) * 8
    for bad in ((0, 1, 8, 8), (1, 0, 8, 8), (1, cap + 1, 8, 8), (1, 1, 1, 8), (1, 1, 8, 1), (1, 1, 8, 1 << 20), (1 << 40, 1, 8, 8)):
        assert lib.gsr_warp_consistency_scratch_bytes(*bad) == 0, bad


def test_bad_arguments_are_refused_before_any_launch(lib):
    one = C.c_void_p(256)                                                      # (any non-null aligned value: validation only, nothing is dereferenced)
    good = dict(images=one, depth=one, c2w=one, K=one, pairs=one, S=2, V=3, P=4, H=8, W=8, tol=0.05, warped=None, mask=one, count=one, sse=one,
                scratch=one, bytes=1 << 20)
    def call(**kw):
        a = {**good, **kw}
        return lib.gsr_warp_consistency(a["images"], a["depth"], a["c2w"], a["K"], a["pairs"], a["S"], a["V"], a["P"], a["H"], a["W"], a["tol"],
                                        a["warped"], a["mask"], a["count"], a["sse"], a["scratch"], a["bytes"], None)
    for kw in (dict(S=0), dict(S=_lib.GSR_CONSISTENCY_MAX_SETS + 1), dict(V=0), dict(P=0), dict(P=-1), dict(H=1), dict(W=1), dict(H=0),
               dict(W=1 << 20), dict(tol=-1.0), dict(tol=float("nan")), dict(images=None), dict(depth=None), dict(c2w=None), dict(K=None),
               dict(pairs=None), dict(mask=None), dict(count=None), dict(sse=None), dict(scratch=None), dict(scratch=C.c_void_p(260))):
        assert call(**kw) == -1, kw
    assert call(bytes=4 * 1 * 3 * 8 - 1) == -2                                 # GSR_ENOSPACE: 4 pairs x 1 tile x (count + 2 sums) doubles
