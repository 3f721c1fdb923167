"""-m gpu: gsr_warp_consistency (csrc/gsr_consistency.hip) through metrics.warp_consistency against the float64 restatement on the
builder scenes of tests/consistency_inputs.py -- shapes around the kernel's 32 x 8 tile, 1 / 3 / cap sets, both directions of a pair, a
view onto itself, views that face apart, invalid depth -- then determinism, poisoned scratch and outputs, a second stream, and
evaluation.consistency_step end to end on a small synthetic Gaussian scene."""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

from styl3r_amd import _lib, metrics
from tests import poison
from tests.consistency_inputs import ALL_PAIRS, DEPTH_TOL, random_scene, summation_bound

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
CAP, TW, TH = _lib.GSR_CONSISTENCY_MAX_SETS, _lib.GSR_CONSISTENCY_TILE_W, _lib.GSR_CONSISTENCY_TILE_H
SHAPES = [(2, 2), (TH - 1, TW - 1), (TH, TW), (TH + 1, TW + 1), (TH + 1, TW - 1), (TH - 1, TW + 1)]


@functools.lru_cache(maxsize=None)
def case(S, H, W, pairs=ALL_PAIRS):
    """(scene, the float64 expression's result on the CPU): computed once, shared, never modified"""
    sc = random_scene(5, S, H, W, pairs=pairs)
    ref = metrics.warp_consistency_expression(sc["images"], sc["depth"], sc["c2w"], sc["K"], sc["pairs"], depth_tol=DEPTH_TOL, return_warped=True)
    return sc, ref


def on_device(sc):
    return [sc[k].to(DEV) for k in ("images", "depth", "c2w", "K", "pairs")]


def check(res, ref, H, W, tag):
    mismatch = int((res.mask.cpu() != ref.mask).sum())
    got, want = res.warped.cpu().numpy(), ref.warped.numpy()
    ulps = np.abs(got - want) / np.spacing(np.maximum(np.abs(got), np.abs(want)))
    sse, sse_ref = res.sse.cpu().numpy(), ref.sse.numpy()
    rel = np.abs(sse - sse_ref) / np.where(sse_ref > 0, sse_ref, 1.0)
    print(f"{tag}: mask mismatches {mismatch}, counts {res.count.tolist()}, warped max {ulps.max():.2f} ulp, sse rel {rel.max():.2e} of bound "
          f"{summation_bound(H, W):.2e}")
    assert res.mask.dtype == torch.bool and mismatch == 0
    assert res.count.dtype == torch.int32 and torch.equal(res.count.cpu(), ref.count)
    assert ulps.max() <= 1.0
    assert (rel <= summation_bound(H, W)).all()
    assert torch.equal(res.rmse.isnan().cpu(), ref.rmse.isnan()) and torch.equal(res.valid.cpu(), ref.valid)


@pytest.mark.parametrize("S", [1, 3, CAP])
@pytest.mark.parametrize("hw", SHAPES)
def test_kernel_against_the_float64_expression(hw, S):
    sc, ref = case(S, *hw)
    before = dict(metrics.CALLS)
    res = metrics.warp_consistency(*on_device(sc), depth_tol=DEPTH_TOL, return_warped=True)
    assert metrics.CALLS["consistency_hip"] == before["consistency_hip"] + 1 and metrics.CALLS["consistency_expression"] == before["consistency_expression"]
    check(res, ref, *hw, f"{hw} S={S}")
    assert ref.count[3] == 0 and ref.count[4] == 0 and bool(res.rmse[:, 3:].isnan().all())        # the views that face apart
    if hw != (2, 2):
        assert 0 < int(ref.count[0]) < hw[0] * hw[1]                                              # invalid depth and the occluder took pixels
    plain = metrics.warp_consistency(*on_device(sc), depth_tol=DEPTH_TOL)                          # no warped output asked for
    assert plain.warped is None and torch.equal(plain.sse, res.sse) and torch.equal(plain.mask, res.mask)


def test_one_pair_and_a_single_set_given_as_four_dimensions():
    sc, ref = case(1, TH + 1, TW + 1, pairs=((0, 1),))
    images, depth, c2w, K, pairs = on_device(sc)
    res = metrics.warp_consistency(images[0], depth, c2w.float(), K.float(), pairs.int(), depth_tol=DEPTH_TOL, return_warped=True)
    ref32 = metrics.warp_consistency_expression(sc["images"], sc["depth"], sc["c2w"].float(), sc["K"].float(), sc["pairs"], depth_tol=DEPTH_TOL,
                                                return_warped=True)      # fp32 cameras are widened on both sides
    check(res, ref32, TH + 1, TW + 1, "P=1")
    assert res.rmse.shape == (1, 1) and res.mask.shape == (1, TH + 1, TW + 1)


def test_more_sets_than_the_cap_go_in_chunks():
    sc, ref = case(CAP + 3, TH + 1, TW + 1)
    before = metrics.CALLS["consistency_hip"]
    res = metrics.warp_consistency(*on_device(sc), depth_tol=DEPTH_TOL, return_warped=True)
    assert metrics.CALLS["consistency_hip"] == before + 2
    check(res, ref, TH + 1, TW + 1, f"S={CAP + 3}")


def same(a, b):
    return (torch.equal(a.sse, b.sse) and torch.equal(a.count, b.count) and torch.equal(a.mask, b.mask) and torch.equal(a.warped, b.warped)
            and torch.equal(a.rmse.nan_to_num(-1.0), b.rmse.nan_to_num(-1.0)))


def test_two_calls_poisoned_memory_and_a_second_stream_give_the_same_bits():
    sc, ref = case(3, TH + 1, TW + 1)
    args = on_device(sc)
    first = metrics.warp_consistency(*args, depth_tol=DEPTH_TOL, return_warped=True)
    assert same(first, metrics.warp_consistency(*args, depth_tol=DEPTH_TOL, return_warped=True))
    P, H, W = len(ALL_PAIRS), TH + 1, TW + 1
    nbytes = _lib.load().gsr_warp_consistency_scratch_bytes(P, 3, H, W)
    for pattern in poison.PATTERNS:
        with poison.poisoned_allocations(pattern) as record:
            again = metrics.warp_consistency(*args, depth_tol=DEPTH_TOL, return_warped=True)
        assert record.has(nbytes, dtype=torch.uint8) and record.has(shape=(3, P, 3, H, W), dtype=torch.float32), pattern     # scratch, warped
        assert record.has(shape=(3, P), dtype=torch.float64) and record.has(shape=(P,), dtype=torch.int32), pattern          # sse, count
        assert same(first, again), pattern
    torch.cuda.synchronize()
    side = torch.cuda.Stream(DEV)
    with torch.cuda.stream(side):
        other = metrics.warp_consistency(*args, depth_tol=DEPTH_TOL, return_warped=True)
    side.synchronize()
    assert same(first, other)


def test_the_scratch_query_is_exactly_what_the_kernels_touch():
    """direct C-ABI call: a scratch of exactly the stated size with a canary behind it, outputs pre-filled"""
    sc, ref = case(3, TH + 1, TW + 1)
    images, depth, c2w, K, pairs = on_device(sc)
    lib = _lib.load()
    S, P, H, W = 3, len(ALL_PAIRS), TH + 1, TW + 1
    nbytes = lib.gsr_warp_consistency_scratch_bytes(P, S, H, W)
    scratch, intact = poison.guarded(nbytes, pattern="garbage")
    mask = poison.fill_pattern(torch.empty((P, H, W), dtype=torch.uint8, device=DEV), "garbage")
    count = poison.fill_pattern(torch.empty(P, dtype=torch.int32, device=DEV), "garbage")
    sse = poison.fill_pattern(torch.empty((S, P), dtype=torch.float64, device=DEV), "ones")
    pr = pairs.int().contiguous()
    rc = lib.gsr_warp_consistency(images.data_ptr(), depth.data_ptr(), c2w.data_ptr(), K.data_ptr(), pr.data_ptr(), S, 3, P, H, W, DEPTH_TOL, None,
                                  mask.data_ptr(), count.data_ptr(), sse.data_ptr(), scratch.data_ptr(), nbytes,
                                  C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream))
    assert rc == 0
    torch.cuda.synchronize()
    intact()
    assert torch.equal(mask.bool().cpu(), ref.mask) and torch.equal(count.cpu(), ref.count)
    assert (np.abs(sse.cpu().numpy() - ref.sse.numpy()) <= summation_bound(H, W) * ref.sse.numpy()).all()


def test_consistency_step_equals_compute_consistency_on_separately_rendered_frames():
    from styl3r_amd import trajectory
    from styl3r_amd.decoder import DecoderSplattingCUDACfg, Gaussians, get_decoder
    from styl3r_amd.evaluation import consistency_step
    from styl3r_amd.scenes import make_scene
    h = w = 32
    sc = make_scene(n_ctx=2, grid_hw=(48, 48), n_views=2, image_hw=(h, w), sh_degree=0, seed=3, near=0.5)
    geo = (sc.means[None].to(DEV), sc.covariances[None].to(DEV))
    g = torch.Generator().manual_seed(4)
    sets = [Gaussians(*geo, hm[None].to(DEV), sc.opacities[None].to(DEV)) for hm in (sc.harmonics, torch.randn(sc.harmonics.shape, generator=g))]
    dec = get_decoder(DecoderSplattingCUDACfg("splatting_cuda", [0.0, 0.0, 0.0], True)).to(DEV)
    ctx = dict(image=torch.zeros(1, 2, 3, h, w, device=DEV), extrinsics=sc.extrinsics[None].to(DEV), intrinsics=sc.intrinsics[None].to(DEV),
               near=sc.near[None].to(DEV), far=sc.far[None].to(DEV))
    frames, gaps = 6, (1, 3)
    got = consistency_step(dec, sets, ctx, num_frames=frames, frames_per_pass=4, gaps=gaps)
    assert list(got) == ["plain", "style_0"] and set(got["plain"]) == {"short_rmse", "long_rmse", "short_valid", "long_valid"}
    ext, intr, near, far = trajectory.trajectory_cameras(ctx, None, "interpolation", frames)
    assert ext.shape[1] == frames                                                                 # the way out only: no reverse loop
    with torch.no_grad():
        outs = [dec.forward_styles(s, [s.harmonics], ext, intr, near, far, (h, w)) for s in sets]  # one set per pass, all frames at once
    color = torch.stack([o.color[0, 0] for o in outs])
    depth = outs[0].depth[0] * near[0, :, None, None]                                              # the scale-invariant decoder renders z / near
    want = metrics.compute_consistency(color, depth, ext[0], intr[0], gaps=gaps)
    print("consistency_step", got, "separately", want)
    for name, ref in zip(got, want):
        for key, value in ref.items():
            assert got[name][key] == pytest.approx(value, rel=1e-6), (name, key)
    assert got["plain"]["short_valid"] > 0.25 and got["plain"]["long_valid"] > 0.1                # neighbouring frames see the same surface
    assert 0 < got["plain"]["short_rmse"] < 1 and 0 < got["plain"]["long_rmse"] < 1
    assert got["plain"]["short_valid"] == got["style_0"]["short_valid"] and got["plain"]["short_rmse"] != got["style_0"]["short_rmse"]
    # with an LPIPS module: the masked-image convention through the existing compute_lpips, averaged like the RMSE
    module = metrics.get_lpips(DEV)
    with_lpips = metrics.compute_consistency(color, depth, ext[0], intr[0], gaps=gaps, lpips=module, lpips_batch=5)
    pairs = metrics.consistency_pairs(frames, gaps[0])
    res = metrics.warp_consistency(color, depth, ext[0], intr[0], pairs, return_warped=True)
    assert res.warped.is_cuda and bool((res.count > 0).all())
    # the LPIPS values themselves are checked on the host (tests/test_consistency_host.py), where two calls of the module give the same bits;
    # here: the device route runs, returns the keys, and leaves the RMSE as it was (random LPIPS weights: the score may have any sign)
    for s in range(len(got)):
        assert math.isfinite(with_lpips[s]["short_lpips"]) and math.isfinite(with_lpips[s]["long_lpips"])
        assert with_lpips[s]["short_rmse"] == want[s]["short_rmse"] and with_lpips[s]["long_valid"] == want[s]["long_valid"]
