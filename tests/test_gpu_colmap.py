"""GPU tests (-m gpu) of gsr_undistort (csrc/gsr_undistort.hip) through colmap.undistort_frames and inference.prepare_colmap_scene.
Every comparison is of integer views, the device against the host path of styl3r_amd/colmap.py (whose known answers
tests/test_colmap_host.py checks without an oracle), with no tolerance."""
import shutil

import numpy as np
import pytest
import torch

from styl3r_amd import _lib, colmap, inference
from styl3r_amd.inputs import InputCfg
from tests.test_colmap_host import GOLD_DIR, OPENCV_DIST, known_answer_cases, scene_frames, sketch_K

pytestmark = pytest.mark.gpu
DEV = "cuda"
Cam = colmap.UndistortCamera


def both(frames: np.ndarray, cams, frame_cam, **kw) -> np.ndarray:
    """host and device path on the same bytes: equal, returned once"""
    t = torch.from_numpy(frames)
    host = colmap.undistort_frames(t, cams, frame_cam, **kw)
    dev = colmap.undistort_frames(t.to(DEV), cams, frame_cam, **kw)
    assert dev.is_cuda and dev.dtype == torch.uint8 and dev.shape == host.shape
    assert torch.equal(dev.cpu(), host)
    return host.numpy()


def random_frames(shape, seed):
    return np.random.default_rng(seed).integers(0, 256, size=shape, dtype=np.uint8)


def opencv_cam(**kw):
    return Cam(sketch_K(), np.float32(OPENCV_DIST).astype(np.float64), **kw)


def test_known_answers_on_the_device():
    img, K, cases = known_answer_cases()
    frames = torch.from_numpy(img[None]).to(DEV)
    for name, new_K, want in cases:
        for dist in ((0.0, 0.0, 0.0, 0.0), ()):
            out = colmap.undistort_frames(frames, Cam(K, np.array(dist)), [0], new_K=new_K, roi=(0, 0, 13, 9))
            assert np.array_equal(out[0].cpu().numpy(), want), (name, dist)
    assert np.array_equal(colmap.undistort_frames(frames, Cam(K), [0])[0].cpu().numpy(), img)                # the copy path
    win = colmap.undistort_frames(frames, Cam(K), [0], roi=(-2, 5, 6, 7))[0].cpu().numpy()
    want = np.zeros((7, 6, 3), np.uint8)
    want[:4, 2:] = img[5:, :4]
    assert np.array_equal(win, want)


@pytest.mark.parametrize("roi", [None, (5, 3, 41, 29), (0, 36, 53, 1), (52, 0, 1, 37), (-3, -2, 60, 42)])
def test_mixed_cameras_and_windows(roi):
    """cameras [1, 0, 1]: camera 0 without distortion (copied), camera 1 the OPENCV set; the default ROI, an inner window, one row,
    one column and a window larger than the frame"""
    frames = random_frames((3, 37, 53, 3), 1)
    default = colmap.optimal_new_camera(sketch_K(), np.float32(OPENCV_DIST).astype(np.float64), (53, 37))[1]
    cams = [Cam(sketch_K(), roi=default), opencv_cam()]
    out = both(frames, cams, [1, 0, 1], roi=roi)
    x, y, w, h = default if roi is None else roi
    assert out.shape == (3, h, w, 3)
    ys, xs = np.arange(y, y + h), np.arange(x, x + w)
    inside = ((ys >= 0) & (ys < 37))[:, None] & ((xs >= 0) & (xs < 53))[None, :]
    want = frames[1][np.clip(ys, 0, 36)[:, None], np.clip(xs, 0, 52)[None, :]] * inside[..., None].astype(np.uint8)
    assert np.array_equal(out[1], want)                                       # the copied frame is the window itself


@pytest.mark.parametrize("k1", [0.6, -0.6])
def test_strong_distortion_leaves_the_image(k1):
    """the maps run far outside the source: taps half outside and pixels all outside (k1 < 0: the model folds over, kr < 0)"""
    frames = random_frames((2, 37, 53, 3), 2) | 1                               # no zero byte in the source: a zero is the border
    K = sketch_K(f=25.0)
    cam = Cam(K, np.array([k1, 0.0, 0.0, 0.0]))
    near = np.array([[12.0, 0, K[0, 2]], [0, 12.0, K[1, 2]], [0, 0, 1]])
    out = both(frames, cam, [0, 0], new_K=near, roi=(-5, -4, 63, 45))
    zero = (out == 0).all(-1)
    assert zero[:, 0, 0].all() and 0.2 < zero.mean() < 1 and not zero[:, 22, 31].any()      # zero corners around a sampled centre
    table = colmap.undistort_table((37, 53), cam, [0, 0], near, (-5, -4, 63, 45))[0]
    mx, my = colmap._source_maps(table[0], 63, 45)
    assert mx.max() > 60 and mx.min() < -5 and my.max() > 45 and my.min() < -5
    both(frames, cam, [0, 0], roi=(0, 0, 53, 37))                              # the camera's own new matrix over the whole frame
    # coordinates beyond the fixed-point range and non-finite ones give zeros
    far = np.array([[1e-9, 0, K[0, 2]], [0, 1e-9, K[1, 2]], [0, 0, 1]])
    out = both(frames[:1], Cam(K, np.array([k1, 1e300, 0.0, 0.0])), [0], new_K=far, roi=(0, 0, 53, 37))
    assert (out == 0).mean() > 0.99


def test_wide_and_flat_frames_cross_block_boundaries():
    """131 x 5 frames: rows, frames and the 4-pixel groups of a lane do not line up (131 * 5 = 655 pixels per frame), several
    blocks, a partial last group (3 * 655 = 1965 = 4 * 491 + 1)"""
    frames = random_frames((3, 5, 131, 3), 3)
    K = np.array([[90.0, 0, 65.2], [0, 88.0, 2.6], [0, 0, 1]])
    cams = {7: Cam(K, np.array([-0.2, 0.05, 0.001, -0.002])), 2: Cam(K, np.array([0.1, 0.0, 0.0, 0.0]))}
    for roi in ((0, 0, 131, 5), (1, 0, 129, 5), (0, 1, 131, 3)):
        both(frames, cams, [7, 2, 7], roi=roi)
    both(frames[:1], cams, [2], roi=(3, 1, 1, 1))                               # one pixel: only the byte-wise tail


def test_batches_equal_single_frames_and_repeat():
    frames = torch.from_numpy(random_frames((5, 37, 53, 3), 4)).to(DEV)
    cams = [Cam(sketch_K(), roi=(0, 0, 52, 36)), opencv_cam(), Cam(sketch_K(), np.array([0.15, 0.0, 0.0, 0.0]))]
    fc = [1, 0, 2, 1, 2]
    batch = colmap.undistort_frames(frames, cams, fc)
    again = colmap.undistort_frames(frames, cams, fc)
    assert batch.shape == (5, 36, 52, 3) and torch.equal(batch, again)
    for n in range(5):
        assert torch.equal(colmap.undistort_frames(frames[n:n + 1], cams, fc[n:n + 1])[0], batch[n]), n


def test_more_frames_than_one_launch_carries():
    """the frame -> camera table travels in the kernel's arguments, GSR_UNDISTORT_FRAMES_PER_LAUNCH frames at a time: a call with
    more frames is split, and frame n still gets camera n's row"""
    n = _lib.GSR_UNDISTORT_FRAMES_PER_LAUNCH + 7
    frames = random_frames((n, 5, 7, 3), 6)
    K = np.array([[6.0, 0, 3.4], [0, 6.5, 2.2], [0, 0, 1]])
    cams = [Cam(K, np.array([0.2 * s, 0.0, 0.0, 0.0]), new_K=K, roi=(0, 0, 7, 5)) for s in (-1, 0, 1)]
    both(frames, cams, [(i * 5) % 3 for i in range(n)])


def test_byte_offsets_past_2_31():
    """3 frames of 16384 x 16384: source and destination offsets of the last frame lie past 2^31 bytes.  Its bytes must be those of
    the single-frame call, whose offsets are small."""
    side = 16384
    frames = torch.randint(0, 256, (3, side, side, 3), dtype=torch.uint8, device=DEV, generator=torch.Generator(DEV).manual_seed(7))
    K = np.array([[9000.0, 0, side / 2 - 0.3], [0, 9100.0, side / 2 + 0.4], [0, 0, 1]])
    cam = Cam(K, np.float32(OPENCV_DIST).astype(np.float64), roi=(0, 0, side, side))
    batch = colmap.undistort_frames(frames, cam, [0, 0, 0])
    assert batch.numel() > 2 ** 31
    single = colmap.undistort_frames(frames[2:], cam, [0])
    assert torch.equal(batch[2], single[0]) and int(single[0, side // 2, side // 2].sum()) > 0
    del batch, single, frames
    torch.cuda.empty_cache()


def test_prepare_colmap_scene_on_the_device_equals_the_host(tmp_path):
    shutil.copytree(GOLD_DIR / "binary", tmp_path / "capture")
    (tmp_path / "capture" / "images").mkdir()
    sc = colmap.load_colmap_scene(tmp_path / "capture")
    frames = scene_frames()
    cfg = InputCfg(input_image_shape=(24, 32))
    style = torch.from_numpy(random_frames((40, 50, 3), 8))
    host = inference.prepare_colmap_scene(sc, [1, 9], 4, [style], cfg, frames=frames)
    dev = inference.prepare_colmap_scene(sc, [1, 9], 4, [style], cfg, frames=frames, device=DEV)
    for h, d in ((host[0], dev[0]), (host[2], dev[2])):
        for key in ("image", "extrinsics", "intrinsics", "near", "far", "index"):
            assert d[key].is_cuda and d[key].dtype == h[key].dtype and torch.equal(d[key].cpu(), h[key]), key
    assert dev[1][0].is_cuda and torch.equal(dev[1][0].cpu(), host[1][0])
