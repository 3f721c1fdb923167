"""COLMAP scenes: the sparse model of a capture -> what `inference.prepare_colmap_scene` hands to `prepare_scene`, covering the
reference's COLMAP drivers (infer_model_colmap.py:310-498, infer_model_tnt_batch.py, src/dataset/colmap_utils.py and
src/dataset/colmap_parsing_utils.py).  Host code is numpy float64; the one hot path, lens undistortion of the frames, is
`gsr_undistort` (csrc/gsr_undistort.hip) on the device and a vectorised restatement of the same integers in numpy on the CPU.

    scene = load_colmap_scene("capture/")                                   # sparse/0 or sparse, text or binary
    context, styles, target = prepare_colmap_scene(scene, [1, 9], 4, [style], device="cuda")

The readers are written from COLMAP's published file format (cameras / images, text and binary); `points3D` is not read.

Undistortion arithmetic (shared by the host and the device path; written after OpenCV 4's published procedure for
getOptimalNewCameraMatrix(alpha = 0), initUndistortRectifyMap and remap(INTER_LINEAR, 8-bit, constant zero border).  OpenCV is not a
dependency and was not available to compare with: the float64 / integer code HERE is the definition, and a caller who holds OpenCV's
own K_new / ROI passes them through `new_K=` / `roi=`):
  new camera  `optimal_new_camera`: a 9 x 9 grid of fp32 image points is undistorted to normalised coordinates by five fixed-point
              iterations, rounded to fp32; the inner rectangle of the grid gives fx', fy', cx', cy' and, projected through them, the ROI
  map         output pixel (u, v) of the full undistorted frame, float64 in this order, no contraction:
              x = (u - cx') / fx', y = (v - cy') / fy', r2 = x x + y y, kr = 1 + (k2 r2 + k1) r2,
              xd = x kr + p1 (2 x y) + p2 (r2 + 2 x x), yd = y kr + p1 (r2 + 2 y y) + p2 (2 x y), mx = fp32(fx xd + cx), my = fp32(fy yd + cy)
  sample      sx = rint_half_even(mx * 32) (fp32 product), ix = sx >> 5, a = sx & 31, likewise iy, b; per channel
              ((32 - a)(32 - b) p00 + a (32 - b) p01 + (32 - a) b p10 + a b p11 + 512) >> 10, a tap outside the image is 0;
              a non-finite coordinate or |m| * 32 >= 2^30 gives 0
  output      the ROI window of the undistorted frame; a frame whose camera has no distortion is copied through its window

Deviations from the reference, on purpose: its RADIAL / OPENCV branches read `cam.k1` on a dict (AttributeError) -- the dict keys are
used here; and `prepare_colmap_scene` subtracts the ROI origin from cx, cy where the reference crops without moving the principal point.
"""
from __future__ import annotations

import ctypes as C
import os
import struct
from collections import namedtuple
from dataclasses import dataclass, field
from pathlib import Path
from typing import Optional, Sequence

import numpy as np
import torch
from torch import Tensor

from . import _lib

Camera = namedtuple("Camera", ["id", "model", "width", "height", "params"])
Image = namedtuple("Image", ["id", "qvec", "tvec", "camera_id", "name", "xys", "point3D_ids"])

# COLMAP's camera models: id -> (name, number of parameters)
CAMERA_MODELS = {0: ("SIMPLE_PINHOLE", 3), 1: ("PINHOLE", 4), 2: ("SIMPLE_RADIAL", 4), 3: ("RADIAL", 5), 4: ("OPENCV", 8),
                 5: ("OPENCV_FISHEYE", 8), 6: ("FULL_OPENCV", 12), 7: ("FOV", 5), 8: ("SIMPLE_RADIAL_FISHEYE", 4),
                 9: ("RADIAL_FISHEYE", 5), 10: ("THIN_PRISM_FISHEYE", 12)}


# ---- readers ----
def _data_lines(path):
    with open(path, "r") as f:
        for line in f:
            yield line


def read_cameras_text(path) -> dict:
    """cameras.txt: `CAMERA_ID MODEL WIDTH HEIGHT PARAMS[]` per line, '#' comments -> {id: Camera}"""
    cameras = {}
    for line in _data_lines(path):
        line = line.strip()
        if not line or line.startswith("#"):
            continue
        tok = line.split()
        cam_id = int(tok[0])
        cameras[cam_id] = Camera(cam_id, tok[1], int(tok[2]), int(tok[3]), np.array([float(t) for t in tok[4:]], dtype=np.float64))
    return cameras


def _unpack(f, fmt: str):
    size = struct.calcsize(fmt)
    data = f.read(size)
    if len(data) != size:
        raise ValueError(f"{f.name}: file ends inside a record")
    return struct.unpack(fmt, data)


def read_cameras_binary(path) -> dict:
    """cameras.bin (little endian): uint64 count; per camera int32 id, int32 model id, uint64 width, uint64 height, float64 params"""
    cameras = {}
    with open(path, "rb") as f:
        (count,) = _unpack(f, "<Q")
        for _ in range(count):
            cam_id, model_id, width, height = _unpack(f, "<iiQQ")
            if model_id not in CAMERA_MODELS:
                raise ValueError(f"{path}: unknown camera model id {model_id}")
            name, n_params = CAMERA_MODELS[model_id]
            cameras[cam_id] = Camera(cam_id, name, width, height, np.array(_unpack(f, f"<{n_params}d"), dtype=np.float64))
    return cameras


def read_images_text(path) -> dict:
    """images.txt: two lines per image -- `IMAGE_ID QW QX QY QZ TX TY TZ CAMERA_ID NAME`, then `(X Y POINT3D_ID)*` (may be empty)"""
    images = {}
    lines = _data_lines(path)
    for line in lines:
        line = line.strip()
        if not line or line.startswith("#"):
            continue
        tok = line.split()
        tok2 = next(lines, "").split()                 # the observations' line follows at once, empty or not
        xys = np.array([[float(t) for t in tok2[0::3]], [float(t) for t in tok2[1::3]]], dtype=np.float64).T.copy()
        image_id = int(tok[0])
        images[image_id] = Image(image_id, np.array([float(t) for t in tok[1:5]]), np.array([float(t) for t in tok[5:8]]), int(tok[8]),
                                 tok[9], xys, np.array([int(t) for t in tok2[2::3]], dtype=np.int64))
    return images


def read_images_binary(path) -> dict:
    """images.bin: uint64 count; per image int32 id, 4 float64 qvec, 3 float64 tvec, int32 camera id, the name up to a zero byte,
    uint64 n, then n x (float64 x, float64 y, int64 point3D id)"""
    images = {}
    with open(path, "rb") as f:
        (count,) = _unpack(f, "<Q")
        for _ in range(count):
            head = _unpack(f, "<i7di")
            name = bytearray()
            while True:
                ch = f.read(1)
                if not ch:
                    raise ValueError(f"{path}: file ends inside an image name")
                if ch == b"\x00":
                    break
                name += ch
            (n,) = _unpack(f, "<Q")
            rec = np.frombuffer(f.read(24 * n), dtype=np.dtype([("x", "<f8"), ("y", "<f8"), ("id", "<i8")]))
            if rec.shape[0] != n:
                raise ValueError(f"{path}: file ends inside the observations of image {head[0]}")
            xys = np.stack([rec["x"], rec["y"]], axis=1).astype(np.float64)
            images[head[0]] = Image(head[0], np.array(head[1:5]), np.array(head[5:8]), head[8], name.decode("utf-8"), xys,
                                    rec["id"].astype(np.int64))
    return images


def read_model(path, ext: str = ""):
    """(cameras, images) of the model in `path`; ext "", ".txt" or ".bin" ("" = whichever is there, text first as the drivers look)"""
    path = Path(path)
    if ext == "":
        ext = ".txt" if (path / "cameras.txt").exists() else ".bin"
    if ext not in (".txt", ".bin") or not (path / f"cameras{ext}").exists() or not (path / f"images{ext}").exists():
        raise ValueError(f"Could not find cameras{ext or '.txt / .bin'} and images{ext} in {path}")
    if ext == ".txt":
        return read_cameras_text(path / "cameras.txt"), read_images_text(path / "images.txt")
    return read_cameras_binary(path / "cameras.bin"), read_images_binary(path / "images.bin")


def qvec2rotmat(qvec) -> np.ndarray:
    """unit quaternion (w, x, y, z) -> rotation matrix"""
    w, x, y, z = qvec[0], qvec[1], qvec[2], qvec[3]
    return np.array([[1 - 2 * y * y - 2 * z * z, 2 * x * y - 2 * w * z, 2 * z * x + 2 * w * y],
                     [2 * x * y + 2 * w * z, 1 - 2 * x * x - 2 * z * z, 2 * y * z - 2 * w * x],
                     [2 * z * x - 2 * w * y, 2 * y * z + 2 * w * x, 1 - 2 * x * x - 2 * y * y]])


# ---- cameras ----
_PERSPECTIVE = {  # model -> positions of (fl_x, fl_y, cx, cy, k1, k2, p1, p2) in params, None = 0
    "SIMPLE_PINHOLE": (0, 0, 1, 2, None, None, None, None), "PINHOLE": (0, 1, 2, 3, None, None, None, None),
    "SIMPLE_RADIAL": (0, 0, 1, 2, 3, None, None, None), "RADIAL": (0, 0, 1, 2, 3, 4, None, None), "OPENCV": (0, 1, 2, 3, 4, 5, 6, 7)}
_N_DIST = {"SIMPLE_PINHOLE": 0, "PINHOLE": 0, "SIMPLE_RADIAL": 1, "RADIAL": 2, "OPENCV": 4}


def camera_params(camera) -> dict:
    """Camera -> {w, h, fl_x, fl_y, cx, cy, k1, k2, p1, p2, model} for the perspective models; anything else raises ValueError"""
    where = _PERSPECTIVE.get(camera.model)
    if where is None:
        raise ValueError(f"camera model {camera.model!r} is not supported: perspective only (SIMPLE_PINHOLE, PINHOLE, SIMPLE_RADIAL, "
                         "RADIAL, OPENCV)")
    out = {"w": camera.width, "h": camera.height}
    for key, pos in zip(("fl_x", "fl_y", "cx", "cy", "k1", "k2", "p1", "p2"), where):
        out[key] = 0.0 if pos is None else float(camera.params[pos])
    out["model"] = camera.model
    return out


def rotation_matrix_between(a, b) -> np.ndarray:
    """the rotation that turns direction a into direction b (Rodrigues' formula about a x b)"""
    a = a / np.linalg.norm(a)
    b = b / np.linalg.norm(b)
    axis = np.cross(a, b)
    if np.sum(np.abs(axis)) < 1e-6:          # parallel: any axis perpendicular to a
        axis = np.cross(a, np.array([1.0, 0, 0]) if abs(a[0]) < 1e-6 else np.array([0, 1.0, 0]))
    axis = axis / np.linalg.norm(axis)
    skew = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    theta = np.arccos(np.clip(np.dot(a, b), -1, 1))
    return np.eye(3) + np.sin(theta) * skew + (1 - np.cos(theta)) * (skew @ skew)


def auto_orient_and_center_poses(poses: np.ndarray, method: str = "up", center_method: str = "poses"):
    """(n,4,4) camera-to-world -> ((n,3,4) oriented and centred poses, (3,4) transform).  method "up": the mean up vector (column 1)
    is turned onto +z; "none": no rotation.  center_method "poses": the mean camera position moves to the origin; "none": it stays."""
    if method in ("pca", "vertical"):
        raise NotImplementedError(f"auto_orient_and_center_poses: method {method!r} is not implemented ('pca' cannot run in the reference "
                                  "either and no driver uses 'vertical'); use 'up' or 'none'")
    if center_method == "focus":
        raise NotImplementedError("auto_orient_and_center_poses: center_method 'focus' is not implemented (no driver uses it); use "
                                  "'poses' or 'none'")
    if method not in ("up", "none"):
        raise ValueError(f"Unknown value for method: {method}")
    if center_method not in ("poses", "none"):
        raise ValueError(f"Unknown value for center_method: {center_method}")
    mean_origin = np.mean(poses[..., :3, 3], axis=0)
    translation = mean_origin if center_method == "poses" else np.zeros_like(mean_origin)
    if method == "up":
        up = np.mean(poses[:, :3, 1], axis=0)
        up = up / np.linalg.norm(up)
        rotation = rotation_matrix_between(up, np.array([0, 0, 1]))
        transform = np.concatenate([rotation, rotation @ -translation[..., None]], axis=-1)
    else:
        transform = np.eye(4)
        transform[:3, 3] = -translation
        transform = transform[:3, :]
    return transform @ poses, transform


# ---- undistortion: the new camera ----
def _undistort_grid(K: np.ndarray, dist: np.ndarray, size: tuple) -> tuple:
    """the 9 x 9 grid of fp32 image points -> normalised undistorted coordinates (x, y), float64 (9,9), row j = grid row"""
    W, H = size
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    k1, k2, p1, p2 = (float(d) for d in dist)
    i = np.arange(9, dtype=np.float32)
    px = (i * np.float32(W - 1) / np.float32(8)).astype(np.float64)[None, :].repeat(9, 0)
    py = (i * np.float32(H - 1) / np.float32(8)).astype(np.float64)[:, None].repeat(9, 1)
    x0, y0 = (px - cx) * (1.0 / fx), (py - cy) * (1.0 / fy)
    x, y = x0.copy(), y0.copy()
    live = np.ones_like(x, dtype=bool)
    for _ in range(5):
        r2 = x * x + y * y
        icd = 1.0 / (1 + (k2 * r2 + k1) * r2)
        bad = live & (icd < 0)                       # the model folds over: the point keeps its distorted position
        x[bad], y[bad] = x0[bad], y0[bad]
        live &= ~bad
        dx = 2 * p1 * x * y + p2 * (r2 + 2 * x * x)
        dy = p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
        x = np.where(live, (x0 - dx) * icd, x)
        y = np.where(live, (y0 - dy) * icd, y)
    return x, y


def _inner_rectangle(gx: np.ndarray, gy: np.ndarray) -> tuple:
    """fp32-rounded grid -> (x, y, width, height) of the largest rectangle inside its outline, float64"""
    gx, gy = gx.astype(np.float32).astype(np.float64), gy.astype(np.float32).astype(np.float64)
    x0, x1, y0, y1 = gx[:, 0].max(), gx[:, -1].min(), gy[0, :].max(), gy[-1, :].min()
    return x0, y0, x1 - x0, y1 - y0


def _roi_of(K, dist, new_K, size) -> tuple:
    W, H = size
    gx, gy = _undistort_grid(K, dist, size)
    rect = _inner_rectangle(new_K[0, 0] * gx + new_K[0, 2], new_K[1, 1] * gy + new_K[1, 2])
    if not all(np.isfinite(rect)):
        return (0, 0, 0, 0)
    x, y, w, h = (int(np.rint(v)) for v in rect)               # half to even
    xa, ya, xb, yb = max(x, 0), max(y, 0), min(x + w, W), min(y + h, H)
    return (xa, ya, xb - xa, yb - ya) if xb > xa and yb > ya else (0, 0, 0, 0)


def optimal_new_camera(K, dist, size) -> tuple:
    """getOptimalNewCameraMatrix(K, dist, (W, H), alpha = 0) restated in float64: -> (K_new (3,3), roi (x, y, w, h) integers).
    dist = (k1, k2, p1, p2).  See the module docstring; not verified against OpenCV."""
    K = np.asarray(K, dtype=np.float64)
    dist = np.asarray(dist, dtype=np.float64).reshape(-1)
    if dist.shape[0] != 4:
        raise ValueError(f"optimal_new_camera takes (k1, k2, p1, p2); got {dist.shape[0]} coefficients")
    W, H = int(size[0]), int(size[1])
    gx, gy = _undistort_grid(K, dist, (W, H))
    x0, y0, width, height = _inner_rectangle(gx, gy)
    fx, fy = (W - 1) / width, (H - 1) / height
    new_K = np.array([[fx, 0, -fx * x0], [0, fy, -fy * y0], [0, 0, 1]], dtype=np.float64)
    return new_K, _roi_of(K, dist, new_K, (W, H))


@dataclass
class UndistortCamera:
    """one camera as `undistort_frames` takes it.  dist: () for a camera without distortion (its frames are copied through the ROI
    unless new_K is given) or (k1, k2, p1, p2); size (W, H), None = the frames' size; new_K / roi None = `optimal_new_camera`'s
    (roi of an undistorted camera: the whole frame)"""
    K: np.ndarray
    dist: np.ndarray = field(default_factory=lambda: np.zeros(0))
    size: Optional[tuple] = None
    new_K: Optional[np.ndarray] = None
    roi: Optional[tuple] = None


def _resolve(cam: UndistortCamera, W: int, H: int, new_K, roi):
    """-> (table row (16,) float64, roi (x, y, w, h))"""
    if cam.size is not None and (int(cam.size[0]), int(cam.size[1])) != (W, H):
        raise ValueError(f"undistort_frames: frames are {W} x {H} but their camera is {cam.size[0]} x {cam.size[1]}")
    K = np.asarray(cam.K, dtype=np.float64)
    dist = np.asarray(cam.dist, dtype=np.float64).reshape(-1)
    new_K = cam.new_K if new_K is None else new_K
    roi = cam.roi if roi is None else roi
    row = np.zeros(_lib.GSR_UNDISTORT_CAM_DOUBLES)
    row[0:4] = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    if dist.shape[0] == 0 and new_K is None:
        roi = (0, 0, W, H) if roi is None else roi
        row[8:12] = row[0:4]
    else:
        if dist.shape[0] not in (0, 4):
            raise ValueError(f"undistort_frames: distortion is () or (k1, k2, p1, p2); got {dist.shape[0]} coefficients")
        d4 = dist if dist.shape[0] == 4 else np.zeros(4)
        if new_K is None:
            new_K, roi_default = optimal_new_camera(K, d4, (W, H))
        else:
            new_K = np.asarray(new_K, dtype=np.float64)
            roi_default = None
        if roi is None:
            roi = roi_default if roi_default is not None else _roi_of(K, d4, new_K, (W, H))
        row[4:8] = d4
        row[8:12] = new_K[0, 0], new_K[1, 1], new_K[0, 2], new_K[1, 2]
        row[14] = 1.0
    roi = tuple(int(v) for v in roi)
    if len(roi) != 4 or abs(roi[0]) > 32767 or abs(roi[1]) > 32767:
        raise ValueError(f"undistort_frames: bad ROI {roi}")
    row[12:14] = roi[0], roi[1]
    return row, roi


def _pick(override, key, index):
    """a per-call override: None, one value for every camera, or a dict by camera key / a list by camera position"""
    if isinstance(override, dict):
        return override.get(key)
    if isinstance(override, list):
        return override[index]
    return override


def _source_maps(row: np.ndarray, roi_w: int, roi_h: int):
    """the map of one camera over its ROI window: (mx, my) fp32 (roi_h, roi_w)"""
    fx, fy, cx, cy, k1, k2, p1, p2, nfx, nfy, ncx, ncy, x0, y0 = (float(v) for v in row[:14])
    with np.errstate(all="ignore"):                  # a camera whose map leaves the number range gives inf / NaN, which sample as 0
        x = ((np.arange(roi_w, dtype=np.float64) + x0) - ncx) / nfx
        y = ((np.arange(roi_h, dtype=np.float64) + y0) - ncy) / nfy
        x, y = x[None, :], y[:, None]
        r2 = x * x + y * y
        kr = 1.0 + (k2 * r2 + k1) * r2
        xy2 = (2.0 * x) * y
        xd = (x * kr + p1 * xy2) + p2 * (r2 + 2.0 * (x * x))
        yd = (y * kr + p1 * (r2 + 2.0 * (y * y))) + p2 * xy2
        return (fx * xd + cx).astype(np.float32), (fy * yd + cy).astype(np.float32)


def _remap_host(img: np.ndarray, mx: np.ndarray, my: np.ndarray) -> np.ndarray:
    """uint8 (H,W,3) sampled at (mx, my) by the fixed-point rule of the module docstring -> uint8 (h,w,3)"""
    H, W = img.shape[:2]
    with np.errstate(over="ignore", invalid="ignore"):
        fsx, fsy = mx * np.float32(32), my * np.float32(32)
        ok = (np.abs(fsx) < np.float32(2 ** 30)) & (np.abs(fsy) < np.float32(2 ** 30))       # NaN and inf fail the comparison too
    sx = np.rint(np.where(ok, fsx, np.float32(0))).astype(np.int32)
    sy = np.rint(np.where(ok, fsy, np.float32(0))).astype(np.int32)
    ix, iy, a, b = sx >> 5, sy >> 5, (sx & 31).astype(np.int64)[..., None], (sy & 31).astype(np.int64)[..., None]

    def tap(xx, yy):
        inside = (xx >= 0) & (xx < W) & (yy >= 0) & (yy < H)
        return img[np.clip(yy, 0, H - 1), np.clip(xx, 0, W - 1)].astype(np.int64) * inside[..., None]
    acc = (32 - a) * (32 - b) * tap(ix, iy) + a * (32 - b) * tap(ix + 1, iy) + (32 - a) * b * tap(ix, iy + 1) + a * b * tap(ix + 1, iy + 1) + 512
    return ((acc >> 10) * ok[..., None]).astype(np.uint8)


def _copy_host(img: np.ndarray, x0: int, y0: int, roi_w: int, roi_h: int) -> np.ndarray:
    H, W = img.shape[:2]
    xx, yy = np.arange(roi_w) + x0, np.arange(roi_h) + y0
    inside = ((yy >= 0) & (yy < H))[:, None] & ((xx >= 0) & (xx < W))[None, :]
    return img[np.clip(yy, 0, H - 1)[:, None], np.clip(xx, 0, W - 1)[None, :]] * inside[..., None].astype(np.uint8)


def undistort_table(frames_hw: tuple, scene_or_cams, frame_cam, new_K=None, roi=None):
    """-> (table (n_cams,16) float64 as gsr_undistort reads it, frame -> row int32 (N), (roi_w, roi_h), rois per row)"""
    H, W = frames_hw
    cams = scene_or_cams.undistort_cameras() if isinstance(scene_or_cams, ColmapScene) else scene_or_cams
    if isinstance(cams, UndistortCamera):
        cams = [cams]
    keys = list(cams.keys()) if isinstance(cams, dict) else list(range(len(cams)))
    rows, rois = [], []
    for i, key in enumerate(keys):
        row, r = _resolve(cams[key], W, H, _pick(new_K, key, i), _pick(roi, key, i))
        rows.append(row)
        rois.append(r)
    position = {key: i for i, key in enumerate(keys)}
    fc = [int(c) for c in (frame_cam.reshape(-1).tolist() if isinstance(frame_cam, (Tensor, np.ndarray)) else frame_cam)]
    for c in fc:
        if c not in position:
            raise ValueError(f"undistort_frames: frame camera {c} is not among the cameras {keys}")
    index = np.array([position[c] for c in fc], dtype=np.int32)
    sizes = {rois[i][2:] for i in index}
    if len(sizes) != 1:
        raise ValueError(f"undistort_frames: the frames of one call must share one ROI size; got {sorted(sizes)}")
    roi_w, roi_h = sizes.pop()
    if roi_w < 1 or roi_h < 1:
        raise ValueError(f"undistort_frames: empty ROI {roi_w} x {roi_h}")
    if roi_w > 32767 or roi_h > 32767 or W > 32767 or H > 32767:
        raise ValueError(f"undistort_frames: frames {W} x {H} / ROI {roi_w} x {roi_h} above 32767")
    return np.stack(rows), index, (roi_w, roi_h), rois


def undistort_frames(frames: Tensor, scene_or_cams, frame_cam, *, new_K=None, roi=None) -> Tensor:
    """uint8 frames (n,H,W,3) -> uint8 (n, roi_h, roi_w, 3): the ROI window of every frame undistorted by its camera.
      scene_or_cams  a `ColmapScene`, or `UndistortCamera`s as a dict by camera id / a list / one camera
      frame_cam      per frame the camera id (dict, scene) or position (list)
      new_K, roi     overrides of the computed new camera matrix / ROI (x, y, w, h): one value for all cameras, or a dict / list like the cameras
    The ROI size is common to all frames of a call (ValueError otherwise), its origin is per camera.  Device tensors go through ONE
    `gsr_undistort` launch, CPU tensors through the numpy restatement; both give the same bytes."""
    if frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[-1] != 3:
        raise ValueError(f"undistort_frames takes uint8 (n,H,W,3); got {frames.dtype} {tuple(frames.shape)}")
    N, H, W, _ = frames.shape
    table, index, (roi_w, roi_h), _ = undistort_table((H, W), scene_or_cams, frame_cam, new_K, roi)
    if index.shape[0] != N:
        raise ValueError(f"undistort_frames: {index.shape[0]} frame cameras for {N} frames")
    if N == 0:
        return torch.empty((0, roi_h, roi_w, 3), dtype=torch.uint8, device=frames.device)
    src = frames.detach().contiguous()
    if src.is_cuda:
        lib, dev = _lib.load(), src.device
        cams = torch.from_numpy(table).to(dev)
        out = torch.empty((N, roi_h, roi_w, 3), dtype=torch.uint8, device=dev)
        _lib.check(lib.gsr_undistort(src.data_ptr(), N, H, W, cams.data_ptr(), table.shape[0], index.ctypes.data, roi_w, roi_h, out.data_ptr(),
                                     C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)), "gsr_undistort")
        return out
    imgs = src.numpy()
    out = np.empty((N, roi_h, roi_w, 3), np.uint8)
    maps = {}
    for n in range(N):
        row = table[index[n]]
        if row[14] == 0.0:
            out[n] = _copy_host(imgs[n], int(row[12]), int(row[13]), roi_w, roi_h)
            continue
        if int(index[n]) not in maps:
            maps[int(index[n])] = _source_maps(row, roi_w, roi_h)
        out[n] = _remap_host(imgs[n], *maps[int(index[n])])
    return torch.from_numpy(out)


# ---- the scene ----
@dataclass
class ColmapScene:
    image_names: list            # sorted by name
    image_paths: list
    camtoworlds: np.ndarray      # (n,4,4) float64, oriented ("up", "poses") and scaled by scale_factor
    camera_ids: list             # per image
    Ks: dict                     # camera id -> (3,3) pixels; the UNDISTORTED matrix for a camera with distortion
    dist: dict                   # camera id -> () or (k1, k2, p1, p2), float64 holding fp32 values
    sizes: dict                  # camera id -> (width, height)
    rois: dict                   # camera id -> (x, y, w, h) of the valid pixels (the whole frame without distortion)
    transform: np.ndarray        # (3,4) of auto_orient_and_center_poses
    scale_factor: float
    raw_Ks: dict = field(default_factory=dict)     # camera id -> (3,3) of the distorted camera as COLMAP gives it
    name: str = ""

    def undistort_cameras(self) -> dict:
        return {cid: UndistortCamera(self.raw_Ks[cid], self.dist[cid], self.sizes[cid], self.Ks[cid] if len(self.dist[cid]) else None,
                                     self.rois[cid]) for cid in self.Ks}


def load_colmap_scene(data_dir, image_dir: str = "images") -> ColmapScene:
    """A COLMAP capture (`sparse/0` or `sparse`, text or binary, frames under `image_dir`) -> `ColmapScene`: images ordered by id and
    then sorted by name, camera-to-world poses oriented ("up", "poses") and scaled so that the largest |translation| is 1, per
    camera the intrinsics, the distortion rounded through fp32, and for cameras with distortion the new camera matrix and ROI."""
    data_dir = Path(data_dir)
    model_dir = data_dir / "sparse" / "0"
    if not model_dir.exists():
        model_dir = data_dir / "sparse"
    if not model_dir.exists():
        raise ValueError(f"COLMAP directory {model_dir} does not exist")
    cameras, images = read_model(model_dir)
    if len(images) == 0:
        raise ValueError("No images found in COLMAP.")
    parsed = {cid: camera_params(cam) for cid, cam in cameras.items()}
    ids = sorted(images.keys())
    bottom = np.array([0, 0, 0, 1]).reshape(1, 4)
    w2c, camera_ids = [], []
    raw_Ks, dist, sizes = {}, {}, {}
    for im_id in ids:
        im = images[im_id]
        w2c.append(np.concatenate([np.concatenate([qvec2rotmat(im.qvec), im.tvec.reshape(3, 1)], 1), bottom], axis=0))
        camera_ids.append(im.camera_id)
        cam = parsed[im.camera_id]
        raw_Ks[im.camera_id] = np.array([[cam["fl_x"], 0, cam["cx"]], [0, cam["fl_y"], cam["cy"]], [0, 0, 1]])
        sizes[im.camera_id] = (cam["w"], cam["h"])
        coeffs = [cam["k1"], cam["k2"], cam["p1"], cam["p2"]] if _N_DIST[cam["model"]] else []
        dist[im.camera_id] = np.array(coeffs, dtype=np.float32).astype(np.float64)
    camtoworlds = np.linalg.inv(np.stack(w2c, axis=0))
    names = [images[k].name for k in ids]
    order = np.argsort(names)
    names = [names[i] for i in order]
    camtoworlds = camtoworlds[order]
    camera_ids = [camera_ids[i] for i in order]
    if not (data_dir / image_dir).exists():
        raise ValueError(f"Image folder {data_dir / image_dir} does not exist.")
    paths = [os.path.join(str(data_dir / image_dir), f) for f in names]
    camtoworlds, transform = auto_orient_and_center_poses(camtoworlds, method="up", center_method="poses")
    scale_factor = 1.0
    scale_factor /= float(np.max(np.abs(camtoworlds[:, :3, 3])))
    camtoworlds[:, :3, 3] *= scale_factor
    camtoworlds = np.concatenate((camtoworlds, np.repeat(bottom[np.newaxis, :], camtoworlds.shape[0], axis=0)), axis=1)
    Ks, rois = {}, {}
    for cid in raw_Ks:
        if len(dist[cid]) == 0:
            Ks[cid], rois[cid] = raw_Ks[cid], (0, 0, sizes[cid][0], sizes[cid][1])
        else:
            Ks[cid], rois[cid] = optimal_new_camera(raw_Ks[cid], dist[cid], sizes[cid])
    return ColmapScene(names, paths, camtoworlds, camera_ids, Ks, dist, sizes, rois, transform, scale_factor, raw_Ks, data_dir.name)


def select_colmap_views(ctx_indices, num_ctx_views: int):
    """infer_model_colmap.py:480-498 -> (context, target) int64 tensors.  Fewer context indices than views (and more than two views):
    the views are spread evenly between the first and the last index; more: ValueError.  The targets are every index from the first
    context view up to (not including) the last that is no context view -- or that whole range when nothing is left."""
    ctx = torch.as_tensor(ctx_indices, dtype=torch.int64).reshape(-1)
    left, right = int(ctx[0]), int(ctx[-1])
    if ctx.shape[0] < num_ctx_views:
        if num_ctx_views > 2:
            ctx = torch.linspace(left, right, num_ctx_views).long()
    elif ctx.shape[0] > num_ctx_views:
        raise ValueError("You gave more context indices than required!")
    target = torch.arange(left, right)
    keep = ~torch.isin(target, ctx)
    return ctx, (target[keep] if keep.any() else target)


def read_frames(paths: Sequence) -> Tensor:
    """image files -> uint8 (n,H,W,3) (the first three channels); frames of unequal size raise ValueError"""
    from PIL import Image as PILImage
    frames = []
    for p in paths:
        with PILImage.open(p) as im:
            arr = np.asarray(im if im.mode in ("RGB", "RGBA") else im.convert("RGB"))[..., :3]
        if frames and arr.shape != frames[0].shape:
            raise ValueError(f"read_frames: {p} is {arr.shape[1]} x {arr.shape[0]}, the frames before it {frames[0].shape[1]} x {frames[0].shape[0]}")
        frames.append(np.ascontiguousarray(arr, dtype=np.uint8))
    return torch.from_numpy(np.stack(frames)) if frames else torch.empty((0, 0, 0, 3), dtype=torch.uint8)
