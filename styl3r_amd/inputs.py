"""Scene inputs: decoded frames and raw cameras -> the example / batch dict the encoder, `TrainStep`, `test_step` and `stylize_scene`
take.  The names and semantics are the reference's: src/dataset/shims/crop_shim.py (rescale, center_crop, rescale_and_crop,
apply_crop_shim), src/dataset/shims/augmentation_shim.py (reflect_views, apply_augmentation_shim, apply_style_image_augmentation and
its `_larger` twin) and the batch assembly of dataset_re10k_style.py:165-213 / infer_model_colmap.py:513-589.

The reference rescales one image at a time on the host: float -> uint8 -> PIL `resize(..., LANCZOS)` -> float64 / 255 -> float32.
Here ALL images of a call go through one `gsr_resample_crop` (csrc/gsr_inputs.hip) when they live on the device, and through an
integer restatement of the same rules in numpy when they live on the CPU; both read the SAME axis plans, built on the host by
`gsr_resample_plan` (float64, libm's sin).  The result is bit-equal to the reference's PIL path (tests/golden/scene_inputs.npz).

The rules (PIL's 8-bit resize, restated):
  quantise   byte = uint8(clip(x * 255, 0, 255)), fp32 product, truncating cast.  NaN -> 0 (the reference leaves NaN undefined: its cast
             of a NaN to uint8 is whatever the platform does).  uint8 input is taken as it is.
  axis plan  per output index the first tap, the tap count and normalised Lanczos-3 weights in 22-bit fixed point (include/gsr.h)
  passes     horizontal first (if the width changes), then vertical (if the height changes); byte = clamp((2^21 + sum byte * coeff) >> 22);
             the image between the passes is bytes
  float      float32(double(byte) / 255)
  flip       at the source read, before the filter (the reference reflects before it rescales; plans and crop offsets are not symmetric)

Reading `.torch` chunks and decoding their JPEG frames is styl3r_amd/dataset.py, undistortion and the COLMAP parsers
styl3r_amd/colmap.py; the view samplers are in styl3r_amd/views.py and `example_from_scene` runs one in front of `prepare_example`.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from collections import OrderedDict
from functools import lru_cache
from typing import Optional, Sequence

import numpy as np
import torch
from torch import Tensor

from . import _lib

_BITS = 22


class SkipExample(Exception):
    """the example fails a gate of the loader (baseline outside [baseline_min, baseline_max], field of view above max_fov): the
    reference's dataset `continue`s, its inference drivers assert"""


@dataclass
class InputCfg:
    """the fields of the reference's RE10K-style dataset config the transform reads (config/dataset/re10k_style.yaml + base_dataset.yaml;
    near / far are DatasetRE10kStyle's class attributes)"""
    input_image_shape: tuple = (256, 256)
    make_baseline_1: bool = True
    baseline_min: float = 1e-3
    baseline_max: float = 1e10
    relative_pose: bool = True
    max_fov: float = 100.0
    near: float = 0.1
    far: float = 100.0
    augment: bool = True
    style_size: int = 256          # 352: apply_style_image_augmentation_larger


# ---- axis plans ----
@lru_cache(maxsize=256)
def resample_plan(n: int, m: int):
    """(ksize, bounds (m,2) int32, coeffs (m,ksize) int32) of one axis, from the library's host code"""
    lib = _lib.load()
    k = C.c_int32(0)
    _lib.check(lib.gsr_resample_plan(int(n), int(m), C.byref(k), None, None), "gsr_resample_plan")
    bounds = np.zeros((m, 2), np.int32)
    coeffs = np.zeros((m, k.value), np.int32)
    _lib.check(lib.gsr_resample_plan(int(n), int(m), C.byref(k), bounds.ctypes.data, coeffs.ctypes.data), "gsr_resample_plan")
    bounds.setflags(write=False)
    coeffs.setflags(write=False)
    return k.value, bounds, coeffs


_DEVICE_PLANS: "OrderedDict" = OrderedDict()      # (n, m, device) -> int32 buffer, least recently used first
_DEVICE_PLANS_MAX = 64                            # a plan is m * (2 + ksize) words: 64 plans of RE10K's size are under 2 MB


def _device_plan(n: int, m: int, dev: torch.device) -> Tensor:
    """bounds then coefficients as one int32 buffer on `dev`.  Built once per (n, m, device) while it stays among the _DEVICE_PLANS_MAX
    most recently used plans (a stream of style images of ever new sizes does not grow the cache); the upload is ordered on the
    stream that is current at that moment, like every later use through torch."""
    key = (n, m, str(dev))
    plan = _DEVICE_PLANS.get(key)
    if plan is None:
        _, bounds, coeffs = resample_plan(n, m)
        plan = torch.from_numpy(np.concatenate([bounds.reshape(-1), coeffs.reshape(-1)])).to(dev)
        _DEVICE_PLANS[key] = plan
        while len(_DEVICE_PLANS) > _DEVICE_PLANS_MAX:
            _DEVICE_PLANS.popitem(last=False)
    else:
        _DEVICE_PLANS.move_to_end(key)
    return plan


# ---- the core: N images of one size -> window of the scaled images ----
def _as_source(images: Tensor):
    """-> (contiguous source, is_f32, batch shape, H, W): uint8 (..., H, W, 3) interleaved or float (..., 3, H, W) planar"""
    if images.dtype == torch.uint8:
        if images.dim() < 3 or images.shape[-1] != 3:
            raise ValueError(f"uint8 frames are (..., H, W, 3); got {tuple(images.shape)}")
        *batch, H, W, _ = images.shape
        return images.detach().reshape(-1, H, W, 3).contiguous(), False, tuple(batch), H, W
    if not images.is_floating_point() or images.dim() < 3 or images.shape[-3] != 3:
        raise ValueError(f"float images are (..., 3, H, W); got {images.dtype} {tuple(images.shape)}")
    *batch, _, H, W = images.shape
    return images.detach().reshape(-1, 3, H, W).float().contiguous(), True, tuple(batch), H, W


def quantise(x: Tensor) -> Tensor:
    """float (any shape) -> uint8 by the reference's `(image * 255).clip(0, 255).type(torch.uint8)` in fp32; NaN -> 0"""
    v = (x.float() * 255).clip(min=0, max=255)
    return torch.where(torch.isnan(v), torch.zeros_like(v), v).to(torch.uint8)


def _filter_last_axis(img: np.ndarray, n_in: int, m_out: int, lo: int, hi: int) -> np.ndarray:
    """uint8 (..., n_in) -> uint8 (..., hi - lo): outputs lo..hi-1 of the (n_in -> m_out) plan along the last axis"""
    _, bounds, coeffs = resample_plan(n_in, m_out)
    b, c = bounds[lo:hi], coeffs[lo:hi]
    idx = np.minimum(b[:, :1] + np.arange(c.shape[1], dtype=np.int32)[None], n_in - 1)       # taps behind the count have coefficient 0
    acc = (img[..., idx].astype(np.int32) * c).sum(-1, dtype=np.int32) + (1 << (_BITS - 1))
    return np.clip(acc >> _BITS, 0, 255).astype(np.uint8)


def _resample_crop_host(src: Tensor, is_f32: bool, H: int, W: int, sh: int, sw: int, top: int, left: int, oh: int, ow: int, flip) -> Tensor:
    out = np.empty((src.shape[0], 3, oh, ow), np.float32)
    for n in range(src.shape[0]):
        img = (quantise(src[n]) if is_f32 else src[n].permute(2, 0, 1)).numpy()             # (3,H,W) bytes
        if flip is not None and flip[n]:
            img = img[..., ::-1]
        img = _filter_last_axis(img, W, sw, left, left + ow) if sw != W else img[..., left:left + ow]
        img = img.transpose(0, 2, 1)                                                        # (3,ow,H)
        img = _filter_last_axis(img, H, sh, top, top + oh) if sh != H else img[..., top:top + oh]
        out[n] = (img.transpose(0, 2, 1).astype(np.float64) / 255).astype(np.float32)
    return torch.from_numpy(out)


def _stream(dev) -> C.c_void_p:
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _resample_crop_device(src: Tensor, is_f32: bool, H: int, W: int, sh: int, sw: int, top: int, left: int, oh: int, ow: int, flip,
                          flags: int) -> Tensor:
    lib, dev, N = _lib.load(), src.device, src.shape[0]
    px = _device_plan(W, sw, dev) if sw != W else None
    py = _device_plan(H, sh, dev) if sh != H else None
    nbytes = lib.gsr_resample_scratch_bytes(N, H, W, sh, sw, top, left, oh, ow)
    if nbytes == 0:
        raise ValueError(f"resample_crop: bad dimensions N {N}, {H}x{W} -> {sh}x{sw}, window ({top}, {left}, {oh}, {ow})")
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    out = torch.empty((N, 3, oh, ow), dtype=torch.float32, device=dev)
    fl = torch.tensor([int(bool(f)) for f in flip], dtype=torch.int32).to(dev) if flip is not None and any(flip) else None
    _lib.check(lib.gsr_resample_crop(src.data_ptr(), int(is_f32), N, H, W, px.data_ptr() if px is not None else None, sw,
                                     py.data_ptr() if py is not None else None, sh, top, left, oh, ow,
                                     fl.data_ptr() if fl is not None else None, scratch.data_ptr(), nbytes, out.data_ptr(), int(flags),
                                     _stream(dev)), "gsr_resample_crop")
    return out


def resample_crop(images: Tensor, scaled: tuple, window: Optional[tuple] = None, flip=None, flags: int = 0) -> Tensor:
    """All images of one size in one call: uint8 (..., H, W, 3) or float (..., 3, H, W) -> float (..., 3, out_h, out_w), the window
    (top, left, out_h, out_w) of the images rescaled to `scaled` = (h, w) (default: the whole scaled image).  `flip`: None, one bool for
    all, or one per image; a flipped image is mirrored along x BEFORE it is rescaled.  Float inputs keep their dtype, bytes give fp32.
    `flags`: _lib.GSR_RESAMPLE_DIRECT (device path, tests)."""
    src, is_f32, batch, H, W = _as_source(images)
    sh, sw = int(scaled[0]), int(scaled[1])
    top, left, oh, ow = (0, 0, sh, sw) if window is None else map(int, window)
    if sh < 1 or sw < 1 or top < 0 or left < 0 or oh < 1 or ow < 1 or top + oh > sh or left + ow > sw:
        raise ValueError(f"resample_crop: window ({top}, {left}, {oh}, {ow}) is not inside the scaled image {sh} x {sw}")
    N = src.shape[0]
    if flip is not None:
        flip = [bool(flip)] * N if isinstance(flip, (bool, int)) else [bool(f) for f in (flip.reshape(-1).tolist() if isinstance(flip, Tensor) else flip)]
        if len(flip) != N:
            raise ValueError(f"resample_crop: {len(flip)} flip flags for {N} images")
    if N == 0:
        out = torch.empty((0, 3, oh, ow), dtype=torch.float32, device=src.device)
    elif src.is_cuda:
        out = _resample_crop_device(src, is_f32, H, W, sh, sw, top, left, oh, ow, flip, flags)
    else:
        out = _resample_crop_host(src, is_f32, H, W, sh, sw, top, left, oh, ow, flip)
    out = out.reshape(*batch, 3, oh, ow)
    return out.to(images.dtype) if is_f32 else out


# ---- crop_shim.py ----
def rescale(image: Tensor, shape: tuple) -> Tensor:
    """crop_shim.rescale: (…, 3, h_in, w_in) float (or (…, h_in, w_in, 3) uint8) -> (…, 3, h, w) through the 8-bit Lanczos resize.  A size
    that does not change is not filtered, but float values are still quantised to the 1/255 grid."""
    return resample_crop(image, shape)


def _image_hw(images: Tensor):
    return tuple(images.shape[-3:-1]) if images.dtype == torch.uint8 else tuple(images.shape[-2:])


def _crop_intrinsics(intrinsics: Tensor, h_in: int, w_in: int, h_out: int, w_out: int) -> Tensor:
    """normalised intrinsics of the cropped image: a crop keeps the focal length in pixels, so fx and fy grow by size_in / size_out.  The
    products are formed as the reference forms them (an in-place multiply by a Python float), so the fp32 result has its bits."""
    out = intrinsics.clone()
    out[..., 0, 0] *= w_in / w_out
    out[..., 1, 1] *= h_in / h_out
    return out


def center_crop(images: Tensor, intrinsics: Tensor, shape: tuple):
    """crop_shim.center_crop on prepared float images (…, c, h, w) -> (window, intrinsics).  The window starts at the floor of half the
    surplus, so an odd surplus leaves the extra row / column at the far side."""
    h_in, w_in = images.shape[-2:]
    h_out, w_out = shape
    top, left = (h_in - h_out) // 2, (w_in - w_out) // 2
    return images[..., top:top + h_out, left:left + w_out], _crop_intrinsics(intrinsics, h_in, w_in, h_out, w_out)


def scaled_size(h_in: int, w_in: int, shape: tuple):
    """the size rescale_and_crop rescales to before it crops to `shape`: the larger of the two ratios is applied to both sides, each
    rounded by Python's round(); one side must then land on its target (the same two conditions the reference asserts)"""
    h_out, w_out = shape
    assert h_out <= h_in and w_out <= w_in, f"rescale_and_crop only reduces: {h_in} x {w_in} -> {h_out} x {w_out}"
    factor = max(h_out / h_in, w_out / w_in)
    scaled = round(h_in * factor), round(w_in * factor)
    assert scaled[0] == h_out or scaled[1] == w_out, f"neither side of the scaled image {scaled} lands on {h_out} x {w_out}"
    return scaled


def rescale_and_crop(images: Tensor, intrinsics: Tensor, shape: tuple, flip=None):
    """crop_shim.rescale_and_crop: every image (any leading batch axes) in ONE call; only the crop window is computed.
    `flip` (an addition): mirror images along x before the rescale, as reflect_views does ahead of the crop shim."""
    h_in, w_in = _image_hw(images)
    h_out, w_out = int(shape[0]), int(shape[1])
    h_scaled, w_scaled = scaled_size(h_in, w_in, (h_out, w_out))
    window = ((h_scaled - h_out) // 2, (w_scaled - w_out) // 2, h_out, w_out)
    return resample_crop(images, (h_scaled, w_scaled), window, flip), _crop_intrinsics(intrinsics, h_scaled, w_scaled, h_out, w_out)


def apply_crop_shim_to_views(views: dict, shape: tuple) -> dict:
    images, intrinsics = rescale_and_crop(views["image"], views["intrinsics"], shape)
    return {**views, "image": images, "intrinsics": intrinsics}


def apply_crop_shim(example: dict, shape: tuple) -> dict:
    """crop_shim.apply_crop_shim: the context and the target views of an example through `rescale_and_crop`, every other entry as it is"""
    return {**example, "context": apply_crop_shim_to_views(example["context"], shape),
            "target": apply_crop_shim_to_views(example["target"], shape)}


# ---- augmentation_shim.py ----
def style_scaled_size(H: int, W: int, size: int = 256):
    """the short side becomes `size`, the long side int(long / short * size) (the quotient first, as the reference forms it)"""
    if H < W:
        return size, int(W / H * size)
    return int(H / W * size), size


def apply_style_image_augmentation(style_image: Tensor, stage=None, size: int = 256) -> Tensor:
    """augmentation_shim.apply_style_image_augmentation (size = 352: `_larger`): the short side becomes `size`, the long side
    int(ratio * size), then a centre crop of size x size -- for every stage, as in the reference, whose train branch uses the centre crop
    too.  One kernel call: only the crop window is computed.
    The crop offset is torchvision's CenterCrop rule int(round((H - size) / 2.0)) -- Python's round-half-to-even, NOT the // 2 of
    `center_crop`.  torchvision is not a dependency of this package or its tests: that rule is restated here from torchvision's
    functional.center_crop, not recorded from a run of it."""
    H, W = _image_hw(style_image)
    hs, ws = style_scaled_size(H, W, size)
    top, left = int(round((hs - size) / 2.0)), int(round((ws - size) / 2.0))
    return resample_crop(style_image, (hs, ws), (top, left, size, size))


def reflect_extrinsics(extrinsics: Tensor) -> Tensor:
    """reflect @ extrinsics @ reflect with reflect = diag(-1, 1, 1, 1): row 0 and column 0 change sign ([0, 0] twice).  Exact; zeros come
    out as +0, as from the reference's matrix products."""
    sign = torch.ones(4, 4, dtype=extrinsics.dtype, device=extrinsics.device)
    sign[0, 1:] = -1
    sign[1:, 0] = -1
    return extrinsics * sign + 0.0


def reflect_views(views: dict) -> dict:
    return {**views, "image": views["image"].flip(-1), "extrinsics": reflect_extrinsics(views["extrinsics"])}


def apply_augmentation_shim(example: dict, generator: Optional[torch.Generator] = None) -> dict:
    """augmentation_shim.apply_augmentation_shim: ONE torch.rand(()) draw from `generator`; below 0.5 the example comes back as it is,
    otherwise context and target views are mirrored (`reflect_views`)"""
    keep = bool(torch.rand(tuple(), generator=generator) < 0.5)
    if keep:
        return example
    return {**example, "context": reflect_views(example["context"]), "target": reflect_views(example["target"])}


# ---- cameras (host, float64, rounded once) ----
def _inverse3(m: np.ndarray) -> np.ndarray:
    """(..., 3, 3) float64 -> inverse, by the adjugate: row i of the inverse is the cross product of the other two columns over the
    determinant.  Batched numpy, no LAPACK."""
    c0, c1, c2 = m[..., :, 0], m[..., :, 1], m[..., :, 2]
    rows = np.stack([np.cross(c1, c2), np.cross(c2, c0), np.cross(c0, c1)], axis=-2)
    det = (c0 * rows[..., 0, :]).sum(-1)
    return rows / det[..., None, None]


def _inverse4(m: np.ndarray) -> np.ndarray:
    """(..., 4, 4) float64 -> inverse, directly: the adjugate from the 2 x 2 minors of the upper (s) and the lower (c) row pair over the
    determinant (Laplace expansion by complementary minors).  Batched numpy, no LAPACK; valid for any invertible matrix, not only poses."""
    a = lambda i, j: m[..., i, j]
    s0, s1, s2 = a(0, 0) * a(1, 1) - a(1, 0) * a(0, 1), a(0, 0) * a(1, 2) - a(1, 0) * a(0, 2), a(0, 0) * a(1, 3) - a(1, 0) * a(0, 3)
    s3, s4, s5 = a(0, 1) * a(1, 2) - a(1, 1) * a(0, 2), a(0, 1) * a(1, 3) - a(1, 1) * a(0, 3), a(0, 2) * a(1, 3) - a(1, 2) * a(0, 3)
    c5, c4, c3 = a(2, 2) * a(3, 3) - a(3, 2) * a(2, 3), a(2, 1) * a(3, 3) - a(3, 1) * a(2, 3), a(2, 1) * a(3, 2) - a(3, 1) * a(2, 2)
    c2, c1, c0 = a(2, 0) * a(3, 3) - a(3, 0) * a(2, 3), a(2, 0) * a(3, 2) - a(3, 0) * a(2, 2), a(2, 0) * a(3, 1) - a(3, 0) * a(2, 1)
    det = s0 * c5 - s1 * c4 + s2 * c3 + s3 * c2 - s4 * c1 + s5 * c0
    adj = [[a(1, 1) * c5 - a(1, 2) * c4 + a(1, 3) * c3, -a(0, 1) * c5 + a(0, 2) * c4 - a(0, 3) * c3,
            a(3, 1) * s5 - a(3, 2) * s4 + a(3, 3) * s3, -a(2, 1) * s5 + a(2, 2) * s4 - a(2, 3) * s3],
           [-a(1, 0) * c5 + a(1, 2) * c2 - a(1, 3) * c1, a(0, 0) * c5 - a(0, 2) * c2 + a(0, 3) * c1,
            -a(3, 0) * s5 + a(3, 2) * s2 - a(3, 3) * s1, a(2, 0) * s5 - a(2, 2) * s2 + a(2, 3) * s1],
           [a(1, 0) * c4 - a(1, 1) * c2 + a(1, 3) * c0, -a(0, 0) * c4 + a(0, 1) * c2 - a(0, 3) * c0,
            a(3, 0) * s4 - a(3, 1) * s2 + a(3, 3) * s0, -a(2, 0) * s4 + a(2, 1) * s2 - a(2, 3) * s0],
           [-a(1, 0) * c3 + a(1, 1) * c1 - a(1, 2) * c0, a(0, 0) * c3 - a(0, 1) * c1 + a(0, 2) * c0,
            -a(3, 0) * s3 + a(3, 1) * s1 - a(3, 2) * s0, a(2, 0) * s3 - a(2, 1) * s1 + a(2, 2) * s0]]
    return np.stack([np.stack(row, axis=-1) for row in adj], axis=-2) / det[..., None, None]


def convert_poses(poses: Tensor):
    """RE10K's 18-float camera rows (fx, fy, cx, cy, 2 unused, 3x4 w2c row-major) -> (c2w (b,4,4), normalised K (b,3,3)), fp32.
    All b inverses in one batched float64 evaluation, rounded once (the reference inverts in fp32)."""
    p = poses.detach().cpu().double().numpy()
    b = p.shape[0]
    K = np.tile(np.eye(3), (b, 1, 1))
    K[:, 0, 0], K[:, 1, 1], K[:, 0, 2], K[:, 1, 2] = p[:, 0], p[:, 1], p[:, 2], p[:, 3]
    w2c = np.tile(np.eye(4), (b, 1, 1))
    w2c[:, :3] = p[:, 6:].reshape(b, 3, 4)
    return torch.from_numpy(_inverse4(w2c).astype(np.float32)), torch.from_numpy(K.astype(np.float32))


def get_fov_deg(K: np.ndarray) -> np.ndarray:
    """projection.get_fov in float64, degrees: (n,2) = (fov_x, fov_y) of normalised intrinsics (n,3,3) -- the angle between the rays
    through the mid points of the left / right and of the top / bottom image edge.  One batched evaluation for all n cameras."""
    edges = np.array([[0, 0.5, 1], [1, 0.5, 1], [0.5, 0, 1], [0.5, 1, 1]], np.float64)          # left, right, top, bottom
    rays = np.einsum("nij,ej->nei", _inverse3(K), edges)
    rays = rays / np.linalg.norm(rays, axis=-1, keepdims=True)
    cos = np.stack([(rays[:, 0] * rays[:, 1]).sum(-1), (rays[:, 2] * rays[:, 3]).sum(-1)], axis=-1)
    return np.degrees(np.arccos(np.clip(cos, -1.0, 1.0)))


def prepare_cameras_f64(intrinsics: Tensor, extrinsics: Tensor, context_indices, target_indices, cfg: InputCfg, image_hw: tuple,
                        pixel_intrinsics: bool = False, flip: bool = False):
    """Steps 1 - 7 of `prepare_example` on the cameras alone, float64 throughout:
    -> dict(context = (extrinsics, intrinsics, near, far), target = (...), scale) of numpy float64 arrays.  Raises SkipExample."""
    K = intrinsics.detach().cpu().double().numpy().copy()
    E = extrinsics.detach().cpu().double().numpy().copy()
    ci = [int(i) for i in context_indices]
    ti = [int(i) for i in target_indices]
    h, w = image_hw
    if pixel_intrinsics:
        K[:, 0, 0] /= w
        K[:, 1, 1] /= h
        K[:, 0, 2] /= w
        K[:, 1, 2] /= h
    fov = get_fov_deg(K)
    if (fov > cfg.max_fov).any():
        raise SkipExample(f"field of view too wide: {fov.max():.3f} > {cfg.max_fov} degrees")
    scale = 1.0
    if cfg.make_baseline_1:
        scale = float(np.linalg.norm(E[ci[0], :3, 3] - E[ci[-1], :3, 3]))
        if scale < cfg.baseline_min or scale > cfg.baseline_max or scale != scale:
            raise SkipExample(f"baseline out of range: {scale:.6f}")
        E[:, :3, 3] /= scale
    if cfg.relative_pose:
        E = _inverse4(E[ci[0]])[None] @ E
    h_out, w_out = cfg.input_image_shape
    h_scaled, w_scaled = scaled_size(h, w, (h_out, w_out))
    K[:, 0, 0] *= w_scaled / w_out
    K[:, 1, 1] *= h_scaled / h_out
    if flip:
        sign = np.ones((4, 4))
        sign[0, 1:] = -1
        sign[1:, 0] = -1
        E = E * sign + 0.0
    near, far = float(np.float32(cfg.near)) / scale, float(np.float32(cfg.far)) / scale
    views = lambda idx: (E[idx], K[idx], np.full(len(idx), near), np.full(len(idx), far))
    return {"context": views(ci), "target": views(ti), "scale": scale}


def _to_device(frames: Tensor, device) -> Tensor:
    return frames if device is None else frames.to(device)


def prepare_example(frames: Tensor, intrinsics: Tensor, extrinsics: Tensor, context_indices, target_indices, style, cfg: InputCfg, *,
                    stage: str, pixel_intrinsics: bool = False, flip: Optional[bool] = None, scene: str = "", device=None,
                    generator: Optional[torch.Generator] = None, preselected: bool = False) -> dict:
    """Decoded frames + raw cameras of one scene -> the example dict of the reference's dataset/types.py:
    context / target (extrinsics, intrinsics, image, near, far, index), scene, style {"image"}.
      frames       uint8 (n,H,W,3) or float (n,3,H,W), all frames of the scene the indices point into.  CPU bytes are uploaded as bytes
                   (a quarter of the fp32 planes) when `device` is a GPU.
      intrinsics   (n,3,3), normalised, or in pixels with pixel_intrinsics=True; extrinsics (n,4,4) c2w
      style        one image, uint8 (Hs,Ws,3) or float (3,Hs,Ws); None: no "style" entry
      flip         None: the augmentation draw (one torch.rand(()) from `generator`) when stage == "train" and cfg.augment; else as given
      preselected  `frames` holds exactly the context frames followed by the target frames (styl3r_amd.dataset decodes no others); the
                   indices still name the scene's frames and cameras, and the "index" entries carry them
    In the order of the reference's loader: (1) pixel K / (w, h); (2) the FOV gate over all n cameras; (3) baseline-1 scaling of all
    translations with the range gate; (4) camera_normalization against the first context view; (5) near / far over the scale; (6) the
    reflection; (7) the crop shim.  The gates raise SkipExample.  Cameras are computed on the host in float64 (`prepare_cameras_f64`, the
    pivot inverted directly) and rounded once to fp32.  Context and target frames share ONE gsr_resample_crop call, the style image
    gets its own."""
    ci = torch.as_tensor(context_indices, dtype=torch.int64).reshape(-1).cpu()
    ti = torch.as_tensor(target_indices, dtype=torch.int64).reshape(-1).cpu()
    h, w = _image_hw(frames)
    if flip is None:
        flip = bool(stage == "train" and cfg.augment and not (torch.rand(tuple(), generator=generator) < 0.5))
    cams = prepare_cameras_f64(intrinsics, extrinsics, ci.tolist(), ti.tolist(), cfg, (h, w), pixel_intrinsics, bool(flip))
    if preselected:
        if frames.shape[0] != len(ci) + len(ti):
            raise ValueError(f"prepare_example: {frames.shape[0]} preselected frames for {len(ci)} context and {len(ti)} target views")
        picked = _to_device(frames, device)
    else:
        sel = torch.cat([ci, ti]).to(frames.device)
        picked = _to_device(frames.index_select(0, sel), device)
    dev = picked.device
    images, _ = rescale_and_crop(picked, torch.zeros(3, 3), tuple(cfg.input_image_shape), flip=bool(flip))
    # the eight camera arrays travel in ONE upload and are handed out as views of it; the indices in a second one
    parts = [np.asarray(a, dtype=np.float64) for name in ("context", "target") for a in cams[name]]
    packed = torch.from_numpy(np.concatenate([a.reshape(-1) for a in parts]).astype(np.float32)).to(dev)
    arrays = iter(t.reshape(a.shape) for t, a in zip(packed.split([a.size for a in parts]), parts))
    index = torch.cat([ci, ti]).to(dev)
    example = {"scene": scene}
    for name, idx, imgs in (("context", index[:len(ci)], images[:len(ci)]), ("target", index[len(ci):], images[len(ci):])):
        E, K, near, far = (next(arrays) for _ in range(4))
        example[name] = {"extrinsics": E, "intrinsics": K, "image": imgs, "near": near, "far": far, "index": idx}
    if style is not None:
        example["style"] = {"image": apply_style_image_augmentation(_to_device(style, device), stage, cfg.style_size)}
    return example


def example_from_scene(frames: Tensor, intrinsics: Tensor, extrinsics: Tensor, sampler, scene: str, style, cfg: InputCfg, *, stage: str,
                       **kwargs) -> dict:
    """`prepare_example` with the views chosen by a view sampler (styl3r_amd.views): sampler.sample(scene, extrinsics, intrinsics) gives
    the context and target indices.  A scene the sampler refuses (ValueError: "Example does not have enough frames!", no entry in the
    evaluation index) raises SkipExample, where the reference's loader `continue`s (dataset_re10k_style.py:125-133).  kwargs go to
    prepare_example."""
    try:
        picked = sampler.sample(scene, extrinsics, intrinsics)
    except ValueError as err:
        raise SkipExample(str(err)) from err
    return prepare_example(frames, intrinsics, extrinsics, picked[0], picked[1], style, cfg, stage=stage, scene=scene, **kwargs)


def collate(examples: Sequence[dict]) -> dict:
    """examples of one shape -> the batch with its leading b (torch's default collate on this dict: tensors stacked, scenes listed)"""
    def stack(items):
        first = items[0]
        if isinstance(first, dict):
            return {k: stack([it[k] for it in items]) for k in first}
        if isinstance(first, Tensor):
            return torch.stack(list(items))
        return list(items)
    return stack(list(examples))
