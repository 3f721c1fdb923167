"""Validation visuals: the three pictures `ModelWrapperStyle.validation_step` (src/model/model_wrapper_style.py:472-630) logs --
`comparison` (src/visualization/layout.py), `projection` (validation_in_3d.py::render_projections) and `cameras` (render_cameras ->
drawing/cameras.py::draw_cameras -> drawing/lines.py::draw_lines; drawing/points.py::draw_points).

Drawing.  The reference evaluates every pixel against every primitive in about forty tensor ops per draw call, reads the edge mask back,
re-samples the edge pixels 8 x 8 and scatters them; a `draw_cameras` picture is twelve such calls.  Here a draw call is a LAYER (a table of
float64 records in pixel space) and `draw_layers` draws every layer of every image of a batch:
  * fp32 images on the GPU with 0 or 1 MSAA passes: ONE launch of `gsr_draw_layers` (csrc/gsr_draw.hip);
  * anything else (CPU tensors, `num_msaa_passes >= 2`): `draw_layers_reference`, a float64 restatement of the reference in its operation
    order, written in torch so that it runs on the images' device.  On the CPU it is the yardstick of the GPU tests.
Both evaluate the inside tests, the sums and the composite in float64 and round the picture to fp32 once, after the last layer.

Deviations from the reference:
  * float64 drawing: the reference runs in fp32, where a sub-sample on a primitive's edge can fall on either side (measured: up to 8 pixels
    of a 5-camera 256^2 picture off by 0.25 / 64); `sanitize_*` widen to float64 instead of rounding to fp32;
  * labels come from an injected `labeler(text) -> (3,h,w)` (`pil_labeler` restates annotation.draw_label); `labeler=None` draws none;
  * the 2D-AdaIN baseline column is drawn when a `baseline.AdaIN2D` is passed (`baseline=`); its style is one row shared by the views;
  * depth panels are coloured through the byte table of `export.pack_frames` (bytes / 255) instead of the fp32 colour map;
  * colours must be finite (a NaN colour never equals itself in the reference's edge rule; it is an argument error here).
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Callable, Optional, Sequence

import numpy as np
import torch
from torch import Tensor

from . import _lib

CAPS = {"butt": _lib.GSR_DRAW_BUTT, "round": _lib.GSR_DRAW_ROUND, "square": _lib.GSR_DRAW_SQUARE}
REC = _lib.GSR_DRAW_RECORD_DOUBLES
# record fields (include/gsr.h gsr_draw_layers)
_KIND, _CLASS, _SX, _SY, _EX, _EY, _UX, _UY, _HI, _LO, _HW, _R = range(12)
SUBDIVISION = 8
_SAMPLE_BATCH = 1 << 16                          # rendering.py: run_msaa_pass evaluates its samples in batches of 2^16

Labeler = Callable[[str], Tensor]


# ---- drawing/types.py, widened -------------------------------------------------------------------------------------------------------
def _f64(value) -> Tensor:
    if isinstance(value, Tensor):
        return value.detach().to(device="cpu", dtype=torch.float64)
    return torch.tensor(value, dtype=torch.float64)


def sanitize_vector(vector, dim: int) -> Tensor:
    """scalar, list, (dim,), (n, dim) or (n, 1) -> float64 (n | 1, dim) on the host"""
    vector = _f64(vector)
    while vector.ndim < 2:
        vector = vector[None]
    if vector.shape[-1] == 1:
        vector = vector.expand(*vector.shape[:-1], dim)
    if vector.ndim != 2 or vector.shape[-1] != dim:
        raise ValueError(f"expected a scalar, ({dim},) or (n, {dim}); got shape {tuple(vector.shape)}")
    return vector


def sanitize_scalar(scalar) -> Tensor:
    scalar = _f64(scalar)
    while scalar.ndim < 1:
        scalar = scalar[None]
    if scalar.ndim != 1:
        raise ValueError(f"expected a scalar or (n,); got shape {tuple(scalar.shape)}")
    return scalar


def sanitize_pair(pair) -> Tensor:
    pair = _f64(pair)
    if pair.shape != (2,):
        raise ValueError(f"expected a pair; got shape {tuple(pair.shape)}")
    return pair


def generate_conversions(shape, x_range=None, y_range=None):
    """coordinate_conversion.py in float64: (world -> pixel, pixel -> world)"""
    h, w = shape
    x_range = sanitize_pair((0, w) if x_range is None else x_range)
    y_range = sanitize_pair((0, h) if y_range is None else y_range)
    minima, maxima = torch.stack((x_range, y_range), dim=-1)
    wh = torch.tensor((w, h), dtype=torch.float64)
    return (lambda xy: (xy - minima) / (maxima - minima) * wh), (lambda xy: xy / wh * (maxima - minima) + minima)


# ---- layers ----------------------------------------------------------------------------------------------------------------------------
@dataclass
class Layer:
    """one draw call of the reference: float64 records (n, 16) in pixel space (include/gsr.h) and its MSAA passes"""
    records: np.ndarray
    num_msaa_passes: int = 1


def _broadcast(n: int, *tensors):
    try:
        return [t.expand(n, *t.shape[1:]) for t in tensors]
    except RuntimeError as e:
        raise ValueError(f"primitive arguments do not broadcast to {n} primitives") from e


def _finish(rec: Tensor, color: Tensor, passes) -> Layer:
    if not isinstance(passes, int) or isinstance(passes, bool) or passes < 0:
        raise ValueError("num_msaa_passes is an integer >= 0")
    if not torch.isfinite(color).all():
        raise ValueError("colours must be finite")
    color = color + 0.0                                                    # -0.0 -> 0.0: one bit pattern per value
    rec[:, _R:_R + 3] = color
    out = np.ascontiguousarray(rec.numpy())
    if len(out):
        _, first, inverse = np.unique(out[:, _R:_R + 3], axis=0, return_index=True, return_inverse=True)
        out[:, _CLASS] = first[inverse.reshape(-1)]                        # lowest index of an equal colour
    return Layer(out, passes)


def line_layer(shape, start, end, color, width, cap: str = "round", num_msaa_passes: int = 1, x_range=None, y_range=None) -> Layer:
    """the records of one `draw_lines` call on an image of `shape` = (h, w); lines.py:24-47 in float64"""
    if cap not in CAPS:
        raise ValueError(f"cap is one of {sorted(CAPS)}, not {cap!r}")
    start, end, color, width = sanitize_vector(start, 2), sanitize_vector(end, 2), sanitize_vector(color, 3), sanitize_scalar(width)
    try:
        (n,) = torch.broadcast_shapes((start.shape[0],), (end.shape[0],), (color.shape[0],), tuple(width.shape))
    except RuntimeError as e:
        raise ValueError("draw_lines: start, end, color and width do not broadcast") from e
    to_pixel, _ = generate_conversions(shape, x_range, y_range)
    start, end = to_pixel(start), to_pixel(end)
    delta = end - start
    delta_norm = delta.norm(dim=-1, keepdim=True)
    u_delta = delta / delta_norm                                           # NaN for start == end: the body test is then false
    half = 0.5 * width
    extra = half if cap == "square" else torch.zeros_like(half)
    start, end, u_delta, delta_norm, color = _broadcast(n, start, end, u_delta, delta_norm, color)
    half, extra = _broadcast(n, half, extra)
    rec = torch.zeros((n, REC), dtype=torch.float64)
    rec[:, _KIND] = CAPS[cap]
    rec[:, _SX:_SY + 1], rec[:, _EX:_EY + 1], rec[:, _UX:_UY + 1] = start, end, u_delta
    rec[:, _HI], rec[:, _LO], rec[:, _HW] = delta_norm[:, 0] + extra, -extra, half
    return _finish(rec, color, num_msaa_passes)


def point_layer(shape, points, color=(1, 1, 1), radius=1, inner_radius=0, num_msaa_passes: int = 1, x_range=None, y_range=None) -> Layer:
    """the records of one `draw_points` call; points.py:23-38 in float64"""
    points, color = sanitize_vector(points, 2), sanitize_vector(color, 3)
    radius, inner_radius = sanitize_scalar(radius), sanitize_scalar(inner_radius)
    try:
        (n,) = torch.broadcast_shapes((points.shape[0],), (color.shape[0],), tuple(radius.shape), tuple(inner_radius.shape))
    except RuntimeError as e:
        raise ValueError("draw_points: points, color, radius and inner_radius do not broadcast") from e
    to_pixel, _ = generate_conversions(shape, x_range, y_range)
    points = to_pixel(points)
    points, color, radius, inner_radius = _broadcast(n, points, color, radius, inner_radius)
    rec = torch.zeros((n, REC), dtype=torch.float64)
    rec[:, _KIND] = _lib.GSR_DRAW_POINT
    rec[:, _SX:_SY + 1] = points
    rec[:, _HI], rec[:, _HW] = inner_radius, radius
    return _finish(rec, color, num_msaa_passes)


# ---- the float64 restatement (drawing/rendering.py, lines.py:42-81, points.py:40-57) ------------------------------------------------------
def _color_function(rec: Tensor):
    n = rec.shape[0]
    kind = rec[:, _KIND, None]
    order = torch.arange(1, n + 1, device=rec.device)[:, None]

    def fn(xy: Tensor) -> Tensor:                                          # (s, 2) -> (s, 4) RGBA
        x, y = xy[None, :, 0], xy[None, :, 1]
        ix, iy = x - rec[:, _SX, None], y - rec[:, _SY, None]
        ux, uy, hw = rec[:, _UX, None], rec[:, _UY, None], rec[:, _HW, None]
        parallel = ux * ix + uy * iy
        qx, qy = ix - parallel * ux, iy - parallel * uy
        inside = (parallel <= rec[:, _HI, None]) & (parallel > rec[:, _LO, None]) & ((qx * qx + qy * qy).sqrt() < hw)
        from_start = (ix * ix + iy * iy).sqrt()
        jx, jy = x - rec[:, _EX, None], y - rec[:, _EY, None]
        caps = (from_start < hw) | ((jx * jx + jy * jy).sqrt() < hw)
        inside = inside | (caps & (kind == _lib.GSR_DRAW_ROUND))
        annulus = (from_start >= rec[:, _HI, None]) & (from_start <= hw)
        inside = torch.where(kind == _lib.GSR_DRAW_POINT, annulus, inside)
        top = ((inside * order).max(dim=0).values - 1).clamp(min=0)        # highest covering index; 0 where nothing covers
        return torch.cat((rec[top, _R:_R + 3], inside.any(dim=0).to(rec.dtype)[:, None]), dim=-1)
    return fn


def _sample_grid(shape, device) -> Tensor:
    h, w = shape
    x = torch.arange(w, device=device, dtype=torch.float64) + 0.5
    y = torch.arange(h, device=device, dtype=torch.float64) + 0.5
    x, y = torch.meshgrid(x, y, indexing="xy")
    return torch.stack([x, y], dim=-1)


def detect_msaa_pixels(rgba: Tensor) -> Tensor:
    """(b,4,h,w) -> bool (b,h,w): the pixels whose RGBA differs, in any channel, from any of their 8 neighbours inside the image"""
    _, _, h, w = rgba.shape
    edge = torch.zeros(rgba.shape[:1] + rgba.shape[2:], dtype=torch.bool, device=rgba.device)
    for dy, dx in ((-1, -1), (-1, 0), (-1, 1), (0, -1), (0, 1), (1, -1), (1, 0), (1, 1)):
        rows, cols = slice(max(0, -dy), h - max(0, dy)), slice(max(0, -dx), w - max(0, dx))              # pixels that have this neighbour
        beside = rgba[:, :, rows.start + dy:rows.stop + dy, cols.start + dx:cols.stop + dx]
        edge[:, rows, cols] |= (rgba[:, :, rows, cols] != beside).any(dim=1)
    return edge


def _average_samples(rgba: Tensor) -> Tensor:
    """(n,4,s,s) sub-samples with straight alpha -> (n,4): colour weighted by alpha, over the alpha sum + 1e-10; alpha averaged"""
    alpha = rgba[:, 3:]
    covered = alpha.sum(dim=(2, 3))
    weighted = (rgba[:, :3] * alpha).sum(dim=(2, 3))
    return torch.cat((weighted / (covered + 1e-10), covered / (rgba.shape[2] * rgba.shape[3])), dim=-1)


def _msaa_pass(xy: Tensor, fn, scale: float, remaining: int) -> Tensor:
    b, h, w, _ = xy.shape
    color = torch.cat([fn(batch) for batch in xy.reshape(-1, 2).split(_SAMPLE_BATCH)], dim=0)
    color = color.reshape(b, h, w, 4).permute(0, 3, 1, 2)                   # (a view, as the reference's rearrange: its sums follow this layout)
    if remaining > 0:
        bi, ri, ci = torch.where(detect_msaa_pixels(color))
        if bi.numel():
            offsets = (_sample_grid((SUBDIVISION, SUBDIVISION), xy.device) / SUBDIVISION - 0.5) * scale
            fine = _msaa_pass(xy[bi, ri, ci][:, None, None] + offsets, fn, scale / SUBDIVISION, remaining - 1)
            color[bi, :, ri, ci] = _average_samples(fine)
    return color


def render_overlay(shape, layer: Layer, device) -> Tensor:
    """`rendering.render` for one layer: float64 RGBA (4,h,w) with straight alpha"""
    rec = torch.from_numpy(layer.records).to(device)
    return _msaa_pass(_sample_grid(shape, device)[None], _color_function(rec), 1.0, layer.num_msaa_passes)[0]


def _check(images: Tensor, layers) -> None:
    if not isinstance(images, Tensor) or images.ndim != 4 or images.shape[1] != 3 or not images.is_floating_point():
        raise ValueError("draw_layers: images is a floating-point (B,3,H,W) tensor")
    if min(images.shape) < 1:
        raise ValueError("draw_layers: empty images")
    if len(layers) != images.shape[0]:
        raise ValueError(f"draw_layers: {len(layers)} layer stacks for {images.shape[0]} images")
    for stack in layers:
        for layer in stack:
            if not isinstance(layer, Layer) or layer.records.ndim != 2 or layer.records.shape[1] != REC or layer.records.dtype != np.float64:
                raise ValueError("draw_layers: a layer is a Layer of float64 (n, 16) records (line_layer / point_layer make them)")


def draw_layers_reference(images: Tensor, layers: Sequence[Sequence[Layer]], dtype=torch.float32) -> Tensor:
    """The float64 restatement on the images' device: per layer `render_over_image`, composited in float64, rounded to fp32 once
    (`dtype=torch.float64`: not at all)."""
    _check(images, layers)
    out = []
    for image, stack in zip(images, layers):
        image = image.to(torch.float64)
        for layer in stack:
            if len(layer.records) == 0:
                continue
            color, alpha = render_overlay(image.shape[1:], layer, image.device).split((3, 1), dim=0)
            image = image * (1 - alpha) + color * alpha
        out.append(image.to(dtype))
    return torch.stack(out)


def draw_layers(images: Tensor, layers: Sequence[Sequence[Layer]]) -> Tensor:
    """images (B,3,H,W); layers[b] = the ordered `Layer`s of image b.  Returns the drawn images, fp32 (B,3,H,W); the input is left alone."""
    _check(images, layers)
    flat = [layer for stack in layers for layer in stack]
    if not (images.is_cuda and images.dtype == torch.float32) or any(layer.num_msaa_passes > 1 for layer in flat):
        return draw_layers_reference(images, layers)
    dev = images.device
    image_layers = np.cumsum([0] + [len(stack) for stack in layers])
    layer_prims = np.cumsum([0] + [len(layer.records) for layer in flat])
    table = np.concatenate([image_layers, layer_prims, [layer.num_msaa_passes for layer in flat], [0]]).astype(np.int32)   # (+ 1: no empty slice below)
    n_prims = int(layer_prims[-1])
    records = np.concatenate([layer.records for layer in flat] + [np.zeros((1, REC))])        # (never empty: a valid pointer)
    table = torch.from_numpy(table).to(dev)
    records = torch.from_numpy(records).to(dev)
    src = images.detach().contiguous()
    out = torch.empty_like(src)
    B, _, H, W = src.shape
    n_layers = len(flat)
    _lib.check(_lib.load().gsr_draw_layers(src.data_ptr(), out.data_ptr(), B, H, W, table.data_ptr(), table[B + 1:].data_ptr(),
                                           table[B + n_layers + 2:].data_ptr(), n_layers, records.data_ptr(), n_prims,
                                           C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)), "gsr_draw_layers")
    return out


def draw_lines(image: Tensor, start, end, color, width, cap: str = "round", num_msaa_passes: int = 1, x_range=None, y_range=None) -> Tensor:
    """drawing/lines.py::draw_lines: (3,h,w) -> (3,h,w) fp32"""
    if not isinstance(image, Tensor) or image.ndim != 3:
        raise ValueError("draw_lines: image is (3,h,w)")
    return draw_layers(image[None], [[line_layer(image.shape[1:], start, end, color, width, cap, num_msaa_passes, x_range, y_range)]])[0]


def draw_points(image: Tensor, points, color=(1, 1, 1), radius=1, inner_radius=0, num_msaa_passes: int = 1, x_range=None,
                y_range=None) -> Tensor:
    """drawing/points.py::draw_points: (3,h,w) -> (3,h,w) fp32"""
    if not isinstance(image, Tensor) or image.ndim != 3:
        raise ValueError("draw_points: image is (3,h,w)")
    return draw_layers(image[None], [[point_layer(image.shape[1:], points, color, radius, inner_radius, num_msaa_passes, x_range, y_range)]])[0]


# ---- drawing/cameras.py ------------------------------------------------------------------------------------------------------------------
def unproject_frustum_corners(extrinsics: Tensor, intrinsics: Tensor, depth: Tensor) -> Tensor:
    """(b,4,4) c2w, (b,3,3) normalised, (b | 1,) z-depth -> the four image corners at that depth, (b,4,3), in float64 on the host"""
    extrinsics, intrinsics, depth = _f64(extrinsics), _f64(intrinsics), sanitize_scalar(depth)
    xy = torch.tensor([[0.0, 0.0, 1.0], [1.0, 0.0, 1.0], [1.0, 1.0, 1.0], [0.0, 1.0, 1.0]], dtype=torch.float64)     # following them makes a rectangle
    directions = torch.einsum("...ij,...j->...i", intrinsics.inverse()[:, None], xy)
    directions = directions / directions[..., -1:]
    directions = torch.einsum("bij,brj->bri", extrinsics[..., :3, :3], directions)
    return extrinsics[:, None, :3, 3] + depth[:, None, None] * directions


def compute_aabb(extrinsics: Tensor, intrinsics: Tensor, near=None, far=None):
    """the axis-aligned box of the camera origins and, where given, their near / far frustum corners"""
    points = [_f64(extrinsics)[:, :3, 3]]
    for depth in (near, far):
        if depth is not None:
            points.append(unproject_frustum_corners(extrinsics, intrinsics, depth).reshape(-1, 3))
    points = torch.cat(points, dim=0)
    return points.min(dim=0).values, points.max(dim=0).values


def compute_equal_aabb_with_margin(minima: Tensor, maxima: Tensor, margin: float = 0.1):
    midpoint = (maxima + minima) * 0.5
    span = (maxima - minima).max() * (1 + margin)
    return midpoint - 0.5 * span, midpoint + 0.5 * span


def camera_layers(resolution: int, extrinsics: Tensor, intrinsics: Tensor, color, near=None, far=None, margin: float = 0.1,
                  frustum_scale: float = 0.05):
    """the layer stacks of the three projections of `draw_cameras`, float64 from the fp32 cameras to pixel space"""
    if extrinsics.ndim != 3 or extrinsics.shape[1:] != (4, 4) or intrinsics.shape != (extrinsics.shape[0], 3, 3):
        raise ValueError("draw_cameras: extrinsics (n,4,4) and intrinsics (n,3,3)")
    if not isinstance(resolution, int) or resolution < 1:
        raise ValueError("draw_cameras: resolution is a positive integer")
    b = extrinsics.shape[0]
    E = _f64(extrinsics)
    color = sanitize_vector(color, 3).expand(b, 3)
    minima, maxima = compute_aabb(extrinsics, intrinsics, near, far)
    scene_minima, scene_maxima = compute_equal_aabb_with_margin(minima, maxima, margin=margin)
    span = (scene_maxima - scene_minima).max()
    frustum_corners = unproject_frustum_corners(extrinsics, intrinsics, (span * frustum_scale)[None])
    near_corners = None if near is None else unproject_frustum_corners(extrinsics, intrinsics, near)
    far_corners = None if far is None else unproject_frustum_corners(extrinsics, intrinsics, far)
    shape = (resolution, resolution)
    stacks = []
    for axis in range(3):
        ax, ay = (axis + 1) % 3, (axis + 2) % 3
        project = lambda p: torch.stack([p[..., ax], p[..., ay]], dim=-1)
        x_range, y_range = torch.stack((project(scene_minima), project(scene_maxima)), dim=-1)
        grey = dict(color=0.25, width=2, x_range=x_range, y_range=y_range)
        stack = []
        if near_corners is not None:
            ring = project(near_corners)
            stack.append(line_layer(shape, ring.reshape(-1, 2), ring.roll(1, 1).reshape(-1, 2), **grey))
        if far_corners is not None:
            ring = project(far_corners)
            stack.append(line_layer(shape, ring.reshape(-1, 2), ring.roll(1, 1).reshape(-1, 2), **grey))
        if near_corners is not None and far_corners is not None:
            stack.append(line_layer(shape, project(near_corners).reshape(-1, 2), project(far_corners).reshape(-1, 2), **grey))
        origins, corners = project(E[:, :3, 3]), project(frustum_corners)
        start = torch.stack([origins[:, None].expand(b, 4, 2), corners.roll(1, 1)], dim=1).reshape(-1, 2)          # (b r p)
        end = corners[:, None].expand(b, 2, 4, 2).reshape(-1, 2)
        stack.append(line_layer(shape, start, end, color[:, None, None].expand(b, 2, 4, 3).reshape(-1, 3), 2, x_range=x_range, y_range=y_range))
        stacks.append(stack)
    return stacks


def draw_cameras(resolution: int, extrinsics: Tensor, intrinsics: Tensor, color, near=None, far=None, margin: float = 0.1,
                 frustum_scale: float = 0.05, labeler: Optional[Labeler] = None) -> Tensor:
    """drawing/cameras.py::draw_cameras: the cameras projected onto the three axis-aligned planes, (3,3,res,res) fp32 on the cameras'
    device (taller by the label with a labeler).  The three projections and their up to four layers are one `draw_layers` call."""
    stacks = camera_layers(resolution, extrinsics, intrinsics, color, near, far, margin, frustum_scale)
    images = draw_layers(torch.zeros((3, 3, resolution, resolution), dtype=torch.float32, device=extrinsics.device), stacks)
    if labeler is None:
        return images
    return torch.stack([add_label(image, f"{'XYZ'[(axis + 1) % 3]}{'XYZ'[(axis + 2) % 3]} Projection", labeler) for axis, image in enumerate(images)])


def render_cameras(batch: dict, resolution: int, labeler: Optional[Labeler] = None) -> Tensor:
    """validation_in_3d.py:93-115: the first scene's context cameras in white and target cameras in red"""
    ctx, tgt = batch["context"], batch["target"]
    n_ctx, n_tgt = ctx["extrinsics"].shape[1], tgt["extrinsics"].shape[1]
    color = torch.ones((n_ctx + n_tgt, 3), dtype=torch.float32)
    color[n_ctx:, 1:] = 0
    both = lambda k: torch.cat((ctx[k][0], tgt[k][0]))
    return draw_cameras(resolution, both("extrinsics"), both("intrinsics"), color, both("near"), both("far"), labeler=labeler)


# ---- layout.py -----------------------------------------------------------------------------------------------------------------------------
_MAIN = {"horizontal": 2, "vertical": 1}
_CROSS = {"horizontal": 1, "vertical": 2}


def _color_tensor(color) -> Tensor:
    """a number, a sequence or a tensor -> fp32 (1,) or (c,) on the host"""
    return torch.as_tensor(color, dtype=torch.float32).detach().cpu().reshape(-1)


def _offset(base: int, over: int, align: str) -> slice:
    if base < over:
        raise ValueError("overlay: the overlay must fit the base")
    try:
        offset = {"start": 0, "center": (base - over) // 2, "end": base - over}[align]
    except KeyError:
        raise ValueError(f"alignment {align!r}: one of start, center, end") from None
    return slice(offset, offset + over)


def overlay(base: Tensor, overlay: Tensor, main_axis: str, main_axis_alignment: str, cross_axis_alignment: str) -> Tensor:
    """layout.py::overlay: paste `overlay` onto a copy of `base`"""
    if main_axis not in _MAIN:
        raise ValueError("main_axis is horizontal or vertical")
    selector = [slice(None), None, None]
    selector[_MAIN[main_axis]] = _offset(base.shape[_MAIN[main_axis]], overlay.shape[_MAIN[main_axis]], main_axis_alignment)
    selector[_CROSS[main_axis]] = _offset(base.shape[_CROSS[main_axis]], overlay.shape[_CROSS[main_axis]], cross_axis_alignment)
    result = base.clone()
    result[tuple(selector)] = overlay
    return result


def cat(main_axis: str, *images: Tensor, align: str = "center", gap: int = 8, gap_color=1) -> Tensor:
    """layout.py::cat: images in a line, padded on the cross axis to the longest, `gap` pixels of `gap_color` between them"""
    if not images:
        raise ValueError("cat: no images")
    if main_axis not in _MAIN:
        raise ValueError("main_axis is horizontal or vertical")
    device = images[0].device
    gap_color = _color_tensor(gap_color).to(device)
    cross = _CROSS[main_axis]
    length = max(image.shape[cross] for image in images)
    padded = []
    for image in images:
        shape = list(image.shape)
        shape[cross] = length
        base = torch.ones(shape, dtype=torch.float32, device=device) * gap_color[:, None, None]
        padded.append(overlay(base, image, main_axis, "start", align))
    if gap > 0:
        size = [gap, gap]
        size[cross - 1] = length
        separator = torch.ones((images[0].shape[0], *size), dtype=torch.float32, device=device) * gap_color[:, None, None]
        padded = [x for image in padded for x in (separator, image)][1:]
    return torch.cat(padded, dim=_MAIN[main_axis])


_ALIGNMENTS = ("start", "center", "end")


def _alignment(align: str, aliases: dict) -> str:
    align = aliases.get(align, align)
    if align not in _ALIGNMENTS:
        raise ValueError(f"alignment {align!r}: one of {sorted(_ALIGNMENTS + tuple(aliases))}")
    return align


def hcat(*images: Tensor, align: str = "start", gap: int = 8, gap_color=1) -> Tensor:
    """images side by side; `align` also takes top / bottom"""
    return cat("horizontal", *images, align=_alignment(align, {"top": "start", "bottom": "end"}), gap=gap, gap_color=gap_color)


def vcat(*images: Tensor, align: str = "start", gap: int = 8, gap_color=1) -> Tensor:
    """images below one another; `align` also takes left / right"""
    return cat("vertical", *images, align=_alignment(align, {"left": "start", "right": "end"}), gap=gap, gap_color=gap_color)


def add_border(image: Tensor, border: int = 8, color=1) -> Tensor:
    """(c,h,w) -> fp32 (c, h + 2 border, w + 2 border): the image inside a frame of `color`"""
    c, h, w = image.shape
    frame = _color_tensor(color).to(device=image.device).reshape(-1, 1, 1).expand(c, h + 2 * border, w + 2 * border).contiguous()
    frame.narrow(1, border, h).narrow(2, border, w).copy_(image)
    return frame


def pad(images: Sequence[Tensor]) -> list:
    """validation_in_3d.py::pad: every tensor padded with ones, at the end of each dimension, to the largest shape"""
    shape = [max(sizes) for sizes in zip(*(x.shape for x in images))]
    results = []
    for image in images:
        result = torch.ones(shape, dtype=image.dtype, device=image.device)
        result[tuple(slice(0, n) for n in image.shape)] = image
        results.append(result)
    return results


# ---- annotation.py ---------------------------------------------------------------------------------------------------------------------------
def pil_labeler(font=None, font_size: int = 24) -> Labeler:
    """What annotation.draw_label draws, as a labeler: black text on white with no border, as wide as the text and as tall as the font's
    digits, punctuation and letters together.  `font`: a TrueType / OpenType file; PIL's default font when it cannot be opened (the
    reference's own font file is not in its tree, so that is what it uses too).  PIL is imported here, not with the package."""
    import string

    from PIL import Image, ImageDraw, ImageFont
    try:
        face = ImageFont.truetype(str(font), font_size)
    except OSError:
        face = ImageFont.load_default()
    tallest = face.getbbox(string.digits + string.punctuation + string.ascii_letters)
    height = tallest[3] - tallest[1]

    def labeler(text: str) -> Tensor:
        box = face.getbbox(text)
        canvas = Image.new("L", (box[2] - box[0], height), 255)
        ImageDraw.Draw(canvas).text((0, 0), text, font=face, fill=0)
        grey = torch.from_numpy(np.asarray(canvas, dtype=np.float64) / 255).to(torch.float32)
        return grey[None].repeat(3, 1, 1)
    return labeler


def add_label(image: Tensor, label: str, labeler: Optional[Labeler]) -> Tensor:
    """annotation.py::add_label with the label drawn by `labeler`; None leaves the image as it is"""
    if labeler is None:
        return image
    return vcat(labeler(label).to(image.device), image, align="left", gap=4)


# ---- validation_in_3d.py::render_projections -----------------------------------------------------------------------------------------------
def projection_cameras(means: Tensor, margin: float = 0.1) -> list:
    """The three orthographic cameras of `render_projections` (:35-66) for means (b,G,3): per look axis a tuple
    (extrinsics (b,4,4), width (b,), height (b,), near (b,), far (b,)), fp32 on the means' device."""
    if means.ndim != 3 or means.shape[-1] != 3 or means.shape[1] < 1:
        raise ValueError("projection_cameras: means is (b,G,3)")
    b = means.shape[0]
    scene_minima, scene_maxima = compute_equal_aabb_with_margin(means.min(dim=1).values, means.max(dim=1).values, margin=margin)
    extents = scene_maxima - scene_minima
    cameras = []
    for look in range(3):
        right, down = (look + 1) % 3, (look + 2) % 3
        # camera-to-world: x, y, z of the camera are the world's right, down and look axes; it sits at the middle of the box's near face
        origin = 0.5 * (scene_minima + scene_maxima)
        origin[:, look] = scene_minima[:, look]
        axes = torch.eye(3, dtype=torch.float32, device=means.device)[[right, down, look]].T
        extrinsics = torch.eye(4, dtype=torch.float32, device=means.device).repeat(b, 1, 1)
        extrinsics[:, :3, :3] = axes
        extrinsics[:, :3, 3] = origin
        far = extents[:, look]
        cameras.append((extrinsics, extents[:, right], extents[:, down], torch.zeros_like(far), far))
    return cameras


def render_projections(gaussians, resolution: int, margin: float = 0.1, labeler: Optional[Labeler] = None, extra_label: str = "") -> Tensor:
    """validation_in_3d.py::render_projections: the Gaussians seen along the three axes by `render_hip_orthographic` (fov 10 degrees, black
    background), (b,3,3,h,w)."""
    from .decoder import render_hip_orthographic
    b = gaussians.means.shape[0]
    projections = []
    for look, (extrinsics, width, height, near, far) in enumerate(projection_cameras(gaussians.means, margin)):
        projection = render_hip_orthographic(extrinsics, width, height, near, far, (resolution, resolution),
                                             torch.zeros((b, 3), dtype=torch.float32, device=extrinsics.device), gaussians, 1, fov_degrees=10.0)
        if labeler is not None:
            label = f"{'XYZ'[(look + 1) % 3]}{'XYZ'[(look + 2) % 3]} Projection {extra_label}"
            projection = torch.stack([add_label(x, label, labeler) for x in projection])
        projections.append(projection)
    return torch.stack(pad(projections), dim=1)


# ---- the three pictures of validation_step (:528-617) ---------------------------------------------------------------------------------------
def depth_panels(depth: Tensor) -> Tensor:
    """(n,h,w) depths -> (n,3,h,w) fp32 turbo panels over the depths' own log range (utils.vis_depth_map), as bytes / 255"""
    from .export import pack_frames
    return pack_frames([depth], loop_reverse=False).permute(0, 3, 1, 2).to(torch.float32) / 255


def baseline_column(baseline, target_images: Tensor, style_image: Optional[Tensor]) -> tuple:
    """("2D Baseline", the target views stylised by `baseline`, a `baseline.AdaIN2D`) -- model_wrapper_style.py:536-548: the style image
    (3,h,w) in [0, 1] is shared by all views (one style row, `style_index` all zero, instead of the reference's row repeated per view)"""
    if style_image is None:
        raise ValueError("the 2D baseline stylises the targets with the style image: pass `style_image` (or `baseline_style`)")
    with torch.no_grad():
        return "2D Baseline", baseline.stylize(target_images, style_image.to(target_images.device))


def comparison_image(context_images: Tensor, context_depth: Tensor, target_images: Tensor, predicted_color: Tensor, predicted_depth: Tensor,
                     extra_columns: Sequence = (), style_image: Optional[Tensor] = None, labeler: Optional[Labeler] = None,
                     baseline=None, baseline_style: Optional[Tensor] = None) -> Tensor:
    """The `comparison` picture (:528-554) without its border: columns Context (image, depth per view) | Target (Ground Truth) |
    Target (Prediction) | Depth (Prediction), `extra_columns` = [(label, (n,3,h,w) images)] in front of them and the style image in front of
    everything.  `baseline` (a `baseline.AdaIN2D`): "2D Baseline" -- the targets stylised with `baseline_style` (default: `style_image`) --
    is the first column, as in the reference; None: no such column.  Images are in [0, 1]."""
    context = [panel for pair in zip(context_images, depth_panels(context_depth)) for panel in pair]
    columns = [] if baseline is None else [baseline_column(baseline, target_images, style_image if baseline_style is None else baseline_style)]
    columns = [(label, list(images)) for label, images in (*columns, *extra_columns)]
    columns += [("Context", context), ("Target (Ground Truth)", list(target_images)), ("Target (Prediction)", list(predicted_color)),
                ("Depth (Prediction)", list(depth_panels(predicted_depth)))]
    comparison = hcat(*[add_label(vcat(*images), label, labeler) for label, images in columns])
    if style_image is not None:
        comparison = hcat(add_label(style_image, "Style", labeler), comparison)
    return comparison


def validation_images(context_images: Tensor, context_depth: Tensor, target_images: Tensor, predicted_color: Tensor, predicted_depth: Tensor,
                      gaussians, batch: dict, extra_columns: Sequence = (), style_image: Optional[Tensor] = None,
                      labeler: Optional[Labeler] = None, resolution: int = 256, baseline=None, baseline_style: Optional[Tensor] = None) -> dict:
    """The three pictures validation_step logs for the first scene of `batch`, each fp32 (3,H,W) with `add_border` applied:
    `comparison` (see `comparison_image`; `baseline`, `baseline_style` go to it), `projection` = hcat of `render_projections(gaussians)[0]`,
    `cameras` = hcat of `render_cameras(batch)`.
    context_images (v,3,h,w) and target_images / predicted_color (t,3,h,w) in [0, 1]; context_depth (v,h,w); predicted_depth (t,h,w)."""
    comparison = comparison_image(context_images, context_depth, target_images, predicted_color, predicted_depth, extra_columns, style_image, labeler,
                                  baseline=baseline, baseline_style=baseline_style)
    cameras = hcat(*render_cameras(batch, resolution, labeler=labeler))
    images = {"comparison": add_border(comparison), "cameras": add_border(cameras)}
    if gaussians is not None:                                               # (None: no `projection`; it needs the rasterizer and so the GPU)
        images["projection"] = add_border(hcat(*render_projections(gaussians, resolution, labeler=labeler)[0]))
    return images


def train_comparison_image(context_images: Tensor, style_images: Tensor, target_images: Tensor, predicted_color: Tensor, predicted_depth: Tensor,
                           baseline=None, scenes: Optional[Sequence[str]] = None, style_names: Optional[Sequence[str]] = None,
                           labeler: Optional[Labeler] = None) -> tuple:
    """The `train/comparison` picture of training_step (:260-308) and its caption, for the FIRST and the LAST sample of the batch, side by
    side with `add_border` applied: per sample the columns 2D Baseline (the targets stylised by `baseline`, a `baseline.AdaIN2D`; None: no such
    column) | Context (every context view followed by the style image) | Target (Ground Truth) | Target (Prediction) | Depth (Prediction)
    under the label "Sample Index: 0" / "Sample Index: -1".  context_images (b,v,3,h,w), style_images (b,3,hs,ws), target_images and
    predicted_color (b,t,3,h,w) in [0, 1], predicted_depth (b,t,h,w).  Caption: "<scene> | <style name>" of the two samples joined by " | "
    (the samples' indices where no names are given)."""
    comparisons, captions = [], []
    b = target_images.shape[0]
    for index in (0, -1):
        style = style_images[index]
        context = [panel for view in context_images[index] for panel in (view, style)]
        columns = [] if baseline is None else [baseline_column(baseline, target_images[index], style)]
        columns = [(label, list(images)) for label, images in columns]
        columns += [("Context", context), ("Target (Ground Truth)", list(target_images[index])), ("Target (Prediction)", list(predicted_color[index])),
                    ("Depth (Prediction)", list(depth_panels(predicted_depth[index])))]
        comparison = hcat(*[add_label(vcat(*images), label, labeler) for label, images in columns])
        comparisons.append(add_label(comparison, f"Sample Index: {index}", labeler))
        scene = scenes[index] if scenes is not None else f"sample {index % b}"
        name = style_names[index] if style_names is not None else f"style {index % b}"
        captions.append(f"{scene} | {name}")
    return add_border(hcat(*comparisons)), " | ".join(captions)
