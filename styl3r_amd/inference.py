"""Serving one scene in many styles: the flow of the reference's inference drivers (infer_model_re10k.py:472-557,
infer_model_tnt_batch.py) on the scene cache of the encoder and the multi-style pass of the rasterizer.

The reference calls the encoder once with the first context image as "identity" style and once per real style, aligns the target
poses on the un-stylized Gaussians, then renders the plain and every stylized set through the same cameras, one rasterizer pass per
(set, camera list).  Here the style-independent part of the encoder runs once (`encode_scene`), all styles of one image size go
through ONE `restyle` batch, and the plain + S stylized sets -- which share means, covariances and opacities -- are rendered by ONE
`forward_styles` call.  `prepare_scene` is the other end: decoded frames and raw cameras in, the (context, styles, target) that
`stylize_scene` takes out, images rescaled and cropped on the device (inputs.py); `prepare_colmap_scene` is the same end for a COLMAP
capture loaded by `colmap.load_colmap_scene` (infer_model_colmap.py), its frames undistorted on the device first.  `render_flythrough` turns the result into the frames of the drivers' videos (render_video_generic and the
wrapper's three trajectories), `export_scene_ply` into their .ply files and `save_scene_images` into their tree of PNG files;
encoding a video container stays with the caller.

    context, styles, target = prepare_scene(frames_u8, K, c2w, [0, 40], range(0, 41, 5), [style_a, style_b], device="cuda")
    scene = stylize_scene(encoder, decoder, context, styles, target)
    video = render_flythrough(decoder, scene, context)                      # uint8 frames, on the device
    export_scene_ply(scene, "out/")
"""
from __future__ import annotations

from dataclasses import dataclass
from pathlib import Path
from typing import Optional, Sequence, Union

import torch
from torch import Tensor

from .decoder import DecoderOutput, Gaussians
from .evaluation import TestCfg, align_target_poses
from .export import depth_range, export_ply, pack_frames
from .inputs import InputCfg, apply_style_image_augmentation, prepare_example
from .trajectory import KINDS, trajectory_cameras
from . import colmap


@dataclass
class StylizedScene:
    gaussians: list            # [plain, style 0, style 1, ...]: `Gaussians` over the SAME means / covariances / opacities tensors
    extrinsics: Tensor         # (1,v,4,4) target c2w the colours were rendered from (aligned when `align` asked for it)
    color: Tensor              # (1 + S, 1, v, 3, h, w): color[0] the un-stylized render, color[1 + s] style s
    depth: Tensor              # (1,v,h,w), shared by every set
    visualization_dump: dict   # the un-stylized encoder pass's dump (scales / rotations for a PLY export)


def _style_images(styles) -> list:
    """a (S,3,hs,ws) tensor, a {"image": ...} dict, or a sequence of (3,hs,ws) / (1,3,hs,ws) images -> list of (3,hs,ws)"""
    if isinstance(styles, dict):
        styles = styles["image"]
    if isinstance(styles, Tensor):
        return list(styles.reshape(-1, *styles.shape[-3:]))
    return [im.reshape(*im.shape[-3:]) for im in styles]


def prepare_scene(frames: Tensor, intrinsics: Tensor, extrinsics: Tensor, context_indices, target_indices, styles, cfg: Optional[InputCfg] = None,
                  *, pixel_intrinsics: bool = False, scene: str = "", device=None):
    """Decoded frames + raw cameras of one scene -> (context, styles, target) as `stylize_scene` takes them (b == 1), following
    infer_model_colmap.py:513-589: `inputs.prepare_example` at stage "test" (no augmentation; the gates raise `inputs.SkipExample`).
      frames   uint8 (n,H,W,3) or float (n,3,H,W); intrinsics (n,3,3) normalised (or pixels with pixel_intrinsics), extrinsics (n,4,4) c2w
      styles   one style image or a sequence of them, uint8 (Hs,Ws,3) or float (3,Hs,Ws); their sizes may differ, each comes out
               cfg.style_size x cfg.style_size
    Everything is returned on `device` (default: where the frames are)."""
    cfg = cfg or InputCfg()
    style_list = [styles] if isinstance(styles, Tensor) else list(styles)
    ex = prepare_example(frames, intrinsics, extrinsics, context_indices, target_indices, None, cfg, stage="test",
                         pixel_intrinsics=pixel_intrinsics, flip=False, scene=scene, device=device)
    dev = ex["context"]["image"].device
    batch = lambda views: {k: v[None] for k, v in views.items()}
    return batch(ex["context"]), [apply_style_image_augmentation(s.to(dev), "test", cfg.style_size) for s in style_list], batch(ex["target"])


def prepare_colmap_scene(scene: "colmap.ColmapScene", ctx_indices, num_ctx_views: int, styles, cfg: Optional[InputCfg] = None, *,
                         frames: Optional[Tensor] = None, device=None):
    """A loaded COLMAP scene -> (context, styles, target) as `stylize_scene` takes them, following infer_model_colmap.py:480-589:
    `colmap.select_colmap_views`, the selected frames read from `scene.image_paths` (or taken from `frames`, uint8 (n,H,W,3) over ALL
    images of the scene in its order), uploaded as bytes, undistorted in one `colmap.undistort_frames` call, pixel intrinsics per image
    from `scene.Ks`, then `prepare_scene(..., pixel_intrinsics=True)`: baseline-1 rescale, relative poses, near / far, rescale and crop.
    The ROI origin of each camera is subtracted from cx, cy (the reference crops to the ROI without moving the principal point, which
    is harmless only for an origin of (0, 0)).  "index" holds the scene's image indices."""
    import numpy as np
    context_idx, target_idx = colmap.select_colmap_views(ctx_indices, num_ctx_views)
    sel = torch.cat([context_idx, target_idx])
    picked = colmap.read_frames([scene.image_paths[i] for i in sel.tolist()]) if frames is None else frames.index_select(0, sel.to(frames.device))
    if device is not None:
        picked = picked.to(device)
    cam_ids = [scene.camera_ids[i] for i in sel.tolist()]
    undistorted = colmap.undistort_frames(picked, scene, cam_ids)
    K = np.stack([scene.Ks[c] for c in cam_ids]).astype(np.float64)
    K[:, 0, 2] -= np.array([scene.rois[c][0] for c in cam_ids], dtype=np.float64)
    K[:, 1, 2] -= np.array([scene.rois[c][1] for c in cam_ids], dtype=np.float64)
    E = np.asarray(scene.camtoworlds, dtype=np.float64)[sel.numpy()]
    n_ctx = context_idx.shape[0]
    context, style_list, target = prepare_scene(undistorted, torch.from_numpy(K), torch.from_numpy(E), range(n_ctx), range(n_ctx, sel.shape[0]),
                                                styles, cfg, pixel_intrinsics=True, scene=scene.name, device=device)
    dev = context["image"].device
    context["index"], target["index"] = context_idx.to(dev)[None], target_idx.to(dev)[None]
    return context, style_list, target


def stylize_scene(encoder, decoder, context: dict, styles, target: dict, *, align: Optional[TestCfg] = None,
                  losses: Sequence = ()) -> StylizedScene:
    """One scene (b == 1) in S styles, in the order of infer_model_re10k.py:478-502.
      context  the encoder's context dict (image (1,v,3,h,w), intrinsics, ...), already normalised by the encoder's data shim
      styles   S style images (see `_style_images`); sizes may differ between styles
      target   cameras to render: extrinsics (1,n,4,4), intrinsics (1,n,3,3), near / far (1,n), and `image` (1,n,3,h,w) -- the ground
               truth when `align` is given, otherwise only its shape is read (or pass `image_shape=(h, w)` instead)
      align    None: render from target["extrinsics"] as they are.  A `TestCfg`: `align_target_poses` on the UN-stylized Gaussians
               first (test_step_align), with `losses` as its objective.
    The identity style is context["image"][:, 0]; styles of the context's image size share its `restyle` batch, every other size gets
    a batch of its own."""
    images = context["image"]
    if images.shape[0] != 1:
        raise ValueError("stylize_scene serves one scene per call (b == 1), as the reference's inference drivers do")
    style_list = _style_images(styles)
    identity = images[0, 0]
    # batches by image size, the identity style first in its own
    groups: dict = {tuple(identity.shape[-2:]): [(-1, identity)]}
    for i, im in enumerate(style_list):
        groups.setdefault(tuple(im.shape[-2:]), []).append((i, im.to(images)))
    dump: dict = {}
    sets: dict = {}
    with torch.no_grad():
        state = encoder.encode_scene(context)
        for members in groups.values():
            batch = torch.stack([im for _, im in members])
            out = encoder.restyle(state, {"image": batch}, visualization_dump=dump if members[0][0] == -1 else None)
            for (i, _), g in zip(members, out if isinstance(out, list) else [out]):
                sets[i] = g
    gaussians = [sets[i] for i in range(-1, len(style_list))]
    plain = gaussians[0]

    extrinsics = target["extrinsics"]
    if "image" in target:
        h, w = target["image"].shape[-2:]
    else:
        h, w = target["image_shape"]
    if align is not None and align.align_pose:
        extrinsics = align_target_poses(decoder, plain, {"context": context, "target": target}, losses, align)[0]
    with torch.no_grad():
        out: DecoderOutput = decoder.forward_styles(plain, [g.harmonics for g in gaussians], extrinsics, target["intrinsics"],
                                                    target["near"], target["far"], (h, w))
    return StylizedScene(gaussians, extrinsics, out.color, out.depth, dump)


def _panel_set(name, n_sets: int) -> int:
    """panel name -> index into [plain, style 0, style 1, ...]; -1 for the depth"""
    if name == "depth":
        return -1
    if isinstance(name, bool) or not (isinstance(name, int) or name in ("plain", "stylized")):
        raise ValueError(f"unknown panel {name!r}: 'plain', 'depth', 'stylized' or an integer style index")
    i = 0 if name == "plain" else (1 if name == "stylized" else 1 + name)
    if not 0 <= i < n_sets:
        raise ValueError(f"panel {name!r} asks for Gaussian set {i} of {n_sets} ([plain, style 0, ...])")
    return i


def gaussian_sets(scene_or_gaussians) -> list:
    """a `StylizedScene`, its list [plain, style 0, ...] of `Gaussians` over one geometry, or one `Gaussians` -> the list"""
    if isinstance(scene_or_gaussians, StylizedScene):
        return list(scene_or_gaussians.gaussians)
    if isinstance(scene_or_gaussians, Gaussians):
        return [scene_or_gaussians]
    return list(scene_or_gaussians)


def render_frames(decoder, sets: Sequence[Gaussians], used: Sequence[int], extrinsics: Tensor, intrinsics: Tensor, near: Tensor, far: Tensor,
                  image_shape, frames_per_pass: int = 60):
    """The float frames of a camera path (b == 1): sets[i] for i in `used` over the geometry of sets[0] through cameras (1,F,...), one
    `forward_styles` pass per `frames_per_pass` cameras.  Returns (color (len(used),F,3,h,w), depth (F,h,w) the sets share), fp32 on the
    device.  `render_flythrough` packs them into bytes, `evaluation.consistency_step` scores them."""
    if frames_per_pass < 1:
        raise ValueError("render_frames: frames_per_pass >= 1")
    F = extrinsics.shape[1]
    h, w = image_shape
    dev = extrinsics.device
    color = torch.empty((len(used), F, 3, h, w), dtype=torch.float32, device=dev)
    depth = torch.empty((F, h, w), dtype=torch.float32, device=dev)
    with torch.no_grad():
        for f0 in range(0, F, frames_per_pass):
            f1 = min(F, f0 + frames_per_pass)
            out = decoder.forward_styles(sets[0], [sets[i].harmonics for i in used], extrinsics[:, f0:f1], intrinsics[:, f0:f1],
                                         near[:, f0:f1], far[:, f0:f1], (h, w))
            color[:, f0:f1] = out.color[:, 0]
            depth[f0:f1] = out.depth[0]
    return color, depth


def render_flythrough(decoder, scene_or_gaussians: Union[StylizedScene, Gaussians, Sequence[Gaussians]], context: dict,
                      target: Optional[dict] = None, kind: str = "interpolation", num_frames: Optional[int] = None,
                      smooth: Optional[bool] = None, loop_reverse: Optional[bool] = None, panels: Sequence = ("stylized",), axis: int = 0,
                      gap: int = 8, frames_per_pass: int = 60) -> Tensor:
    """The frames of one of the drivers' videos as bytes: uint8 (F', H_out, W_out, 3) on the device.
      scene_or_gaussians  a `StylizedScene`, or its list [plain, style 0, ...] of `Gaussians` over one geometry, or one `Gaussians`
      context / target    as `trajectory_cameras` takes them (context also gives the image size and near / far); b == 1
      kind                "interpolation", "wobble" or "interpolation_exaggerated"; num_frames / smooth / loop_reverse default to the
                          reference's for that kind (60 eased looped frames; exaggerated: 300, linear, no loop)
      panels              up to 4 of "plain", "depth", "stylized" (= style 0) or an integer style index, laid out along `axis` with `gap`
    One `gsr_trajectory` launch, one `forward_styles` pass over the sets the panels name per `frames_per_pass` cameras (the rasterizer's
    workspace is sized for one pass, not for the video), `depth_range` over the whole video if a depth panel is asked for, and one
    `pack_frames`.  Nothing is copied to the host."""
    sets = gaussian_sets(scene_or_gaussians)
    if context["image"].shape[0] != 1:
        raise ValueError("render_flythrough serves one scene per call (b == 1), as the reference's inference drivers do")
    if not 1 <= len(panels) <= 4 or frames_per_pass < 1:
        raise ValueError("render_flythrough takes 1 to 4 panels and frames_per_pass >= 1")
    which = [_panel_set(p, len(sets)) for p in panels]
    used = sorted({i for i in which if i >= 0}) or [0]
    extrinsics, intrinsics, near, far = trajectory_cameras(context, target, kind, num_frames, smooth)
    h, w = context["image"].shape[-2:]
    color, depth = render_frames(decoder, sets, used, extrinsics, intrinsics, near, far, (h, w), frames_per_pass)
    tensors = [depth if i < 0 else color[used.index(i)] for i in which]
    rng = depth_range(depth) if -1 in which else None
    return pack_frames(tensors, axis=axis, gap=gap, loop_reverse=KINDS[kind][2] if loop_reverse is None else loop_reverse, depth_range=rng)


def save_flythrough(path, decoder, scene_or_gaussians, context: dict, *, fps: float = 30, quality: int = 90, **render) -> Tensor:
    """`render_video_generic` of the inference drivers: `render_flythrough(decoder, scene_or_gaussians, context, **render)` followed by
    `image_io.save_video(frames, path, fps, quality)`.  The frames stay on the device between the two -- the JPEG encoder reads the
    uint8 tensor `pack_frames` wrote -- and only the coded bytes come to the host.  `path` ends in `.avi` (Motion-JPEG; the reference
    writes .mp4).  Returns the frames."""
    from .image_io import save_video
    if Path(path).suffix.lower() != ".avi":
        raise ValueError(f"save_flythrough: this build writes Motion-JPEG AVI; name the file .avi, not {Path(path).name!r}")
    frames = render_flythrough(decoder, scene_or_gaussians, context, **render)
    save_video(frames, path, fps=fps, quality=quality)
    return frames


def export_scene_ply(scene: StylizedScene, directory, shift_and_scale: bool = False, save_sh_dc_only: bool = True) -> list:
    """infer_model_re10k.py:542-557: `gaussians.ply` for the un-stylized set and `stylized_gaussians.ply` for the stylized one
    (`stylized_gaussians_<s>.ply` per style when the scene holds several), scales and rotations from the visualization dump.
    Returns the paths written."""
    directory = Path(directory)
    dump = scene.visualization_dump
    scales, rotations = dump["scales"][0].reshape(-1, 3), dump["rotations"][0].reshape(-1, 4)
    n_styles = len(scene.gaussians) - 1
    paths = []
    for i, g in enumerate(scene.gaussians):
        name = "gaussians.ply" if i == 0 else ("stylized_gaussians.ply" if n_styles == 1 else f"stylized_gaussians_{i - 1}.ply")
        export_ply(g.means[0], scales, rotations, g.harmonics[0], g.opacities[0], directory / name, shift_and_scale=shift_and_scale,
                   save_sh_dc_only=save_sh_dc_only)
        paths.append(directory / name)
    return paths


def save_scene_images(output_dir, scene: str, style_image_name: str, batch: dict, output, stylized_output) -> list:
    """infer_model_re10k.py:505-535: the picture tree of one stylized scene under `output_dir / f"{scene} | {style_image_name[:-4]}"` --
    the style image under `batch["style"]["image_name"]` (its own suffix: Pillow unless it is .png), then `context/`, `target/`, `color/`
    and `stylized_color/`, every file `<index:0>6>.png`; context images go through the inverse normalisation (x * 0.5 + 0.5) first.
    `output` / `stylized_output`: anything with `.color` (1,v,3,h,w) -- two `DecoderOutput`s, or views of a `StylizedScene`.
    One `image_io.save_images` call, i.e. one encoder call, per directory.  Returns the paths written."""
    from .image_io import save_image, save_images
    root = Path(output_dir) / f"{scene} | {style_image_name[:-4]}"
    name = batch["style"]["image_name"]
    name = name if isinstance(name, str) else name[0]
    written = [root / name]
    save_image(batch["style"]["image"][0], written[0])
    ctx_index, tgt_index = batch["context"]["index"][0], batch["target"]["index"][0]
    groups = (("context", ctx_index, batch["context"]["image"][0].detach() * 0.5 + 0.5), ("target", tgt_index, batch["target"]["image"][0]),
              ("color", tgt_index, output.color[0]), ("stylized_color", tgt_index, stylized_output.color[0]))
    for folder, index, frames in groups:
        paths = [root / f"{folder}/{int(k):0>6}.png" for k in index]
        save_images(frames.detach().float(), paths)
        written += paths
    return written
