"""Serving one scene in many styles: the flow of the reference's inference drivers (infer_model_re10k.py:472-557,
infer_model_tnt_batch.py) on the scene cache of the encoder and the multi-style pass of the rasterizer.

The reference calls the encoder once with the first context image as "identity" style and once per real style, aligns the target
poses on the un-stylized Gaussians, then renders the plain and every stylized set through the same cameras, one rasterizer pass per
(set, camera list).  Here the style-independent part of the encoder runs once (`encode_scene`), all styles of one image size go
through ONE `restyle` batch, and the plain + S stylized sets -- which share means, covariances and opacities -- are rendered by ONE
`forward_styles` call.  Trajectory interpolation, video / PLY files and the dataset readers stay with the caller: the function takes
cameras, so a video is a call whose target holds the 60 interpolated extrinsics.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Sequence

import torch
from torch import Tensor

from .decoder import DecoderOutput, Gaussians
from .evaluation import TestCfg, align_target_poses


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
