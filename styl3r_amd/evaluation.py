"""The test step: `ModelWrapperStyle.test_step` + `test_step_align` (src/model/model_wrapper_style.py:317-364, 391-461), the path every
number the reference reports goes through -- encoder, target-pose alignment, final render, PSNR / SSIM / LPIPS.

Deviations from the reference:
  * b >= 1 scenes per call (the reference asserts b == 1).  The alignment objective is b x the batch loss: every loss averages over the
    b scenes, so each scene's deltas then receive the gradient of their own b = 1 objective, and Adam is element-wise.  Scores are per
    scene, shape (b,).
  * The encoder runs under `no_grad` and its `requires_grad` flags are left alone (the reference sets them all False and switches the
    encoder to eval mode in test_step_align; nothing trains here, and the caller owns the module's mode).
  * LPIPS scores mean something only with learned weights: `scores["lpips_weights_loaded"]` says whether the module had them.
  * `test.save_image` is off by default (the reference's main.yaml turns it on): nothing is written unless the caller asks.
  * `test.save_video` writes Motion-JPEG `.avi` files (`image_io.save_video`), not the reference's `.mp4`.
Dataset loading, the evaluation index, saving comparisons and logging stay with the caller.

`estimate_relative_pose` (below) is the reference's other evaluation, `PoseEvaluator.test_step` (src/evaluation/pose_evaluator.py:48-164): the
pose of the context views relative to the first from a PnP-RANSAC initialisation and the same alignment loop with the SSIM-structure term added.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from pathlib import Path
from typing import Optional, Sequence, Union

import torch

from . import metrics
from .losses import LPIPS, LossMse

ADAM_BETAS, ADAM_EPS = (0.9, 0.999), 1e-8       # torch.optim.Adam defaults (test_step_align builds Adam(opt_params) without options)


@dataclass
class TestCfg:
    """the fields of `test` (config/main.yaml:55-63) that the test step reads"""
    __test__ = False                             # (not a pytest test class)
    align_pose: bool = True
    pose_align_steps: int = 100
    rot_opt_lr: float = 0.005
    trans_opt_lr: float = 0.005
    compute_scores: bool = True
    save_image: bool = False                     # write the rendered target views as <output_path>/<scene>/color/<index:0>6>.png
    save_video: bool = False                     # write them as <output_path>/video/<scene>_frame_<context indices>.avi as well
    output_path: Union[str, Path] = "outputs/test"


def save_color_images(cfg: TestCfg, batch: dict, output) -> list:
    """model_wrapper_style.py:366-372 for b >= 1 scenes: the rendered colours of scene i under `cfg.output_path / batch["scene"][i] / color`,
    named by the target indices; one `image_io.save_images` call (one encoder call) per scene.  Returns the paths written."""
    from .image_io import save_images
    scenes = batch["scene"]
    scenes = [scenes] if isinstance(scenes, str) else list(scenes)
    index = batch["target"]["index"]
    if len(scenes) != output.color.shape[0]:
        raise ValueError(f"save_color_images: {len(scenes)} scene names for {output.color.shape[0]} scenes")
    written = []
    for i, scene in enumerate(scenes):
        paths = [Path(cfg.output_path) / scene / f"color/{int(k):0>6}.png" for k in index[i]]
        save_images(output.color[i].detach(), paths)
        written += paths
    return written


def save_color_videos(cfg: TestCfg, batch: dict, output, fps: float = 30) -> list:
    """model_wrapper_style.py:374-379 for b >= 1 scenes: the rendered colours of scene i as one video,
    `cfg.output_path / "video" / f"{scene}_frame_{context indices joined by _}.avi"` (`<scene>.avi` when the context carries no `index`);
    one `image_io.save_video` call, i.e. one encoder call, per scene.  Returns the paths written."""
    from .image_io import save_video
    scenes = batch["scene"]
    scenes = [scenes] if isinstance(scenes, str) else list(scenes)
    if len(scenes) != output.color.shape[0]:
        raise ValueError(f"save_color_videos: {len(scenes)} scene names for {output.color.shape[0]} scenes")
    index = batch["context"].get("index")
    written = []
    for i, scene in enumerate(scenes):
        name = scene if index is None else f"{scene}_frame_" + "_".join(str(int(k)) for k in index[i])
        written.append(Path(cfg.output_path) / "video" / f"{name}.avi")
        save_video(output.color[i].detach().float(), written[-1], fps=fps)
    return written


def align_target_poses(decoder, gaussians, batch: dict, losses: Sequence, cfg: TestCfg, global_step: int = 0):
    """test_step_align (:391-447): `cfg.pose_align_steps` Adam steps on zero deltas (cam_rot_delta, cam_trans_delta) of every target view,
    folded into the target c2w after each step.  Objective: sum of `loss.forward(output, batch, gaussians, global_step)` over `losses`; a
    `LossMse` among them is computed inside the decoder's composite kernels (`mse_target`), the others are added on top.
    Per step: one decoder forward + backward and one `gsr_pose_adam_update` launch; the per-step losses stay on the device until the end.
    Returns (aligned extrinsics (b, v, 4, 4), per-step losses as floats)."""
    from . import _lib
    tgt = batch["target"]
    image = tgt["image"]
    b, v, _, h, w = image.shape
    dev = image.device
    if not losses:
        raise ValueError("align_target_poses: the alignment objective needs at least one loss")
    mse = next((fn for fn in losses if isinstance(fn, LossMse)), None)
    if mse is not None and not (image.is_cuda and image.dtype == torch.float32 and not image.requires_grad):
        raise ValueError("align_target_poses: the fused LossMse needs fp32 ground-truth target images on the GPU")
    rest = [fn for fn in losses if fn is not mse]
    fused = {} if mse is None else {"mse_target": image, "mse_weight": mse.cfg.weight}
    n = b * v
    rot = torch.zeros((b, v, 3), device=dev, requires_grad=True)
    trans = torch.zeros((b, v, 3), device=dev, requires_grad=True)
    extrinsics = tgt["extrinsics"].detach().float().contiguous().clone()          # updated in place by the kernel
    exp_avg = torch.zeros((n, 6), device=dev)                                     # Adam state per view: (rot xyz, trans xyz)
    exp_avg_sq = torch.zeros((n, 6), device=dev)
    lib = _lib.load()
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    history = []
    for step in range(1, cfg.pose_align_steps + 1):
        with torch.enable_grad():
            out = decoder.forward(gaussians, extrinsics, tgt["intrinsics"], tgt["near"], tgt["far"], (h, w),
                                  cam_rot_delta=rot, cam_trans_delta=trans, **fused)
            total = out.loss_mse if mse is not None else 0
            for fn in rest:
                total = total + fn.forward(out, batch, gaussians, global_step)
            g_rot, g_trans = torch.autograd.grad(total * b if b > 1 else total, [rot, trans], allow_unused=True)
        history.append(total.detach())
        g_rot = torch.zeros_like(rot) if g_rot is None else g_rot.contiguous()
        g_trans = torch.zeros_like(trans) if g_trans is None else g_trans.contiguous()
        _lib.check(lib.gsr_pose_adam_update(extrinsics.data_ptr(), exp_avg.data_ptr(), exp_avg_sq.data_ptr(), g_rot.data_ptr(),
                                            g_trans.data_ptr(), n, step, cfg.rot_opt_lr, cfg.trans_opt_lr, ADAM_BETAS[0], ADAM_BETAS[1],
                                            ADAM_EPS, stream), "gsr_pose_adam_update")
    return extrinsics, (torch.stack(history).tolist() if history else [])


def test_step(encoder, decoder, batch: dict, losses: Sequence, cfg: TestCfg = TestCfg(), lpips: Optional[LPIPS] = None,
              style: Optional[dict] = None, global_step: int = 0):
    """test_step (:317-364) for b >= 1 scenes.  Returns (DecoderOutput of the (aligned) target views, scores): scores has the reference's
    keys `psnr_ours`, `ssim_ours`, `lpips_ours` -- each the mean over a scene's target views, shape (b,) -- and `lpips_weights_loaded`;
    empty when `cfg.compute_scores` is off.  With `cfg.save_image` the rendered views are also written as PNG files (`save_color_images`;
    `batch["scene"]` and `batch["target"]["index"]` name them), with `cfg.save_video` as one Motion-JPEG AVI per scene (`save_color_videos`)."""
    tgt = batch["target"]
    b, v, _, h, w = tgt["image"].shape
    style = style if style is not None else {"image": batch["context"]["image"][:, 0]}
    with torch.no_grad():
        gaussians = encoder(batch["context"], style, global_step)
    extrinsics = align_target_poses(decoder, gaussians, batch, losses, cfg, global_step)[0] if cfg.align_pose else tgt["extrinsics"]
    with torch.no_grad():
        output = decoder.forward(gaussians, extrinsics, tgt["intrinsics"], tgt["near"], tgt["far"], (h, w))
    if cfg.save_image:
        save_color_images(cfg, batch, output)
    if cfg.save_video:
        save_color_videos(cfg, batch, output)
    if not cfg.compute_scores:
        return output, {}
    gt, pred = tgt["image"].reshape(b * v, -1, h, w), output.color.reshape(b * v, -1, h, w)
    module = lpips if lpips is not None else metrics.get_lpips(pred.device)
    psnr, ssim = metrics.image_scores(gt, pred)
    lp = metrics.compute_lpips(gt, pred, module)
    per_scene = lambda t: t.reshape(b, v).mean(dim=1)
    return output, {"lpips_ours": per_scene(lp), "ssim_ours": per_scene(ssim), "psnr_ours": per_scene(psnr),
                    "lpips_weights_loaded": bool(getattr(module, "weights_loaded", False))}


test_step.__test__ = False                       # (not a pytest test function where a test module imports it)


def validation_step(encoder, decoder, batch: dict, step: int = 0, labeler=None, lpips: Optional[LPIPS] = None, style: Optional[dict] = None,
                    extra_columns: Sequence = (), resolution: int = 256, baseline=None):
    """validation_step (:472-617) for the first scene of `batch` (the reference asserts b == 1): encoder and decoder as `test_step` runs them, the
    three scores as `val/psnr`, `val/ssim`, `val/lpips` (means over the target views) and the three pictures of
    `visualization.validation_images`.  The style is `style` if given, else `batch["style"]` as the reference takes it -- its image rescaled to
    [-1, 1] for an encoder with `stylized` set, and shown unscaled as the Style panel -- else the first context image, without a Style panel
    (the reference needs `batch["style"]`).  Images of the batch are in [0, 1], as everywhere in this package (the reference un-normalises its
    context images here).  The context depth is the dump's depth; more than one value per pixel is averaged (the reference averages exactly
    three and shows one as it is).  `baseline` (a `baseline.AdaIN2D`; None: no such column): "2D Baseline" is the comparison's first column, the
    target views stylised with the Style panel's image (`batch["style"]`'s, unscaled), else with `style["image"][0]` as given, which must then be
    in [0, 1].  Returns (DecoderOutput, scores, images); logging, the videos and the encoder visualizer stay with the caller."""
    from .visualization import validation_images
    ctx, tgt = batch["context"], batch["target"]
    _, v, _, h, w = tgt["image"].shape
    style_panel = None
    if style is None and "style" in batch:
        style = dict(batch["style"])
        style_panel = style["image"][0]
        if getattr(encoder, "stylized", False):
            style["image"] = (style["image"] - 0.5) / 0.5
    elif style is None:
        style = {"image": ctx["image"][:, 0]}
    dump = {}
    with torch.no_grad():
        gaussians = encoder(ctx, style, step, visualization_dump=dump)
        output = decoder.forward(gaussians, tgt["extrinsics"], tgt["intrinsics"], tgt["near"], tgt["far"], (h, w))
    gt, pred = tgt["image"][0], output.color[0]
    module = lpips if lpips is not None else metrics.get_lpips(pred.device)
    psnr, ssim = metrics.image_scores(gt, pred)
    scores = {"val/psnr": psnr.mean(), "val/ssim": ssim.mean(), "val/lpips": metrics.compute_lpips(gt, pred, module).mean(),
              "lpips_weights_loaded": bool(getattr(module, "weights_loaded", False))}
    context_depth = dump["depth"][0].reshape(ctx["image"].shape[1], *ctx["image"].shape[-2:], -1)
    context_depth = context_depth[..., 0] if context_depth.shape[-1] == 1 else context_depth.mean(dim=-1)
    images = validation_images(ctx["image"][0], context_depth, gt, pred, output.depth[0], gaussians, batch, extra_columns=extra_columns,
                               style_image=style_panel, labeler=labeler, resolution=resolution, baseline=baseline,
                               baseline_style=None if baseline is None or style_panel is not None else style["image"][0])
    return output, scores, images


# ---- relative pose between the context views (src/evaluation/pose_evaluator.py:48-164) ------------------------------------------------
@dataclass
class PoseEvalCfg:
    """what `PoseEvaluator.test_step` and `get_pnp_pose` hard-code, as fields"""
    steps: int = 200
    rot_lr: float = 0.005
    trans_lr: float = 0.005
    opacity_threshold: float = 0.3
    pnp_iterations: int = 100
    reprojection_error: float = 5.0
    ssim_structure_weight: float = 1.0
    seed: int = 0
    pixel_offset: float = 0.0
    context_normalized: bool = True             # context images are in [-1, 1]: the photometric target is image * 0.5 + 0.5


def estimate_relative_pose(encoder, decoder, batch: dict, losses: Sequence, cfg: PoseEvalCfg = PoseEvalCfg(), style: Optional[dict] = None,
                           init_pose: Optional[torch.Tensor] = None, global_step: int = 0) -> dict:
    """The pose of every context view but the first, relative to the first, for b >= 1 scenes: the encoder once (no gradients, with a
    visualization dump), `pose_align.pnp_pose` on each view's per-pixel means and opacities -- (b, v - 1) problems in one call -- unless
    `init_pose` (b, v - 1, 4, 4) is given, then `cfg.steps` Adam steps of `align_target_poses` on the photometric objective
    `losses + [LossSsimStructure]` against those context images.  Returns `pose_init`, `pose` (b, v - 1, 4, 4), `losses` (per step),
    `pnp_status` (None with `init_pose`) and, when the context has ground-truth extrinsics, `e_t_ours`, `e_R_ours`,
    `e_pose_ours = max(e_t, e_R)` in degrees, (b, v - 1), against the ground truth expressed in the first view's frame."""
    from .losses import LossSsimStructure
    from .pose_align import align_poses, pnp_pose
    ctx = batch["context"]
    b, v, _, h, w = ctx["image"].shape
    if v < 2:
        raise ValueError("estimate_relative_pose needs at least two context views")
    style = style if style is not None else {"image": ctx["image"][:, 0]}
    dump: dict = {}
    with torch.no_grad():
        gaussians = encoder(ctx, style, global_step, visualization_dump=dump)
    status = None
    if init_pose is None:
        means, opac = dump["means"], dump["opacities"]
        means = means.reshape(b, v, h, w, -1, 3)[:, 1:, :, :, 0]
        opac = opac.reshape(b, v, h, w, -1)[:, 1:, :, :, 0]
        pose_init, status = pnp_pose(means, opac, ctx["intrinsics"][:, 1:], (h, w), cfg.opacity_threshold, cfg.pnp_iterations,
                                     cfg.reprojection_error, cfg.seed, cfg.pixel_offset)
    else:
        pose_init = init_pose.detach().float().reshape(b, v - 1, 4, 4)
    image = ctx["image"][:, 1:].detach()
    image = (image * 0.5 + 0.5 if cfg.context_normalized else image).contiguous()
    target = {"image": image, "extrinsics": pose_init, "intrinsics": ctx["intrinsics"][:, 1:], "near": ctx["near"][:, 1:],
              "far": ctx["far"][:, 1:]}
    inner = {**batch, "target": target}
    objective = list(losses) + [LossSsimStructure(cfg.ssim_structure_weight)]
    if image.is_cuda:
        pose, history = align_target_poses(decoder, gaussians, inner, objective,
                                           TestCfg(pose_align_steps=cfg.steps, rot_opt_lr=cfg.rot_lr, trans_opt_lr=cfg.trans_lr), global_step)
    else:                                       # host tensors: the framework loop with the same objective
        from types import SimpleNamespace
        fn = lambda color, _t: sum(f.forward(SimpleNamespace(color=color), inner, gaussians, global_step) for f in objective)
        pose, history = align_poses(decoder, gaussians, image, pose_init, target["intrinsics"], target["near"], target["far"],
                                    steps=cfg.steps, rot_lr=cfg.rot_lr, trans_lr=cfg.trans_lr, loss_fn=fn)
    out = {"pose_init": pose_init, "pose": pose.detach(), "losses": history, "pnp_status": status}
    if "extrinsics" in ctx:
        E = ctx["extrinsics"].detach().float()
        gt = torch.linalg.inv(E[:, :1]) @ E[:, 1:]
        e_t, _, e_R = metrics.compute_pose_error(gt, out["pose"].to(gt.device))
        out.update(e_t_ours=e_t, e_R_ours=e_R, e_pose_ours=torch.maximum(e_t, e_R))
    return out


# ---- multi-view consistency of a fly-through (metrics.compute_consistency) ------------------------------------------------------------
def consistency_step(decoder, scene_or_gaussians, context: dict, *, target: Optional[dict] = None, kind: str = "interpolation",
                     num_frames: int = 60, frames_per_pass: int = 60, gaps=(metrics.SHORT_RANGE_GAP, metrics.LONG_RANGE_GAP),
                     lpips: Optional[LPIPS] = None, depth_tol: float = 0.05) -> dict:
    """The score of a stylized scene, which has no ground truth: short- and long-range multi-view consistency of the frames of one
    fly-through, for the un-stylized render and every style at once (b == 1).
      scene_or_gaussians  an `inference.StylizedScene`, its list [plain, style 0, ...] of `Gaussians` over one geometry, or one `Gaussians`
      context / target    as `trajectory.trajectory_cameras` takes them; `kind` and `num_frames` pick the path, WITHOUT the reverse loop of
                          the videos (a frame pair (t, t + gap) of the way back is a pair of the way out)
    The float frames come from `inference.render_frames` -- the passes `render_flythrough` runs, `frames_per_pass` cameras each -- then ONE
    `metrics.compute_consistency` call over all sets: the warp is geometric, through the depth map the sets share and the path's exact
    cameras.  A scale-invariant decoder renders depth in units of each camera's near plane; it is brought back to the cameras' units here.
    Returns {"plain": {...}, "style_0": {...}, ...}, each as `compute_consistency` describes it."""
    from .inference import gaussian_sets, render_frames
    from .trajectory import trajectory_cameras
    sets = gaussian_sets(scene_or_gaussians)
    if context["image"].shape[0] != 1:
        raise ValueError("consistency_step scores one scene per call (b == 1)")
    extrinsics, intrinsics, near, far = trajectory_cameras(context, target, kind, num_frames, None)
    h, w = context["image"].shape[-2:]
    color, depth = render_frames(decoder, sets, range(len(sets)), extrinsics, intrinsics, near, far, (h, w), frames_per_pass)
    if getattr(decoder, "make_scale_invariant", False):
        depth = depth * near[0, :, None, None].to(depth)
    scores = metrics.compute_consistency(color, depth, extrinsics[0], intrinsics[0], gaps=gaps, lpips=lpips, depth_tol=depth_tol)
    return {("plain" if i == 0 else f"style_{i - 1}"): s for i, s in enumerate(scores)}
