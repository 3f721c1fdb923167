#!/usr/bin/env python
"""The test step (evaluation.test_step: encoder, 100-step target-pose alignment, final render, PSNR / SSIM / LPIPS) at the C2 shape: 2 context
+ 3 target views of 256 x 256 on the full-size encoder (random init, heads re-centred by scenes.recentre_output_heads_ so that it renders),
target poses perturbed as in bench.py's align_pose leg.  One JSON line:
  * per-phase times of one scene (encoder, alignment, final render, scoring) and their total;
  * the alignment per step for the [mse, lpips] objective of the NVS experiments and for MSE only, new path (align_target_poses: fused MSE,
    one gsr_pose_adam_update launch, no read-back in the loop) against pose_align.align_poses with the same objective as its loss_fn,
    alternating in this process;
  * the device time of gsr_image_scores (+ its fold) at 3 and 40 images of 3 x 256 x 256;
  * scenes/s of the whole test step at b = 1 and b = 4.
LPIPS weights are not loaded (random He-scaled VGG16, lin weights in [0, 1]): the LPIPS scores are meaningless, the time is not.
  python tools/bench_eval.py [--steps 100] [--rounds 3]
"""
import argparse
import json
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import torch

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=100)
ap.add_argument("--rounds", type=int, default=3, help="alternating A/B rounds of the alignment")
ap.add_argument("--profile", action="store_true", help="only one warm-up and one test step, then gsr_image_scores at 40 images (run under rocprofv3)")
args = ap.parse_args()
assert torch.cuda.is_available(), "bench_eval needs the MI355X"

from styl3r_amd import evaluation, metrics, vit_ops
from styl3r_amd.decoder import DecoderSplattingCUDACfg, get_decoder
from styl3r_amd.encoder import EncoderNoPoSplatMultiTokenStyle, EncoderNoPoSplatTokenStyleCfg
from styl3r_amd.losses import LPIPS, LossLpips, LossMse, mse_loss
from styl3r_amd.pose_align import align_poses
from styl3r_amd.scenes import make_scene, recentre_output_heads_

dev = torch.device("cuda:0")
torch.manual_seed(0)
with torch.device(dev):
    enc = EncoderNoPoSplatMultiTokenStyle(EncoderNoPoSplatTokenStyleCfg()).eval()
enc.head_streams = True
dec = get_decoder(DecoderSplattingCUDACfg("splatting_cuda", [0.0, 0.0, 0.0], True)).to(dev)
H, V_CTX, V_TGT = 256, 2, 3
sc = make_scene(n_ctx=V_CTX, grid_hw=(8, 8), n_views=V_TGT, image_hw=(H, H), seed=1234)
g = torch.Generator(dev).manual_seed(1234)
ctx = dict(image=torch.rand(1, V_CTX, 3, H, H, device=dev, generator=g) * 2 - 1,
           intrinsics=sc.intrinsics[:1].to(dev).expand(1, V_CTX, 3, 3).contiguous())
style = dict(image=ctx["image"][:, 0])
recentre_output_heads_(enc, ctx, style)
ex = lambda t: t.to(dev)[None].contiguous()
E, K, NEAR, FAR = ex(sc.extrinsics), ex(sc.intrinsics), ex(sc.near), ex(sc.far)
with torch.no_grad():
    gs = enc(ctx, style, 0)
    target = dec.forward(gs, E, K, NEAR, FAR, (H, H)).color
gq = torch.Generator(dev).manual_seed(7)
pert = E.clone()
pert[..., :3, 3] += 0.01 * torch.randn(1, V_TGT, 3, device=dev, generator=gq)
batch = {"context": ctx, "target": {"image": target, "extrinsics": pert, "intrinsics": K, "near": NEAR, "far": FAR}}

lp = LPIPS()
with torch.no_grad():
    for mod in lp.net.modules():
        if isinstance(mod, torch.nn.Conv2d):
            mod.weight.normal_(0, (2.0 / mod.weight[0].numel()) ** 0.5); mod.bias.normal_(0, 0.01)
    for k in range(5):
        getattr(lp, f"lin{k}").model[1].weight.uniform_(0, 1)
lp = lp.to(dev).eval().requires_grad_(False)
OBJECTIVES = {"mse_lpips": [LossMse(), LossLpips(lpips=lp)], "mse": [LossMse()]}


def loss_fn(name):
    """the same objective as align_poses' loss_fn(pred, target)"""
    if name == "mse":
        return lambda pred, t: mse_loss(pred, t)
    w = OBJECTIVES[name][1].cfg.weight
    return lambda pred, t: mse_loss(pred, t) + w * lp(pred.reshape(-1, 3, H, H), t.reshape(-1, 3, H, H), normalize=True).mean()


def sync_time(fn):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize(dev)
    return time.perf_counter() - t0, r


def run_new(name, steps):
    return evaluation.align_target_poses(dec, gs, batch, OBJECTIVES[name], evaluation.TestCfg(pose_align_steps=steps))


def run_old(name, steps):
    t = batch["target"]
    return align_poses(dec, gs, t["image"], t["extrinsics"], t["intrinsics"], t["near"], t["far"], steps=steps, rot_lr=0.005, trans_lr=0.005,
                       loss_fn=loss_fn(name))


if args.profile:
    evaluation.test_step(enc, dec, batch, OBJECTIVES["mse_lpips"], evaluation.TestCfg(pose_align_steps=3), lpips=lp)
    evaluation.test_step(enc, dec, batch, OBJECTIVES["mse_lpips"], evaluation.TestCfg(pose_align_steps=args.steps), lpips=lp)
    a = torch.rand(40, 3, H, H, device=dev, generator=g)
    for _ in range(10):
        metrics.image_scores(a, a.flip(-1))
    torch.cuda.synchronize(dev)
    sys.exit(0)

out = {"metric": "test step at C2: 2 ctx + 3 tgt views 256x256, batch 1, 100 pose-alignment steps", "linear_arithmetic": vit_ops.LINEAR_MODE,
       "lpips_weights_loaded": lp.weights_loaded, "data": "synthetic, random-init weights"}
align = {}
for name in OBJECTIVES:
    run_new(name, 5); run_old(name, 5)                               # warm-up of both paths
    new_ms, old_ms = [], []
    for _ in range(args.rounds):
        dt, (_, h_new) = sync_time(lambda: run_new(name, args.steps))
        new_ms.append(1e3 * dt / args.steps)
        dt, (_, h_old) = sync_time(lambda: run_old(name, args.steps))
        old_ms.append(1e3 * dt / args.steps)
    align[name] = {"new_ms_per_step": round(min(new_ms), 3), "align_poses_ms_per_step": round(min(old_ms), 3),
                   "new_ms_per_step_all": [round(x, 3) for x in new_ms], "align_poses_ms_per_step_all": [round(x, 3) for x in old_ms],
                   "speedup": round(min(old_ms) / min(new_ms), 2), "loss_first_last_new": [h_new[0], h_new[-1]],
                   "loss_first_last_align_poses": [h_old[0], h_old[-1]]}
out["align"] = align

# per-phase times of one test step (b = 1, [mse, lpips])
cfg = evaluation.TestCfg(pose_align_steps=args.steps)
evaluation.test_step(enc, dec, batch, OBJECTIVES["mse_lpips"], evaluation.TestCfg(pose_align_steps=3), lpips=lp)      # warm-up
with torch.no_grad():
    t_enc, gs1 = sync_time(lambda: enc(ctx, style, 0))
t_align, (E1, _) = sync_time(lambda: evaluation.align_target_poses(dec, gs1, batch, OBJECTIVES["mse_lpips"], cfg))
with torch.no_grad():
    t_render, o = sync_time(lambda: dec.forward(gs1, E1, K, NEAR, FAR, (H, H)))
gt_f, pr_f = target.reshape(V_TGT, 3, H, H), o.color.reshape(V_TGT, 3, H, H)
t_score, _ = sync_time(lambda: (metrics.image_scores(gt_f, pr_f), metrics.compute_lpips(gt_f, pr_f, lp)))
out["phases_ms"] = {"encoder": round(1e3 * t_enc, 2), "align": round(1e3 * t_align, 2), "render": round(1e3 * t_render, 2),
                    "scores": round(1e3 * t_score, 2), "total": round(1e3 * (t_enc + t_align + t_render + t_score), 2)}

# gsr_image_scores device time (two launches: the pass and the fold), events around 50 back-to-back calls
kern = {}
for n in (3, 40):
    a = torch.rand(n, 3, H, H, device=dev, generator=g); b = (a + 0.05 * torch.randn(a.shape, device=dev, generator=g)).clamp(0, 1)
    for _ in range(5):
        metrics.image_scores(a, b)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(50):
        metrics._scores_hip(a, b)
    e1.record(); torch.cuda.synchronize(dev)
    us = 1e3 * e0.elapsed_time(e1) / 50
    kern[f"{n}x3x{H}x{H}"] = {"us_per_call": round(us, 2), "GB_per_s_of_both_images": round(2 * a.numel() * 4 / (us * 1e-6) / 1e9, 1)}
out["image_scores_kernel"] = kern

# scenes/s of the whole test step
sps = {}
for b in (1, 4):
    rep = lambda t: t.expand(b, *t.shape[1:]).contiguous()
    bb = {"context": {k: rep(v) for k, v in ctx.items()},
          "target": {k: rep(v) for k, v in batch["target"].items()}}
    evaluation.test_step(enc, dec, bb, OBJECTIVES["mse_lpips"], evaluation.TestCfg(pose_align_steps=3), lpips=lp)
    dt, (_, scores) = sync_time(lambda: evaluation.test_step(enc, dec, bb, OBJECTIVES["mse_lpips"], cfg, lpips=lp))
    sps[f"b{b}"] = {"s_per_call": round(dt, 3), "scenes_per_s": round(b / dt, 2),
                    "psnr_ours": [round(float(x), 3) for x in scores["psnr_ours"]], "ssim_ours": [round(float(x), 5) for x in scores["ssim_ours"]]}
out["test_step"] = sps
print(json.dumps(out))
