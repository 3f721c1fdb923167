#!/usr/bin/env python
"""The relative-pose evaluation (evaluation.estimate_relative_pose) piece by piece on the MI355X.  One JSON line:
  (a) `pnp_pose` (gsr_pnp_ransac: 100 six-point hypotheses, scoring, 10 LM steps) at P = 1 and P = 8 problems of 256 x 256 points, 30 % gross
      outliers, 20 % under the opacity threshold, ~1 px noise;
  (b) `ssim_structure` forward + backward at 1 x 3 x 256^2 and 40 x 3 x 256^2: the two HIP kernels against the same formula composed of
      framework ops (losses._structure_expression: the reference's path) on the same GPU, alternating in this process; and the forward
      (with adjoint maps) and the backward alone with their algorithmic bytes;
  (c) one refinement step and the whole `--steps`-step estimate for one pair of 256 x 256 context views with [mse, lpips, ssim-structure]
      (Gaussians of scenes.make_scene behind a stand-in encoder: the encoder is timed by tools/bench_eval.py), PnP included.
LPIPS weights are not loaded (random He-scaled VGG16): the loss values are meaningless, the times are not.
  python tools/bench_pose.py [--steps 200] [--rounds 3]
"""
import argparse
import json
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import torch

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=200)
ap.add_argument("--rounds", type=int, default=3, help="alternating A/B rounds")
args = ap.parse_args()
assert torch.cuda.is_available(), "bench_pose needs the MI355X"

from styl3r_amd import evaluation, vit_ops
from styl3r_amd.decoder import DecoderSplattingCUDACfg, Gaussians, get_decoder
from styl3r_amd.losses import LPIPS, LossLpips, LossMse, _SsimStructureHip, _structure_expression, ssim_structure_per_image
from styl3r_amd.pose_align import SE3_exp, pnp_pose
from styl3r_amd.scenes import make_scene

dev = torch.device("cuda:0")
H = 256
out = {"metric": "relative-pose evaluation: PnP-RANSAC init + SSIM-structure refinement, 256x256", "linear_arithmetic": vit_ops.LINEAR_MODE,
       "data": "synthetic, random-init LPIPS weights"}


def event_ms(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize(dev)
    return e0.elapsed_time(e1) / reps


# ---- (a) PnP ------------------------------------------------------------------------------------------------------------------------------
def pnp_problem(seed):
    g = torch.Generator().manual_seed(seed)
    K = torch.tensor([[0.86, 0, 0.5], [0, 0.86, 0.5], [0, 0, 1.0]], dtype=torch.float64)
    Kp = K.clone(); Kp[0] *= H; Kp[1] *= H
    c2w = SE3_exp(torch.tensor([0.7, -0.4, 0.5, 0.2, -0.25, 0.1], dtype=torch.float64)).inverse()
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(H, dtype=torch.float64), indexing="ij")
    d = 1 + 4 * torch.rand(H, H, generator=g, dtype=torch.float64)
    lift = lambda px, py: torch.stack([(px - Kp[0, 2]) / Kp[0, 0] * d, (py - Kp[1, 2]) / Kp[1, 1] * d, d], -1) @ c2w[:3, :3].T + c2w[:3, 3]
    world = lift(xs, ys) + (d / Kp[0, 0])[..., None] * torch.randn(H, H, 3, generator=g, dtype=torch.float64)
    bad = torch.rand(H, H, generator=g) < 0.3
    world = torch.where(bad[..., None], lift(xs + 40, ys - 30), world)
    op = 0.31 + 0.69 * torch.rand(H, H, generator=g)
    low = torch.rand(H, H, generator=g) < 0.2
    op[low] = 0.1
    world[low] = 1e4
    return world.float(), op.float(), K.float(), c2w


pnp = {}
for P in (1, 8):
    prs = [pnp_problem(10 + i) for i in range(P)]
    means, op, K = (torch.stack([q[k] for q in prs]).to(dev) for k in range(3))
    run = lambda: pnp_pose(means, op, K, (H, H))
    for _ in range(3):
        pose, st = run()
    ms = min(event_ms(run, 300) for _ in range(args.rounds))
    err = max(float((pose[i].cpu().double() - prs[i][3]).abs().max()) for i in range(P))
    pnp[f"P{P}"] = {"ms_per_call": round(ms, 3), "ms_per_problem": round(ms / P, 3), "inliers": st["inliers"].tolist(),
                    "masked": st["masked"].tolist(), "max_abs_pose_error": float(f"{err:.3g}")}
out["pnp_256x256_100_hypotheses"] = pnp

# ---- (b) SSIM structure -------------------------------------------------------------------------------------------------------------------
g = torch.Generator(dev).manual_seed(3)
ssim = {}
for n in (1, 40):
    x = torch.rand(n, 3, H, H, device=dev, generator=g)
    y = (x + 0.1 * torch.randn(x.shape, device=dev, generator=g)).clamp(0, 1)

    def fwd_bwd(fn):
        yy = y.detach().requires_grad_(True)
        (1 - fn(x, yy).mean()).backward()
        return yy.grad
    hip = lambda: fwd_bwd(ssim_structure_per_image)
    ops = lambda: fwd_bwd(_structure_expression)
    for _ in range(3):
        ga, gb = hip(), ops()
    reps = 2000 if n == 1 else 100
    t_hip, t_ops = [], []
    for _ in range(args.rounds):
        t_hip.append(event_ms(hip, reps)); t_ops.append(event_ms(ops, reps))
    # the kernels alone: forward with adjoint maps (+ its fold), then the backward
    yy = y.detach().requires_grad_(True)
    per = ssim_structure_per_image(x, yy)
    gout = torch.full_like(per, -1.0 / n)
    t_f = min(event_ms(lambda: _SsimStructureHip.apply(yy, x), reps) for _ in range(args.rounds))
    t_b = min(event_ms(lambda: torch.autograd.grad(per, yy, gout, retain_graph=True), reps) for _ in range(args.rounds))
    px, mp = n * 3 * H * H, n * 3 * (H - 10) * (H - 10)
    bytes_f, bytes_b = 4 * (2 * px + 3 * mp), 4 * (3 * mp + 2 * px + px)
    ssim[f"{n}x3x{H}x{H}"] = {
        "hip_fwd_bwd_ms": round(min(t_hip), 4), "framework_ops_fwd_bwd_ms": round(min(t_ops), 4),
        "hip_all": [round(t, 4) for t in t_hip], "framework_ops_all": [round(t, 4) for t in t_ops], "speedup": round(min(t_ops) / min(t_hip), 2),
        "grad_max_abs_diff_over_max": float(f"{float((ga - gb).abs().max() / gb.abs().max()):.3g}"),
        "fwd_call_ms": round(t_f, 4), "fwd_algorithmic_MB": round(bytes_f / 1e6, 2), "fwd_GB_per_s": round(bytes_f / (t_f * 1e-3) / 1e9, 1),
        "bwd_call_ms": round(t_b, 4), "bwd_algorithmic_MB": round(bytes_b / 1e6, 2), "bwd_GB_per_s": round(bytes_b / (t_b * 1e-3) / 1e9, 1)}
out["ssim_structure"] = ssim


# ---- (c) the refinement and the whole estimate ----------------------------------------------------------------------------------------------
class SceneEncoder(torch.nn.Module):
    def __init__(self, gs):
        super().__init__()
        self.gs = gs

    def forward(self, context, style, global_step=0, visualization_dump=None):
        if visualization_dump is not None:
            visualization_dump["means"] = self.gs.means.reshape(1, 2, H, H, 1, 3)
            visualization_dump["opacities"] = self.gs.opacities.reshape(1, 2, H, H, 1, 1)
        return self.gs


sc = make_scene(n_ctx=2, grid_hw=(H, H), n_views=2, image_hw=(H, H), sh_degree=0, seed=1234).to(dev)
gs = Gaussians(sc.means[None], sc.covariances[None], sc.harmonics[None], sc.opacities[None])
dec = get_decoder(DecoderSplattingCUDACfg("splatting_cuda", [0.0, 0.0, 0.0], True)).to(dev)
E = torch.eye(4, device=dev).repeat(1, 2, 1, 1)
E[:, 1, 0, 3] = 1.0
Kc, near, far = sc.intrinsics[None], sc.near[None], sc.far[None]
with torch.no_grad():
    image = dec.forward(gs, E, Kc, near, far, (H, H)).color
batch = {"context": {"image": image * 2 - 1, "extrinsics": E, "intrinsics": Kc, "near": near, "far": far}}
lp = LPIPS()
with torch.no_grad():
    for mod in lp.net.modules():
        if isinstance(mod, torch.nn.Conv2d):
            mod.weight.normal_(0, (2.0 / mod.weight[0].numel()) ** 0.5); mod.bias.normal_(0, 0.01)
    for k in range(5):
        getattr(lp, f"lin{k}").model[1].weight.uniform_(0, 1)
lp = lp.to(dev).eval().requires_grad_(False)
losses = [LossMse(), LossLpips(lpips=lp)]
enc = SceneEncoder(gs)
init = (SE3_exp(torch.tensor([0.02, -0.015, 0.01, 0.01, -0.008, 0.012], device=dev)) @ E[0, 1].inverse()).inverse()[None, None]


def estimate(steps, init_pose=None):
    cfg = evaluation.PoseEvalCfg(steps=steps, pixel_offset=0.5)
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    r = evaluation.estimate_relative_pose(enc, dec, batch, losses, cfg, init_pose=init_pose)
    torch.cuda.synchronize(dev)
    return time.perf_counter() - t0, r


estimate(5); estimate(5, init)                                       # warm-up of both entries
step_ms = min(estimate(50, init)[0] / 50 for _ in range(args.rounds)) * 1e3
t_all, r = min((estimate(args.steps) for _ in range(args.rounds)), key=lambda tr: tr[0])
t_pert, rp = estimate(args.steps, init)
out["estimate_one_pair"] = {"refinement_ms_per_step": round(step_ms, 3), "steps": args.steps, "pnp_plus_refinement_s": round(t_all, 3),
                            "e_R_deg": round(float(r["e_R_ours"]), 4), "e_t_deg": round(float(r["e_t_ours"]), 4),
                            "from_perturbed_init": {"s": round(t_pert, 3), "loss_first_last": [rp["losses"][0], rp["losses"][-1]],
                                                    "e_R_deg": round(float(rp["e_R_ours"]), 4), "e_t_deg": round(float(rp["e_t_ours"]), 4)}}
print(json.dumps(out))
