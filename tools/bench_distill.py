#!/usr/bin/env python
"""Point-map distillation at the C3 shape (b = 10 scenes, 2 context views 256 x 256): the frozen full-size teacher's forward
(distiller.Dust3R, random init: the checkpoints are absent), the Regr3D loss forward + backward on the HIP kernels and, on the same device,
as `regr3d_expression` (the reference's op sequence: two torch.quantile row sorts, ~20 element-wise launches, two boolean gathers), and
the C3 train step without and with `distiller=`.  One JSON line.
  python tools/bench_distill.py [--scenes 10] [--size 256] [--reps 20] [--steps 3] [--no-step]
"""
import argparse, json, sys
from pathlib import Path
sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import torch
from styl3r_amd.distiller import DISTILLER_PARAMS, Dust3R
from styl3r_amd.losses import Regr3D, regr3d_expression

ap = argparse.ArgumentParser()
ap.add_argument("--scenes", type=int, default=10); ap.add_argument("--size", type=int, default=256)
ap.add_argument("--reps", type=int, default=20); ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--steps", type=int, default=3); ap.add_argument("--no-step", action="store_true", help="skip the two train-step timings")
args = ap.parse_args()
assert torch.cuda.is_available(), "bench_distill needs the MI355X"
dev = torch.device("cuda:0")
torch.manual_seed(0)
b, H = args.scenes, args.size
g = torch.Generator(dev).manual_seed(1)


def timed(fn, reps=args.reps, warmup=args.warmup):
    """median ms per call over `reps` calls, each between two device events"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize(dev)
    ts = []
    for _ in range(reps):
        a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); e.record()
        torch.cuda.synchronize(dev)
        ts.append(a.elapsed_time(e))
    return sorted(ts)[len(ts) // 2]


# ---- the teacher ----------------------------------------------------------------------------------------------------------------------------
with torch.device(dev):
    teacher = Dust3R(**DISTILLER_PARAMS)
with torch.no_grad():      # random-init heads give |xyz| ~ 0 and confidence ~ 2: shift the output biases so that the loss sees a populated valid set
    for head in (teacher.downstream_head1, teacher.downstream_head2):
        head.dpt.head[4].bias.copy_(torch.tensor([0.0, 0.0, 1.2, 1.0], device=dev))
ctx = dict(image=torch.rand(b, 2, 3, H, H, device=dev, generator=g) * 2 - 1)
teacher_ms = timed(lambda: teacher(ctx, False), reps=max(3, args.reps // 4), warmup=2)
gt1, gt2 = teacher(ctx, False)
res = {"metric": "point-map distillation, C3 shape", "scenes": b, "size": H, "teacher_forward_ms": round(teacher_ms, 3),
       "teacher_params": sum(p.numel() for p in teacher.parameters()), "teacher_valid_share": round(float((gt1["conf"] >= 3).float().mean()), 3)}

# ---- the loss: kernels vs the expression, both on this device ---------------------------------------------------------------------------------
means = torch.stack((gt1["pts3d"], gt2["pts3d"]), dim=1).unsqueeze(-2)                       # (b, 2, h, w, 1, 3), as visualization_dump["means"]
means = (means + 0.1 * torch.randn(means.shape, device=dev, generator=g)).requires_grad_(True)
for tag, norm_mode in (("none", None), ("avg_dis", "avg_dis")):
    loss_fn = Regr3D(norm_mode=norm_mode)

    def hip():
        means.grad = None
        loss_fn(gt1["pts3d"], gt2["pts3d"], means[:, 0].squeeze(-2), means[:, 1].squeeze(-2), gt1["conf"], gt2["conf"]).backward()

    def expr():
        means.grad = None
        regr3d_expression(gt1["pts3d"], gt2["pts3d"], means[:, 0].squeeze(-2), means[:, 1].squeeze(-2), gt1["conf"], gt2["conf"],
                          norm_mode=norm_mode).backward()

    hip(); g_hip = means.grad.clone(); expr(); g_exp = means.grad.clone()
    a = timed(hip); e = timed(expr); a2 = timed(hip)                                        # A / B / A: the spread of the same route
    res[f"loss_{tag}"] = {"hip_fwd_bwd_ms": round(a, 4), "hip_again_ms": round(a2, 4), "expression_fwd_bwd_ms": round(e, 4),
                          "speedup": round(e / a, 2), "grad_rel_diff": float((g_hip - g_exp).abs().max() / g_exp.abs().max())}
del means

# ---- the C3 step without and with the distiller ------------------------------------------------------------------------------------------------
if not args.no_step:
    from styl3r_amd import dist_utils
    from styl3r_amd.decoder import DecoderSplattingCUDACfg, get_decoder
    from styl3r_amd.encoder import EncoderNoPoSplatMultiTokenStyle, EncoderNoPoSplatTokenStyleCfg
    from styl3r_amd.scenes import make_scene, recentre_output_heads_
    from styl3r_amd.train import TrainStep
    enc = EncoderNoPoSplatMultiTokenStyle(EncoderNoPoSplatTokenStyleCfg(stylized=False)).to(dev)
    dec = get_decoder(DecoderSplattingCUDACfg("splatting_cuda", [0.0, 0.0, 0.0], True)).to(dev)
    sc = make_scene(n_ctx=2, grid_hw=(8, 8), n_views=4, image_hw=(H, H), seed=1234)
    ex = lambda t: t.to(dev)[None].expand(b, *t.shape).contiguous()
    batch = dict(context=dict(image=ctx["image"], intrinsics=sc.intrinsics[:1].to(dev).expand(b, 2, 3, 3).contiguous()),
                 target=dict(image=torch.rand(b, 4, 3, H, H, device=dev, generator=g), extrinsics=ex(sc.extrinsics), intrinsics=ex(sc.intrinsics),
                             near=ex(sc.near), far=ex(sc.far)))
    recentre_output_heads_(enc, batch["context"], dict(image=batch["context"]["image"][:, 0]))
    step = TrainStep(enc, dec, warm_up_steps=2000)
    sync = lambda: torch.cuda.synchronize(dev)
    step(batch)
    plain = dist_utils.timed_steps(lambda: step(batch), args.steps, sync, None, dev)
    step.distiller, step.distiller_loss = teacher, Regr3D(norm_mode=None)                   # same step object: same encoder, optimizer state, batch
    step(batch)
    with_d = dist_utils.timed_steps(lambda: step(batch), args.steps, sync, None, dev)
    step.distiller = None
    plain2 = dist_utils.timed_steps(lambda: step(batch), args.steps, sync, None, dev)
    res["c3_step"] = {"ms_per_step": round(1e3 * plain / args.steps, 2), "again_ms_per_step": round(1e3 * plain2 / args.steps, 2),
                      "with_distiller_ms_per_step": round(1e3 * with_d / args.steps, 2), "peak_mem_GB": round(torch.cuda.max_memory_allocated(dev) / 2**30, 1)}
print(json.dumps(res))
