#!/usr/bin/env python
"""The depth-smoothness loss at the C3 shape (b = 10 scenes x 4 target views of 256 x 256): forward + backward on the HIP kernels
(losses.depth_smoothness: gsr_depth_smooth_fwd / _bwd) against the torch restatement (losses.depth_smoothness_expression) on the same device,
in the four configurations of (sigma_image None / 10, first / second derivative).  Per configuration: the median and the spread of `--reps`
windows of `--calls` back-to-back forward + backward calls each (device events around a window, the two routes alternating), the launches
one forward + backward makes on each route (torch.profiler's device events), and the largest gradient difference between the routes.
One JSON line.
  python tools/bench_depth_loss.py [--scenes 10] [--views 4] [--size 256] [--reps 7] [--calls 300] [--warmup 20]
"""
import argparse, json, sys
from pathlib import Path
sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import torch
from styl3r_amd import losses

ap = argparse.ArgumentParser()
ap.add_argument("--scenes", type=int, default=10); ap.add_argument("--views", type=int, default=4); ap.add_argument("--size", type=int, default=256)
ap.add_argument("--reps", type=int, default=7); ap.add_argument("--calls", type=int, default=300); ap.add_argument("--warmup", type=int, default=20)
args = ap.parse_args()
assert torch.cuda.is_available(), "bench_depth_loss needs the MI355X"
dev = torch.device("cuda:0")
b, v, H = args.scenes, args.views, args.size
g = torch.Generator(dev).manual_seed(7)
near = 0.5 + torch.rand(b, v, device=dev, generator=g)
far = 50.0 + 50.0 * torch.rand(b, v, device=dev, generator=g)
lo, hi = near.log()[..., None, None], far.log()[..., None, None]
# a smooth surface plus noise, from a little below the near bound to a little beyond the far one; a tenth of the pixels uncovered (depth 0)
yy, xx = torch.meshgrid(torch.linspace(0, 1, H, device=dev), torch.linspace(0, 1, H, device=dev), indexing="ij")
depth = lo - 0.1 + (hi - lo + 0.2) * (0.5 + 0.45 * torch.sin(6 * xx + 3 * yy)) + 0.02 * torch.randn(b, v, H, H, device=dev, generator=g)
depth = torch.where(torch.rand(b, v, H, H, device=dev, generator=g) < 0.1, torch.zeros((), device=dev), depth).requires_grad_(True)
image = torch.rand(b, v, 3, H, H, device=dev, generator=g)


def window(fn, calls):
    a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    e.record()
    torch.cuda.synchronize(dev)
    return a.elapsed_time(e) / calls


def launches(fn):
    """device events (kernels, copies, fills) of one call"""
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize(dev)
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn(); torch.cuda.synchronize(dev)
    return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA)


stats = lambda ts: {"median_ms": round(sorted(ts)[len(ts) // 2], 4), "min_ms": round(min(ts), 4), "max_ms": round(max(ts), 4)}
res = {"metric": "depth-smoothness loss forward + backward, HIP kernels vs the torch expression on the same device", "scenes": b, "views": v, "size": H,
       "reps": args.reps, "calls_per_window": args.calls, "bytes_depth_MB": round(depth.numel() * 4 / 1e6, 1), "bytes_image_MB": round(image.numel() * 4 / 1e6, 1)}
for tag, (sigma, second) in {"plain": (None, False), "second": (None, True), "bilateral": (10.0, False), "bilateral_second": (10.0, True)}.items():
    def hip():
        depth.grad = None
        losses.depth_smoothness(depth, near, far, image, 0.25, sigma, second).backward()

    def expr():
        depth.grad = None
        losses.depth_smoothness_expression(depth, near, far, image, 0.25, sigma, second).backward()

    n0 = losses.CALLS["depth_hip_bwd"]
    hip(); g_hip = depth.grad.clone(); expr(); g_exp = depth.grad.clone()
    assert losses.CALLS["depth_hip_bwd"] == n0 + 1, "depth_smoothness did not take the HIP route"
    for _ in range(args.warmup):
        hip(); expr()
    t_hip, t_exp = [], []
    for _ in range(args.reps):
        t_hip.append(window(hip, args.calls)); t_exp.append(window(expr, args.calls))
    res[tag] = {"hip": stats(t_hip), "expression": stats(t_exp), "speedup_of_medians": round(stats(t_exp)["median_ms"] / stats(t_hip)["median_ms"], 2),
                "hip_launches": launches(hip), "expression_launches": launches(expr),
                # (unlike the tests' inputs these are not sign-safe: where a difference is within rounding of 0 the two routes may pick another sign)
                "grad_max_diff_over_max": float((g_hip - g_exp).abs().max() / g_exp.abs().max()),
                "grad_share_differing_1e-3": float(((g_hip - g_exp).abs() > 1e-3 * g_exp.abs().max()).float().mean())}
print(json.dumps(res))
