#!/usr/bin/env python
"""Validation visuals at the reference's settings (validation_step: 256 x 256 pictures) on the MI355X:
  (a) `render_cameras` for 2 context + 3 target cameras with near / far planes -- three projections of four layers, 100 lines each: wall
      clock from device cameras to the picture (host float64 geometry, two table uploads, ONE `gsr_draw_layers` launch);
  (b) the drawing alone on prebuilt layers: `draw_layers` (kernel; the wrapper's table uploads included) against
      `draw_layers_reference`, the float64 torch restatement of the reference's drawing, ON THE SAME DEVICE -- hipEvent medians; the two
      pictures compared;
  (c) the same restatement on the host (one run, wall clock), the time the reference's own fp32 drawing is of the order of;
  (d) `render_projections` of --gaussians Gaussians (three `render_hip_orthographic` calls), hipEvent median.
Timing: everything is warmed; medians over --reps.  One JSON line; --out writes it to a file as well.
  python tools/bench_vis.py [--reps 10] [--calls 20] [--out profiles/r20_bench_vis.json]
"""
import argparse, json, sys, time
from pathlib import Path
sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import numpy as np
import torch
from styl3r_amd import visualization as vis
from styl3r_amd.decoder import Gaussians

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=10); ap.add_argument("--calls", type=int, default=20); ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--resolution", type=int, default=256); ap.add_argument("--gaussians", type=int, default=131072); ap.add_argument("--out", default=None)
args = ap.parse_args()
assert torch.cuda.is_available(), "bench_vis needs the MI355X"
dev = torch.device("cuda:0")


def median(ts):
    return sorted(ts)[len(ts) // 2]


def device_ms(fn, calls):
    for _ in range(args.warmup):
        fn()
    ts = []
    for _ in range(args.reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize(dev)
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) / calls)
    return median(ts)


def wall_ms(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize(dev)
        ts.append(1e3 * (time.perf_counter() - t0))
    return median(ts)


def cameras(n, seed):
    rng = np.random.default_rng(seed)
    E = np.tile(np.eye(4), (n, 1, 1))
    for v in range(n):
        a, b = rng.normal(size=2) * 0.3
        ry = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
        rx = np.array([[1, 0, 0], [0, np.cos(b), -np.sin(b)], [0, np.sin(b), np.cos(b)]])
        E[v, :3, :3] = ry @ rx
        E[v, :3, 3] = rng.normal(size=3) * 0.4 + [0.3 * v, 0, 0]
    K = np.tile(np.eye(3), (n, 1, 1))
    K[:, 0, 0], K[:, 1, 1], K[:, 0, 2], K[:, 1, 2] = 0.86, 1.53, 0.5, 0.5
    f = lambda x: torch.from_numpy(np.asarray(x, np.float32)).to(dev)
    return f(E), f(K), f(rng.uniform(0.5, 0.8, n)), f(rng.uniform(2.0, 3.0, n))


res = args.resolution
E, K, near, far = cameras(5, 20)
batch = {"context": dict(extrinsics=E[None, :2], intrinsics=K[None, :2], near=near[None, :2], far=far[None, :2]),
         "target": dict(extrinsics=E[None, 2:], intrinsics=K[None, 2:], near=near[None, 2:], far=far[None, 2:])}
color = torch.ones((5, 3)); color[2:, 1:] = 0
stacks = vis.camera_layers(res, E, K, color, near, far)
black = torch.zeros((3, 3, res, res), device=dev)
kernel = vis.draw_layers(black, stacks)
restated = vis.draw_layers_reference(black, stacks)
result = {"bench": "vis", "resolution": res, "cameras": [2, 3], "layers_per_image": [len(s) for s in stacks],
          "primitives": int(sum(len(l.records) for s in stacks for l in s)),
          "edge_pixels": int(sum(int(((a > 0) & (a < 1)).sum()) for s in stacks for a in [vis.render_overlay((res, res), l, dev)[3] for l in s])),
          "max_abs_kernel_vs_restatement": float((kernel.double() - restated.double()).abs().max()),
          "pictures_equal": bool(torch.equal(kernel, restated))}
result["render_cameras_wall_ms"] = wall_ms(lambda: vis.render_cameras(batch, res), args.reps, args.warmup)
result["draw_layers_kernel_ms"] = device_ms(lambda: vis.draw_layers(black, stacks), args.calls)
result["draw_layers_restatement_device_ms"] = device_ms(lambda: vis.draw_layers_reference(black, stacks), 1)
t0 = time.perf_counter()
on_host = vis.draw_layers_reference(black.cpu(), stacks)
result["draw_layers_restatement_host_ms"] = 1e3 * (time.perf_counter() - t0)                      # one run: seconds on the host
result["kernel_equals_host_restatement"] = bool(torch.equal(kernel.cpu(), on_host))

g = torch.Generator().manual_seed(20)
n = args.gaussians
means = torch.randn((1, n, 3), generator=g) * torch.tensor([1.0, 0.5, 1.5]) + torch.tensor([0.2, -0.1, 2.0])
L = torch.randn((1, n, 3, 3), generator=g) * 0.02
cov = L @ L.transpose(-1, -2) + 1e-4 * torch.eye(3)
gs = Gaussians(means.to(dev), cov.to(dev), torch.rand((1, n, 3, 1), generator=g).to(dev), (torch.rand((1, n), generator=g) * 0.8 + 0.1).to(dev))
result["gaussians"] = n
result["render_projections_ms"] = device_ms(lambda: vis.render_projections(gs, res), 2)
line = json.dumps(result)
print(line)
if args.out:
    Path(args.out).write_text(line + "\n")
