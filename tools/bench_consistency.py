#!/usr/bin/env python
"""Multi-view consistency at the fly-through shape (60 frames of 256 x 256, 5 colour sets, gaps 1 and 7: 112 pairs): the HIP route
(metrics.warp_consistency: gsr_warp_consistency) against the float64 restatement (metrics.warp_consistency_expression) on the same device and
against a plain fp32 `grid_sample` formulation of the same score.  Per route: the median and the spread of `--reps` windows of `--calls`
back-to-back calls (device events around a window, the routes alternating) and the device launches one call makes (torch.profiler).  The
kernel entry is also timed alone through the C ABI on pre-allocated buffers (its two launches, no wrapper work): that time over the bytes
the algorithm asks for -- per pair and pixel: dst depth, the src depth and 3 S src colour planes each touched about once, 3 S dst colours,
one mask byte -- is the achieved rate, next to the HBM time of the same bytes at 6.3 TB/s and of the unique footprint (the frames read once).
One JSON line.
  python tools/bench_consistency.py [--frames 60] [--size 256] [--sets 5] [--reps 7] [--calls 20] [--warmup 3]
"""
import argparse, ctypes as C, json, math, sys
from pathlib import Path
sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import torch
import torch.nn.functional as F
from styl3r_amd import _lib, metrics

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=60); ap.add_argument("--size", type=int, default=256); ap.add_argument("--sets", type=int, default=5)
ap.add_argument("--reps", type=int, default=7); ap.add_argument("--calls", type=int, default=20); ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--tol", type=float, default=0.05)
args = ap.parse_args()
assert torch.cuda.is_available(), "bench_consistency needs the MI355X"
dev = torch.device("cuda:0")
Fr, H, S = args.frames, args.size, args.sets
W = H
HBM = 6.3e12                                   # achievable HBM rate of the MI355X (bytes / s)

# a fly-through: the camera slides 0.6 along x and turns a little while it looks at a smooth surface 2..4 away; the depth of every frame
# is that surface seen from the frame's camera only approximately (a smooth field per frame), so the occlusion test rejects a share of
# the pixels, as it does on rendered depth.  Colours: smooth fields plus noise, per set.
g = torch.Generator(dev).manual_seed(7)
t = torch.linspace(0, 1, Fr, device=dev, dtype=torch.float64)
ang = 0.1 * (t - 0.5)
c2w = torch.eye(4, device=dev, dtype=torch.float64).repeat(Fr, 1, 1)
c2w[:, 0, 0], c2w[:, 0, 2], c2w[:, 2, 0], c2w[:, 2, 2] = ang.cos(), ang.sin(), -ang.sin(), ang.cos()
c2w[:, 0, 3], c2w[:, 1, 3] = 0.6 * t, 0.05 * (3 * t).sin()
K = torch.tensor([[0.9, 0, 0.5], [0, 0.9, 0.5], [0, 0, 1.0]], device=dev, dtype=torch.float64).repeat(Fr, 1, 1)
yy, xx = torch.meshgrid(torch.linspace(0, 1, H, device=dev), torch.linspace(0, 1, W, device=dev), indexing="ij")
depth = (3.0 + 0.02 * torch.sin(5 * xx + 3 * yy)[None] + 0.002 * torch.randn(Fr, H, W, device=dev, generator=g)).float().contiguous()
images = (0.5 + 0.4 * torch.sin(9 * xx + torch.arange(S * Fr * 3, device=dev).reshape(S, Fr, 3, 1, 1) * 0.37) * torch.cos(7 * yy)
          + 0.05 * torch.rand(S, Fr, 3, H, W, device=dev, generator=g)).clamp(0, 1).float().contiguous()
pairs = torch.cat([metrics.consistency_pairs(Fr, metrics.SHORT_RANGE_GAP), metrics.consistency_pairs(Fr, metrics.LONG_RANGE_GAP)]).to(dev)
P = pairs.shape[0]


def hip():
    return metrics.warp_consistency(images, depth, c2w, K, pairs, depth_tol=args.tol)


def expression():
    return metrics.warp_consistency_expression(images, depth, c2w, K, pairs, depth_tol=args.tol)


c2w32, K32 = c2w.float(), K.float()


def grid_sample_fp32():
    """the same score as a user would write it in fp32: matmul geometry, one grid_sample over (src depth, all src colours) per call"""
    src, dst = pairs[:, 0], pairs[:, 1]
    ys, xs = torch.meshgrid((torch.arange(H, device=dev) + 0.5) / H, (torch.arange(W, device=dev) + 0.5) / W, indexing="ij")
    d = depth[dst]                                                               # (P,H,W)
    Kj, Ki = K32[dst], K32[src]
    cam = torch.stack([(xs - Kj[:, 0, 2, None, None]) / Kj[:, 0, 0, None, None] * d, (ys - Kj[:, 1, 2, None, None]) / Kj[:, 1, 1, None, None] * d, d], -1)
    world = cam @ c2w32[dst][:, None, :3, :3].transpose(-1, -2) + c2w32[dst][:, None, None, :3, 3]
    local = (world - c2w32[src][:, None, None, :3, 3]) @ c2w32[src][:, None, :3, :3]
    z = local[..., 2]
    px = (Ki[:, 0, 0, None, None] * local[..., 0] / z + Ki[:, 0, 2, None, None]) * W - 0.5
    py = (Ki[:, 1, 1, None, None] * local[..., 1] / z + Ki[:, 1, 2, None, None]) * H - 0.5
    ok = (d > 0) & torch.isfinite(d) & (z > 0) & (px >= 0) & (px <= W - 1) & (py >= 0) & (py <= H - 1)
    grid = torch.stack([(px + 0.5) / W * 2 - 1, (py + 0.5) / H * 2 - 1], -1)
    stack = torch.cat([depth[src][:, None], images[:, src].permute(1, 0, 2, 3, 4).reshape(P, S * 3, H, W)], 1)
    smp = F.grid_sample(stack, grid, mode="bilinear", padding_mode="border", align_corners=False)
    D = smp[:, 0]
    ok = ok & (D > 0) & ((z - D).abs() <= args.tol * D)
    diff = smp[:, 1:].reshape(P, S, 3, H, W) - images[:, dst].permute(1, 0, 2, 3, 4)
    sse = (diff * diff * ok[:, None, None]).sum(dim=(2, 3, 4)).t()
    count = ok.sum(dim=(1, 2))
    return (sse / (3 * count)).sqrt(), count


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


# the entry alone: pre-allocated buffers, the two launches of gsr_warp_consistency and nothing else
lib = _lib.load()
nbytes = lib.gsr_warp_consistency_scratch_bytes(P, S, H, W)
assert S <= _lib.GSR_CONSISTENCY_MAX_SETS and nbytes, "the entry-alone timing takes one chunk of sets"
scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
mask, count, sse = torch.empty((P, H, W), dtype=torch.uint8, device=dev), torch.empty(P, dtype=torch.int32, device=dev), torch.empty((S, P), dtype=torch.float64, device=dev)
pairs32 = pairs.int().contiguous()
stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def entry():
    _lib.check(lib.gsr_warp_consistency(images.data_ptr(), depth.data_ptr(), c2w.data_ptr(), K.data_ptr(), pairs32.data_ptr(), S, Fr, P, H, W, args.tol,
                                        None, mask.data_ptr(), count.data_ptr(), sse.data_ptr(), scratch.data_ptr(), nbytes, stream), "gsr_warp_consistency")


n0 = metrics.CALLS["consistency_hip"]
r_hip, r_exp, (rmse32, count32) = hip(), expression(), grid_sample_fp32()
assert metrics.CALLS["consistency_hip"] == n0 + 1, "warp_consistency did not take the HIP route"
entry(); torch.cuda.synchronize(dev)
routes = {"hip": hip, "entry_alone": entry, "expression_fp64": expression, "grid_sample_fp32": grid_sample_fp32}
for _ in range(args.warmup):
    for fn in routes.values():
        fn()
times = {k: [] for k in routes}
for _ in range(args.reps):
    for k, fn in routes.items():
        times[k].append(window(fn, args.calls))
stats = lambda ts: {"median_ms": round(sorted(ts)[len(ts) // 2], 4), "min_ms": round(min(ts), 4), "max_ms": round(max(ts), 4)}
asked = P * H * W * (4 + 4 + 3 * S * 4 * 2 + 1) + nbytes                       # bytes the algorithm asks for per call
unique = (S * 3 + 1) * Fr * H * W * 4 + P * H * W + nbytes                       # every frame read once, the mask written once
seen = r_hip.count > 0
med = {k: stats(v)["median_ms"] for k, v in times.items()}
res = {"metric": "multi-view consistency (warp + mask + RMSE), HIP kernel vs the float64 expression vs fp32 grid_sample, same device",
       "frames": Fr, "size": H, "sets": S, "pairs": P, "reps": args.reps, "calls_per_window": args.calls,
       **{k: stats(v) for k, v in times.items()},
       "launches": {k: launches(fn) for k, fn in routes.items()},
       "speedup_vs_expression_fp64": round(med["expression_fp64"] / med["hip"], 2), "speedup_vs_grid_sample_fp32": round(med["grid_sample_fp32"] / med["hip"], 2),
       "bytes_asked_MB": round(asked / 1e6, 1), "bytes_unique_MB": round(unique / 1e6, 1),
       "entry_achieved_TBps_of_asked": round(asked / (med["entry_alone"] * 1e-3) / 1e12, 3),
       "hbm_floor_ms_asked": round(asked / HBM * 1e3, 4), "hbm_floor_ms_unique": round(unique / HBM * 1e3, 4),
       "entry_share_of_hbm_floor_asked": round(asked / HBM * 1e3 / med["entry_alone"], 3),
       "mean_valid": float(r_hip.valid.mean()),
       "mask_mismatches_vs_expression": int((r_hip.mask != r_exp.mask).sum()),   # (these inputs are not kept off the thresholds, unlike the tests')
       "sse_max_rel_diff_vs_expression": float(((r_hip.sse - r_exp.sse).abs() / r_exp.sse.clamp_min(1e-300))[:, seen].max()),
       "rmse_max_abs_diff_grid_sample_fp32": float((r_hip.rmse - rmse32.double()).abs()[:, seen].max()),
       "count_max_abs_diff_grid_sample_fp32": int((r_hip.count - count32).abs().max())}
print(json.dumps(res))
