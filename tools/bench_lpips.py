#!/usr/bin/env python
"""LPIPS-VGG forward + backward at the C3 shape (40 views of 256 x 256) on the HIP route (VGG16 on Conv2dX6 with the ReLUs folded in,
vit_maxpool2x2, the fused tail vit_lpips_fwd / _bwd) and, in the same process, through the plain expression it replaces (the same
Conv2dX6 modules, framework ReLU / max-pool and the torch tail).  Also: the tail kernels alone with their algorithmic bytes and the share
of 8 TB/s, and the VGG16 time split into the library's 64-channel conv1_x layers and the Conv2dX6 layers.  Random He-scaled weights
(no LPIPS weights offline; timing does not depend on them).  One JSON line.
  python tools/bench_lpips.py [--images 40] [--size 256] [--reps 10] [--linear-mode bf16x6]
"""
import argparse, json, sys
from pathlib import Path
sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import torch
from styl3r_amd import vit_ops
from styl3r_amd.losses import LPIPS

ap = argparse.ArgumentParser()
ap.add_argument("--images", type=int, default=40); ap.add_argument("--size", type=int, default=256)
ap.add_argument("--reps", type=int, default=10); ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--linear-mode", choices=["bf16x6", "bf16x3", "f16x3"], default=None)
args = ap.parse_args()
assert torch.cuda.is_available(), "bench_lpips needs the MI355X"
if args.linear_mode:
    vit_ops.LINEAR_MODE = args.linear_mode
dev = torch.device("cuda:0")
torch.manual_seed(0)
m = LPIPS()
with torch.no_grad():
    for mod in m.net.modules():
        if isinstance(mod, torch.nn.Conv2d):
            mod.weight.normal_(0, (2.0 / mod.weight[0].numel()) ** 0.5); mod.bias.normal_(0, 0.01)
    for k in range(5):
        getattr(m, f"lin{k}").model[1].weight.uniform_(0, 1)
m = m.to(dev).eval().requires_grad_(False)
N, S = args.images, args.size
g = torch.Generator(dev).manual_seed(1)
tgt = torch.rand(N, 3, S, S, device=dev, generator=g)
pred = (tgt + 0.1 * torch.randn(tgt.shape, device=dev, generator=g)).clamp(0, 1).requires_grad_(True)


def timed(fn, reps=args.reps, warmup=args.warmup):
    """median ms per call over `reps` calls, each between two device events"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize(dev)
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record()
        torch.cuda.synchronize(dev)
        ts.append(a.elapsed_time(b))
    return sorted(ts)[len(ts) // 2]


def route_new():
    pred.grad = None
    m(pred, tgt, normalize=True).mean().backward()


def route_old():
    pred.grad = None
    m._forward_expression(2 * pred - 1, 2 * tgt - 1).mean().backward()


before = dict(vit_ops.CALLS)
route_new()
assert vit_ops.CALLS["lpips_hip_fwd"] > before["lpips_hip_fwd"], "the HIP route was not taken"
g_new = pred.grad.clone()
route_old()
g_old = pred.grad.clone()
grad_rel = float((g_new - g_old).abs().max() / g_old.abs().max())
torch.cuda.reset_peak_memory_stats(dev)
new_ms = timed(route_new)
peak_new = torch.cuda.max_memory_allocated(dev)
torch.cuda.reset_peak_memory_stats(dev)
old_ms = timed(route_old)
peak_old = torch.cuda.max_memory_allocated(dev)
new_ms2 = timed(route_new)                                   # alternate A/B/A: the spread of the same route

# ---- the tail kernels alone --------------------------------------------------------------------------------------------------------------
with torch.no_grad():
    fb = m.net.preacts((2 * tgt - 1 - m.shift) / m.scale)
    fa = [t.clone() for t in m.net.preacts((2 * pred - 1 - m.shift) / m.scale)]
ws = [getattr(m, f"lin{k}").model[1].weight for k in range(5)]
fa = [t.requires_grad_(True) for t in fa]
chw = sum(t[0].numel() for t in fa)
hw = sum(t.shape[2] * t.shape[3] for t in fa)
fwd_bytes = 2 * 4 * N * chw + 16 * N * hw
bwd_bytes = 3 * 4 * N * chw + 16 * N * hw
d = vit_ops.lpips_tail(fa, fb, ws, relu_in=True)
up = torch.ones(N, device=dev)
tail_fwd_ms = timed(lambda: vit_ops.lpips_tail(fa, fb, ws, relu_in=True))
tail_bwd_ms = timed(lambda: torch.autograd.grad(d, fa, up, retain_graph=True))


def tail_expression():
    tot = 0
    for k, (x, y) in enumerate(zip(fa, fb)):
        x, y = torch.relu(x), torch.relu(y)
        x = x / (x.pow(2).sum(1, keepdim=True).sqrt() + 1e-10)
        y = y / (y.pow(2).sum(1, keepdim=True).sqrt() + 1e-10)
        tot = tot + getattr(m, f"lin{k}")((x - y) ** 2).mean(dim=(2, 3), keepdim=True)
    torch.autograd.grad(tot.sum(), fa)


tail_expr_ms = timed(tail_expression)

# ---- VGG16 per layer: forward + input gradient, library (conv1_x) vs Conv2dX6 ------------------------------------------------------------
layers, x = [], (2 * pred.detach() - 1 - m.shift) / m.scale
first = True
for s in range(1, 6):
    for mod in getattr(m.net, f"slice{s}"):
        if isinstance(mod, torch.nn.MaxPool2d):
            xin = x.detach().requires_grad_(True)
            layers.append(("maxpool", xin, vit_ops.maxpool2x2))
            x = vit_ops.maxpool2x2(x.detach())
        elif isinstance(mod, torch.nn.Conv2d):
            xin = x.detach().requires_grad_(not first)         # (conv1_1's input is the image: no gradient needed past it in the loss)
            fn = mod if first else mod.forward_fused
            kind = "library" if (first or not mod._x6_ok(xin)) else "conv_x6"
            layers.append((kind, xin, fn))
            with torch.no_grad():
                x = fn(xin)
            first = False
split = {"library": 0.0, "conv_x6": 0.0, "maxpool": 0.0}
per_layer = []
for kind, xin, fn in layers:
    def one(xin=xin, fn=fn):
        y = fn(xin)
        if xin.requires_grad:
            torch.autograd.grad(y, xin, torch.ones_like(y))
    t = timed(one, reps=max(3, args.reps // 2), warmup=2)
    split[kind] += t
    per_layer.append({"kind": kind, "shape": list(xin.shape), "ms": round(t, 3)})

print(json.dumps({
    "metric": f"LPIPS-VGG forward+backward, {N} x {S}^2 (pred needs a gradient, target is ground truth)",
    "linear_mode": vit_ops.LINEAR_MODE,
    "hip_route_ms": round(new_ms, 3), "hip_route_ms_repeat": round(new_ms2, 3), "expression_ms": round(old_ms, 3),
    "speedup": round(old_ms / new_ms, 3), "peak_mem_gb_hip": round(peak_new / 1e9, 3), "peak_mem_gb_expression": round(peak_old / 1e9, 3),
    "grad_rel_diff_vs_expression": grad_rel,
    "tail": {"fwd_ms": round(tail_fwd_ms, 4), "bwd_ms": round(tail_bwd_ms, 4), "expression_fwd_bwd_ms": round(tail_expr_ms, 3),
             "fwd_bytes": fwd_bytes, "bwd_bytes": bwd_bytes,
             "fwd_tb_s": round(fwd_bytes / tail_fwd_ms / 1e9, 3), "bwd_tb_s": round(bwd_bytes / tail_bwd_ms / 1e9, 3),
             "fwd_frac_of_8tb_s": round(fwd_bytes / tail_fwd_ms / 1e9 / 8.0, 3), "bwd_frac_of_8tb_s": round(bwd_bytes / tail_bwd_ms / 1e9 / 8.0, 3),
             "timing": "device events around one call (host launch included), median"},
    "vgg16_one_side_fwd_plus_dx_ms": {k: round(v, 3) for k, v in split.items()},
    "vgg16_layers": per_layer,
}))
