#!/usr/bin/env python
"""The two AdaAttN kernels at the train step's own shape (10 scenes x 4 views of 256 x 256 against 10 style images, relu3_1 = 64 x 64:
40 images / 10 styles, Nq = M = 4096, D = 448, C = 256): vit_adaattn_stats (losses.adaattn_stats) and the tail vit_adaattn_l1
(losses.adaattn_l1, forward + backward) against the torch expression on the same device (losses.adaattn_stats_expression in chunks of
`--chunk` images: one image's attention matrix is 64 MiB in fp32; the tail's expression is instance_norm, two elementwise passes, |.| and a
mean).  Per route: the median and the spread of `--reps` windows of `--calls` back-to-back calls (device events around a window, the routes
alternating), and for the stats kernel the achieved FLOP/s from the operation count 2 Bq Nq M (D + 2 C).  One JSON line.
  python tools/bench_adaattn.py [--scenes 10] [--views 4] [--n 4096] [--m 4096] [--d 448] [--c 256] [--reps 5] [--calls 3] [--warmup 2] [--chunk 4]
"""
import argparse, json, sys
from pathlib import Path
sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import torch
import torch.nn.functional as F
from styl3r_amd import losses

ap = argparse.ArgumentParser()
ap.add_argument("--scenes", type=int, default=10); ap.add_argument("--views", type=int, default=4)
ap.add_argument("--n", type=int, default=4096); ap.add_argument("--m", type=int, default=4096)
ap.add_argument("--d", type=int, default=448); ap.add_argument("--c", type=int, default=256)
ap.add_argument("--reps", type=int, default=5); ap.add_argument("--calls", type=int, default=3); ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--chunk", type=int, default=4)
args = ap.parse_args()
assert torch.cuda.is_available(), "bench_adaattn needs the MI355X"
dev = torch.device("cuda:0")
bs, bq, N, M, D, Cc = args.scenes, args.scenes * args.views, args.n, args.m, args.d, args.c
g = torch.Generator(dev).manual_seed(7)
relu_like = lambda *shape: (torch.rand(*shape, device=dev, generator=g) - 0.4).clamp_(min=0) * 3
q_hat, k_hat, s = F.instance_norm(relu_like(bq, D, N)), F.instance_norm(relu_like(bs, D, M)), relu_like(bs, Cc, M)
index = torch.arange(bs, dtype=torch.int32).repeat_interleave(args.views)
p = relu_like(bq, Cc, N).requires_grad_(True)
c = relu_like(bq, Cc, N)


def window(fn, calls):
    a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    e.record()
    torch.cuda.synchronize(dev)
    return a.elapsed_time(e) / calls


def stats_expr():
    outs = [losses.adaattn_stats_expression(q_hat[i:i + args.chunk], k_hat, s, index[i:i + args.chunk]) for i in range(0, bq, args.chunk)]
    return torch.cat([o[0] for o in outs]), torch.cat([o[1] for o in outs])


stats_hip = lambda: losses.adaattn_stats(q_hat, k_hat, s, index)
n0 = losses.CALLS["adaattn_hip_stats"]
mean, std = stats_hip()
assert losses.CALLS["adaattn_hip_stats"] == n0 + 1, "adaattn_stats did not take the HIP route"
mean_e, std_e = stats_expr()


def tail_hip():
    p.grad = None
    losses.adaattn_l1(p, c, mean, std).backward()


def tail_expr():
    p.grad = None
    (p - (F.instance_norm(c) * std + mean)).abs().mean().backward()


n0 = losses.CALLS["adaattn_hip_l1"]
tail_hip(); g_hip = p.grad.clone(); tail_expr(); g_exp = p.grad.clone()
assert losses.CALLS["adaattn_hip_l1"] == n0 + 1, "adaattn_l1 did not take the HIP route"
summary = lambda ts: {"median_ms": round(sorted(ts)[len(ts) // 2], 3), "min_ms": round(min(ts), 3), "max_ms": round(max(ts), 3)}
res = {"metric": "AdaAttN kernels vs the torch expression on the same device", "images": bq, "styles": bs, "Nq": N, "M": M, "D": D, "C": Cc,
       "reps": args.reps, "calls_per_window": args.calls, "expression_chunk_images": args.chunk}
for name, hip, expr, calls in (("stats", stats_hip, stats_expr, args.calls), ("tail_fwd_bwd", tail_hip, tail_expr, 10 * args.calls)):
    for _ in range(args.warmup):
        hip(); expr()
    t_hip, t_exp = [], []
    for _ in range(args.reps):
        t_hip.append(window(hip, calls)); t_exp.append(window(expr, calls))
    res[name] = {"hip": summary(t_hip), "expression": summary(t_exp), "speedup_of_medians": round(summary(t_exp)["median_ms"] / summary(t_hip)["median_ms"], 2)}
flop = 2.0 * bq * N * M * (D + 2 * Cc)
res["stats"]["flop"] = flop
res["stats"]["hip_tflops"] = round(flop / (res["stats"]["hip"]["median_ms"] * 1e-3) / 1e12, 1)
res["stats"]["max_mean_diff"] = float((mean - mean_e).abs().max())
res["stats"]["max_var_diff"] = float((std ** 2 - std_e ** 2).abs().max())
res["tail_fwd_bwd"]["grad_share_differing"] = float((g_hip != g_exp).float().mean())      # (signs within rounding of a tie, and sign(0))
print(json.dumps(res))
