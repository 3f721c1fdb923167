#!/usr/bin/env python
"""View selection at the reference's settings (config/generate_evaluation_index.yaml: min_distance 45, max_distance 135, 3 targets,
min_overlap 0.6, max_overlap 1.0, seed 123) on a synthetic 200-frame scene, at 256 x 256 and at 360 x 640:
  (a) the overlap of ALL candidate partners of one context frame (both directions, P pairs) in one `gsr_view_overlap` call: hipEvent
      time on device-resident cameras and pairs (two launches, the Python wrapper's allocations included);
  (b) the same pairs through the package's batched float64 torch restatement (`views.overlap_counts_torch`) on the same device
      (hipEvent time) and on the host (wall clock), with the three count tables compared as integers;
  (c) `EvaluationIndexGenerator.add_scene`, wall clock from host cameras to the entry: device cameras through the kernel, device
      cameras through the torch restatement, host cameras through the torch restatement; the three entries compared;
  (d) rays per second of (a) and (b): 2 P H W rays over the measured time.
Timing: every shape is warmed; medians over --reps.  One JSON line; --out writes it to a file as well.
  python tools/bench_views.py [--reps 10] [--calls 20] [--out profiles/r19_bench_views.json]
"""
import argparse, json, sys, time
from pathlib import Path
sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import numpy as np
import torch
from styl3r_amd import views as vw

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=10); ap.add_argument("--calls", type=int, default=20); ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--frames", type=int, default=200);
ap.add_argument("--shapes", default="256x256,360x640"); ap.add_argument("--out", default=None)
args = ap.parse_args()
assert torch.cuda.is_available(), "bench_views needs the MI355X"
dev = torch.device("cuda:0")
CFG = dict(num_target_views=3, min_distance=45, max_distance=135, min_overlap=0.6, max_overlap=1.0, output_path=Path("unused"),
           save_previews=False, seed=123)


def median(ts):
    return sorted(ts)[len(ts) // 2]


def scene(n):
    """a slow pan: yaw 0.2 degrees and 1.5 cm sideways per frame, so that the walk accepts partners far beyond min_distance"""
    E = np.tile(np.eye(4), (n, 1, 1))
    rng = np.random.default_rng(19)
    for v in range(n):
        a, b = 0.0035 * v + rng.normal() * 1e-3, 0.0008 * v + rng.normal() * 1e-3
        ry = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
        rx = np.array([[1, 0, 0], [0, np.cos(b), -np.sin(b)], [0, np.sin(b), np.cos(b)]])
        E[v, :3, :3] = ry @ rx
        E[v, :3, 3] = np.array([0.015, 0.001, 0.003]) * v + rng.normal(size=3) * 2e-3
    K = np.tile(np.eye(3), (n, 1, 1))
    K[:, 0, 0], K[:, 1, 1], K[:, 0, 2], K[:, 1, 2] = 0.86, 1.53, 0.5, 0.5
    return torch.from_numpy(E.astype(np.float32)), torch.from_numpy(K.astype(np.float32))


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


def add_scene(E, K, shape, through_torch=False):
    gen = vw.EvaluationIndexGenerator(vw.EvaluationIndexGeneratorCfg(**CFG))
    keep = vw.view_overlap_device
    if through_torch:
        vw.view_overlap_device = lambda e, k, p, s: vw.overlap_counts_torch(e, k, p, s)
    try:
        return gen.add_scene("bench", E, K, shape)
    finally:
        vw.view_overlap_device = keep


E, K = scene(args.frames)
Ed, Kd = E.to(dev), K.to(dev)
gen = vw.EvaluationIndexGenerator(vw.EvaluationIndexGeneratorCfg(**CFG))
context = args.frames // 2
walks = gen.candidates(context, args.frames)
pairs = torch.tensor([(context, f) for f in walks[0] + walks[1]], dtype=torch.int32)
pairs_d = pairs.to(dev)
result = {"bench": "views", "frames": args.frames, "cfg": {k: v for k, v in CFG.items() if k != "output_path"}, "context": context,
          "pairs": int(pairs.shape[0]), "shapes": {}}
for name in args.shapes.split(","):
    H, W = (int(s) for s in name.split("x"))
    r = {}
    kernel = vw.view_overlap_device(Ed, Kd, pairs_d, (H, W)).cpu()
    on_device = vw.overlap_counts_torch(Ed, Kd, pairs, (H, W)).cpu()
    r["kernel_ms"] = device_ms(lambda: vw.view_overlap_device(Ed, Kd, pairs_d, (H, W)), args.calls)
    r["torch_device_ms"] = device_ms(lambda: vw.overlap_counts_torch(Ed, Kd, pairs_d, (H, W)), 2)
    t0 = time.perf_counter()
    on_host = vw.overlap_counts_torch(E, K, pairs, (H, W))
    r["torch_host_ms"] = 1e3 * (time.perf_counter() - t0)
    r["counts_equal"] = {"kernel_vs_torch_device": bool(torch.equal(kernel, on_device)), "kernel_vs_torch_host": bool(torch.equal(kernel, on_host))}
    r["rays"] = int(2 * pairs.shape[0] * H * W)
    r["overlap_min_max"] = [float(kernel.min()) / (H * W), float(kernel.max()) / (H * W)]
    r["grays_per_s"] = {k: r["rays"] / (r[k + "_ms"] * 1e-3) / 1e9 for k in ("kernel", "torch_device", "torch_host")}
    entries = [add_scene(Ed, Kd, (H, W)), add_scene(Ed, Kd, (H, W), True)]
    t0 = time.perf_counter()
    entries.append(add_scene(E, K, (H, W)))
    r["add_scene_torch_host_ms"] = 1e3 * (time.perf_counter() - t0)          # one run: seconds on the host
    r["entry"] = None if entries[0] is None else {"context": list(entries[0].context), "target": list(entries[0].target)}
    r["entries_equal"] = bool(entries[0] == entries[1] == entries[2])
    r["add_scene_kernel_ms"] = wall_ms(lambda: add_scene(E.to(dev), K.to(dev), (H, W)), args.reps, args.warmup)
    r["add_scene_torch_device_ms"] = wall_ms(lambda: add_scene(E.to(dev), K.to(dev), (H, W), True), max(2, args.reps // 3), 1)
    result["shapes"][name] = r
line = json.dumps(result)
print(line)
if args.out:
    Path(args.out).write_text(line + "\n")
