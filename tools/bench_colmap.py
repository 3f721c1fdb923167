#!/usr/bin/env python
"""COLMAP scene inputs at a size a user brings: 10 frames of 1080 x 1920 from one OPENCV camera (k1, k2, p1, p2 = -0.12, 0.03, 0.002, -0.001).
  (a) `gsr_undistort` alone: hipEvent pairs around `calls` back-to-back launches into buffers allocated once (camera table and frames
      already on the device) -- the kernel and its launch;
  (b) `colmap.undistort_frames` on device frames (table upload and output allocation of the Python wrapper included), and from host
      frames, pageable and pinned: wall clock around upload + call + synchronise;
  (c) the numpy host path of the same arithmetic on THIS box, and whether its bytes equal the device's;
  (d) bytes the kernel must move -- every source byte once, every output byte once -- over (a), against the HBM peak;
  (e) `inference.prepare_colmap_scene` end to end from frames held in host memory: view selection, upload, undistortion, cameras,
      Lanczos rescale + crop to 256 x 256, synchronised;
  (f) OpenCV's remap on this host for the same maps, only where `import cv2` works; otherwise "not measured".
Every shape is warmed.  One JSON line; --out writes it to a file as well.
  python tools/bench_colmap.py [--reps 20] [--calls 20] [--out profiles/r21_bench_colmap.json]
"""
import argparse, ctypes as C, json, sys, time
from pathlib import Path
sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import numpy as np
import torch
from styl3r_amd import _lib, colmap, inference

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=20); ap.add_argument("--calls", type=int, default=20); ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--frames", type=int, default=10); ap.add_argument("--out", default=None)
ap.add_argument("--no-host-path", action="store_true", help="skip (c), the numpy host path (about a second per frame)")
args = ap.parse_args()
assert torch.cuda.is_available(), "bench_colmap needs the MI355X"
dev = torch.device("cuda:0")
HBM_PEAK = 8.0e12          # bytes / s (spec)
N, H, W = args.frames, 1080, 1920
K = np.array([[1400.0, 0, W / 2 - 0.3], [0, 1410.0, H / 2 + 0.4], [0, 0, 1]])
DIST = np.float32([-0.12, 0.03, 0.002, -0.001]).astype(np.float64)


def median(ts):
    return sorted(ts)[len(ts) // 2]


def device_ms(fn):
    for _ in range(args.warmup):
        fn()
    ts = []
    for _ in range(args.reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize(dev)
        a.record()
        for _ in range(args.calls):
            fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) / args.calls)
    return median(ts), min(ts), max(ts)


def wall_ms(fn, reps=None, sync=True):
    for _ in range(args.warmup if sync else 1):
        fn()
    ts = []
    for _ in range(reps or args.reps):
        if sync:
            torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        fn()
        if sync:
            torch.cuda.synchronize(dev)
        ts.append(1e3 * (time.perf_counter() - t0))
    return median(ts)


frames_host = torch.randint(0, 256, (N, H, W, 3), generator=torch.Generator().manual_seed(21), dtype=torch.uint8)
frames_pinned = frames_host.pin_memory()
frames_dev = frames_host.to(dev)
new_K, roi = colmap.optimal_new_camera(K, DIST, (W, H))
cam = colmap.UndistortCamera(K, DIST, (W, H), new_K, roi)
fc = [0] * N
table, index, (roi_w, roi_h), _ = colmap.undistort_table((H, W), cam, fc)
res = {"metric": "COLMAP scene inputs: lens undistortion + scene hand-over", "device": torch.cuda.get_device_name(0), "frames": N, "frame_hw": [H, W],
       "roi_xywh": list(roi), "new_K_fx_fy_cx_cy": [float(new_K[0, 0]), float(new_K[1, 1]), float(new_K[0, 2]), float(new_K[1, 2])],
       "reps": args.reps, "calls_per_event_pair": args.calls}

# (a) the kernel
lib = _lib.load()
table_dev = torch.from_numpy(table).to(dev)
out_dev = torch.empty((N, roi_h, roi_w, 3), dtype=torch.uint8, device=dev)
stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def launch():
    _lib.check(lib.gsr_undistort(frames_dev.data_ptr(), N, H, W, table_dev.data_ptr(), 1, index.ctypes.data, roi_w, roi_h, out_dev.data_ptr(), stream),
               "gsr_undistort")


med, lo, hi = device_ms(launch)
res["kernel_events_ms"] = {"median": round(med, 4), "min": round(lo, 4), "max": round(hi, 4)}
must = N * (H * W * 3 + roi_h * roi_w * 3)
res["roofline"] = {"bytes_that_must_move": int(must), "GBps_over_kernel_events": round(must / (med * 1e-3) / 1e9, 1),
                   "least_time_at_hbm_peak_ms": round(must / HBM_PEAK * 1e3, 5), "share_of_hbm_peak": round(must / HBM_PEAK / (med * 1e-3), 4),
                   "megapixels_per_ms": round(N * roi_h * roi_w / 1e6 / med, 2),
                   "note": "fp64 map evaluation per pixel (one IEEE division, a second one per row) and 12 byte gathers next to 6 bytes per pixel: the time is event time per launch, not a profiler's kernel time"}

# (b) the wrapper
med, lo, hi = device_ms(lambda: colmap.undistort_frames(frames_dev, cam, fc))
res["undistort_frames_device_ms"] = {"median": round(med, 4), "min": round(lo, 4), "max": round(hi, 4)}
res["undistort_frames_from_host_pageable_ms"] = round(wall_ms(lambda: colmap.undistort_frames(frames_host.to(dev), cam, fc)), 3)
res["undistort_frames_from_host_pinned_ms"] = round(wall_ms(lambda: colmap.undistort_frames(frames_pinned.to(dev, non_blocking=True), cam, fc)), 3)
res["h2d_bytes"] = int(frames_host.numel())

# (c) the numpy host path on this box
held = {}
if args.no_host_path:
    res["numpy_host_path_ms"] = "not measured (--no-host-path)"
else:
    res["numpy_host_path_ms"] = round(wall_ms(lambda: held.update(out=colmap.undistort_frames(frames_host, cam, fc)), reps=2, sync=False), 1)
    res["device_bytes_equal_host_bytes"] = bool(torch.equal(colmap.undistort_frames(frames_dev, cam, fc).cpu(), held["out"]))

# (e) the public entry point
c2w = np.tile(np.eye(4), (N, 1, 1))
c2w[:, 0, 3] = np.linspace(-1, 1, N)
scene = colmap.ColmapScene([f"{i:04d}.jpg" for i in range(N)], [f"{i:04d}.jpg" for i in range(N)], c2w, [1] * N, {1: new_K}, {1: DIST}, {1: (W, H)},
                           {1: roi}, np.eye(4)[:3], 1.0, {1: K}, "bench")
style = torch.randint(0, 256, (512, 512, 3), generator=torch.Generator().manual_seed(3), dtype=torch.uint8)
call = lambda: inference.prepare_colmap_scene(scene, [0, N - 1], 2, [style], frames=frames_host, device=dev)
ctx, _, tgt = call()
assert ctx["image"].shape == (1, 2, 3, 256, 256) and tgt["image"].shape == (1, N - 2, 3, 256, 256)
res["prepare_colmap_scene_from_host_frames_ms"] = round(wall_ms(call), 3)
res["prepare_colmap_scene_from_device_frames_ms"] = round(wall_ms(lambda: inference.prepare_colmap_scene(scene, [0, N - 1], 2, [style], frames=frames_dev)), 3)

# (f) OpenCV on this host, where there is one
try:
    import cv2
except ImportError:
    cv2 = None
if cv2 is None:
    res["opencv_on_this_host"] = "not measured (cv2 does not import here)"
else:
    mapx, mapy = cv2.initUndistortRectifyMap(K, DIST, None, new_K, (W, H), cv2.CV_32FC1)
    x, y, w, h = roi
    remap_all = lambda: [cv2.remap(f, mapx, mapy, cv2.INTER_LINEAR)[y:y + h, x:x + w] for f in frames_host.numpy()]
    res["opencv_on_this_host"] = {"remap_ms": round(wall_ms(remap_all, reps=5, sync=False), 2), "version": cv2.__version__,
                                  "note": "timing only; tools/compare_undistort_cv2.py reports the differences"}
line = json.dumps(res)
print(line)
if args.out:
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(line + "\n")
