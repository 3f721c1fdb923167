#!/usr/bin/env python
"""JPEG frames at the shape the package is used at: the C3 training load of one rank and step, 10 scenes x (2 context + 4 target) = 60
frames of 360 x 640, 4:2:0, quality 90, synthesised from a seed (low-frequency waves, edges, grain) and encoded by Pillow.
  (a) the reference's formulation on THIS host: `Image.open(BytesIO(...)).convert("RGB")` per frame, one core;
  (b) `gsr_jpeg_entropy` alone (the C call into a pinned buffer that already exists) at 1 and at 8 threads;
  (c) the upload of the used coefficient prefix and the descriptors, pinned -> device, wall clock to a synchronise;
  (d) `gsr_jpeg_pixels`: hipEvent time around `calls` back-to-back calls on coefficients that already live on the device, and the bytes
      its two launches must read and write over that time against the HBM peak;
  (e) `decode_jpeg` end to end: bytes in host memory -> synchronised uint8 frames on the device.  (e) against (a) is the comparison;
  (f) one batch of 10 scenes from a `.torch` chunk on disk (50 frames per scene) through ChunkDataset + iter_batches(prefetch=0), chunk
      read included, next to tools/bench_inputs.py's leg (f) measured here on the same scenes: 10 x `prepare_example` on frames that
      are ALREADY decoded + `collate`.
Every leg is warmed; each figure is the median over `reps` with the smallest and the largest next to it.  The decoded frames are
compared with Pillow's byte for byte before anything is timed.  One JSON line; --out writes it to a file as well.
  python tools/bench_jpeg.py [--reps 15] [--calls 20] [--out profiles/bench_jpeg.json]
"""
import argparse, ctypes as C, json, sys, tempfile, time
from io import BytesIO
from pathlib import Path
sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import numpy as np
import torch
from PIL import Image
from styl3r_amd import _lib, dataset as ds, inputs as si, views

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=15); ap.add_argument("--calls", type=int, default=20); ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--out", default=None)
args = ap.parse_args()
assert torch.cuda.is_available(), "bench_jpeg needs the MI355X"
dev = torch.device("cuda:0")
HBM_PEAK = 8.0e12          # bytes / s (spec)
N, H, W = 60, 360, 640
lib = _lib.load()


def spread(ts):
    ts = sorted(ts)
    return {"median_ms": round(ts[len(ts) // 2], 4), "min_ms": round(ts[0], 4), "max_ms": round(ts[-1], 4)}


def wall(fn, sync=True, reps=None):
    for _ in range(args.warmup):
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
    return spread(ts)


def synth(rng, t):
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    img = np.zeros((H, W, 3))
    for c in range(3):
        for _ in range(5):
            fx, fy = rng.uniform(0.005, 0.2, 2)
            img[..., c] += rng.uniform(15, 50) * np.sin(fx * x + fy * y + rng.uniform(0, 6.28) + 0.1 * t)
        img[..., c] += 128 + 40 * ((x // 37 + y // 29 + t) % 2) + rng.normal(0, 5, (H, W))
    return np.clip(img, 0, 255).astype(np.uint8)


rng = np.random.default_rng(23)
blobs = []
for t in range(N):
    buf = BytesIO()
    Image.fromarray(synth(rng, t)).save(buf, "JPEG", quality=90, subsampling=2)
    blobs.append(buf.getvalue())
res = {"metric": "JPEG frames: host entropy stage + HIP IDCT / upsampling / colour", "device": torch.cuda.get_device_name(0), "frames": N,
       "shape": [H, W], "sampling": "4:2:0", "quality": 90, "stream_bytes": int(sum(map(len, blobs))), "reps": args.reps,
       "calls_per_event_pair": args.calls}

pil_loop = lambda: np.stack([np.asarray(Image.open(BytesIO(b)).convert("RGB")) for b in blobs])
want = pil_loop()
got = ds.decode_jpeg(blobs, device=dev)
res["bit_equal_to_pillow"] = bool(np.array_equal(got.cpu().numpy(), want))
res["fallback_images"] = ds.CALLS["jpeg_fallback"]
assert res["bit_equal_to_pillow"] and res["fallback_images"] == 0

# (a)
res["a_pillow_loop"] = wall(pil_loop, sync=False, reps=max(5, args.reps // 3))
res["a_pillow_per_frame_ms"] = round(res["a_pillow_loop"]["median_ms"] / N, 4)

# (b)
coefs = torch.empty(lib.gsr_jpeg_coef_bytes(N, H, W) // 2, dtype=torch.int16, pin_memory=True)
desc = (_lib.GsrJpegDesc * N)()
status = np.zeros(N, np.int32)
ptrs = (C.c_void_p * N)(*[C.cast(C.c_char_p(b), C.c_void_p) for b in blobs])
lens = (C.c_size_t * N)(*[len(b) for b in blobs])
for threads in (1, 8):
    call = lambda: lib.gsr_jpeg_entropy(ptrs, lens, N, H, W, coefs.data_ptr(), C.addressof(desc), status.ctypes.data, threads)
    res[f"b_entropy_{threads}_threads"] = wall(call, sync=False)
    assert not status.any()
res["b_entropy_per_frame_1_thread_ms"] = round(res["b_entropy_1_threads"]["median_ms"] / N, 4)
used = max(int(d.coef_offset + d.coef_count) for d in desc)
res["coefficient_bytes_used"] = 2 * used
res["coefficient_bytes_of_the_size_query"] = 2 * coefs.numel()

# (c)
desc_host = torch.frombuffer(desc, dtype=torch.uint8).pin_memory()
upload = lambda: (coefs[:used].to(dev, non_blocking=True), desc_host.to(dev, non_blocking=True))
res["c_upload"] = wall(upload)
res["c_upload_GBps"] = round((2 * used + desc_host.numel()) / (res["c_upload"]["median_ms"] * 1e-3) / 1e9, 2)

# (d)
coefs_dev, desc_dev = upload()
nbytes = lib.gsr_jpeg_scratch_bytes(N, H, W)
scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
out = torch.empty((N, H, W, 3), dtype=torch.uint8, device=dev)
stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
pixels = lambda: _lib.check(lib.gsr_jpeg_pixels(coefs_dev.data_ptr(), desc_dev.data_ptr(), N, H, W, scratch.data_ptr(), nbytes, out.data_ptr(), stream), "gsr_jpeg_pixels")
for _ in range(args.warmup):
    pixels()
ts = []
for _ in range(args.reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(dev)
    a.record()
    for _ in range(args.calls):
        pixels()
    b.record()
    b.synchronize()
    ts.append(a.elapsed_time(b) / args.calls)
res["d_pixels_device"] = spread(ts)
assert np.array_equal(out.cpu().numpy(), want)
must = 2 * used + used + used + N * H * W * 3          # coefficients in, planes out, planes in, pixels out
sec = res["d_pixels_device"]["median_ms"] * 1e-3
res["d_bytes_moved"] = int(must)
res["d_GBps"] = round(must / sec / 1e9, 1)
res["d_share_of_hbm_peak"] = round(must / HBM_PEAK / sec, 4)
res["d_note"] = "hipEvent time per call of two launches, launch overhead included; the byte planes (one third of the bytes) stay in L2 / Infinity Cache"

# (e)
res["e_decode_jpeg_end_to_end"] = wall(lambda: ds.decode_jpeg(blobs, device=dev))
res["e_over_a"] = round(res["e_decode_jpeg_end_to_end"]["median_ms"] / res["a_pillow_loop"]["median_ms"], 4)

# (f)
n_scene, n_scenes = 50, 10
E = torch.eye(4).repeat(n_scene, 1, 1)
E[:, 0, 3] = torch.arange(n_scene) * 0.05
E[:, 2, 3] = torch.arange(n_scene) * 0.01
w2c = torch.linalg.inv(E)
cams = torch.cat([torch.tensor([[0.9, 1.6, 0.5, 0.5, 0.0, 0.0]]).expand(n_scene, -1), w2c[:, :3].reshape(n_scene, 12)], 1).contiguous()
with tempfile.TemporaryDirectory() as tmp:
    tmp = Path(tmp)
    (tmp / "data" / "train").mkdir(parents=True)
    (tmp / "style" / "train").mkdir(parents=True)
    chunk = [{"key": f"s{i}", "cameras": cams, "images": [torch.from_numpy(np.frombuffer(blobs[(i * 7 + k) % N], np.uint8).copy()) for k in range(n_scene)]}
             for i in range(n_scenes)]
    torch.save(chunk, tmp / "data" / "train" / "000000.torch")
    (tmp / "data" / "train" / "index.json").write_text(json.dumps({f"s{i}": "000000.torch" for i in range(n_scenes)}))
    Image.fromarray(synth(rng, 0)[:, :512]).save(tmp / "style" / "train" / "style.png")
    (tmp / "style" / "train" / "scene_style_mapping_all.json").write_text(json.dumps({f"s{i}": "style.png" for i in range(n_scenes)}))
    cfg = ds.DatasetRE10kStyleCfg(name="bench", roots=[tmp / "data"], baseline_min=1e-3, baseline_max=1e10, max_fov=100.0, make_baseline_1=True,
                                  augment=True, relative_pose=True, skip_bad_shape=True, style_root=tmp / "style")
    sampler = views.ViewSamplerBounded(views.ViewSamplerBoundedCfg("bounded", 2, 4, 20, 45, 0, 0, 20, 45), "train", False, False, None)
    dataset = ds.ChunkDataset(cfg, "train", sampler, device=dev)

    def one_batch():
        batch = next(iter(ds.iter_batches(dataset, n_scenes, prefetch=0)))
        assert batch["target"]["image"].shape == (n_scenes, 4, 3, 256, 256)
    torch.manual_seed(0)
    res["f_chunk_dataset_batch_of_10"] = wall(one_batch, reps=max(5, args.reps // 3))
    res["f_chunk_read_alone"] = wall(lambda: ds.read_chunk(tmp / "data" / "train" / "000000.torch"), sync=False, reps=5)
    style = dataset.read_style_image("s0")
frames = torch.from_numpy(want[:n_scene])
Kn = torch.eye(3).repeat(n_scene, 1, 1)
Kn[:, 0, 0], Kn[:, 1, 1], Kn[:, 0, 2], Kn[:, 1, 2] = 0.9, 1.6, 0.5, 0.5
icfg = si.InputCfg()
draws = torch.Generator().manual_seed(3)
decoded = lambda: si.collate([si.prepare_example(frames, Kn, E, [5, 45], [10, 20, 30, 40], style, icfg, stage="train", scene=str(i), device=dev,
                                                 generator=draws) for i in range(n_scenes)])
res["f_bench_inputs_leg_f_frames_already_decoded"] = wall(decoded)
line = json.dumps(res)
print(line)
if args.out:
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(line + "\n")
