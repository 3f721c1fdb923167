#!/usr/bin/env python
"""Scene inputs at the shapes the package is used at:
  (a) the C3 training load of one rank and step: 10 scenes x (2 context + 4 target) = 60 uint8 frames of 360 x 640 -> 256 x 256 in ONE
      gsr_resample_crop call, plus 10 style images of mixed sizes (one call each) -> 256 x 256;
  (b) the C2 serving load: 2 context frames + 1 style image;
  (c) the same work in the reference's formulation on THIS host -- per image: bytes -> PIL resize(LANCZOS) -> / 255 -> fp32, crop, then the
      fp32 planes uploaded -- if PIL imports here; otherwise "not measured".  Where it runs, its pixels are compared bit for bit with (a);
  (d) bytes the two kernels must read and write, from the shapes, over the measured time, against the HBM peak; and the integer
      multiply-adds over the same time -- which of the two bounds the call;
  (e) host-to-device bytes: the uint8 frames against the fp32 planes the package used to be handed;
  (f) the public entry points, wall clock from host tensors to a synchronised device batch: 10 x `prepare_example` (each a scene of 50 decoded
      frames with their cameras, 2 context + 4 target views, one style image, the augmentation draw) + `collate` for C3, one `prepare_scene`
      for C2, and `convert_poses` on the 200 camera rows of a long RE10K scene.  This is what a user of the module waits for: host camera
      arithmetic, frame selection, upload, kernels.
Timing: every shape is warmed; "device" times are hipEvent pairs around `calls` back-to-back calls on frames that already live on the
device (what two launches cost, allocator and launch overhead of the Python wrapper included); "from host" times are wall clock around
upload + call + synchronise.  One JSON line; --out writes it to a file as well.
  python tools/bench_inputs.py [--reps 20] [--calls 50] [--out profiles/r18_bench_inputs.json]
"""
import argparse, json, sys, time
from pathlib import Path
sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import numpy as np
import torch
from styl3r_amd import inputs as si

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=20); ap.add_argument("--calls", type=int, default=50); ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--out", default=None)
args = ap.parse_args()
assert torch.cuda.is_available(), "bench_inputs needs the MI355X"
dev = torch.device("cuda:0")
HBM_PEAK = 8.0e12          # bytes / s (spec)
INT_MAC_PEAK = 256 * 64 * 2.4e9 / 4     # ASSUMED, not measured: 256 CUs x 64 lanes x 2.4 GHz with the 32-bit integer multiply at quarter rate
SHAPE = (256, 256)
STYLE_SIZES = [(512, 512), (600, 800), (768, 1024), (1024, 683), (480, 640), (900, 1200), (1080, 1920), (333, 500), (256, 256), (800, 533)]
gen = torch.Generator().manual_seed(18)


def median(ts):
    return sorted(ts)[len(ts) // 2]


def device_ms(fn):
    """median over reps of (hipEvent time around `calls` back-to-back calls) / calls"""
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
    return median(ts)


def wall_ms(fn, reps=None):
    for _ in range(args.warmup):
        fn()
    ts = []
    for _ in range(reps or args.reps):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize(dev)
        ts.append(1e3 * (time.perf_counter() - t0))
    return median(ts)


def traffic(N, H, W, shape, window, src_bytes_per_sample):
    """bytes and integer multiply-adds of one gsr_resample_crop call, from the plans (what the kernels read, write and compute)"""
    sh, sw = shape
    top, left, oh, ow = window
    kx, bx, _ = si.resample_plan(W, sw) if sw != W else (1, np.stack([np.arange(sw), np.ones(sw, int)], 1), None)
    ky, by, _ = si.resample_plan(H, sh) if sh != H else (1, np.stack([np.arange(sh), np.ones(sh, int)], 1), None)
    rows = by[top + oh - 1].sum() - by[top, 0]
    cols = bx[left + ow - 1].sum() - bx[left, 0]
    pitch = (ow + 3) // 4 * 4
    src = N * rows * cols * 3 * src_bytes_per_sample
    mid = N * 3 * rows * pitch
    out = N * 3 * oh * ow * 4
    macs = N * 3 * (rows * int(bx[left:left + ow, 1].sum()) + ow * int(by[top:top + oh, 1].sum()))
    return {"source_bytes": int(src), "intermediate_bytes_written_and_read": int(2 * mid), "output_bytes": int(out), "int_macs": int(macs),
            "taps": [int(kx), int(ky)], "source_rows_read": int(rows), "source_columns_read": int(cols)}


def crop_args(H, W, shape):
    hs, ws = si.scaled_size(H, W, shape)
    return (hs, ws), ((hs - shape[0]) // 2, (ws - shape[1]) // 2, *shape)


def style_args(H, W, size=256):
    hs, ws = si.style_scaled_size(H, W, size)
    return (hs, ws), (int(round((hs - size) / 2.0)), int(round((ws - size) / 2.0)), size, size)


res = {"metric": "scene inputs: Lanczos rescale + crop + batch assembly", "device": torch.cuda.get_device_name(0), "reps": args.reps,
       "calls_per_event_pair": args.calls}
frames_host = torch.randint(0, 256, (60, 360, 640, 3), generator=gen, dtype=torch.uint8)
styles_host = [torch.randint(0, 256, (h, w, 3), generator=gen, dtype=torch.uint8) for h, w in STYLE_SIZES]
frames_pinned = frames_host.pin_memory()
K = torch.eye(3).repeat(60, 1, 1)

for tag, n_frames, n_styles in (("c3_60_frames_10_styles", 60, 10), ("c2_2_frames_1_style", 2, 1)):
    fh, fp = frames_host[:n_frames], frames_pinned[:n_frames]
    fd = fh.to(dev)
    sd = [s.to(dev) for s in styles_host[:n_styles]]
    frames_call = lambda: si.rescale_and_crop(fd, K[:n_frames], SHAPE)[0]
    styles_call = lambda: [si.apply_style_image_augmentation(s, "train") for s in sd]
    r = {"frames_device_ms": round(device_ms(frames_call), 4), "styles_device_ms": round(device_ms(styles_call), 4)}
    r["frames_from_host_pageable_ms"] = round(wall_ms(lambda: si.rescale_and_crop(fh.to(dev), K[:n_frames], SHAPE)), 4)
    r["frames_from_host_pinned_ms"] = round(wall_ms(lambda: si.rescale_and_crop(fp.to(dev, non_blocking=True), K[:n_frames], SHAPE)), 4)
    r["styles_from_host_ms"] = round(wall_ms(lambda: [si.apply_style_image_augmentation(s.to(dev), "train") for s in styles_host[:n_styles]]), 4)
    # (d) roofline of the frames call
    t = traffic(n_frames, 360, 640, *crop_args(360, 640, SHAPE), 1)
    must = t["source_bytes"] + t["output_bytes"]
    moved = must + t["intermediate_bytes_written_and_read"]
    sec = r["frames_device_ms"] * 1e-3
    t_mem, t_alu = must / HBM_PEAK, t["int_macs"] / INT_MAC_PEAK
    share = max(t_mem, t_alu) / sec
    t.update(bytes_that_must_move=int(must), bytes_moved_with_intermediate=int(moved), must_move_GBps=round(must / sec / 1e9, 1),
             moved_GBps=round(moved / sec / 1e9, 1), least_time_bytes_at_hbm_peak_ms=round(t_mem * 1e3, 5),
             least_time_int_macs_ms=round(t_alu * 1e3, 5), int_gmacs_per_s=round(t["int_macs"] / sec / 1e9, 1),
             bound=("memory" if t_mem >= t_alu else "integer ALU") + " (the larger of the two least times; the ALU peak is an assumed quarter-rate figure)",
             share_of_that_bound=round(share, 4), time_used="hipEvent time per call through the Python wrapper, not kernel time")
    r["frames_roofline"] = t
    st = [traffic(1, h, w, *style_args(h, w), 1) for h, w in STYLE_SIZES[:n_styles]]
    r["styles_bytes_that_must_move"] = int(sum(x["source_bytes"] + x["output_bytes"] for x in st))
    # (e) host-to-device bytes
    r["h2d_bytes_uint8"] = int(fh.numel() + sum(s.numel() for s in styles_host[:n_styles]))
    r["h2d_bytes_fp32_planes_of_the_prepared_batch"] = int(4 * 3 * 256 * 256 * (n_frames + n_styles))
    r["h2d_bytes_fp32_planes_of_the_decoded_frames"] = int(4 * r["h2d_bytes_uint8"])
    res[tag] = r

# (f) the public entry points
from styl3r_amd.inference import prepare_scene
n_scene = 50
scene_frames = frames_host[:n_scene]
E = torch.eye(4).repeat(n_scene, 1, 1)
E[:, 0, 3] = torch.arange(n_scene) * 0.05
E[:, 2, 3] = torch.arange(n_scene) * 0.01
Kn = torch.eye(3).repeat(n_scene, 1, 1)
Kn[:, 0, 0], Kn[:, 1, 1], Kn[:, 0, 2], Kn[:, 1, 2] = 0.9, 1.6, 0.5, 0.5
cfg = si.InputCfg()
draws = torch.Generator().manual_seed(3)


def c3_batch():
    return si.collate([si.prepare_example(scene_frames, Kn, E, [5, 45], [10, 20, 30, 40], styles_host[i], cfg, stage="train", scene=str(i),
                                          device=dev, generator=draws) for i in range(10)])


batch = c3_batch()
assert batch["context"]["image"].shape == (10, 2, 3, 256, 256) and batch["target"]["image"].shape == (10, 4, 3, 256, 256)
rows = torch.cat([torch.tensor([[0.9, 1.6, 0.5, 0.5, 0.0, 0.0]]).expand(200, -1), torch.eye(4)[:3].reshape(1, 12).expand(200, -1)], 1).contiguous()


def host_ms(fn, reps=20):
    """median wall ms of host-only work"""
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(1e3 * (time.perf_counter() - t0))
    return median(ts)


res["entry_points"] = {
    "c3_10x_prepare_example_plus_collate_ms": round(wall_ms(c3_batch), 3),
    "c2_prepare_scene_ms": round(wall_ms(lambda: prepare_scene(scene_frames, Kn, E, [5, 45], [25], styles_host[0], cfg, device=dev)), 3),
    "c3_camera_arithmetic_only_ms": round(host_ms(lambda: [si.prepare_cameras_f64(Kn, E, [5, 45], [10, 20, 30, 40], cfg, (360, 640)) for _ in range(10)]), 3),
    "convert_poses_200_rows_ms": round(host_ms(lambda: si.convert_poses(rows)), 3), "frames_per_scene": n_scene}

# (c) the reference's formulation on this host
try:
    from PIL import Image
except ImportError:
    Image = None
if Image is None:
    res["reference_formulation_on_this_host"] = "not measured (PIL does not import here)"
else:
    def pil_path(images, args_of):
        outs = []
        for im in images:
            (hs, ws), (top, left, oh, ow) = args_of(*im.shape[:2])
            planes = im.permute(2, 0, 1).float() / 255                                      # what the reference's loader holds after ToTensor
            b = (planes * 255).clip(min=0, max=255).type(torch.uint8).permute(1, 2, 0).numpy()
            scaled = np.array(Image.fromarray(b).resize((ws, hs), Image.LANCZOS)) / 255
            outs.append(torch.tensor(scaled, dtype=torch.float32).permute(2, 0, 1)[:, top:top + oh, left:left + ow])
        return torch.stack(outs).to(dev)
    r = {}
    for tag, n_frames, n_styles in (("c3", 60, 10), ("c2", 2, 1)):
        r[f"{tag}_frames_ms"] = round(wall_ms(lambda: pil_path(frames_host[:n_frames], lambda h, w: crop_args(h, w, SHAPE)), reps=5), 3)
        r[f"{tag}_styles_ms"] = round(wall_ms(lambda: [pil_path([s], style_args) for s in styles_host[:n_styles]], reps=5), 3)
    r["per_frame_360x640_ms"] = round(r["c3_frames_ms"] / 60, 4)
    ours = si.rescale_and_crop(frames_host.to(dev), K, SHAPE)[0]
    theirs = pil_path(frames_host, lambda h, w: crop_args(h, w, SHAPE))
    r["c3_frames_bit_equal_to_the_hip_path"] = bool(torch.equal(ours.view(torch.int32), theirs.view(torch.int32)))
    ours = torch.stack([si.apply_style_image_augmentation(s.to(dev), "train") for s in styles_host])
    theirs = torch.cat([pil_path([s], style_args) for s in styles_host])
    r["styles_bit_equal_to_the_hip_path"] = bool(torch.equal(ours.view(torch.int32), theirs.view(torch.int32)))
    import PIL
    r["pil_version"] = PIL.__version__
    res["reference_formulation_on_this_host"] = r
line = json.dumps(res)
print(line)
if args.out:
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(line + "\n")
