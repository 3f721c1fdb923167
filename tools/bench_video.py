#!/usr/bin/env python
"""JPEG frames and Motion-JPEG videos at the shapes the package writes them at: (A) the 60 frames 256 x 256 x 3 of a fly-through, rendered
from a synthetic scene (`scenes.make_scene` through the decoder, packed to uint8 (60,256,256,3) on the device as `render_flythrough`
returns them), and (B) 10 frames 1080 x 1920 x 3 (synthesised bytes on the device).  Quality 90, 4:2:0.  Per workload:
  (a) the route there was before the encoder, on THIS host: the frames copied to the host, then `Image.fromarray(x).save(format="JPEG")`
      per frame into memory, one core;
  (b) `gsr_jpeg_enc_scans` alone: hipEvent time around `calls` back-to-back calls (four launches each), with the launch geometry;
  (c) `encode_jpeg` end to end: device frames -> JPEG files as bytes in host memory, synchronised; beside it the two read-backs alone;
  (d) `save_video` into a temporary directory, against route (a) wrapped by the same `wrap_avi` and written to a file.
Every leg is warmed; each figure is the median over `reps` with the smallest and the largest next to it.  Before anything is timed the
device files are compared with Pillow's, byte for byte.  One JSON line; --out writes it to a file as well.
  python tools/bench_video.py [--reps 15] [--calls 20] [--out profiles/bench_video.json]
"""
import argparse, ctypes as C, json, sys, tempfile, time
from io import BytesIO
from pathlib import Path
sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import numpy as np
import torch
from PIL import Image
from styl3r_amd import _lib, image_io as io

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=15); ap.add_argument("--calls", type=int, default=20); ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--out", default=None)
args = ap.parse_args()
assert torch.cuda.is_available(), "bench_video needs the MI355X"
dev = torch.device("cuda:0")
lib = _lib.load()
QUALITY, SAMPLING = 90, "4:2:0"


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


def events(fn):
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
    return spread(ts)


def rendered_frames():
    """60 views of a synthetic scene through the decoder, packed as the fly-through packs them: uint8 (60,256,256,3) on the device"""
    from styl3r_amd.decoder import DecoderSplattingCUDACfg, Gaussians, get_decoder
    from styl3r_amd.export import pack_frames
    from styl3r_amd.scenes import make_scene
    sc = make_scene(n_ctx=2, grid_hw=(128, 128), n_views=60, image_hw=(256, 256), sh_degree=0, seed=7).to(dev)
    g = Gaussians(sc.means[None], sc.covariances[None], sc.harmonics[None], sc.opacities[None])
    dec = get_decoder(DecoderSplattingCUDACfg("splatting_cuda", [0.0, 0.0, 0.0], True)).to(dev)
    with torch.no_grad():
        color = dec.forward(g, sc.extrinsics[None], sc.intrinsics[None], sc.near[None], sc.far[None], (256, 256)).color[0].contiguous()
    return pack_frames([color], loop_reverse=False)


def synth_1080(rng, t):
    H, W = 1080, 1920
    y, x = np.mgrid[0:H, 0:W].astype(np.float32)
    img = np.zeros((H, W, 3), np.float32)
    for c in range(3):
        for _ in range(3):
            fx, fy = rng.uniform(0.003, 0.05, 2)
            img[..., c] += rng.uniform(15, 50) * np.sin(fx * x + fy * y + rng.uniform(0, 6.28) + 0.1 * t)
        img[..., c] += 128 + 40 * ((x // 97 + y // 61 + t) % 2) + rng.normal(0, 3, (H, W))
    img[H // 3:H // 2, W // 4:W // 2] = 0                       # a flat panel, as a rendered background gives
    return np.clip(img, 0, 255).astype(np.uint8)


def workload(frames):
    """frames: uint8 (N,H,W,3) on the device"""
    N, H, W, _ = frames.shape
    r = {"frames": N, "shape": [H, W, 3], "quality": QUALITY, "subsampling": SAMPLING}

    def pillow_route():
        out = []
        for x in frames.cpu().numpy():
            buf = BytesIO()
            Image.fromarray(x).save(buf, format="JPEG", quality=QUALITY, subsampling=io.JPEG_SAMPLING[SAMPLING][3])
            out.append(buf.getvalue())
        return out
    files, pil_files = io.encode_jpeg(frames, QUALITY, SAMPLING), pillow_route()
    r["equal_to_pillow_byte_for_byte"] = files == pil_files
    r["file_bytes"] = sum(map(len, files))
    reps_host = max(3, args.reps // 5)
    r["a_copy_and_pillow_loop"] = wall(pillow_route, reps=reps_host)

    code = io.JPEG_SAMPLING[SAMPLING][0]
    nbytes, bound = lib.gsr_jpeg_enc_scratch_bytes(N, H, W, code), lib.gsr_jpeg_enc_stream_bound(H, W, code)
    stride = (bound + 15) & ~15
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    out = torch.empty(N * stride, dtype=torch.uint8, device=dev)
    lengths = torch.empty(N, dtype=torch.int32, device=dev)
    quant = np.ascontiguousarray(io.jpeg_quant_tables(QUALITY))
    s = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    k = lambda: _lib.check(lib.gsr_jpeg_enc_scans(frames.data_ptr(), _lib.GSR_JPEG_ENC_SRC_U8, N, H, W, code, quant.ctypes.data, scratch.data_ptr(), nbytes,
                                                  out.data_ptr(), stride, lengths.data_ptr(), s), "gsr_jpeg_enc_scans")
    mcus = (-(-H // 16)) * (-(-W // 16))
    r["b_geometry"] = {"segments": N * (-(-mcus // 16)), "mcus_per_segment": 16, "threads": [256, 256, 128, 256], "scratch_bytes": int(nbytes),
                       "stream_bound_bytes": int(bound)}
    r["b_kernels"] = events(k)
    r["b_kernels_per_frame_ms"] = round(r["b_kernels"]["median_ms"] / N, 5)

    r["c_encode_jpeg_end_to_end"] = wall(lambda: io.encode_jpeg(frames, QUALITY, SAMPLING))

    def read_back():
        n = lengths.cpu().tolist()
        return out.view(N, stride)[:, :max(n)].cpu()
    r["c_read_backs_alone"] = wall(read_back)
    r["c_over_a"] = round(r["c_encode_jpeg_end_to_end"]["median_ms"] / r["a_copy_and_pillow_loop"]["median_ms"], 4)

    with tempfile.TemporaryDirectory() as tmp:
        tmp = Path(tmp)
        r["d_save_video"] = wall(lambda: io.save_video(frames, tmp / "hip.avi", quality=QUALITY, subsampling=SAMPLING), reps=reps_host)
        r["d_pillow_route_to_avi"] = wall(lambda: (tmp / "pil.avi").write_bytes(io.wrap_avi(pillow_route(), H, W, 30)), reps=reps_host)
        r["d_files_equal"] = (tmp / "hip.avi").read_bytes() == (tmp / "pil.avi").read_bytes()
    r["d_over_pillow_route"] = round(r["d_save_video"]["median_ms"] / r["d_pillow_route_to_avi"]["median_ms"], 4)
    return r


res = {"metric": "JPEG frames and Motion-JPEG AVI: HIP baseline encoder, host header and container", "device": torch.cuda.get_device_name(0),
       "reps": args.reps, "calls_per_event_pair": args.calls}
res["A_flythrough_60x256x256"] = workload(rendered_frames())
rng = np.random.default_rng(29)
res["B_10x1080x1920"] = workload(torch.from_numpy(np.stack([synth_1080(rng, t) for t in range(10)])).to(dev))
res["fallback_images"] = io.CALLS["jpeg_enc_fallback"]
line = json.dumps(res)
print(line)
if args.out:
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(line + "\n")
