#!/usr/bin/env python
"""PNG frames at the shapes the package writes them at: (A) the 60 frames 256 x 256 x 3 of a fly-through, rendered from a synthetic
scene (`scenes.make_scene` through the decoder, fp32 planar on the device, as the drivers hold them), and (B) 10 frames 1080 x 1920 x 3
(synthesised bytes on the device).  Per workload:
  (a) the reference's formulation on THIS host: `Image.fromarray(prep_image(x)).save(...)` per frame into memory, one core (the copy
      of the floats to the host is not in it);
  (b) `gsr_png_chunks` and `gsr_png_assemble`: hipEvent time around `calls` back-to-back calls of each, with the launch geometry;
  (c) `encode_png` end to end: device frames -> PNG files as bytes in host memory, synchronised; beside it the two read-backs alone
      (lengths, then the used bytes) and the CRC-32 + container alone (zlib.crc32 over every stream);
  (d) `save_images` into a temporary directory, and the Pillow loop saving into one;
  (e) the file sizes of both next to each other, and zlib's Z_RLE construction on one frame (tests/test_png_host.py's yardstick).
Every leg is warmed; each figure is the median over `reps` with the smallest and the largest next to it.  Every file is decoded by
Pillow and compared with the frame's bytes, and the device bytes with the CPU restatement's on one frame, before anything is timed.
One JSON line; --out writes it to a file as well.
  python tools/bench_png.py [--reps 15] [--calls 20] [--out profiles/bench_png.json]
"""
import argparse, ctypes as C, json, sys, tempfile, time, zlib
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
assert torch.cuda.is_available(), "bench_png needs the MI355X"
dev = torch.device("cuda:0")
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
    """60 views of a synthetic scene through the decoder: fp32 (60,3,256,256) on the device"""
    from styl3r_amd.decoder import DecoderSplattingCUDACfg, Gaussians, get_decoder
    from styl3r_amd.scenes import make_scene
    sc = make_scene(n_ctx=2, grid_hw=(128, 128), n_views=60, image_hw=(256, 256), sh_degree=0, seed=7).to(dev)
    g = Gaussians(sc.means[None], sc.covariances[None], sc.harmonics[None], sc.opacities[None])
    dec = get_decoder(DecoderSplattingCUDACfg("splatting_cuda", [0.0, 0.0, 0.0], True)).to(dev)
    with torch.no_grad():
        return dec.forward(g, sc.extrinsics[None], sc.intrinsics[None], sc.near[None], sc.far[None], (256, 256)).color[0].contiguous()


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


def workload(tag, frames):
    """frames: fp32 (N,3,H,W) or uint8 (N,H,W,3) on the device"""
    planar = frames.dtype == torch.float32
    N, (H, W) = frames.shape[0], (frames.shape[2:] if planar else frames.shape[1:3])
    host_u8 = (io._bytes_host(frames))                         # what every decoded file is compared with
    host_in = frames.cpu()
    r = {"frames": N, "shape": [H, W, 3], "input": "fp32 planar" if planar else "uint8 interleaved"}
    files = io.encode_png(frames)
    for png, want in zip(files, host_u8):
        assert np.array_equal(np.asarray(Image.open(BytesIO(png))), want)
    assert files[0] == io.encode_png(host_in[:1])[0], "device bytes differ from the CPU restatement's"
    r["decodes_to_the_input_bytes"], r["equal_to_cpu_restatement_frame_0"] = True, True

    def pillow_loop(directory=None):
        out = []
        for i, x in enumerate(host_in):
            a = io.prep_image(x).numpy() if planar else x.numpy()
            if directory is None:
                buf = BytesIO()
                Image.fromarray(a).save(buf, format="PNG")
                out.append(buf.getvalue())
            else:
                Image.fromarray(a).save(directory / f"{i:0>6}.png")
        return out
    pil_files = pillow_loop()
    reps_host = max(3, args.reps // 5)
    r["a_pillow_loop"] = wall(pillow_loop, sync=False, reps=reps_host)
    r["a_pillow_per_frame_ms"] = round(r["a_pillow_loop"]["median_ms"] / N, 4)

    rows = io.chunk_rows(H, W, 3)
    chunks = N * (-(-H // rows))
    nbytes, bound = lib.gsr_png_scratch_bytes(N, H, W, 3), lib.gsr_png_stream_bound(H, W, 3)
    stride = (bound + 15) & ~15
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    out = torch.empty(N * stride, dtype=torch.uint8, device=dev)
    lengths = torch.empty(N, dtype=torch.int32, device=dev)
    s = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    kind = _lib.GSR_PNG_SRC_F32_PLANAR if planar else _lib.GSR_PNG_SRC_U8
    k1 = lambda: _lib.check(lib.gsr_png_chunks(frames.data_ptr(), kind, N, H, W, 3, 0, scratch.data_ptr(), nbytes, s), "gsr_png_chunks")
    k2 = lambda: _lib.check(lib.gsr_png_assemble(scratch.data_ptr(), nbytes, N, H, W, 3, out.data_ptr(), stride, lengths.data_ptr(), s), "gsr_png_assemble")
    r["b_geometry"] = {"workgroups": chunks, "threads": 256, "rows_per_chunk": rows, "chunk_bytes": rows * (1 + 3 * W), "lds_bytes_per_workgroup": 40784,
                       "scratch_bytes": int(nbytes)}
    r["b_chunks_kernel"] = events(k1)
    r["b_assemble_kernel"] = events(k2)
    r["b_kernels_per_frame_ms"] = round((r["b_chunks_kernel"]["median_ms"] + r["b_assemble_kernel"]["median_ms"]) / N, 5)

    r["c_encode_png_end_to_end"] = wall(lambda: io.encode_png(frames))
    sizes = lengths.cpu().tolist()

    def read_back():
        n = lengths.cpu().tolist()
        return out.view(N, stride)[:, :max(n)].cpu()
    r["c_read_backs_alone"] = wall(read_back)
    used = read_back().numpy()
    streams = [used[i, :n].tobytes() for i, n in enumerate(sizes)]
    r["c_crc_and_container_alone"] = wall(lambda: [io.wrap_png(st, H, W, 3) for st in streams], sync=False)
    r["c_crc_share_of_end_to_end"] = round(r["c_crc_and_container_alone"]["median_ms"] / r["c_encode_png_end_to_end"]["median_ms"], 4)
    r["c_over_a"] = round(r["c_encode_png_end_to_end"]["median_ms"] / r["a_pillow_loop"]["median_ms"], 4)

    with tempfile.TemporaryDirectory() as tmp:
        tmp = Path(tmp)
        paths = [tmp / "hip" / f"{i:0>6}.png" for i in range(N)]
        r["d_save_images"] = wall(lambda: io.save_images(frames, paths), reps=reps_host)
        (tmp / "pil").mkdir()
        r["d_pillow_loop_to_files"] = wall(lambda: pillow_loop(tmp / "pil"), sync=False, reps=reps_host)

    ours, pil = sum(map(len, files)), sum(map(len, pil_files))
    r["e_file_bytes"] = {"hip": ours, "pillow": pil, "hip_over_pillow": round(ours / pil, 4), "raw_pixels": N * H * W * 3}
    filt = io.filter_rows(host_u8[0].reshape(H, W * 3), 3, 0)
    z = zlib.compressobj(6, zlib.DEFLATED, -15, 8, zlib.Z_RLE)
    ref = 11 + sum(len(z.compress(filt[y:y + rows].tobytes())) + len(z.flush(zlib.Z_SYNC_FLUSH)) for y in range(0, H, rows))
    r["e_frame_0_stream_bytes"] = {"hip": len(io.idat_payload(files[0])), "zlib_rle_same_chunks": ref, "pillow": len(io.idat_payload(pil_files[0]))}
    return r


res = {"metric": "PNG frames: HIP filter + run-length deflate, host container", "device": torch.cuda.get_device_name(0), "reps": args.reps,
       "calls_per_event_pair": args.calls, "chunk_limit_bytes": _lib.GSR_PNG_CHUNK_BYTES}
res["A_flythrough_60x256x256"] = workload("A", rendered_frames())
rng = np.random.default_rng(29)
res["B_10x1080x1920"] = workload("B", torch.from_numpy(np.stack([synth_1080(rng, t) for t in range(10)])).to(dev))
res["fallback_images"] = io.CALLS["png_fallback"]
line = json.dumps(res)
print(line)
if args.out:
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(line + "\n")
