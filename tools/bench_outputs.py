#!/usr/bin/env python
"""Scene outputs at the serving shape (C2: 2 context views 256 x 256 -> G = 131 072 Gaussians, a 60-frame fly-through, plain + 4 styles):
  * gsr_trajectory against the host round trip (copy to the CPU, the float64 restatement of trajectory.py there, copy back -- the shape
    of the reference's route, whose Euler steps run in scipy on the host);
  * depth_range + pack_frames against the torch expression on the same device (two torch.quantile sorts, the colour index through a
    host look-up as matplotlib does it, clip / scale / cast, stack, flip and cat), for a vcat(rgb, depth) video and a 4-panel hcat one (pack_frames takes at most 4 panels);
  * ply_vertex_table + the copy to the host against the reference-shaped host route (numpy concatenate, then the per-Gaussian tuple
    loop) at G = 131 072 and 1 048 576;
  * the whole render_flythrough.
Every pair is timed A / B / A in one process, device-synchronised, after warm-up.  Bytes moved by the pack kernel come from the shapes.
One JSON line.
  python tools/bench_outputs.py [--frames 60] [--size 256] [--reps 20] [--no-big-ply]
"""
import argparse, json, sys, time
from pathlib import Path
sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import numpy as np
import torch
from styl3r_amd import export as ex
from styl3r_amd import trajectory as tj
from styl3r_amd.decoder import DecoderSplattingCUDACfg, Gaussians, get_decoder
from styl3r_amd.inference import render_flythrough
from styl3r_amd.scenes import make_scene

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=60); ap.add_argument("--size", type=int, default=256)
ap.add_argument("--reps", type=int, default=20); ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--styles", type=int, default=4); ap.add_argument("--no-big-ply", action="store_true", help="skip G = 1 048 576")
args = ap.parse_args()
assert torch.cuda.is_available(), "bench_outputs needs the MI355X"
dev = torch.device("cuda:0")
F, H = args.frames, args.size
g = torch.Generator(dev).manual_seed(1)


def timed(fn, reps=args.reps, warmup=args.warmup):
    """median wall ms per call, the device drained before and after each call (the host routes do host work)"""
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize(dev)
        ts.append(1e3 * (time.perf_counter() - t0))
    return sorted(ts)[len(ts) // 2]


def aba(a, b, **kw):
    x = timed(a, **kw); y = timed(b, **kw); x2 = timed(a, **kw)
    return {"hip_ms": round(x, 4), "hip_again_ms": round(x2, 4), "other_ms": round(y, 4), "speedup": round(y / x, 2)}


sc = make_scene(n_ctx=2, grid_hw=(H, H), n_views=2, image_hw=(H, H), sh_degree=0, seed=1234)
ctx = dict(image=torch.zeros(1, 2, 3, H, H, device=dev), extrinsics=sc.extrinsics[None, :2].to(dev), intrinsics=sc.intrinsics[None, :2].to(dev),
           near=sc.near[None, :2].to(dev), far=sc.far[None, :2].to(dev))
res = {"metric": "scene outputs, C2 serving shape", "frames": F, "size": H, "gaussians": int(sc.means.shape[0]), "styles": args.styles}

# ---- cameras ----------------------------------------------------------------------------------------------------------------------------------
t = tj.smooth_time(F, True, device=dev)
A, B, Ka, Kb = ctx["extrinsics"][:, 0], ctx["extrinsics"][:, 1], ctx["intrinsics"][:, 0], ctx["intrinsics"][:, 1]


def cams_host():
    e = tj._interpolate_extrinsics_f64(A.cpu(), B.cpu(), t.cpu(), 1e-4).float().to(dev)
    return e, tj.interpolate_intrinsics(Ka, Kb, t)


res["trajectory"] = aba(lambda: tj.trajectory_hip(A, B, Ka, Kb, t), cams_host)

# ---- frames -----------------------------------------------------------------------------------------------------------------------------------
color = torch.rand(1 + args.styles, F, 3, H, H, device=dev, generator=g) * 1.2 - 0.1
depth = torch.rand(F, H, H, device=dev, generator=g) * 4 + 0.5
lut = torch.from_numpy(ex.turbo_table().astype(np.float32) / 255)


def frames_expression(panels, axis, gap=8):
    d = [p for p in panels if p.dim() == 3]
    cols = {}
    if d:
        far = d[0].reshape(-1)[:16_000_000].quantile(0.99).log()
        near = d[0][d[0] > 0][:16_000_000].quantile(0.01).log()
        x = (1 - (d[0].log() - near) / (far - near)).clip(min=0, max=1).cpu().numpy()          # the colour map is host work in the reference
        idx = np.minimum((x * 256).astype(np.int64), 255)
        cols[id(d[0])] = lut[torch.from_numpy(idx)].to(dev).permute(0, 3, 1, 2)
    images = []
    for f in range(panels[0].shape[0]):
        parts = []
        for i, p in enumerate(panels):
            if i and gap:
                parts.append(torch.ones((3, gap, H) if axis == 0 else (3, H, gap), device=dev))
            parts.append(cols[id(p)][f] if p.dim() == 3 else p[f])
        images.append(torch.cat(parts, dim=1 + axis))
    video = (torch.stack(images).clip(min=0, max=1) * 255).type(torch.uint8)
    return torch.cat([video, video.flip(0)[1:-1]])


for tag, panels, axis in (("vcat_rgb_depth", [color[1], depth], 0), ("hcat_plain_3_styles", list(color[:4]), 1)):
    hip = lambda: ex.pack_frames(panels, axis=axis, gap=8, loop_reverse=True)
    r = aba(hip, lambda: frames_expression(panels, axis))
    rng = ex.depth_range(depth) if any(p.dim() == 3 for p in panels) else None
    pack_only = timed(lambda: ex.pack_frames(panels, axis=axis, gap=8, loop_reverse=True, depth_range=rng))
    out = hip()
    read = sum(p.numel() * 4 for p in panels) * (2 * F - 2) / F                 # every frame but the two ends is read twice (loop_reverse)
    moved = read + out.numel()
    r.update(pack_only_ms=round(pack_only, 4), bytes_moved=int(moved), pack_GBps=round(moved / pack_only / 1e6, 1), out_shape=list(out.shape))
    if rng is not None:
        r["depth_range_ms"] = round(timed(lambda: ex.depth_range(depth)), 4)
    res[f"frames_{tag}"] = r

# ---- PLY --------------------------------------------------------------------------------------------------------------------------------------
def ply_host(means, scales, rots, sh, opac):
    """the reference-shaped route: everything to the host, numpy concatenate, then one Python tuple per Gaussian into a structured array"""
    q = ex._quat_round_trip_host(rots.cpu().numpy())
    attrs = np.concatenate([means.cpu().numpy(), np.zeros((means.shape[0], 3), np.float32), sh[..., 0].cpu().contiguous().numpy(),
                            opac[:, None].cpu().numpy(), scales.log().cpu().numpy(), q], axis=1)
    elements = np.empty(means.shape[0], dtype=[(n, "f4") for n in ex.attribute_names(0)])
    elements[:] = list(map(tuple, attrs))
    return elements


for G_ in (131072,) + (() if args.no_big_ply else (1048576,)):
    gg = torch.Generator(dev).manual_seed(G_)
    inp = (torch.randn(G_, 3, device=dev, generator=gg), torch.rand(G_, 3, device=dev, generator=gg) * 0.1 + 1e-3,
           torch.randn(G_, 4, device=dev, generator=gg), torch.randn(G_, 3, 25, device=dev, generator=gg), torch.rand(G_, device=dev, generator=gg))
    res[f"ply_table_G{G_}"] = aba(lambda: ex.ply_vertex_table(*inp)[0].cpu(), lambda: ply_host(*inp), reps=3 if G_ > 200000 else 5, warmup=1)
    res[f"ply_table_G{G_}"]["hip_shift_and_scale_ms"] = round(timed(lambda: ex.ply_vertex_table(*inp, shift_and_scale=True)[0].cpu(), reps=5, warmup=1), 4)
    del inp

# ---- the whole video --------------------------------------------------------------------------------------------------------------------------
dec = get_decoder(DecoderSplattingCUDACfg("splatting_cuda", [0.0, 0.0, 0.0], True)).to(dev)
geo = dict(means=sc.means[None].to(dev), covariances=sc.covariances[None].to(dev), opacities=sc.opacities[None].to(dev))
sets = [Gaussians(harmonics=(sc.harmonics[None].to(dev) + 0.3 * s).contiguous(), **geo) for s in range(1 + args.styles)]
for tag, panels, axis in (("stylized", ("stylized",), 0), ("plain_depth_2_styles", ("plain", "depth", 0, 1), 1)):
    fn = lambda: render_flythrough(dec, sets, ctx, num_frames=F, panels=panels, axis=axis)
    res[f"render_flythrough_{tag}_ms"] = round(timed(fn, reps=max(3, args.reps // 4), warmup=2), 3)
print(json.dumps(res))
