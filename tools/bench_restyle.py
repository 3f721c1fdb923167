#!/usr/bin/env python
"""Multi-style serving at the C2 shape (1 scene, 2 context views of 256 x 256 -> 131 072 Gaussians, sh degree 0, full-size encoder with
random-init weights and re-centred heads) against the way the same job is done without it, in ONE process, alternating, warmed up,
medians.  One JSON line per case:
  * raster  S x `decoder.forward` under no_grad  vs  one `decoder.forward_styles`            S in {2, 4, 8} x V in {3, 60}
            (+ the composite kernels' device time per call from the library's stage timer, and S = 4 as 2 + 2 instead of one launch of 4)
  * encoder S x `encoder.forward`                vs  `encode_scene` + one `restyle` of S styles   S in {2, 4, 8}
  python tools/bench_restyle.py [--reps 15] [--warmup 3] [--only raster|encoder] [--profile]
--profile: a few un-timed calls of each rasterizer form at S = 4, V = 60 (the program to put behind `rocprofv3 --kernel-trace --stats --`).
"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import torch

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=15)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--only", choices=("raster", "encoder"), default=None)
ap.add_argument("--profile", action="store_true")
args = ap.parse_args()
assert torch.cuda.is_available(), "bench_restyle needs the MI355X"

from styl3r_amd import _lib, rasterizer, vit_ops
from styl3r_amd.decoder import DecoderSplattingCUDACfg, Gaussians, get_decoder
from styl3r_amd.encoder import EncoderNoPoSplatMultiTokenStyle, EncoderNoPoSplatTokenStyleCfg
from styl3r_amd.scenes import make_scene, recentre_output_heads_

dev = torch.device("cuda:0")
torch.manual_seed(0)
H, V_CTX = 256, 2
DIGEST = _lib.built_digest()
assert DIGEST == _lib.build_digest(), "libgsr_hip.so was not built from this tree"
sync = lambda: torch.cuda.synchronize(dev)


def ab(fa, fb, reps, warm):
    """alternating A / B wall-clock times (ms) around a device sync: medians and all samples"""
    ta, tb = [], []
    for i in range(warm + reps):
        for f, acc in ((fa, ta), (fb, tb)):
            sync(); t0 = time.perf_counter(); f(); sync()
            if i >= warm:
                acc.append(1e3 * (time.perf_counter() - t0))
    return statistics.median(ta), statistics.median(tb), ta, tb


def cameras(n):
    sc = make_scene(n_ctx=V_CTX, grid_hw=(8, 8), n_views=n, image_hw=(H, H), seed=1234)
    ex = lambda t: t.to(dev)[None].contiguous()
    return [ex(sc.extrinsics), ex(sc.intrinsics), ex(sc.near), ex(sc.far)]


with torch.device(dev):
    enc = EncoderNoPoSplatMultiTokenStyle(EncoderNoPoSplatTokenStyleCfg()).eval()
enc.head_streams = True
dec = get_decoder(DecoderSplattingCUDACfg("splatting_cuda", [0.0, 0.0, 0.0], True)).to(dev)
g = torch.Generator(dev).manual_seed(1234)
ctx = dict(image=torch.rand(1, V_CTX, 3, H, H, device=dev, generator=g) * 2 - 1,
           intrinsics=cameras(3)[1][:, :1].expand(1, V_CTX, 3, 3).contiguous())
identity = dict(image=ctx["image"][:, 0])
recentre_output_heads_(enc, ctx, identity)
STYLES = torch.rand(8, 3, H, H, device=dev, generator=g) * 2 - 1
common = {"shape": "C2: 1 scene, 2 ctx views 256x256, 131072 Gaussians, sh degree 0", "build_digest": DIGEST, "linear_arithmetic": vit_ops.LINEAR_MODE,
          "reps": args.reps, "warmup": args.warmup, "timing": "wall clock around a device sync, alternating A/B in one process, medians",
          "data": "synthetic, random-init weights, re-centred heads"}

with torch.no_grad():
    state = enc.encode_scene(ctx)
    sets = enc.restyle(state, dict(image=STYLES))
    harmonics = [s.harmonics for s in sets]
    geo = sets[0]


def raster_case(S, V):
    cams = cameras(V)
    gs = [Gaussians(geo.means, geo.covariances, harmonics[s], geo.opacities) for s in range(S)]

    def separate():
        with torch.no_grad():
            return [dec.forward(x, *cams, (H, H)).color for x in gs]

    def together():
        with torch.no_grad():
            return dec.forward_styles(geo, harmonics[:S], *cams, (H, H)).color

    a, b = separate(), together()
    diff = max(float((b[s] - a[s]).abs().max()) for s in range(S))
    pairs = rasterizer.LAST_STATS["pairs"]
    assert pairs > geo.means.shape[1], f"rendered (nearly) nothing: {rasterizer.LAST_STATS}"
    ms_a, ms_b, all_a, all_b = ab(separate, together, args.reps, args.warmup)
    rec = {"case": "raster", "S": S, "V": V, "separate_forwards_ms": round(ms_a, 3), "forward_styles_ms": round(ms_b, 3),
           "ratio": round(ms_a / ms_b, 3), "pairs_R": pairs, "max_abs_diff_to_separate": diff,
           "separate_all_ms": [round(x, 3) for x in all_a], "forward_styles_all_ms": [round(x, 3) for x in all_b]}
    # device time of the composite stage alone (two event records around it; the other stages untimed)
    prof = _lib.StageProfile(4 * S + 8)
    prof.set_stages(["composite_fwd"])
    rasterizer.PROFILE = prof
    try:
        n = 4
        for _ in range(n):
            separate()
        sync(); k5 = prof.read()["composite_fwd"]
        for _ in range(n):
            together()
        sync(); k5s = prof.read()["composite_fwd"]
        rec["composite_us_per_style"] = {"k_composite_fwd": round(1e3 * k5[0] / max(k5[1], 1), 2),
                                         "k_composite_fwd_styles": round(1e3 * k5s[0] / (n * S), 2)}
        if S == 4:      # one launch of 4 styles against two launches of 2
            rasterizer.STYLES_EXTRA_FLAGS = 2 << _lib.GSR_FLAG_STYLES_CHUNK_SHIFT
            for _ in range(n):
                together()
            sync(); k22 = prof.read()["composite_fwd"]
            rec["composite_us_per_style"]["as_2_plus_2"] = round(1e3 * k22[0] / (n * S), 2)
            rasterizer.STYLES_EXTRA_FLAGS = 0
            def together_2_2():
                rasterizer.STYLES_EXTRA_FLAGS = 2 << _lib.GSR_FLAG_STYLES_CHUNK_SHIFT
                try:
                    return together()
                finally:
                    rasterizer.STYLES_EXTRA_FLAGS = 0
            rasterizer.PROFILE = None
            _, ms_22, _, _ = ab(together, together_2_2, args.reps, 1)
            rec["forward_styles_as_2_plus_2_ms"] = round(ms_22, 3)
    finally:
        rasterizer.PROFILE = None
        rasterizer.STYLES_EXTRA_FLAGS = 0
        prof.close()
    return rec


def encoder_case(S):
    styles = [dict(image=STYLES[s:s + 1]) for s in range(S)]
    batch = dict(image=STYLES[:S])

    def separate():
        with torch.no_grad():
            return [enc(ctx, st, 0) for st in styles]

    def cached():
        with torch.no_grad():
            return enc.restyle(enc.encode_scene(ctx), batch)

    a, b = separate(), cached()
    b = b if isinstance(b, list) else [b]
    scale = max(float(x.harmonics.abs().max()) for x in a)
    diff = max(float((y.harmonics - x.harmonics).abs().max()) for x, y in zip(a, b)) / scale
    ms_a, ms_b, all_a, all_b = ab(separate, cached, args.reps, args.warmup)
    return {"case": "encoder", "S": S, "separate_forwards_ms": round(ms_a, 3), "encode_scene_plus_restyle_ms": round(ms_b, 3),
            "ratio": round(ms_a / ms_b, 3), "harmonics_rel_diff_to_separate": diff, "head_streams": True,
            "separate_all_ms": [round(x, 3) for x in all_a], "cached_all_ms": [round(x, 3) for x in all_b]}


if args.profile:
    cams = cameras(60)
    with torch.no_grad():
        for _ in range(3):
            for s in range(4):
                dec.forward(Gaussians(geo.means, geo.covariances, harmonics[s], geo.opacities), *cams, (H, H))
            dec.forward_styles(geo, harmonics[:4], *cams, (H, H))
            dec.forward_styles(geo, harmonics[:2], *cams, (H, H))
    sync()
    sys.exit(0)

if args.only in (None, "raster"):
    for V in (3, 60):
        for S in (2, 4, 8):
            print(json.dumps({**raster_case(S, V), **common}), flush=True)
if args.only in (None, "encoder"):
    for S in (2, 4, 8):
        print(json.dumps({**encoder_case(S), **common}), flush=True)
