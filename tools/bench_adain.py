#!/usr/bin/env python
"""The 2D-AdaIN baseline (styl3r_amd/baseline.py) on the device, at the two sizes the wrapper uses it: the validation picture (4 target views
of 256 x 256, one style) and the training picture (2 samples x 4 views, 2 styles).  Per arithmetic mode and case:
  a. `stylize` on the package's route against the torch expression of the same network (framework pad / conv2d / relu / interpolate, TF32
     off) -- time and kernel launches for the whole call and for the decoder alone -- and every decoder layer rc1 .. rc9 three ways: the
     flagged launch (source modes of vit_conv_x6_fwd; rc9: vit_conv3_rgb_fwd), the materialised route (framework relu / interpolate / pad,
     vit_conv_x6_forward on the padded map, crop) and the framework's own convolution;
  b. vit_adain_fwd and vit_conv3_rgb_fwd as bytes moved (what the algorithm needs: every input and output once) over the time of a call,
     against the HBM peak (8.0 TB/s spec; 6.29 TB/s is what a float4 copy reaches on this chip).
Timing: every variant warmed, then `--reps` windows of `--calls` back-to-back calls per variant, the variants ALTERNATING window by window
in one process; device events around a window; median and spread (max - min) over the windows.  Launches: kernels in a torch.profiler
trace of one call (None where the profiler is unavailable).  One JSON line.
  python tools/bench_adain.py [--hw 256] [--style-hw 256] [--reps 5] [--calls 3] [--warmup 2] [--modes bf16x6,bf16x3,f16x3]
"""
import argparse, json, statistics, sys
from pathlib import Path
sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import torch
import torch.nn.functional as F
from styl3r_amd import baseline, losses, vit_ops

ap = argparse.ArgumentParser()
ap.add_argument("--hw", type=int, default=256); ap.add_argument("--style-hw", type=int, default=256)
ap.add_argument("--reps", type=int, default=5); ap.add_argument("--calls", type=int, default=3); ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--modes", default="bf16x6,bf16x3,f16x3")
args = ap.parse_args()
assert torch.cuda.is_available(), "bench_adain needs the MI355X"
dev = torch.device("cuda:0")
torch.backends.cudnn.allow_tf32 = torch.backends.cuda.matmul.allow_tf32 = False
HBM_SPEC, HBM_COPY = 8.0e12, 6.29e12

g = torch.Generator().manual_seed(3)
model = baseline.AdaIN2D()
for name, buf in model.named_buffers():
    if buf.dim() == 4:
        buf.copy_((torch.rand(buf.shape, generator=g) * 2 - 1) * (6.0 / buf[0].numel()) ** 0.5)      # variance 2 / fan_in
    elif not name.startswith("_denorm"):
        buf.copy_(torch.rand(buf.shape, generator=g) * 0.1 - 0.05 + (4.0 if name == "vgg_encoder.features.19.bias" else 0.0))
model = model.to(dev)


def window(fn, calls):
    a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    e.record()
    torch.cuda.synchronize(dev)
    return a.elapsed_time(e) / calls


def alternate(variants: dict) -> dict:
    """{name: fn} -> {name: {ms, spread_ms}}: warm all, then reps x (one window of each, in turn)"""
    for fn in variants.values():
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize(dev)
    times = {k: [] for k in variants}
    for _ in range(args.reps):
        for k, fn in variants.items():
            times[k].append(window(fn, args.calls))
    return {k: dict(ms=round(statistics.median(v), 4), spread_ms=round(max(v) - min(v), 4)) for k, v in times.items()}


def launches(fn):
    try:
        from torch.profiler import ProfilerActivity, profile
        fn(); torch.cuda.synchronize(dev)
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn(); torch.cuda.synchronize(dev)
        return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and not e.name.lower().startswith("memcpy"))
    except Exception:
        return None


def case(tag, samples, views, mode):
    vit_ops.LINEAR_MODE = mode
    B = samples * views
    images = torch.rand((B, 3, args.hw, args.hw), generator=g).to(dev)
    styles = torch.rand((samples, 3, args.style_hw, args.style_hw), generator=g).to(dev)
    index = torch.arange(samples, dtype=torch.int32).repeat_interleave(views)
    x, s = losses._imagenet_normalize(images), losses._imagenet_normalize(styles)
    n0 = dict(baseline.CALLS)
    with torch.no_grad():
        out = model.stylize(images, styles, style_index=index)
        assert [baseline.CALLS[k] - n0[k] for k in ("adain_hip", "conv_rc_x6", "conv_rgb_hip", "adain2d_expression")] == [1, 8, 1, 0]
        assert out.shape == images.shape
        raw, ref = model.generate(x, s, 1.0, style_index=index), model.generate_expression(x, s, 1.0, index)
        res = dict(B=B, styles=samples, rel_diff_to_fp32_expression=float((raw - ref).abs().max() / ref.abs().max()))
        whole = dict(route=lambda: model.stylize(images, styles, style_index=index),
                     expression=lambda: model.generate_expression(losses._imagenet_normalize(images), losses._imagenet_normalize(styles), 1.0, index, denorm=True))
        res["stylize"] = alternate(whole)
        res["stylize_launches"] = {k: launches(fn) for k, fn in whole.items()}
        fc, fs = model.vgg_encoder(x, output_last_feature=True), model.vgg_encoder(s, output_last_feature=True)
        t = baseline.adain(fc, fs, 1.0, index)
        sc, sh = model._denorm_scale.view(1, 3, 1, 1), model._denorm_shift.view(1, 3, 1, 1)
        dec = dict(route=lambda: model._decode_hip(t, True), materialised=lambda: model._decode_materialised(t, True),
                   expression=lambda: torch.clamp(model.decoder(t) * sc + sh, 0, 1))
        res["decoder"] = alternate(dec)
        res["decoder_launches"] = {k: launches(fn) for k, fn in dec.items()}
        # per layer: h = the input of layer k as the route holds it (the pre-activation output of layer k - 1; rc1: the AdaIN output)
        h, layers = t, {}
        for k, rc in enumerate(model.decoder.layers(), 1):
            w, b, up2, relu_in = rc.conv.weight, rc.conv.bias, k in baseline.UPSAMPLED, k > 1
            pre = lambda h=h, up2=up2, relu_in=relu_in: F.pad(F.interpolate(torch.relu(h) if relu_in else h, scale_factor=2) if up2 else
                                                              (torch.relu(h) if relu_in else h), (1, 1, 1, 1), mode="reflect")
            if k < 9:
                variants = dict(flagged=lambda h=h, w=w, b=b, up2=up2, relu_in=relu_in: baseline.conv_rc_x6(h, w, b, up2=up2, relu_in=relu_in),
                                materialised=lambda pre=pre, w=w, b=b: vit_ops.conv_x6_forward(pre(), w, b)[..., 1:-1, 1:-1],
                                framework=lambda pre=pre, w=w, b=b: F.conv2d(pre(), w, b))
            else:
                variants = dict(flagged=lambda h=h, w=w, b=b: baseline.conv_rgb(h, w, b, relu_in=True, scale=model._denorm_scale, shift=model._denorm_shift),
                                framework=lambda pre=pre, w=w, b=b: torch.clamp(F.conv2d(pre(), w, b) * sc + sh, 0, 1))
            layers[f"rc{k}"] = dict(shape=[*h.shape[:2], w.shape[0], *( (2 * h.shape[2], 2 * h.shape[3]) if up2 else h.shape[2:])], **alternate(variants))
            h = variants["flagged"]() if k < 9 else h
        res["layers"] = layers
        # b. the two new kernels as bytes over time
        (Bc, Cc, hh, ww), M = fc.shape, fs.shape[2] * fs.shape[3]
        ms = alternate(dict(adain=lambda: baseline.adain(fc, fs, 1.0, index)))["adain"]
        nbytes = (2 * Bc * Cc * hh * ww + samples * Cc * M) * 4
        res["adain_kernel"] = dict(**ms, bytes=nbytes, TBps=round(nbytes / ms["ms"] / 1e9, 4), share_of_spec=round(nbytes / ms["ms"] / 1e-3 / HBM_SPEC, 4),
                                   share_of_copy=round(nbytes / ms["ms"] / 1e-3 / HBM_COPY, 4))
        ms = layers["rc9"]["flagged"]
        nbytes = (h.numel() + B * 3 * h.shape[2] * h.shape[3]) * 4
        res["rgb_kernel"] = dict(ms=ms["ms"], spread_ms=ms["spread_ms"], bytes=nbytes, TBps=round(nbytes / ms["ms"] / 1e9, 4),
                                 share_of_spec=round(nbytes / ms["ms"] / 1e-3 / HBM_SPEC, 4), share_of_copy=round(nbytes / ms["ms"] / 1e-3 / HBM_COPY, 4))
    return res


result = dict(device=torch.cuda.get_device_name(0), hw=args.hw, reps=args.reps, calls=args.calls)
for mode in args.modes.split(","):
    result[mode] = dict(validation=case("validation", 1, 4, mode), training=case("training", 2, 4, mode))
print(json.dumps(result))
