"""GPU tests (-m gpu) of the AdaAttN kernels (csrc/vit_adaattn.hip behind vit_adaattn_stats / vit_adaattn_l1) through losses.adaattn_stats,
adaattn_l1, LossAdaAttN and the train step.  The yardstick is always the float64 expression on the CPU, on the fp32-rounded inputs of
tests/adaattn_inputs.py; `e32` is the error of the package's fp32 expression on the CPU for the same inputs (the reference's op sequence,
pinned by test_adaattn_host.py).  The bars:
  stats   max |mean - mean64| <= max(4 e32_mean, 2^-20 max |s|),  max |std^2 - var64| <= max(4 e32_var, 2^-19 max s^2)
          (4: a tiled online summation order against one bmm; the floors: the resolution of a two-piece split, needed where the fp32
          expression is exact); std itself is only required finite and >= 0 (the square root near zero variance)
  tail    value within max(4 e32, 1e-6 |value|); gradient EQUAL to sign64 / numel outside {0 < |p - cs|64 < 1e-4} (cs carries ~1e-5 of fp32
          error at these magnitudes), which holds at most 0.1 % of the elements; planted exact ties give exactly 0
  loss    value / content / style within 1e-4 relative (the bar of test_gpu_lpips.py for VGG-chain quantities); cs rms error <= 4 x the fp32
          expression's; gradient relative L2 <= 1e-4 against a float64 chain that takes the device's cs on the active near-ties"""
import ctypes as C
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from styl3r_amd import losses, vit_ops
from tests import adaattn_inputs as ai

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 4096


@functools.lru_cache(maxsize=None)
def stats_reference(name):
    q_hat, k_hat, s, index = ai.stats_inputs(name)
    mean64, std64 = losses.adaattn_stats_expression(q_hat.double(), k_hat.double(), s.double(), index)
    mean32, std32 = losses.adaattn_stats_expression(q_hat, k_hat, s, index)
    var64 = std64 ** 2
    e32_mean = float((mean32.double() - mean64).abs().max())
    e32_var = float((std32.double() ** 2 - var64).abs().max())
    return (q_hat, k_hat, s, index), mean64, var64, e32_mean, e32_var


def raw_stats(q_hat, k_hat, s, index):
    """vit_adaattn_stats into NaN-filled outputs with a guard region behind each; returns (mean, std) on the CPU"""
    lib = vit_ops.load()
    (bq, d, nq), (bs, c, m) = q_hat.shape, s.shape
    n = bq * c * nq
    bufs = [torch.full((n + GUARD,), float("nan"), device=DEV) for _ in range(2)]
    for b in bufs:
        b[n:] = -7.25
    qd, kd, sd, idev = q_hat.to(DEV), k_hat.to(DEV), s.to(DEV), index.to(DEV)
    rc = lib.vit_adaattn_stats(qd.data_ptr(), kd.data_ptr(), sd.data_ptr(), index.data_ptr(), idev.data_ptr(), bq, bs, d, c, nq, m,
                               bufs[0].data_ptr(), bufs[1].data_ptr(), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, lib.vit_last_error()
    torch.cuda.synchronize()
    for b in bufs:
        assert bool((b[n:] == -7.25).all()), "the guard region behind an output was written"
    return bufs[0][:n].view(bq, c, nq).cpu(), bufs[1][:n].view(bq, c, nq).cpu()


@pytest.mark.parametrize("name", list(ai.STATS_REGIMES))
def test_stats_kernel(name):
    (q_hat, k_hat, s, index), mean64, var64, e32_mean, e32_var = stats_reference(name)
    mean, std = raw_stats(q_hat, k_hat, s, index)
    assert bool(torch.isfinite(mean).all()) and bool(torch.isfinite(std).all()) and bool((std >= 0).all())
    n0 = dict(losses.CALLS)
    mean2, std2 = losses.adaattn_stats(q_hat.to(DEV), k_hat.to(DEV), s.to(DEV), index)
    assert losses.CALLS["adaattn_hip_stats"] == n0["adaattn_hip_stats"] + 1 and losses.CALLS["adaattn_expr_stats"] == n0["adaattn_expr_stats"]
    assert torch.equal(mean2.cpu(), mean) and torch.equal(std2.cpu(), std), "two runs differ"
    err_mean = float((mean.double() - mean64).abs().max())
    err_var = float((std.double() ** 2 - var64).abs().max())
    bar_mean = max(4 * e32_mean, 2.0 ** -20 * float(s.abs().max()))
    bar_var = max(4 * e32_var, 2.0 ** -19 * float(s.max()) ** 2)
    print(f"{name}: mean error {err_mean:.3e} (e32 {e32_mean:.3e}, bar {bar_mean:.3e}), variance error {err_var:.3e} (e32 {e32_var:.3e}, "
          f"bar {bar_var:.3e}), std error {float((std.double() - var64.sqrt()).abs().max()):.3e}")
    assert err_mean <= bar_mean
    assert err_var <= bar_var
    if name == "one_key":                                                   # one key: the softmax is 1, the mean is the style value itself
        want = s[index.long()].expand(-1, -1, q_hat.shape[2])
        assert torch.equal(mean, want)
    if name == "flat_channels":
        assert bool((std[:, ai.ZERO_CHANNEL] == 0).all()) and bool((mean[:, ai.ZERO_CHANNEL] == 0).all())
        assert float((mean[:, ai.CONST_CHANNEL] - 0.7).abs().max()) <= bar_mean


def test_stats_beyond_the_fast_path_take_the_expression():
    """VGG layers 4 - 5 (D = 960, 1472; C = 512): routed to the expression on the device, and counted"""
    g = torch.Generator().manual_seed(0)
    q_hat, k_hat, s = torch.randn(1, 512, 9, generator=g), torch.randn(1, 512, 12, generator=g), torch.rand(1, 64, 12, generator=g)
    n0 = dict(losses.CALLS)
    mean, std = losses.adaattn_stats(q_hat.to(DEV), k_hat.to(DEV), s.to(DEV))
    assert losses.CALLS["adaattn_expr_stats"] == n0["adaattn_expr_stats"] + 1 and losses.CALLS["adaattn_hip_stats"] == n0["adaattn_hip_stats"]
    m64, _ = losses.adaattn_stats_expression(q_hat.double(), k_hat.double(), s.double())
    assert float((mean.cpu().double() - m64).abs().max()) < 1e-4


@pytest.mark.parametrize("shape", ai.TAIL_SHAPES)
def test_tail_kernel(shape):
    """(the planted ties are compared like every other element -- sign64 is exactly 0 there -- so the set that is left out holds the natural
    near-ties only; with the ties counted in, as {|p - cs|64 < 1e-4}, it is still below 0.1 % at the larger shape)"""
    p, c, mean, std, ties = ai.tail_inputs(shape)
    numel = p.numel()
    c64 = c.double()
    c_hat = (c64 - c64.mean(-1, keepdim=True)) / (c64.var(-1, unbiased=False, keepdim=True) + 1e-5).sqrt()
    cs64 = c_hat * std.double() + mean.double()
    d64 = p.double() - cs64
    value64 = float(d64.abs().mean())
    e32 = abs(float(losses.adaattn_l1(p, c, mean, std)) - value64)
    pd = p.to(DEV).requires_grad_(True)
    details = {}
    n0 = dict(losses.CALLS)
    loss = losses.adaattn_l1(pd, c.to(DEV), mean.to(DEV), std.to(DEV), details)
    (3.0 * loss).backward()
    assert losses.CALLS["adaattn_hip_l1"] == n0["adaattn_hip_l1"] + 1
    err = abs(float(loss.detach()) - value64)
    print(f"{shape}: value error {err:.3e} (e32 {e32:.3e}, bar {max(4 * e32, 1e-6 * value64):.3e})")
    assert err <= max(4 * e32, 1e-6 * abs(value64))
    near = (d64.abs() < ai.TIE_MARGIN) & (d64 != 0)
    assert int(near.sum()) <= 1e-3 * numel, int(near.sum())
    if numel > 100000:
        assert int((d64.abs() < ai.TIE_MARGIN).sum()) <= 1e-3 * numel
    want = torch.sign(d64).float() * np.float32(1.0 / numel)
    got = details["feature_grad"].cpu()
    assert torch.equal(got[~near], want[~near])
    assert bool((got.view(-1)[ties] == 0).all()) and len(ties) == (ai.N_TIES if numel >= 64 else 0)
    assert torch.equal(pd.grad.cpu(), 3.0 * got)
    cs = details["cs"].cpu()
    assert float((cs.double() - cs64).abs().max()) <= 1e-4
    if shape[-1] == 1:
        assert torch.equal(cs, mean)                                        # one position: instance_norm(c) = 0


@functools.lru_cache(maxsize=None)
def loss_reference(tag):
    """the float64 chain on the CPU for the fixture's shapes: features, cs per layer, parts; and the fp32 expression's cs error (rms)"""
    cfg = ai.CONFIGS[tag]
    depth = max(*cfg["content_loss_layers"], *cfg["style_loss_layers"])
    target, pred, style = ai.images(**ai.FIXTURE_SHAPE)
    b, v = target.shape[:2]
    index = torch.arange(b, dtype=torch.int32).repeat_interleave(v)
    flat = lambda t: t.reshape(b * v, *t.shape[2:])
    out, feats = {}, {}
    for dtype in (torch.float64, torch.float32):
        net = losses.NormalizedVGG(depth)
        net.load_normalised_vgg(ai.vgg_state_dict())
        net.to(dtype)
        with torch.no_grad():
            fp, fc, fs = net(flat(pred.to(dtype))), net(flat(target.to(dtype))), net(style.to(dtype))
            d = {}
            losses.adaattn_expression(fp, fc, fs, style_index=index, details=d, **cfg)
            if dtype == torch.float64:
                margin = ai.activation_margin(net, flat(pred.double()))
        out[dtype], feats[dtype] = d, fp
    rms32 = {l: float((out[torch.float32][f"cs{l}"].double() - out[torch.float64][f"cs{l}"]).pow(2).mean().sqrt()) for l in cfg["content_loss_layers"]}
    # the gradient comparison needs a prediction whose ReLU and pooling decisions an fp32 pass cannot take the other way (adaattn_inputs.
    # activation_margin): the margin is at least 4 x the largest error of the fp32 expression's own features
    e32_feat = max(float((a.double() - b).abs().max()) for a, b in zip(feats[torch.float32], feats[torch.float64]))
    print(f"{tag}: activation margin {margin:.3e}, fp32 feature error {e32_feat:.3e}")
    assert margin >= 4 * e32_feat, (margin, e32_feat)
    return out[torch.float64], rms32, (target, pred, style, index)


@pytest.mark.parametrize("mode", ["bf16x6", "f16x3", "bf16x3"])
@pytest.mark.parametrize("tag", list(ai.CONFIGS))
def test_whole_loss(tag, mode, monkeypatch):
    monkeypatch.setattr(vit_ops, "LINEAR_MODE", mode)
    cfgd = ai.CONFIGS[tag]
    cfg = losses.LossAdaAttNCfg(**cfgd)
    ref, rms32, (target, pred, style, index) = loss_reference(tag)
    depth = max(*cfg.content_loss_layers, *cfg.style_loss_layers)
    net = losses.NormalizedVGG(depth)
    net.load_normalised_vgg(ai.vgg_state_dict())
    fn = losses.LossAdaAttN(cfg, net).to(DEV)
    color = pred.to(DEV).requires_grad_(True)
    batch = {"target": {"image": target.to(DEV)}, "style": {"image": style.to(DEV)}}
    details = {}
    n0 = dict(losses.CALLS)
    loss = fn(SimpleNamespace(color=color), batch, None, 0, details=details)
    loss.backward()
    k = len(cfg.content_loss_layers)
    assert losses.CALLS["adaattn_hip_stats"] == n0["adaattn_hip_stats"] + k and losses.CALLS["adaattn_hip_l1"] == n0["adaattn_hip_l1"] + k
    assert losses.CALLS["adaattn_expr_stats"] == n0["adaattn_expr_stats"]
    want = float(ref["content"]) + cfg.lam * float(ref["style"])
    rel = lambda a, b: abs(float(a) - float(b)) / abs(float(b))
    print(f"{tag} {mode}: value {rel(loss.detach(), want):.2e} content {rel(details['content'], ref['content']):.2e} style {rel(details['style'], ref['style']):.2e}")
    # the float64 chain of the gradient: cs is the float64 one except on the active near-ties, where it is the device's
    net64 = losses.NormalizedVGG(depth)
    net64.load_normalised_vgg(ai.vgg_state_dict())
    net64.double()
    b, v = target.shape[:2]
    p64 = pred.double().requires_grad_(True)
    fp = net64(p64.reshape(b * v, *pred.shape[2:]))
    with torch.no_grad():
        fs = net64(style.double())
    chain = 0
    for l in cfg.content_loss_layers:
        p, cs64, cs_dev = fp[l - 1].flatten(2), ref[f"cs{l}"], details[f"cs{l}"].cpu().double()
        rms = float((cs_dev - cs64).pow(2).mean().sqrt())
        active = p.detach() > 0
        t_active = active & ((p.detach() - cs64).abs() < 1e-3)
        print(f"  layer {l}: cs rms error {rms:.3e} (fp32 expression {rms32[l]:.3e}), active near-ties {int(t_active.sum())} of {int(active.sum())}")
        assert rms <= 4 * rms32[l]
        assert int(t_active.sum()) <= 5e-3 * int(active.sum())
        chain = chain + (p - torch.where(t_active, cs_dev, cs64)).abs().mean()
    chain = chain + cfg.lam * losses.adaattn_style_term(fp, fs, cfg.style_loss_layers, cfg.style_loss_stats, index)
    chain.backward()
    g, g64 = color.grad.cpu().double(), p64.grad
    gerr = float((g - g64).norm() / g64.norm())
    print(f"  gradient relative L2 {gerr:.3e}")
    assert rel(loss.detach(), want) <= 1e-4 and rel(details["content"], ref["content"]) <= 1e-4 and rel(details["style"], ref["style"]) <= 1e-4
    assert gerr <= 1e-4


def test_train_step_with_the_adaattn_loss(lr=1e-4, nsteps=3):
    """(lr: AdamW's first steps move every weight by about lr whatever the gradient's size; 1e-4 keeps three steps of the random-init tiny
    encoder inside the range where a step along the gradient lowers the loss)"""
    from styl3r_amd.decoder import DecoderSplattingCUDACfg, get_decoder
    from styl3r_amd.encoder import EncoderNoPoSplatMultiTokenStyle, EncoderNoPoSplatTokenStyleCfg
    from styl3r_amd.scenes import make_scene
    from styl3r_amd.train import TrainStep
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    tiny = dict(enc_depth=1, dec_depth=12, enc_embed_dim=1024, dec_embed_dim=128, enc_num_heads=16, dec_num_heads=2,
                pos_embed="RoPE100", img_size=(512, 512))
    enc = EncoderNoPoSplatMultiTokenStyle(EncoderNoPoSplatTokenStyleCfg(stylized=False), trunk_params=tiny).to(dev).eval()   # eval: no head dropout
    with torch.no_grad():      # a random-init point head puts every Gaussian behind / beside the cameras: start them in view
        for h in (enc.downstream_head1, enc.downstream_head2):
            h.dpt.head[4].bias.copy_(torch.tensor([0.0, 0.0, 1.2], device=dev))
    dec = get_decoder(DecoderSplattingCUDACfg("splatting_cuda", [0.0, 0.0, 0.0], True)).to(dev)
    cfg = losses.LossAdaAttNCfg()
    net = losses.NormalizedVGG(3)
    net.load_normalised_vgg(ai.vgg_state_dict())
    fn = losses.LossAdaAttN(cfg, net).to(dev)
    step = TrainStep(enc, dec, lr=lr, clip=0.5, extra_losses=[fn])
    b, v, vt, H = 1, 2, 2, 64
    sc = make_scene(n_ctx=2, grid_hw=(8, 8), n_views=vt, image_hw=(H, H), seed=3)
    ex = lambda t: t.to(dev)[None].expand(b, *t.shape).contiguous()
    g = torch.Generator(dev).manual_seed(1)
    batch = dict(context=dict(image=torch.rand(b, v, 3, H, H, device=dev, generator=g) * 2 - 1, intrinsics=ex(sc.intrinsics[:1].expand(v, 3, 3))),
                 target=dict(image=torch.rand(b, vt, 3, H, H, device=dev, generator=g) * 0.5 + 0.25, extrinsics=ex(sc.extrinsics),
                             intrinsics=ex(sc.intrinsics), near=ex(sc.near), far=ex(sc.far)),
                 style=dict(image=torch.rand(b, 3, 48, H, device=dev, generator=g)))
    tgt = batch["target"]
    registry = losses.get_losses([losses.LossMseCfg(), cfg])
    registry[1].vgg = fn.vgg                                                # (the registry builds its own random VGG: compare on the same one)
    with torch.no_grad():          # on the weights the step starts from: [mse] fused + adaattn, and the registry's list with nothing fused
        gs, out = step._render(batch["context"], {"image": batch["context"]["image"][:, 0]}, tgt, tgt["image"])
        want = float(out.loss_mse) + float(fn(out, batch, gs, 0))
        gs2, out2 = step._render(batch["context"], {"image": batch["context"]["image"][:, 0]}, tgt)
        want_registry = float(sum(m(out2, batch, gs2, 0) for m in registry))
    before = enc.downstream_head1.dpt.head[4].weight.detach().clone()
    n0 = dict(losses.CALLS)
    totals = [float(step(batch)) for _ in range(nsteps)]
    print(f"train step totals {totals}, fused form {want:.9f}, registry form {want_registry:.9f}")
    assert all(np.isfinite(totals)) and totals[-1] < totals[0]
    assert abs(totals[0] - want) <= 1e-4 * want and abs(want_registry - want) <= 1e-4 * want      # (the whole-loss bar of this file)
    assert losses.CALLS["adaattn_hip_stats"] == n0["adaattn_hip_stats"] + nsteps and losses.CALLS["adaattn_hip_l1"] == n0["adaattn_hip_l1"] + nsteps
    assert not torch.equal(enc.downstream_head1.dpt.head[4].weight, before)
    step.losses, step.extra_losses = registry, []
    assert np.isfinite(float(step(batch))) and losses.CALLS["adaattn_hip_l1"] == n0["adaattn_hip_l1"] + nsteps + 1
