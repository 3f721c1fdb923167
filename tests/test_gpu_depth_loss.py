"""GPU tests (-m gpu) of the depth-smoothness kernels (csrc/gsr_depth.hip behind gsr_depth_smooth_fwd / _bwd) through losses.depth_smoothness,
LossDepth, the decoder and the train step.  Yardsticks: the golden vectors of the reference's own LossDepth (float64), and the float64 torch
restatement on CPU copies for the shapes the fixture does not cover.  Every input keeps the sign of every difference unambiguous in fp32
(tests/depth_loss_inputs.py), so no element is left out of a comparison; the tolerances are derived there, not observed."""
import functools

import numpy as np
import pytest
import torch

from styl3r_amd import losses
from tests.depth_loss_inputs import CONFIGS, GRAD_RTOL, assert_sign_condition, make_inputs, value_tolerance

pytestmark = pytest.mark.gpu
DEV = "cuda"
TILE_H, TILE_W = 8, 128            # a workgroup of k_depth_smooth_fwd / _bwd (csrc/gsr_depth.hip DS_TH, DS_TW)


def on_device(depth, near, far, image, weight, sigma, second, upstream=1.0):
    """value and d (upstream * loss) / d depth of the HIP route, back on the CPU"""
    d = depth.to(DEV).requires_grad_(True)
    n0 = dict(losses.CALLS)
    value = losses.depth_smoothness(d, near.to(DEV), far.to(DEV), image.to(DEV), weight, sigma, second)
    (upstream * value).backward()
    assert losses.CALLS["depth_hip_fwd"] == n0["depth_hip_fwd"] + 1 and losses.CALLS["depth_hip_bwd"] == n0["depth_hip_bwd"] + 1
    assert value.dtype == torch.float32 and value.shape == () and d.grad.shape == depth.shape
    return float(value.detach()), d.grad.double().cpu().numpy()


def check(tag, got_v, got_g, ref_v, ref_g, weight, sigma, upstream=1.0):
    scale = np.abs(ref_g).max()
    verr, gerr = abs(got_v - ref_v), float(np.abs(got_g - upstream * ref_g).max())
    print(f"{tag}: value error {verr:.3e} (bound {value_tolerance(weight, sigma):.3e}), gradient error {gerr:.3e} (bound {GRAD_RTOL * upstream * scale:.3e})")
    assert np.isfinite(got_g).all()
    assert verr <= value_tolerance(weight, sigma)
    assert gerr <= GRAD_RTOL * upstream * scale


@pytest.mark.parametrize("tag", list(CONFIGS))
def test_fixture_parity(tag):
    gold = np.load(__file__.rsplit("/", 1)[0] + "/golden/depth_loss_ref.npz")
    depth, near, far, image = (torch.from_numpy(gold[k]) for k in ("depth", "near", "far", "image"))
    assert_sign_condition(depth, near, far, image)
    sigma, second = CONFIGS[tag]
    weight = float(gold["weight"])
    ref_v, ref_g = float(gold[f"{tag}_value"]), gold[f"{tag}_grad"]
    check(tag, *on_device(depth, near, far, image, weight, sigma, second), ref_v, ref_g, weight, sigma)
    v3, g3 = on_device(depth, near, far, image, weight, sigma, second, upstream=3.0)                # (3 * loss).backward(): grad_loss is read on the device
    check(tag + " x3", v3, g3, ref_v, ref_g, weight, sigma, upstream=3.0)


@functools.lru_cache(maxsize=None)
def reference(shape, seed=5):
    """inputs of `shape` under the sign condition and the float64 restatement's value / gradient for the four configurations, computed once"""
    depth, near, far, image = make_inputs(*shape, seed)
    assert_sign_condition(depth, near, far, image)
    out = {}
    for tag, (sigma, second) in CONFIGS.items():
        if min(shape[-2:]) < (3 if second else 2):
            continue
        d = depth.double().requires_grad_(True)
        v = losses.depth_smoothness_expression(d, near.double(), far.double(), image.double(), 1.0, sigma, second)
        v.backward()
        out[tag] = (float(v.detach()), d.grad.numpy())
    return (depth, near, far, image), out


EDGE_SHAPES = ([(1, 1, 2, 2), (1, 1, 3, 3)] + [(1, 1, 3, w) for w in (5, 6, 7, 8)]                    # least sizes; every row-tail residue, unaligned rows
               + [(1, 2, h, w) for h in (TILE_H - 1, TILE_H, TILE_H + 1) for w in (TILE_W - 1, TILE_W, TILE_W + 1)]
               + [(3, 4, 72, 272)])                                                                  # 324 workgroups: the fold's lanes add more than one partial each


@pytest.mark.parametrize("shape", EDGE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_edge_shapes(shape):
    inputs, refs = reference(shape)
    assert refs and ("second" in refs) == (min(shape[-2:]) >= 3)
    for tag, (ref_v, ref_g) in refs.items():
        sigma, second = CONFIGS[tag]
        check(f"{shape} {tag}", *on_device(*inputs, 1.0, sigma, second), ref_v, ref_g, 1.0, sigma)


def test_tiny_shapes_are_refused_on_the_device_too():
    one = torch.ones(1, 1, device=DEV)
    with pytest.raises(ValueError, match="no difference"):
        losses.depth_smoothness(torch.zeros(1, 1, 2, 5, device=DEV), one, 2 * one, use_second_derivative=True)


def test_forward_is_deterministic_and_a_view_does_not_depend_on_the_batch():
    (depth, near, far, image), refs = reference((1, 1, 19, 37))
    for tag, (sigma, second) in CONFIGS.items():
        args = (depth.to(DEV), near.to(DEV), far.to(DEV), image.to(DEV), 1.0, sigma, second)
        a, b = losses.depth_smoothness(*args), losses.depth_smoothness(*args)
        assert torch.equal(a, b)                                                                     # bit-identical from run to run
        # the same view behind two views that lie beyond far (they add exactly 0 to both sums): every count is 3 x as large
        N = 3
        d3 = torch.cat([torch.full((1, N - 1, 19, 37), 1e3), depth], dim=1)
        n3, f3 = torch.cat([torch.ones(1, N - 1), near], dim=1), torch.cat([torch.full((1, N - 1), 2.0), far], dim=1)
        i3 = torch.cat([image.flip(-1).expand(1, N - 1, -1, -1, -1), image], dim=1)
        c = losses.depth_smoothness(d3.to(DEV), n3.to(DEV), f3.to(DEV), i3.to(DEV), 1.0, sigma, second)
        print(f"{tag}: alone {float(a):.9f}, in a batch of {N} x {N}: {N * float(c):.9f}, float64 {refs[tag][0]:.9f}")
        assert abs(N * float(c) - float(a)) <= value_tolerance(1.0, sigma)
        assert abs(float(a) - refs[tag][0]) <= value_tolerance(1.0, sigma)


def test_ties_and_clamps():
    H, W = 5, 9
    near, far = torch.tensor([[1.0, 1.0]]), torch.tensor([[20.0, 20.0]])
    image = torch.full((1, 2, 3, H, W), 0.5)
    hi = float(torch.tensor(20.0).double().log())
    depth = torch.zeros(1, 2, H, W)                                       # view 0: an uncovered render, depth 0 = log(near) everywhere
    depth[0, 1] = 1.0                                                     # view 1: in range ...
    depth[0, 1, 2, 4] = 0.0                                               # ... one pixel exactly on the lower bound
    depth[0, 1, 0, 0], depth[0, 1, 4, 8] = -1.0, 5.0                      # ... and one beyond each bound
    d = depth.double().requires_grad_(True)
    ref = losses.depth_smoothness_expression(d, near.double(), far.double(), None, 1.0, None, False)
    ref.backward()
    v, g = on_device(depth, near, far, image, 1.0, None, False)
    check("ties", v, g, float(ref.detach()), d.grad.numpy(), 1.0, None)
    assert (g[0, 0] == 0).all()                                           # flat view at the bound: sign(0) = 0 everywhere
    assert g[0, 1, 0, 0] == 0 and g[0, 1, 4, 8] == 0                      # outside the bounds: exactly 0
    # the tie: four differences of size 1 / hi leave the pixel, each pulls it up with 1 / count; half of that arrives
    count_x, count_y = 2 * H * (W - 1), 2 * (H - 1) * W
    want = -0.5 * (2 / count_x + 2 / count_y) / hi
    assert abs(g[0, 1, 2, 4] - want) <= GRAD_RTOL * abs(want)
    inner = g[0, 1, 2, 2]                                                 # an in-range pixel among equals: no gradient
    assert inner == 0
    alone = depth[:, :1]
    v0, g0 = on_device(alone, near[:, :1], far[:, :1], image[:, :1], 1.0, 10.0, True)
    assert v0 == 0 and (g0 == 0).all()                                    # all-zero depth with near = 1: zero loss, zero gradient


def _scene(dev):
    from styl3r_amd.decoder import DecoderSplattingCUDACfg, Gaussians, get_decoder
    from styl3r_amd.scenes import make_scene
    res = (64, 80)
    sc = make_scene(n_ctx=1, grid_hw=(64, 64), n_views=2, image_hw=res, sh_degree=0, seed=41)
    st = lambda n: getattr(sc, n)[None].to(dev)
    dec = get_decoder(DecoderSplattingCUDACfg("splatting_cuda", [0.0, 0.0, 0.0], True)).to(dev)
    target = torch.rand(1, 2, 3, *res, device=dev, generator=torch.Generator(dev).manual_seed(3))
    return sc, st, dec, target, res, Gaussians


def test_gradient_through_the_rasterizer_equals_the_torch_restatement():
    """loss_mse (fused in the composite kernels) + LossDepth on the HIP route, against loss_mse + the torch restatement on `out.depth`: both
    runs share the composite backward, only g_depth differs"""
    from tests.gpu_utils import assert_close_rel
    dev = torch.device("cuda:0")
    sc, st, dec, target, res, Gaussians = _scene(dev)
    cfg = losses.LossDepthCfg(sigma_image=10.0)
    batch = {"target": {"near": st("near"), "far": st("far"), "image": target}}

    def run(hip):
        g = Gaussians(*(st(n).requires_grad_(True) for n in ("means", "covariances", "harmonics", "opacities")))
        out = dec.forward(g, st("extrinsics"), st("intrinsics"), st("near"), st("far"), res, mse_target=target)
        n0 = losses.CALLS["depth_hip_bwd"]
        if hip:
            extra = losses.LossDepth(cfg)(out, batch, g, 0)
        else:
            extra = losses.depth_smoothness_expression(out.depth, st("near"), st("far"), target, cfg.weight, cfg.sigma_image, cfg.use_second_derivative)
        grads = torch.autograd.grad(out.loss_mse + extra, (g.means, g.covariances, g.harmonics, g.opacities))
        assert losses.CALLS["depth_hip_bwd"] == n0 + int(hip)
        return float(extra), [x.detach().cpu().numpy() for x in grads]

    (va, a), (vb, b) = run(True), run(False)
    print(f"depth loss on the rendered depth: HIP {va:.9f}, torch fp32 {vb:.9f}")
    assert va > 0 and abs(va - vb) <= value_tolerance(cfg.weight, cfg.sigma_image)
    for x, y, name in zip(a, b, ("means", "cov", "sh", "opac")):
        assert np.abs(y).max() > 0
        assert_close_rel(x, y, 1e-4, f"LossDepth through the rasterizer d{name}")


def test_train_step_with_the_depth_loss():
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
    cfg = losses.LossDepthCfg(sigma_image=10.0)
    step = TrainStep(enc, dec, lr=5e-4, clip=0.5, extra_losses=[losses.LossDepth(cfg)])
    b, v, vt, H = 1, 2, 2, 64
    sc = make_scene(n_ctx=2, grid_hw=(8, 8), n_views=vt, image_hw=(H, H), seed=3)
    ex = lambda t: t.to(dev)[None].expand(b, *t.shape).contiguous()
    g = torch.Generator(dev).manual_seed(1)
    batch = dict(context=dict(image=torch.rand(b, v, 3, H, H, device=dev, generator=g) * 2 - 1, intrinsics=ex(sc.intrinsics[:1].expand(v, 3, 3))),
                 target=dict(image=torch.rand(b, vt, 3, H, H, device=dev, generator=g) * 0.5 + 0.25, extrinsics=ex(sc.extrinsics),
                             intrinsics=ex(sc.intrinsics), near=ex(sc.near), far=ex(sc.far)))
    tgt = batch["target"]
    with torch.no_grad():                                                  # [mse] + depth evaluated separately, on the weights the step starts from
        _, out = step._render(batch["context"], {"image": batch["context"]["image"][:, 0]}, tgt, tgt["image"])
        depth_term = losses.depth_smoothness_expression(out.depth.double().cpu(), tgt["near"].double().cpu(), tgt["far"].double().cpu(),
                                                        tgt["image"].double().cpu(), cfg.weight, cfg.sigma_image, cfg.use_second_derivative)
        want = float(out.loss_mse) + float(depth_term)
    before = enc.downstream_head1.dpt.head[4].weight.detach().clone()
    n0 = dict(losses.CALLS)
    total = step(batch)
    print(f"train step total {float(total):.9f}, [mse] {float(out.loss_mse):.9f} + depth {float(depth_term):.9f}")
    assert torch.isfinite(total) and float(depth_term) > 0
    assert abs(float(total) - want) <= value_tolerance(cfg.weight, cfg.sigma_image)
    assert losses.CALLS["depth_hip_fwd"] == n0["depth_hip_fwd"] + 1 and losses.CALLS["depth_hip_bwd"] == n0["depth_hip_bwd"] + 1
    assert not torch.equal(enc.downstream_head1.dpt.head[4].weight, before)
    # the same step object with what TrainStep(losses=get_losses([...])) stores: the registry's list, nothing fused into the composite kernels
    step.losses, step.extra_losses = losses.get_losses([losses.LossMseCfg(), cfg]), []
    assert torch.isfinite(step(batch)) and losses.CALLS["depth_hip_bwd"] == n0["depth_hip_bwd"] + 2
