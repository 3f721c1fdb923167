"""-m gpu: LPIPS-VGG on the HIP kernels (csrc/vit_lpips.hip): the fused tail vit_lpips_fwd / _bwd against the torch expression in
float64, the whole LPIPS module against itself in float64 in each split-arithmetic mode, LossLpips on the device, and the train step's
`[mse, lpips]` (`extra_losses`) against the unfused `losses=[LossMse(), LossLpips()]`."""
import copy
from types import SimpleNamespace

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
CHANNELS = (64, 128, 256, 512, 512)


def _ref_tail(fa, fb, ws, relu):
    """losses.LPIPS.forward's tail in float64 (the norm clamped away from 0 so that an all-zero pixel differentiates like the kernel:
    the Jacobian of a / (|a| + 1e-10) at 0 is I / 1e-10; the plain expression gives 0 * inf there)"""
    total = 0
    for a, b, w in zip(fa, fb, ws):
        if relu:
            a, b = torch.relu(a), torch.relu(b)
        a = a / (a.pow(2).sum(1, keepdim=True).clamp_min(1e-300).sqrt() + 1e-10)
        b = b / (b.pow(2).sum(1, keepdim=True).clamp_min(1e-300).sqrt() + 1e-10)
        total = total + ((a - b) ** 2 * w.view(1, -1, 1, 1)).sum(1).mean(dim=(1, 2))
    return total


def _taps(N, sizes, case, gen):
    fa, fb = [], []
    for C, (H, W) in zip(CHANNELS, sizes):
        b = torch.randn(N, C, H, W, device=DEV, generator=gen, dtype=torch.float64)
        if case == "near":                                  # prediction = target (1 + 1e-3 noise): the late-training regime
            a = b * (1 + 1e-3 * torch.randn(b.shape, device=DEV, generator=gen, dtype=torch.float64))
        else:
            a = torch.randn(N, C, H, W, device=DEV, generator=gen, dtype=torch.float64)
        if case == "zeros":                                 # all-zero pixels: on both sides (the 1e-10 path) and on the target only
            a[:, :, 0, 0] = 0; b[:, :, 0, 0] = 0
            b[:, :, -1, -1] = 0
        fa.append(a.float().double()); fb.append(b.float().double())
    return fa, fb


SIZES = {"odd": [(7, 11), (8, 8), (5, 3), (4, 4), (3, 3)], "small": [(16, 16), (8, 8), (4, 4), (2, 2), (1, 1)]}


@pytest.mark.parametrize("N,sizes,case,relu", [
    (1, "odd", "plain", False), (1, "odd", "plain", True), (40, "small", "plain", True), (40, "small", "plain", False),
    (3, "odd", "zeros", False), (40, "small", "zeros", True), (2, "odd", "near", False), (40, "small", "near", True), (1, "odd", "near", True)])
def test_lpips_tail_matches_float64(N, sizes, case, relu):
    from styl3r_amd import vit_ops
    gen = torch.Generator(DEV).manual_seed(7 + N)
    fa64, fb64 = _taps(N, SIZES[sizes], case, gen)
    ws64 = [torch.rand(C, device=DEV, generator=gen, dtype=torch.float64).float().double() for C in CHANNELS]
    g64 = torch.randn(N, device=DEV, generator=gen, dtype=torch.float64).float().double()
    fa = [t.float().requires_grad_(True) for t in fa64]
    fb = [t.float() for t in fb64]
    ws = [w.float() for w in ws64]
    before = dict(vit_ops.CALLS)
    d = vit_ops.lpips_tail(fa, fb, ws, relu_in=relu)
    d.backward(g64.float())
    assert vit_ops.CALLS["lpips_hip_fwd"] == before["lpips_hip_fwd"] + 1 and vit_ops.CALLS["lpips_hip_bwd"] == before["lpips_hip_bwd"] + 1
    ra = [t.clone().requires_grad_(True) for t in fa64]
    r = _ref_tail(ra, fb64, ws64, relu)
    r.backward(g64)
    rel = float(((d.double() - r).abs() / r.abs()).max())
    assert rel <= 1e-4, (case, rel)
    for k, (x, y) in enumerate(zip(fa, ra)):
        err = float((x.grad.double() - y.grad).abs().max())
        assert err <= 1e-5 * float(y.grad.abs().max()), (case, k, err, float(y.grad.abs().max()))
    # two launches on the same inputs: bit-identical distances and gradients
    fa2 = [t.detach().clone().requires_grad_(True) for t in fa]
    d2 = vit_ops.lpips_tail(fa2, fb, ws, relu_in=relu)
    d2.backward(g64.float())
    assert torch.equal(d2, d) and all(torch.equal(x.grad, y.grad) for x, y in zip(fa, fa2))


def test_maxpool2x2_matches_the_framework():
    from styl3r_amd import vit_ops
    gen = torch.Generator(DEV).manual_seed(3)
    x = torch.randn(3, 5, 12, 10, device=DEV, generator=gen)
    x[0, 0, :2, :2] = 1.5                                    # a tie: the first element in row-major order takes the gradient
    x[1, 1, 2:4, 2:4] = torch.tensor([[0.0, 2.0], [2.0, 1.0]], device=DEV)
    xa, xb = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
    before = dict(vit_ops.CALLS)
    ya, yb = vit_ops.maxpool2x2(xa), torch.nn.functional.max_pool2d(xb, 2, 2)
    g = torch.randn(ya.shape, device=DEV, generator=gen)
    ya.backward(g); yb.backward(g)
    assert torch.equal(ya, yb) and torch.equal(xa.grad, xb.grad)
    assert vit_ops.CALLS["maxpool_hip_fwd"] == before["maxpool_hip_fwd"] + 1 and vit_ops.CALLS["maxpool_hip_bwd"] == before["maxpool_hip_bwd"] + 1
    odd = torch.randn(1, 2, 5, 6, device=DEV)                # odd sizes: the framework's kernel
    assert torch.equal(vit_ops.maxpool2x2(odd), torch.nn.functional.max_pool2d(odd, 2, 2))
    assert vit_ops.CALLS["framework_maxpool"] == before["framework_maxpool"] + 1


def _he_lpips(seed):
    from styl3r_amd.losses import LPIPS
    torch.manual_seed(seed)
    m = LPIPS()
    with torch.no_grad():
        for mod in m.net.modules():
            if isinstance(mod, torch.nn.Conv2d):
                fan_in = mod.weight[0].numel()
                mod.weight.normal_(0, (2.0 / fan_in) ** 0.5)
                mod.bias.normal_(0, 0.01)
        for k in range(5):
            getattr(m, f"lin{k}").model[1].weight.uniform_(0, 1)
    return m.eval().requires_grad_(False)


class _OpCounter(torch.utils._python_dispatch.TorchDispatchMode):
    def __init__(self):
        super().__init__()
        self.ops = []

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        self.ops.append(str(func.overloadpacket))
        return func(*args, **(kwargs or {}))


@pytest.mark.parametrize("shape", [(8, 64), (2, 256)])
@pytest.mark.parametrize("mode", ["bf16x6", "bf16x3", "f16x3"])
def test_lpips_module_on_the_kernels_matches_float64(mode, shape, monkeypatch):
    from styl3r_amd import vit_ops
    n, hw = shape
    m = _he_lpips(11).to(DEV)
    ref = copy.deepcopy(m).double()
    gen = torch.Generator(DEV).manual_seed(hw + n)
    tgt = torch.rand(n, 3, hw, hw, device=DEV, generator=gen)
    pred = (tgt + 0.1 * torch.randn(tgt.shape, device=DEV, generator=gen)).clamp(0, 1)
    monkeypatch.setattr(vit_ops, "LINEAR_MODE", mode)
    x = pred.clone().requires_grad_(True)
    before = dict(vit_ops.CALLS)
    with _OpCounter() as ops:
        d = m(x, tgt, normalize=True)
    d.sum().backward()
    took = {k: vit_ops.CALLS[k] - before[k] for k in vit_ops.CALLS}
    assert took["lpips_hip_fwd"] == 1 and took["lpips_hip_bwd"] == 1, took
    assert took["maxpool_hip_fwd"] == 8 and took["maxpool_hip_bwd"] == 4 and took["framework_maxpool"] == 0, took
    assert took["conv_x6_fwd"] == 22, took                 # conv2_1 .. conv5_3 on both sides (conv1_x: the library)
    assert not any("max_pool" in o for o in ops.ops) and ops.ops.count("aten.relu") == 2, sorted(set(ops.ops))   # relu in front of conv1_2, per side
    x64 = pred.double().requires_grad_(True)
    d64 = ref(x64, tgt.double(), normalize=True)
    d64.sum().backward()
    rel = float(((d.double() - d64).abs() / d64.abs()).max())
    assert rel <= (1e-3 if mode == "bf16x3" else 1e-4), (mode, rel)
    err = float((x.grad.double() - x64.grad).abs().max() / x64.grad.abs().max())
    # the input gradient crosses 13 ReLUs and 4 max-pools: an activation (or a 2 x 2 window's runner-up) within the arithmetic's round-off of
    # zero (of the maximum) takes another branch than in fp64.  bf16x3 rounds each product at 2^-16: such flips then move the gradient
    # of whole pixels, in the plain expression on the same bf16x3 convolutions as much as here, so that expression is its yardstick too
    err_mode = 0.0
    if mode == "bf16x3":
        xm = pred.clone().requires_grad_(True)
        m._forward_expression(2 * xm - 1, 2 * tgt - 1).sum().backward()
        err_mode = float((xm.grad.double() - x64.grad).abs().max() / x64.grad.abs().max())
    monkeypatch.setattr(vit_ops, "LINEAR_MODE", "f32")     # the framework's fp32 path: the expression on the library convolutions
    x32 = pred.clone().requires_grad_(True)
    m(x32, tgt, normalize=True).sum().backward()
    err_lib = float((x32.grad.double() - x64.grad).abs().max() / x64.grad.abs().max())
    assert err <= max(1e-4, 3 * err_lib, 3 * err_mode), (mode, err, err_lib, err_mode)


def test_loss_lpips_gating_and_identity_on_the_gpu():
    from styl3r_amd import vit_ops
    from styl3r_amd.losses import LossLpips, LossLpipsCfg
    loss = LossLpips(LossLpipsCfg(weight=0.05, apply_after_step=10), _he_lpips(2)).to(DEV)
    img = torch.rand(1, 2, 3, 32, 32, device=DEV)
    batch = {"target": {"image": img}}
    pred = SimpleNamespace(color=img.clone().requires_grad_(True))
    before = vit_ops.CALLS["lpips_hip_fwd"]
    assert float(loss(pred, batch, None, 5)) == 0.0 and vit_ops.CALLS["lpips_hip_fwd"] == before
    assert abs(float(loss(pred, batch, None, 10))) < 1e-12 and vit_ops.CALLS["lpips_hip_fwd"] == before + 1
    other = SimpleNamespace(color=(img * 0.5).requires_grad_(True))
    val = loss(other, batch, None, 10)
    val.backward()
    assert torch.isfinite(val) and float(val) > 0 and other.color.grad.abs().sum() > 0 and torch.isfinite(other.color.grad).all()


def _tiny_setup(seed=0):
    from styl3r_amd.decoder import DecoderSplattingCUDACfg, get_decoder
    from styl3r_amd.encoder import EncoderNoPoSplatMultiTokenStyle, EncoderNoPoSplatTokenStyleCfg
    from styl3r_amd.scenes import make_scene
    torch.manual_seed(seed)
    tiny = dict(enc_depth=1, dec_depth=12, enc_embed_dim=1024, dec_embed_dim=128, enc_num_heads=16, dec_num_heads=2,
                pos_embed="RoPE100", img_size=(512, 512))
    enc = EncoderNoPoSplatMultiTokenStyle(EncoderNoPoSplatTokenStyleCfg(stylized=False), trunk_params=tiny).to(DEV).eval()
    with torch.no_grad():
        for h in (enc.downstream_head1, enc.downstream_head2):
            h.dpt.head[4].bias.copy_(torch.tensor([0.0, 0.0, 1.2], device=DEV))
    dec = get_decoder(DecoderSplattingCUDACfg("splatting_cuda", [0.0, 0.0, 0.0], True)).to(DEV)
    b, v, vt, H = 2, 2, 2, 64
    sc = make_scene(n_ctx=2, grid_hw=(8, 8), n_views=vt, image_hw=(H, H), seed=3)
    ex = lambda t: t.to(DEV)[None].expand(b, *t.shape).contiguous()
    g = torch.Generator(DEV).manual_seed(1)
    batch = dict(context=dict(image=torch.rand(b, v, 3, H, H, device=DEV, generator=g) * 2 - 1, intrinsics=ex(sc.intrinsics[:1].expand(v, 3, 3))),
                 target=dict(image=torch.rand(b, vt, 3, 8, 8, device=DEV, generator=g).repeat_interleave(8, -1).repeat_interleave(8, -2) * 0.5 + 0.25,
                             extrinsics=ex(sc.extrinsics), intrinsics=ex(sc.intrinsics), near=ex(sc.near), far=ex(sc.far)))
    return enc, dec, batch


def test_train_step_mse_plus_lpips_equals_the_unfused_losses():
    """TrainStep(extra_losses=[LossLpips()]): MSE inside the composite kernels, LPIPS's image gradient added in the same composite
    backward -- the same loss and encoder gradients as losses=[LossMse(), LossLpips()] (MSE on its own kernels, the image gradient summed
    by autograd)"""
    from styl3r_amd import vit_ops
    from styl3r_amd.losses import LossLpips, LossMse
    from styl3r_amd.train import TrainStep
    enc, dec, batch = _tiny_setup()
    enc2, enc3 = copy.deepcopy(enc), copy.deepcopy(enc)
    lp = LossLpips(lpips=_he_lpips(4)).to(DEV)
    before = vit_ops.CALLS["lpips_hip_bwd"]
    with pytest.raises(ValueError):
        TrainStep(enc2, dec, losses=[LossMse()], extra_losses=[lp])
    fused = TrainStep(enc, dec, lr=5e-4, clip=None, extra_losses=[lp])
    plain = TrainStep(enc2, dec, lr=5e-4, clip=None, losses=[LossMse(), lp])
    again = TrainStep(enc3, dec, lr=5e-4, clip=None, losses=[LossMse(), lp])
    l1, l2, l3 = float(fused(batch)), float(plain(batch)), float(again(batch))
    assert vit_ops.CALLS["lpips_hip_bwd"] == before + 3
    assert abs(l1 - l2) <= 1e-5 * abs(l2), (l1, l2, l3)
    n_cmp = 0
    top = max(float(p.grad.abs().max()) for p in enc2.parameters() if p.grad is not None)
    for (name, p1), p2, p3 in zip(enc.named_parameters(), enc2.parameters(), enc3.parameters()):
        if p1.grad is None:
            assert p2.grad is None or float(p2.grad.abs().max()) == 0.0, name
            continue
        scale = float(p2.grad.abs().max())
        err, noise = float((p1.grad - p2.grad).abs().max()), float((p3.grad - p2.grad).abs().max())
        # noise: two runs of the SAME unfused step differ by this much where a kernel of the step is not run-to-run reproducible.  The
        # two image gradients differ by fp32 rounding, which reaches every parameter as an error of the size of the whole backward's
        # magnitudes: a tensor whose gradient is ~1e-5 of the largest (cancellation) sees it as ~1e-4 of its own max -- hence the floor
        assert err <= 1e-4 * scale + 1e-7 * top + noise, (name, err, noise, scale, top)
        n_cmp += 1
    assert n_cmp > 50


def test_train_step_with_lpips_reduces_the_loss():
    """the criterion of test_train_step.py::test_nvs_training_reduces_the_loss_end_to_end, with `[mse, lpips]`"""
    from styl3r_amd.losses import LossLpips
    from styl3r_amd.train import TrainStep
    enc, dec, batch = _tiny_setup()
    step = TrainStep(enc, dec, lr=5e-4, clip=0.5, extra_losses=[LossLpips(lpips=_he_lpips(4)).to(DEV)])
    losses = [float(step(batch)) for _ in range(40)]
    assert all(torch.isfinite(torch.tensor(losses)))
    first, last = sum(losses[:3]) / 3, sum(losses[-3:]) / 3
    assert last < 0.9 * first, (first, last, losses[::5])
