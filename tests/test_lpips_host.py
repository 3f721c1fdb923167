"""CPU tests of the LPIPS host logic: `LPIPS.load_lpips_weights` on synthetic dicts in the `lpips` package's and torchvision's layouts,
the C ABI of the LPIPS kernels as far as it runs without a device (sizes, argument checks), and the CPU route staying the expression."""
import ctypes as C

import pytest
import torch

from styl3r_amd.losses import LPIPS

VGG16_CONVS = (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28)
WIDTHS = (64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512, 512)


def _synthetic(seed=0):
    g = torch.Generator().manual_seed(seed)
    lin = {f"lin{k}.model.1.weight": torch.rand(1, c, 1, 1, generator=g) for k, c in enumerate((64, 128, 256, 512, 512))}
    vgg, c_in = {}, 3
    for n, c in zip(VGG16_CONVS, WIDTHS):
        vgg[f"features.{n}.weight"] = torch.randn(c, c_in, 3, 3, generator=g)
        vgg[f"features.{n}.bias"] = torch.randn(c, generator=g)
        c_in = c
    vgg["classifier.0.weight"] = torch.zeros(4, 4)          # torchvision's full vgg16 state dict: the classifier is ignored
    return lin, vgg


def test_load_lpips_weights_maps_package_and_torchvision_layouts():
    lin, vgg = _synthetic()
    m = LPIPS()
    net_before = {k: v.clone() for k, v in m.state_dict().items() if k.startswith("net.")}
    m.load_lpips_weights(lin)                                # lin only: the trunk is left as it was
    sd = m.state_dict()
    assert all(torch.equal(sd[k], v) for k, v in lin.items())
    assert all(torch.equal(sd[k], v) for k, v in net_before.items())
    m.load_lpips_weights(lin, vgg)
    sd = m.state_dict()
    slices = {0: 1, 2: 1, 5: 2, 7: 2, 10: 3, 12: 3, 14: 3, 17: 4, 19: 4, 21: 4, 24: 5, 26: 5, 28: 5}
    expected = dict(lin)
    for n, s in slices.items():
        expected[f"net.slice{s}.{n}.weight"] = vgg[f"features.{n}.weight"]
        expected[f"net.slice{s}.{n}.bias"] = vgg[f"features.{n}.bias"]
    assert set(sd) == set(expected)
    assert all(torch.equal(sd[k], v) for k, v in expected.items())


def test_load_lpips_weights_rejects_missing_and_extra_keys():
    lin, vgg = _synthetic()
    m = LPIPS()
    with pytest.raises(KeyError, match="missing"):
        m.load_lpips_weights({k: v for k, v in lin.items() if k != "lin3.model.1.weight"})
    with pytest.raises(KeyError, match="unexpected"):
        m.load_lpips_weights({**lin, "lin5.model.1.weight": torch.zeros(1, 8, 1, 1)})
    with pytest.raises(KeyError, match="missing"):
        m.load_lpips_weights(lin, {k: v for k, v in vgg.items() if k != "features.19.bias"})
    with pytest.raises(KeyError, match="unexpected"):
        m.load_lpips_weights(lin, {**vgg, "features.30.weight": torch.zeros(1)})
    with pytest.raises(RuntimeError):                        # a shape that does not fit
        m.load_lpips_weights({**lin, "lin0.model.1.weight": torch.zeros(1, 65, 1, 1)})


def test_cpu_route_is_the_expression():
    """CPU tensors (and the f32 mode) keep the plain torch expression: no kernel counter moves"""
    from styl3r_amd import vit_ops
    torch.manual_seed(0)
    m = LPIPS().eval()
    a, b = torch.rand(2, 3, 32, 32), torch.rand(2, 3, 32, 32)
    before = dict(vit_ops.CALLS)
    d = m(a, b, normalize=True)
    assert d.shape == (2, 1, 1, 1) and vit_ops.CALLS == before
    fa, fb = m.net((2 * a - 1 - m.shift) / m.scale), m.net((2 * b - 1 - m.shift) / m.scale)
    want = 0
    for k, (x, y) in enumerate(zip(fa, fb)):
        x = x / (x.pow(2).sum(1, keepdim=True).sqrt() + 1e-10)
        y = y / (y.pow(2).sum(1, keepdim=True).sqrt() + 1e-10)
        want = want + (getattr(m, f"lin{k}").model[1].weight * (x - y) ** 2).sum(1, keepdim=True).mean(dim=(2, 3), keepdim=True)
    assert torch.allclose(d, want, rtol=1e-5, atol=0)
    assert torch.equal(vit_ops.maxpool2x2(a), torch.nn.functional.max_pool2d(a, 2, 2))


def test_lpips_kernel_sizes_and_argument_checks_without_a_gpu():
    from styl3r_amd import vit_ops
    vit_ops.build_library()
    lib = vit_ops.load()
    one = C.c_void_p(16)                                     # (any non-null value: validation only, nothing is dereferenced)
    sizes = [(256, 256), (128, 128), (64, 64), (32, 32), (16, 16)]
    taps = (vit_ops.VitLpipsTap * 5)(*[vit_ops.VitLpipsTap(16, 16, 16, 16, c, h, w) for c, (h, w) in zip((64, 128, 256, 512, 512), sizes)])
    blocks = sum((h * w + 255) // 256 for h, w in sizes)     # one 64-lane workgroup per 256 pixels of one image of one tap
    assert blocks == 341
    assert lib.vit_lpips_scratch_bytes(taps, 5, 40) == 4 * 40 * blocks
    assert lib.vit_lpips_stats_bytes(taps, 5, 40) == 16 * 40 * sum(h * w for h, w in sizes)     # 16 B per pixel: 55.9 MB at 40 x 256^2
    odd = (vit_ops.VitLpipsTap * 1)(vit_ops.VitLpipsTap(16, 16, 16, 16, 8, 7, 11))
    assert lib.vit_lpips_stats_bytes(odd, 1, 3) == 16 * 3 * 80                       # planes padded to a multiple of 4 pixels
    assert lib.vit_lpips_fwd(None, 5, 40, 1, one, one, None, None) == -1
    assert lib.vit_lpips_fwd(taps, 6, 40, 1, one, one, None, None) == -1              # at most five taps
    assert lib.vit_lpips_fwd(taps, 5, 0, 1, one, one, None, None) == -1
    assert lib.vit_lpips_fwd(taps, 5, 40, 1, None, one, None, None) == -1             # no output
    assert lib.vit_lpips_fwd(taps, 5, 40, 1, one, one, C.c_void_p(20), None) == -1    # misaligned statistics
    bad = (vit_ops.VitLpipsTap * 1)(vit_ops.VitLpipsTap(16, None, 16, 16, 8, 4, 4))
    assert lib.vit_lpips_fwd(bad, 1, 1, 0, one, one, None, None) == -1                # no target tap
    nodfa = (vit_ops.VitLpipsTap * 1)(vit_ops.VitLpipsTap(16, 16, 16, None, 8, 4, 4))
    assert lib.vit_lpips_bwd(nodfa, 1, 1, 0, one, one, None) == -1                    # the backward needs its output
    assert lib.vit_lpips_bwd(taps, 5, 40, 1, None, one, None) == -1                   # no upstream gradient
    assert lib.vit_maxpool2x2_fwd(one, one, 4, 5, 6, None) == -1                      # odd height
    assert lib.vit_maxpool2x2_fwd(one, one, 4, 6, 7, None) == -1                      # odd width
    assert lib.vit_maxpool2x2_bwd(one, one, None, 4, 6, 6, None) == -1
    for key in ("lpips_hip_fwd", "lpips_hip_bwd", "maxpool_hip_fwd", "maxpool_hip_bwd"):
        assert key in vit_ops.CALLS


def test_train_step_takes_extra_losses_only_on_top_of_the_default_mse():
    from styl3r_amd.losses import LossLpips, LossMse
    from styl3r_amd.train import TrainStep
    with pytest.raises(ValueError, match="extra_losses"):
        TrainStep(torch.nn.Linear(2, 2), None, losses=[LossMse()], extra_losses=[LossLpips()])


def test_preactivation_taps_are_the_taps_before_their_relu():
    """the device route's VGG16 (ReLUs folded into the next convolution, max-pool on pre-activations) computes the same taps: on the CPU
    every piece is the framework op, so relu(preacts) equals the expression's features"""
    torch.manual_seed(1)
    m = LPIPS().eval()
    x = torch.randn(2, 3, 32, 32)
    with torch.no_grad():
        for got, want in zip(m.net.preacts(x), m.net(x)):
            assert torch.allclose(torch.relu(got), want, rtol=1e-5, atol=1e-6)
