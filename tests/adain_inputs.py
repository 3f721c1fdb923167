"""Inputs of the 2D-AdaIN baseline tests (tests/golden/make_adain_fixtures.py, test_adain_host.py, test_gpu_adain.py): the weights of the
eighteen convolutions and the images, shared by the generator and the tests so that no weight is stored.

Every number is a closed form of (a tag, the flat index): a 64-bit integer mix (the finaliser of splitmix64) of `tag * 2^40 + index`, whose
top 53 bits are a double in [0, 1).  Integer arithmetic only, so the values are bit-identical on every platform and numpy version -- no RNG
stream, no libm.  The weights are variance-scaled for ReLU (uniform with variance 2 / fan_in), so activations neither die nor explode over
the 21 layers.  Two layers deviate, for the conditions the generator asserts:
  * conv4_1 (the layer in front of relu4_1) has bias RELU41_BIAS: relu4_1 of a 16 x 16 image is 2 x 2, and with a zero-mean
    pre-activation a channel can be negative at all four positions -- content std 0, which AdaIN divides by.  The bias keeps the
    pre-activations positive (their std is ~1), so every channel keeps the spread of its pre-activation;
  * rc9 is scaled by RC9_GAIN.  The maps in front of it are positive with a mean several times their spread, so each output channel is an
    offset of a few units (at gain 1) plus a spatial part a tenth of that; the gain brings the offsets of all three channels inside the
    range that de-normalises into (0, 1), so that no channel is clamped flat and the clamp cannot hide an error.
"""
import functools

import numpy as np
import torch

# torchvision's layer index, c_in, c_out of vgg19().features[:21], and the reference's slice of each (vgg_model.py:83-86)
VGG_CONVS = ((0, 3, 64), (2, 64, 64), (5, 64, 128), (7, 128, 128), (10, 128, 256), (12, 256, 256), (14, 256, 256), (16, 256, 256), (19, 256, 512))
SLICE_OF = {0: 1, 2: 2, 5: 2, 7: 3, 10: 3, 12: 4, 14: 4, 16: 4, 19: 4}
DECODER_CONVS = ((512, 256), (256, 256), (256, 256), (256, 256), (256, 128), (128, 128), (128, 64), (64, 64), (64, 3))
IMAGENET_MEAN, IMAGENET_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
RELU41_BIAS = 4.0
RC9_GAIN = 0.1
# scene -> (views, H, W, style h, style w): A has relu4_1 of 2 x 2, the smallest size reflection allows; B has an odd 3 x 5 relu4_1 and a last
# decoder frame (24 x 40) that crosses the 32-pixel tile edge with a ragged 8-pixel tile
SCENES = {"A": (4, 16, 16, 16, 16), "B": (2, 24, 40, 32, 16)}
_M64 = np.uint64(0xFFFFFFFFFFFFFFFF)


def unit(tag: int, n: int) -> np.ndarray:
    """n doubles in [0, 1): the closed form above for indices 0 .. n - 1"""
    with np.errstate(over="ignore"):
        z = (np.arange(n, dtype=np.uint64) + np.uint64(tag) * np.uint64(1 << 40) + np.uint64(0x9E3779B97F4A7C15)) & _M64
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return (z >> np.uint64(11)).astype(np.float64) * (1.0 / (1 << 53))


def _u(tag, shape, lo=0.0, hi=1.0):
    return unit(tag, int(np.prod(shape))).reshape(shape) * (hi - lo) + lo


def _f32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64).astype(np.float32))


def _conv(tag, ci, co, gain=1.0, bias=0.0):
    a = np.sqrt(6.0 / (ci * 9)) * gain                      # uniform(-a, a): variance 2 / fan_in
    return _f32(_u(2 * tag, (co, ci, 3, 3), -a, a)), _f32(_u(2 * tag + 1, (co,), -0.05, 0.05) + bias)


@functools.lru_cache(maxsize=None)
def reference_state_dict() -> dict:
    """fp32 weights under the reference AdaIN2D's keys: `vgg_encoder.slice{s}.{N}.weight / .bias`, `decoder.rc{k}.conv.weight / .bias`"""
    sd = {}
    for idx, ci, co in VGG_CONVS:
        w, b = _conv(100 + idx, ci, co, bias=RELU41_BIAS if idx == 19 else 0.0)
        sd[f"vgg_encoder.slice{SLICE_OF[idx]}.{idx}.weight"], sd[f"vgg_encoder.slice{SLICE_OF[idx]}.{idx}.bias"] = w, b
    for k, (ci, co) in enumerate(DECODER_CONVS, 1):
        w, b = _conv(200 + k, ci, co, gain=RC9_GAIN if k == 9 else 1.0)
        sd[f"decoder.rc{k}.conv.weight"], sd[f"decoder.rc{k}.conv.bias"] = w, b
    return sd


def images(scene: str):
    """targets (v, 3, H, W) and the style (3, hs, ws) of a scene in [0, 1], fp32: coarse blocks plus pixel noise"""
    v, H, W, hs, ws = SCENES[scene]
    t = 2000 + 10 * sorted(SCENES).index(scene)
    target = np.clip(np.kron(_u(t, (v, 3, H // 4, W // 4)), np.ones((4, 4))) * 0.7 + 0.3 * _u(t + 1, (v, 3, H, W)), 0, 1)
    style = np.clip(np.kron(_u(t + 2, (3, hs // 2, ws // 2)), np.ones((2, 2))) * 0.6 + 0.4 * _u(t + 3, (3, hs, ws)), 0, 1)
    return _f32(target), _f32(style)


def conv_case(tag: int, B: int, Ci: int, Co: int, h: int, w: int, Ho: int, Wo: int):
    """x (B, Ci, h, w) sign-changing with exact zeros' neighbourhood (a ReLU matters), weight (Co, Ci, 3, 3), bias (Co), residual
    (B, Co, Ho, Wo); fp32 CPU tensors"""
    a, t = np.sqrt(6.0 / (Ci * 9)), 3000 + 4 * tag
    return (_f32(_u(t, (B, Ci, h, w), -1.0, 1.5)), _f32(_u(t + 1, (Co, Ci, 3, 3), -a, a)), _f32(_u(t + 2, (Co,), -0.5, 0.5)),
            _f32(_u(t + 3, (B, Co, Ho, Wo), -1.0, 1.0)))


def adain_case(tag: int, B: int, Bs: int, C: int, N: int, M: int):
    """content (B, C, N) and style (Bs, C, M) ReLU-shaped (exact zeros, a mean far from zero relative to the spread), fp32 CPU tensors"""
    relu_like = lambda t, shape: np.maximum(_u(t, shape) - 0.3, 0.0) * 3.0 + 0.01 * _u(t + 1, shape)
    return _f32(relu_like(5000 + 4 * tag, (B, C, N))), _f32(relu_like(5002 + 4 * tag, (Bs, C, M)))
