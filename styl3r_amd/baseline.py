"""The 2D-AdaIN baseline of the comparison pictures (src/test/vgg_model.py: `AdaIN2D`, `adain`, `RC`, `Decoder`; used by
model_wrapper_style.py:279-286 and :536-545 for the "2D Baseline" column): VGG19 to relu4_1, adaptive instance normalisation, a
nine-layer reflection-padded decoder with three nearest x2 upsamplings.  Its weights are the reference's `ckpts/model_state.pth`.

Route of `generate` / `stylize` on fp32 device tensors (under no_grad, in a split-arithmetic mode of vit_ops):
  * the VGG front as `losses.VGGEncoder` runs it today;
  * `vit_adain_fwd` (csrc/vit_adain.hip): two launches, the views of a scene share one style row (`style_index`);
  * rc1 .. rc8 on `vit_conv_x6_fwd` with VIT_CONV_REFLECT -- the reflection padding is an index map in the halo fetch -- plus VIT_CONV_UP2 on
    rc2, rc6 and rc8 (the nearest upsampling in front of them is an index map too) and VIT_CONV_RELU_IN from rc2 on: the ReLU behind layer
    n is the input ReLU of layer n + 1, because ReLU commutes with both index maps.  No padded, upsampled or ReLU'd map reaches memory;
  * rc9 (64 -> 3) on `vit_conv3_rgb_fwd` with RELU_IN | REFLECT; `stylize` has the de-normalisation and the clamp of `vgg_denorm` in its store.
Twelve launches behind the VGG front, plus one `vit_amax` pass in f16x3 for the AdaIN output (every later layer's input |max| is published
by the convolution in front of it).  Anything else -- CPU tensors, other dtypes, an input that requires a gradient, the library-arithmetic
mode "f32" -- is `generate_expression`, the torch restatement, which is also the float64 yardstick of the tests.  `CALLS` counts the routes.
"""
from __future__ import annotations

from typing import Optional

import torch
import torch.nn as nn
import torch.nn.functional as F
from torch import Tensor

from . import vit_ops
from .losses import CALLS, IMAGENET_MEAN, IMAGENET_STD, VGGEncoder, _adaattn_index, _imagenet_normalize, calc_mean_std

CALLS.update({"adain_hip": 0, "conv_rc_x6": 0, "conv_rgb_hip": 0, "adain2d_expression": 0})
VIT_CONV_RELU_IN, VIT_CONV_REFLECT, VIT_CONV_UP2 = 1, 4, 8        # include/vit_ops.h
ADAIN_EPS = 1e-8
# (c_in, c_out) of rc1 .. rc9 and the layers with F.interpolate(scale_factor=2) in front of them (vgg_model.py:118-144)
DECODER_LAYERS = ((512, 256), (256, 256), (256, 256), (256, 256), (256, 128), (128, 128), (128, 64), (64, 64), (64, 3))
UPSAMPLED = (2, 6, 8)
# torchvision's layer index -> the reference's slice (vgg_model.py:83-86): the keys of its VGGEncoder keep the torchvision indices
_SLICE_OF = {0: 1, 2: 2, 5: 2, 7: 3, 10: 3, 12: 4, 14: 4, 16: 4, 19: 4}


def adain_expression(content_features: Tensor, style_features: Tensor, alpha: float = 1.0, style_index: Optional[Tensor] = None) -> Tensor:
    """`adain` and the alpha blend of `AdaIN2D.generate` (vgg_model.py:29-49,156-157) as plain torch ops, in their operation order, in the
    tensors' dtype; image b takes style row `style_index[b]` (None: row b)."""
    if style_index is not None:
        style_features = style_features[style_index.to(style_features.device, torch.long)]
    b, c = content_features.shape[:2]
    shape = (b, c) + (1,) * (content_features.dim() - 2)
    c_mean, c_std = (t.reshape(shape) for t in calc_mean_std(content_features, ADAIN_EPS))
    s_mean, s_std = (t.reshape(shape) for t in calc_mean_std(style_features, ADAIN_EPS))
    t = s_std * (content_features - c_mean) / c_std + s_mean
    return alpha * t + (1 - alpha) * content_features


def adain(content_features: Tensor, style_features: Tensor, alpha: float = 1.0, style_index: Optional[Tensor] = None) -> Tensor:
    """alpha * AdaIN(content, style) + (1 - alpha) * content: content (B, C, ...), style (Bs, C, ...), image b normalised to the channel
    statistics (mean, unbiased std + 1e-8) of style row style_index[b] (None: B == Bs, row b).  fp32 device tensors that need no gradient
    run on vit_adain_fwd (and raise if libvit_hip.so is missing); anything else is `adain_expression`."""
    if content_features.dim() < 3 or style_features.dim() < 3 or content_features.shape[1] != style_features.shape[1]:
        raise ValueError(f"adain: content (B, C, ...) and style (Bs, C, ...), got {tuple(content_features.shape)}, {tuple(style_features.shape)}")
    b, c = content_features.shape[:2]
    bs = style_features.shape[0]
    if (style_index is None and b != bs) or (style_index is not None and style_index.numel() != b):
        raise ValueError(f"adain: {b} images and {bs} styles need a style_index of {b} entries")
    n, m = content_features[0, 0].numel(), style_features[0, 0].numel()
    if n < 2 or m < 2:
        raise ValueError(f"adain: the unbiased std needs at least two positions per channel, got {n} and {m}")
    hip = all(t.is_cuda and t.dtype == torch.float32 and not (t.requires_grad and torch.is_grad_enabled()) for t in (content_features, style_features))
    if not hip:
        return adain_expression(content_features, style_features, alpha, style_index)
    host, devi = _adaattn_index(style_index, b, bs, content_features.device)
    x, s = vit_ops._aligned(content_features.detach()), vit_ops._aligned(style_features.detach())
    lib = vit_ops.load()
    out = torch.empty(x.shape, dtype=torch.float32, device=x.device)
    scratch = torch.empty(lib.vit_adain_scratch_bytes(b, bs, c), dtype=torch.uint8, device=x.device)
    CALLS["adain_hip"] += 1
    vit_ops._check(lib.vit_adain_fwd(x.data_ptr(), s.data_ptr(), host.data_ptr(), devi.data_ptr(), b, bs, c, n, m, float(alpha), ADAIN_EPS,
                                     out.data_ptr(), scratch.data_ptr(), vit_ops._stream(x.device)), "vit_adain_fwd")
    return out


def conv_rc_x6(x: Tensor, weight: Tensor, bias: Optional[Tensor], up2: bool = False, relu_in: bool = False, publish: bool = False) -> Tensor:
    """conv2d(ReflectionPad2d(1)([interpolate(scale_factor=2)](relu?(x))), weight) + bias in one vit_conv_x6_fwd launch (no autograd): the
    padding and the upsampling are source modes of the kernel's halo fetch.  `publish`: f16x3 -- the launch publishes its output's |max|."""
    B, Ci, h, w = x.shape
    Co = weight.shape[0]
    H, W = (2 * h, 2 * w) if up2 else (h, w)
    x = vit_ops._aligned(x)
    out = torch.empty((B, Co, H, W), dtype=torch.float32, device=x.device)
    wp = vit_ops.split_conv_weight(weight)
    if vit_ops._f16():
        vit_ops._announce(vit_ops._amax_of(x))       # the SOURCE tensor's |max|: every value the window reads is one of its values
    pub = vit_ops._want_output_amax(x.device) if publish else None
    flags = VIT_CONV_REFLECT | (VIT_CONV_UP2 if up2 else 0) | (VIT_CONV_RELU_IN if relu_in else 0)
    CALLS["conv_rc_x6"] += 1
    vit_ops._check(vit_ops.load().vit_conv_x6_fwd(x.data_ptr(), wp.data_ptr(), bias.data_ptr() if bias is not None else None, None, out.data_ptr(),
                                                  B, Ci, Co, H, W, 3, flags, vit_ops._stream(x.device)), "vit_conv_x6_fwd (reflect)")
    if pub is not None:
        vit_ops._publish(out, pub)
    return out


def conv_rgb(x: Tensor, weight: Tensor, bias: Optional[Tensor], relu_in: bool = False, reflect: bool = True,
             scale: Optional[Tensor] = None, shift: Optional[Tensor] = None, lo: float = 0.0, hi: float = 1.0) -> Tensor:
    """3 x 3 convolution to at most four channels on vit_conv3_rgb_fwd (exact fp32 FMAs, no autograd): conv(pad(relu?(x))) + bias, then
    clamp(y * scale[co] + shift[co], lo, hi) when `scale` is given."""
    B, Ci, H, W = x.shape
    Co = weight.shape[0]
    x, wt = vit_ops._aligned(x), vit_ops._aligned(weight.detach())
    out = torch.empty((B, Co, H, W), dtype=torch.float32, device=x.device)
    flags = (VIT_CONV_RELU_IN if relu_in else 0) | (VIT_CONV_REFLECT if reflect else 0)
    CALLS["conv_rgb_hip"] += 1
    vit_ops._check(vit_ops.load().vit_conv3_rgb_fwd(x.data_ptr(), wt.data_ptr(), bias.data_ptr() if bias is not None else None,
                                                    scale.data_ptr() if scale is not None else None, shift.data_ptr() if shift is not None else None,
                                                    float(lo), float(hi), out.data_ptr(), B, Ci, Co, H, W, flags, vit_ops._stream(x.device)),
                   "vit_conv3_rgb_fwd")
    return out


def _to_buffers(module: nn.Module) -> None:
    """the reference's convert_to_buffer: every parameter becomes a buffer of the same name (same state-dict keys; nothing trains)"""
    for m in module.modules():
        for name, p in list(m._parameters.items()):
            if p is not None:
                del m._parameters[name]
                m.register_buffer(name, p.detach())


class RC(nn.Module):
    """ReflectionPad2d(1) + Conv2d(3) [+ ReLU] (vgg_model.py:101-115); keys `conv.weight`, `conv.bias`"""

    def __init__(self, in_channels: int, out_channels: int, activated: bool = True):
        super().__init__()
        self.conv = nn.Conv2d(in_channels, out_channels, 3)
        self.activated = activated

    def forward(self, x: Tensor) -> Tensor:
        h = F.conv2d(F.pad(x, (1, 1, 1, 1), mode="reflect"), self.conv.weight, self.conv.bias)
        return F.relu(h) if self.activated else h


class Decoder(nn.Module):
    """rc1 .. rc9 with nearest x2 upsampling in front of rc2, rc6 and rc8 (vgg_model.py:118-144): the torch expression"""

    def __init__(self):
        super().__init__()
        for k, (ci, co) in enumerate(DECODER_LAYERS, 1):
            setattr(self, f"rc{k}", RC(ci, co, activated=k < len(DECODER_LAYERS)))

    def layers(self):
        return [getattr(self, f"rc{k}") for k in range(1, len(DECODER_LAYERS) + 1)]

    def forward(self, features: Tensor) -> Tensor:
        h = features
        for k, rc in enumerate(self.layers(), 1):
            if k in UPSAMPLED:
                h = F.interpolate(h, scale_factor=2)
            h = rc(h)
        return h


class AdaIN2D(nn.Module):
    """The reference's AdaIN2D for inference: `generate` and `stylize`.  The state dict has exactly the reference's keys --
    `vgg_encoder.slice{1..4}.{torchvision index}.weight / .bias` and `decoder.rc{1..9}.conv.weight / .bias` -- so `load_state_dict` of
    `ckpts/model_state.pth` loads strictly; the VGG keys are mapped onto `losses.VGGEncoder.features`.  All tensors are buffers."""

    def __init__(self):
        super().__init__()
        self.vgg_encoder = VGGEncoder()
        self.decoder = Decoder()
        _to_buffers(self)
        self.register_buffer("_denorm_scale", torch.tensor(IMAGENET_STD, dtype=torch.float32), persistent=False)
        self.register_buffer("_denorm_shift", torch.tensor(IMAGENET_MEAN, dtype=torch.float32), persistent=False)
        self._register_state_dict_hook(self._reference_keys)
        self._register_load_state_dict_pre_hook(self._package_keys)

    # ---- the reference's key layout ----
    @staticmethod
    def _reference_keys(module, state_dict, prefix, local_metadata):
        head = prefix + "vgg_encoder.features."
        items = list(state_dict.items())
        state_dict.clear()                                   # (re-filled in the original order: the reference's order of keys)
        for key, val in items:
            if key.startswith(head):
                key = f"{prefix}vgg_encoder.slice{_SLICE_OF[int(key[len(head):].split('.')[0])]}.{key[len(head):]}"
            state_dict[key] = val
        return state_dict

    @staticmethod
    def _package_keys(state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs):
        head = prefix + "vgg_encoder.slice"
        for key in [k for k in state_dict if k.startswith(head)]:
            s, rest = key[len(head):].split(".", 1)
            idx = rest.split(".")[0]
            if s.isdigit() and idx.isdigit() and _SLICE_OF.get(int(idx)) == int(s):        # (any other key stays and is reported as unexpected)
                state_dict[f"{prefix}vgg_encoder.features.{rest}"] = state_dict.pop(key)

    # ---- the network ----
    def _hip_ok(self, *tensors: Tensor) -> bool:
        return all(t.is_cuda and t.dtype == torch.float32 and not (t.requires_grad and torch.is_grad_enabled()) for t in tensors) and vit_ops._x6()

    def generate_expression(self, content_images: Tensor, style_images: Tensor, alpha: float = 1.0, style_index: Optional[Tensor] = None,
                            denorm: bool = False) -> Tensor:
        """`generate` as the reference states it, in the dtype of the module's tensors (call `.double()` first for the float64 yardstick):
        framework pad, conv2d, relu and interpolate.  `denorm`: vgg_denorm (clamp(x * std + mean, 0, 1)) applied to the result."""
        t = adain_expression(self._encode_plain(content_images), self._encode_plain(style_images), alpha, style_index)
        out = self.decoder(t)
        if denorm:
            out = torch.clamp(out * self._denorm_scale.to(out.dtype).view(1, 3, 1, 1) + self._denorm_shift.to(out.dtype).view(1, 3, 1, 1), 0, 1)
        return out

    def _encode_plain(self, x: Tensor) -> Tensor:
        """relu4_1 through the framework's own convolutions (no split-arithmetic kernels), on any device"""
        for m in self.vgg_encoder.features:
            x = F.conv2d(x, m.weight, m.bias, padding=1) if isinstance(m, nn.Conv2d) else m(x)
        return x

    def _decode_hip(self, t: Tensor, denorm: bool) -> Tensor:
        rcs = self.decoder.layers()
        h = t
        for k, rc in enumerate(rcs[:-1], 1):
            h = conv_rc_x6(h, rc.conv.weight, rc.conv.bias, up2=k in UPSAMPLED, relu_in=k > 1, publish=k < len(rcs) - 1)
        last = rcs[-1].conv
        return conv_rgb(h, last.weight, last.bias, relu_in=True, reflect=True, scale=self._denorm_scale if denorm else None,
                        shift=self._denorm_shift if denorm else None)

    def _decode_materialised(self, t: Tensor, denorm: bool) -> Tensor:
        """the same decoder with every padded, upsampled and ReLU'd map in memory: framework pad / interpolate / relu around
        vit_ops.conv_x6_forward on the padded map, cropped by one pixel (what the package could do before the source modes).  The A/B
        partner of `_decode_hip` in tests and tools/bench_adain.py; nothing routes here."""
        rcs = self.decoder.layers()
        h = t
        for k, rc in enumerate(rcs, 1):
            if k in UPSAMPLED:
                h = F.interpolate(h, scale_factor=2)
            hp = F.pad(h, (1, 1, 1, 1), mode="reflect")
            if k < len(rcs):
                h = torch.relu(vit_ops.conv_x6_forward(hp, rc.conv.weight, rc.conv.bias)[..., 1:-1, 1:-1])
            else:
                h = F.conv2d(hp, rc.conv.weight, rc.conv.bias)
        if denorm:
            h = torch.clamp(h * self._denorm_scale.view(1, 3, 1, 1) + self._denorm_shift.view(1, 3, 1, 1), 0, 1)
        return h

    def _generate(self, content_images: Tensor, style_images: Tensor, alpha: float, style_index: Optional[Tensor], denorm: bool,
                  materialised: bool = False) -> Tensor:
        if content_images.dim() != 4 or style_images.dim() != 4:
            raise ValueError(f"AdaIN2D: content (B, 3, H, W) and style (Bs, 3, h, w), got {tuple(content_images.shape)}, {tuple(style_images.shape)}")
        if not self._hip_ok(content_images, style_images):
            CALLS["adain2d_expression"] += 1
            return self.generate_expression(content_images, style_images, alpha, style_index, denorm)
        with torch.no_grad():
            fc = self.vgg_encoder(content_images, output_last_feature=True)
            fs = self.vgg_encoder(style_images, output_last_feature=True)
            if materialised:
                return self._decode_materialised(adain_expression(fc, fs, alpha, style_index), denorm)
            return self._decode_hip(adain(fc, fs, alpha, style_index), denorm)

    def generate(self, content_images: Tensor, style_images: Tensor, alpha: float = 1.0, style_index: Optional[Tensor] = None) -> Tensor:
        """The reference's `generate` (vgg_model.py:153-159): ImageNet-normalised content (B, 3, H, W) and style images -> the decoder's raw
        output (B, 3, H', W'), H' = 8 (H // 8).  `style_index` (an addition): `style_images` is (Bs, 3, h, w) with one row per scene and image b
        uses row style_index[b], instead of a row repeated per view."""
        return self._generate(content_images, style_images, alpha, style_index, denorm=False)

    def stylize(self, images01: Tensor, style01: Tensor, alpha: float = 1.0, style_index: Optional[Tensor] = None) -> Tensor:
        """What both wrapper sites do (model_wrapper_style.py:279-285, :537-542): ImageNet-normalise images (B, 3, H, W) and the style --
        (3, h, w), shared by all images, or (Bs, 3, h, w) with `style_index` -- both in [0, 1], `generate`, de-normalise and clamp to
        [0, 1].  On the device route the de-normalisation and the clamp sit in the last kernel's store."""
        if style01.dim() == 3:
            style01 = style01[None]
            if style_index is None:
                style_index = torch.zeros(images01.shape[0], dtype=torch.int32)
        return self._generate(_imagenet_normalize(images01), _imagenet_normalize(style01), alpha, style_index, denorm=True)

    def forward(self, *args, **kwargs):
        raise NotImplementedError("AdaIN2D.forward is the loss that trains the AdaIN network itself (vgg_model.py:174-188); the reference calls "
                                  "it nowhere and this package does not train that network: use generate() or stylize()")
