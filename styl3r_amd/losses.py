"""Loss consumers of the rendered RGB: same interface `loss(prediction, batch, gaussians, step)`.

Mirrors
  * `LossMse`        src/loss/loss_mse.py:22-31
  * `LossStyle`      src/loss/loss_style.py:25-79   (VGG19 relu1_1 / 2_1 / 3_1 / 4_1 mean-std style + content)
  * `IdentityLoss`   src/loss/loss_identity.py:13-52
  * `VGGEncoder`, `calc_mean_std`   src/test/vgg_model.py:19-28,79-98
  * `LossAdaAttN`, `NormalizedVGG`  src/loss/loss_adaattn.py:61-191, src/model/encoder/stylizer/stylizer.py:23-73, stylizer/vgg.py:5-92
torchvision is not installed and the ImageNet VGG19 weights cannot be downloaded: `VGGEncoder` rebuilds the
`vgg19().features[:21]` stack with torchvision's parameter names (`N.weight`, N in 0,2,5,7,10,12,14,16,19), so
`load_vgg19_features(state_dict)` accepts the stock `vgg19-dcbb9e9d.pth` when it is available; until then the
weights are random and only the arithmetic is testable.  LPIPS (loss_lpips.py) needs its own learned weights too:
`LPIPS.load_lpips_weights` takes the `lpips` package's `vgg.pth` and torchvision's vgg16 features when they are available.
On the GPU (fp32 device tensors, a split-arithmetic mode of vit_ops) LPIPS runs on the HIP kernels: the VGG16 convolutions on
Conv2dX6 with their ReLUs folded in, vit_maxpool2x2 and the fused tail vit_lpips_fwd / _bwd; elsewhere the plain expression.
"""
from __future__ import annotations

from dataclasses import dataclass

import torch
import torch.nn as nn
import torch.nn.functional as F
from torch import Tensor

from . import vit_ops
from .vit_ops import Conv2dX6   # nn.Conv2d on the CPU; bf16x6 implicit-GEMM kernels for eligible layers on the GPU

_VGG19_CFG = [64, 64, "M", 128, 128, "M", 256, 256, 256, 256, "M", 512]   # features[:21] ends after relu4_1
IMAGENET_MEAN, IMAGENET_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def calc_mean_std(x: Tensor, eps: float = 1e-8):
    """channel-wise instance mean / (unbiased) std over the flattened spatial dims -> (N, C, 1) each."""
    f = x.flatten(2)
    return f.mean(dim=-1, keepdim=True), f.std(dim=-1, keepdim=True) + eps


class VGGEncoder(nn.Module):
    """h1..h4 = relu1_1, relu2_1, relu3_1, relu4_1 of VGG19 (slices [:2], [2:7], [7:12], [12:21])."""

    def __init__(self):
        super().__init__()
        layers, c_in = [], 3
        for v in _VGG19_CFG:
            if v == "M":
                layers.append(nn.MaxPool2d(2, 2))
            else:
                layers += [Conv2dX6(c_in, v, 3, padding=1), nn.ReLU(inplace=False)]
                c_in = v
        self.features = nn.Sequential(*layers)
        assert len(self.features) == 21
        self.requires_grad_(False)

    def load_vgg19_features(self, state_dict: dict):
        """accepts torchvision's vgg19 state dict (`features.N.*`) or the bare `features` dict (`N.*`)."""
        sd = {k[len("features."):] if k.startswith("features.") else k: v for k, v in state_dict.items()}
        return self.features.load_state_dict({k: v for k, v in sd.items() if int(k.split(".")[0]) < 21}, strict=True)

    def forward(self, images: Tensor, output_last_feature: bool = False):
        h1 = self.features[:2](images)
        h2 = self.features[2:7](h1)
        h3 = self.features[7:12](h2)
        h4 = self.features[12:21](h3)
        return h4 if output_last_feature else (h1, h2, h3, h4)


def _imagenet_normalize(x: Tensor) -> Tensor:
    mean = torch.tensor(IMAGENET_MEAN, device=x.device, dtype=x.dtype).view(1, 3, 1, 1)
    std = torch.tensor(IMAGENET_STD, device=x.device, dtype=x.dtype).view(1, 3, 1, 1)
    return (x - mean) / std


@dataclass
class LossMseCfg:
    weight: float = 1.0


_MSE_SCRATCH: dict = {}   # (device, stream) -> zero-initialised ticket/partials buffer of gsr_mse_forward


class _MseHip(torch.autograd.Function):
    """weight * mean((pred - target)^2) on libgsr_hip.so (include/gsr.h gsr_mse_forward/backward): 2 launches
    instead of the 7 of the torch expression; the target needs no gradient (it is ground truth)."""

    @staticmethod
    def forward(ctx, pred, target, weight):
        import ctypes as C
        from . import _lib
        lib = _lib.load()
        pred, target = pred.contiguous(), target.contiguous()
        dev = pred.device
        stream = torch.cuda.current_stream(dev).cuda_stream
        key = (dev.index, stream)
        if key not in _MSE_SCRATCH:
            _MSE_SCRATCH[key] = torch.zeros(lib.gsr_mse_scratch_bytes(), dtype=torch.uint8, device=dev)
        loss = torch.empty((), dtype=torch.float32, device=dev)
        _lib.check(lib.gsr_mse_forward(pred.data_ptr(), target.data_ptr(), pred.numel(), float(weight),
                                       _MSE_SCRATCH[key].data_ptr(), loss.data_ptr(), C.c_void_p(stream)), "gsr_mse_forward")
        ctx.save_for_backward(pred, target)
        ctx.weight = float(weight)
        return loss

    @staticmethod
    def backward(ctx, g):
        import ctypes as C
        from . import _lib
        pred, target = ctx.saved_tensors
        grad = torch.empty_like(pred)
        g = g.contiguous().float()
        _lib.check(_lib.load().gsr_mse_backward(pred.data_ptr(), target.data_ptr(), g.data_ptr(), pred.numel(), ctx.weight,
                                                grad.data_ptr(), C.c_void_p(torch.cuda.current_stream(pred.device).cuda_stream)),
                   "gsr_mse_backward")
        return grad, None, None


def mse_loss(pred: Tensor, target: Tensor, weight: float = 1.0) -> Tensor:
    """`weight * ((pred - target) ** 2).mean()` (loss_mse.py:27-31).  Device fp32 tensors with a ground-truth target go
    through the fused HIP kernels (and raise if libgsr_hip.so is missing); anything else is the plain torch expression."""
    if pred.is_cuda and pred.dtype == torch.float32 and target.dtype == torch.float32 and not target.requires_grad \
            and pred.shape == target.shape and pred.numel() > 0:
        return _MseHip.apply(pred, target, weight)
    return weight * ((pred - target) ** 2).mean()


class LossMse(nn.Module):
    def __init__(self, cfg: LossMseCfg = LossMseCfg()):
        super().__init__()
        self.cfg = cfg

    def forward(self, prediction, batch, gaussians=None, global_step: int = 0) -> Tensor:
        return mse_loss(prediction.color, batch["target"]["image"], self.cfg.weight)


# ---------------------------------------------------------------------------
# Edge-aware depth smoothness (src/loss/loss_depth.py:26-60, config/loss/depth.yaml): the one registered loss that consumes the
# rasterizer's depth; its gradient reaches the Gaussians as `g_depth` of the composite backward.
# ---------------------------------------------------------------------------
@dataclass
class LossDepthCfg:
    weight: float = 0.25
    sigma_image: float | None = None
    use_second_derivative: bool = False


CALLS = {"depth_hip_fwd": 0, "depth_hip_bwd": 0}   # launches of the HIP route of depth_smoothness (tests and benchmarks check the route taken)
_DEPTH_SCRATCH: dict = {}   # (device, stream) -> partials buffer of gsr_depth_smooth_fwd, grown on demand (needs no initialisation)


def depth_smoothness_expression(depth: Tensor, near: Tensor, far: Tensor, image: Tensor | None = None, weight: float = 1.0,
                                sigma_image: float | None = None, use_second_derivative: bool = False) -> Tensor:
    """`LossDepth.forward` as plain torch ops in the inputs' dtype: the CPU path and, in float64, the yardstick of the kernels.
    depth (b, v, H, W), near / far (b, v), image (b, v, 3, H, W)."""
    lo, hi = near.log()[..., None, None], far.log()[..., None, None]           # (log bounds around the raw depth: see depth_smoothness)
    n = (torch.maximum(torch.minimum(depth, hi), lo) - lo) / (hi - lo)
    dx, dy = n.diff(dim=-1), n.diff(dim=-2)
    if use_second_derivative:
        dx, dy = dx.diff(dim=-1), dy.diff(dim=-2)
    if sigma_image is not None:
        cx, cy = image.diff(dim=-1).amax(dim=-3), image.diff(dim=-2).amax(dim=-3)   # the signed difference, not its magnitude
        if use_second_derivative:
            cx, cy = torch.maximum(cx[..., 1:], cx[..., :-1]), torch.maximum(cy[..., 1:, :], cy[..., :-1, :])
        dx, dy = dx * torch.exp(-cx * sigma_image), dy * torch.exp(-cy * sigma_image)
    return weight * (dx.abs().mean() + dy.abs().mean())


class _DepthSmoothHip(torch.autograd.Function):
    """depth smoothness on libgsr_hip.so (include/gsr.h gsr_depth_smooth_fwd / _bwd): the pass + an ordered fold forward, one gather launch
    backward that recomputes signs and bilateral weights from the saved inputs.  near, far and the image are ground truth."""

    @staticmethod
    def forward(ctx, depth, near, far, image, weight, sigma_image, second):
        import ctypes as C
        from . import _lib
        lib = _lib.load()
        depth, near, far = depth.contiguous(), near.contiguous(), far.contiguous()
        image = image.contiguous() if image is not None else None
        h, w = depth.shape[-2:]
        n = depth.numel() // (h * w)
        dev = depth.device
        stream = torch.cuda.current_stream(dev).cuda_stream
        key, need = (dev.index, stream), lib.gsr_depth_smooth_scratch_bytes(n, h, w)
        if key not in _DEPTH_SCRATCH or _DEPTH_SCRATCH[key].numel() < need:
            _DEPTH_SCRATCH[key] = torch.empty(need, dtype=torch.uint8, device=dev)
        loss = torch.empty((), dtype=torch.float32, device=dev)
        _lib.check(lib.gsr_depth_smooth_fwd(depth.data_ptr(), image.data_ptr() if image is not None else None, near.data_ptr(), far.data_ptr(),
                                            n, h, w, float(weight), float(sigma_image or 0.0), int(second), _DEPTH_SCRATCH[key].data_ptr(),
                                            loss.data_ptr(), C.c_void_p(stream)), "gsr_depth_smooth_fwd")
        CALLS["depth_hip_fwd"] += 1
        ctx.save_for_backward(depth, near, far, *([image] if image is not None else []))
        ctx.args = (float(weight), float(sigma_image or 0.0), int(second))
        return loss

    @staticmethod
    def backward(ctx, g):
        import ctypes as C
        from . import _lib
        depth, near, far, *image = ctx.saved_tensors
        h, w = depth.shape[-2:]
        grad = torch.empty_like(depth)
        g = g.contiguous().float()
        _lib.check(_lib.load().gsr_depth_smooth_bwd(depth.data_ptr(), image[0].data_ptr() if image else None, near.data_ptr(), far.data_ptr(),
                                                    g.data_ptr(), depth.numel() // (h * w), h, w, *ctx.args, grad.data_ptr(),
                                                    C.c_void_p(torch.cuda.current_stream(depth.device).cuda_stream)), "gsr_depth_smooth_bwd")
        CALLS["depth_hip_bwd"] += 1
        return grad, None, None, None, None, None, None


def depth_smoothness(depth: Tensor, near: Tensor, far: Tensor, image: Tensor | None = None, weight: float = 1.0,
                     sigma_image: float | None = None, use_second_derivative: bool = False) -> Tensor:
    """`weight * (mean |d_x n| + mean |d_y n|)` of the rendered depth (b, v, H, W) scaled into its per-view bounds (loss_depth.py:34-60):
    n = (clamp(depth, log near, log far) - log near) / (log far - log near), first or second differences, and with `sigma_image` each
    difference times exp(-sigma_image * c), c the channel maximum of the target image's SIGNED difference at the same place.
    The bounds are logarithms while the depth is not: that is how the reference is written and it is reproduced, not repaired.
    One stated departure, on every path: H or W below 2 (below 3 with second derivatives) raises ValueError (the reference returns NaN,
    the mean of an empty tensor).  fp32 device tensors with ground-truth near / far / image go through the HIP kernels, whose gradient
    reaches `depth` only (they raise if libgsr_hip.so is missing); anything else is `depth_smoothness_expression`."""
    if depth.dim() < 2 or near.shape != depth.shape[:-2] or far.shape != near.shape:
        raise ValueError(f"depth_smoothness: depth (..., H, W) with near / far (...), got {tuple(depth.shape)}, {tuple(near.shape)}, {tuple(far.shape)}")
    if sigma_image is not None and (image is None or image.shape != (*near.shape, 3, *depth.shape[-2:])):
        raise ValueError("depth_smoothness: sigma_image needs the target image (..., 3, H, W)")
    if min(depth.shape[-2:]) < (3 if use_second_derivative else 2) or depth.numel() == 0:
        raise ValueError(f"depth_smoothness: {tuple(depth.shape[-2:])} leaves no difference to average")
    used = image if sigma_image is not None else None
    if all(t.is_cuda and t.dtype == torch.float32 for t in (depth, near, far) + ((used,) if used is not None else ())) \
            and not (near.requires_grad or far.requires_grad or (used is not None and used.requires_grad)):
        return _DepthSmoothHip.apply(depth, near, far, used, weight, sigma_image, use_second_derivative)
    return depth_smoothness_expression(depth, near, far, used, weight, sigma_image, use_second_derivative)


class LossDepth(nn.Module):
    def __init__(self, cfg: LossDepthCfg = LossDepthCfg()):
        super().__init__()
        self.cfg = cfg

    def forward(self, prediction, batch, gaussians=None, global_step: int = 0) -> Tensor:
        tgt = batch["target"]
        return depth_smoothness(prediction.depth, tgt["near"], tgt["far"], tgt["image"] if self.cfg.sigma_image is not None else None,
                                self.cfg.weight, self.cfg.sigma_image, self.cfg.use_second_derivative)


@dataclass
class LossStyleCfg:
    style_weight: float = 10.0


class LossStyle(nn.Module):
    def __init__(self, cfg: LossStyleCfg = LossStyleCfg(), vgg: VGGEncoder | None = None):
        super().__init__()
        self.cfg = cfg
        self.vgg = vgg or VGGEncoder()

    def forward(self, prediction, batch, gaussians=None, global_step: int = 0) -> Tensor:
        b, v = batch["target"]["image"].shape[:2]
        flat = lambda t: t.reshape(b * v, *t.shape[2:])
        target = _imagenet_normalize(flat(batch["target"]["image"]))
        pred = _imagenet_normalize(flat(prediction.color))
        style = _imagenet_normalize(batch["style"]["image"])
        # loss_style.py:53-60 repeats the style image v times and runs the VGG on the b*v copies; the feature statistics of
        # identical images are identical, so the VGG sees each style image ONCE and its (mean, std) are repeated instead
        fp, ft, fs = self.vgg(pred), self.vgg(target), self.vgg(style)
        content = F.mse_loss(fp[-2], ft[-2]) + F.mse_loss(fp[-1], ft[-1])
        style_loss = 0
        rep = lambda t: t[:, None].expand(b, v, *t.shape[1:]).reshape(b * v, *t.shape[1:])
        for a, s in zip(fp, fs):
            am, astd = calc_mean_std(a)
            sm, sstd = calc_mean_std(s)
            style_loss = style_loss + F.mse_loss(am, rep(sm)) + F.mse_loss(astd, rep(sstd))
        return content + self.cfg.style_weight * style_loss


class IdentityLoss(nn.Module):
    def __init__(self, weight_1: float = 70, weight_2: float = 1, vgg: VGGEncoder | None = None):
        super().__init__()
        self.weight_1, self.weight_2 = weight_1, weight_2
        self.vgg = vgg or VGGEncoder()

    def forward(self, prediction, batch, gaussians=None, global_step: int = 0) -> Tensor:
        b, v = batch["target"]["image"].shape[:2]
        target = batch["target"]["image"].reshape(b * v, *batch["target"]["image"].shape[2:])
        pred = prediction.color.reshape(b * v, *prediction.color.shape[2:])
        l1 = F.mse_loss(pred, target)
        fp, ft = self.vgg(_imagenet_normalize(pred)), self.vgg(_imagenet_normalize(target))
        l2 = sum(F.mse_loss(a, t) for a, t in zip(fp, ft))
        return l1 * self.weight_1 + l2 * self.weight_2


def compute_psnr(ground_truth: Tensor, predicted: Tensor) -> Tensor:
    """src/evaluation/metrics.py:11-20 (per image, inputs in [0,1])."""
    mse = ((ground_truth.clip(0, 1) - predicted.clip(0, 1)) ** 2).flatten(1).mean(dim=1)
    return -10 * mse.log10()


# ---------------------------------------------------------------------------
# LPIPS (src/loss/loss_lpips.py:27-54 uses `lpips.LPIPS(net="vgg")`, a third-party package that is not installed here and
# whose weights cannot be fetched).  This is the published LPIPS-VGG architecture with the package's parameter names, so
# its `state_dict` (vgg16 features + the five 1x1 "lin" layers) loads unchanged; without weights it is random-init.
# ---------------------------------------------------------------------------
class _LpipsLin(nn.Module):
    def __init__(self, c_in: int):
        super().__init__()
        self.model = nn.Sequential(nn.Dropout(), nn.Conv2d(c_in, 1, 1, bias=False))      # keys: linK.model.1.weight

    def forward(self, x):
        return self.model(x)


class _LpipsVgg16(nn.Module):
    """torchvision vgg16().features split at relu1_2, relu2_2, relu3_3, relu4_3, relu5_3 (keys: net.sliceK.<idx>.weight)"""
    _CFG = ((64, 64), (128, 128), (256, 256, 256), (512, 512, 512), (512, 512, 512))

    def __init__(self):
        super().__init__()
        idx, c_in = 0, 3
        for s, widths in enumerate(self._CFG, start=1):
            block = nn.Sequential()
            if s > 1:
                block.add_module(str(idx), nn.MaxPool2d(2, 2)); idx += 1
            for w in widths:
                block.add_module(str(idx), Conv2dX6(c_in, w, 3, padding=1)); idx += 1
                block.add_module(str(idx), nn.ReLU(inplace=False)); idx += 1
                c_in = w
            setattr(self, f"slice{s}", block)

    def forward(self, x):
        feats = []
        for s in range(1, 6):
            x = getattr(self, f"slice{s}")(x)
            feats.append(x)
        return feats

    def preacts(self, x):
        """the five taps BEFORE their ReLU (device route): every ReLU is folded into what reads its output -- the next convolution
        (Conv2dX6.forward_fused: conv of relu(x); for the 64-channel conv1_2 on the library path that is one framework ReLU), the
        max-pool (pools the pre-activations: max commutes with ReLU) and vit_lpips_fwd (relu_in) -- so no ReLU'd copy is stored."""
        feats, first = [], True
        for s in range(1, 6):
            for m in getattr(self, f"slice{s}"):
                if isinstance(m, nn.MaxPool2d):
                    x = vit_ops.maxpool2x2(x)
                elif isinstance(m, Conv2dX6):
                    x = m(x) if first else m.forward_fused(x)
                    first = False
            feats.append(x)
        return feats


class LPIPS(nn.Module):
    def __init__(self):
        super().__init__()
        self.net = _LpipsVgg16()
        for k, c in enumerate((64, 128, 256, 512, 512)):
            setattr(self, f"lin{k}", _LpipsLin(c))
        self.register_buffer("shift", torch.tensor([-.030, -.088, -.188]).view(1, 3, 1, 1), persistent=False)
        self.register_buffer("scale", torch.tensor([.458, .448, .450]).view(1, 3, 1, 1), persistent=False)
        # True once load_lpips_weights has loaded both the lin layers and the VGG16 features: until then the distance is meaningless
        self.weights_loaded = False

    _VGG16_CONVS = (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28)     # torchvision vgg16().features indices of the convolutions

    def load_lpips_weights(self, lin_sd: dict, vgg16_sd: dict | None = None) -> None:
        """lin_sd: the `lpips` package's weights file (vgg.pth: `lin{k}.model.1.weight`, k = 0..4).  vgg16_sd: torchvision's vgg16 state
        dict (`features.N.weight` / `.bias` for the 13 convolutions; `classifier.*` entries are ignored), mapped onto `net.slice{s}.N.*`.
        Strict: a missing or an extra key raises, and so does a shape mismatch."""
        want = {f"lin{k}.model.1.weight" for k in range(5)}
        _same_keys(set(lin_sd), want, "lpips lin weights")
        sd = dict(lin_sd)
        if vgg16_sd is not None:
            feats = {k: v for k, v in vgg16_sd.items() if not k.startswith("classifier.")}
            _same_keys(set(feats), {f"features.{n}.{p}" for n in self._VGG16_CONVS for p in ("weight", "bias")}, "vgg16 features")
            for k, v in feats.items():
                n, param = int(k.split(".")[1]), k.split(".")[2]
                sd[f"net.slice{1 + sum(n >= b for b in (4, 9, 16, 23))}.{n}.{param}"] = v
        res = self.load_state_dict(sd, strict=vgg16_sd is not None)
        assert not res.unexpected_keys and all(k.startswith("net.") for k in res.missing_keys), res
        self.weights_loaded = vgg16_sd is not None

    def _hip_ok(self, a: Tensor, b: Tensor) -> bool:
        """device route: fp32 device images, a split-arithmetic mode, a ground-truth `b`, no active dropout and no trained lin weight"""
        if not (a.is_cuda and b.is_cuda and a.dtype == torch.float32 and b.dtype == torch.float32 and a.dim() == 4 and a.shape == b.shape
                and self.net.slice1[0].weight.is_cuda and self.net.slice1[0].weight.dtype == torch.float32):
            return False
        if vit_ops.LINEAR_MODE not in ("bf16x6", "bf16x3", "f16x3") or b.requires_grad:
            return False
        lins = [getattr(self, f"lin{k}").model for k in range(5)]
        if any(m[0].training and m[0].p > 0 for m in lins):
            return False
        return not (torch.is_grad_enabled() and any(m[1].weight.requires_grad for m in lins))

    def forward(self, a: Tensor, b: Tensor, normalize: bool = False) -> Tensor:
        if normalize:                                                       # [0,1] -> [-1,1]
            a, b = 2 * a - 1, 2 * b - 1
        if self._hip_ok(a, b):
            with torch.no_grad():                                           # the target side saves nothing
                fb = self.net.preacts((b - self.shift) / self.scale)
            fa = self.net.preacts((a - self.shift) / self.scale)
            ws = [getattr(self, f"lin{k}").model[1].weight for k in range(5)]
            return vit_ops.lpips_tail(fa, fb, ws, relu_in=True).view(-1, 1, 1, 1)
        return self._forward_expression(a, b)

    def _forward_expression(self, a: Tensor, b: Tensor) -> Tensor:
        """the plain expression (CPU, the f32 mode, a target that needs a gradient); a and b already in [-1, 1]"""
        fa, fb = self.net((a - self.shift) / self.scale), self.net((b - self.shift) / self.scale)
        total = 0
        for k, (x, y) in enumerate(zip(fa, fb)):
            x = x / (x.pow(2).sum(1, keepdim=True).sqrt() + 1e-10)
            y = y / (y.pow(2).sum(1, keepdim=True).sqrt() + 1e-10)
            total = total + getattr(self, f"lin{k}")((x - y) ** 2).mean(dim=(2, 3), keepdim=True)
        return total                                                        # (N,1,1,1)


def _same_keys(got: set, want: set, what: str) -> None:
    if got != want:
        raise KeyError(f"{what}: missing {sorted(want - got)}, unexpected {sorted(got - want)}")


@dataclass
class LossLpipsCfg:
    weight: float = 0.05
    apply_after_step: int = 0


class LossLpips(nn.Module):
    def __init__(self, cfg: LossLpipsCfg = LossLpipsCfg(), lpips: LPIPS | None = None):
        super().__init__()
        self.cfg = cfg
        self.lpips = (lpips or LPIPS()).eval()
        for p in self.lpips.parameters():                                   # convert_to_buffer(..., persistent=False)
            p.requires_grad_(False)

    def forward(self, prediction, batch, gaussians=None, global_step: int = 0) -> Tensor:
        image = batch["target"]["image"]
        if global_step < self.cfg.apply_after_step:
            return torch.tensor(0, dtype=torch.float32, device=image.device)
        b, v = image.shape[:2]
        loss = self.lpips(prediction.color.reshape(b * v, *image.shape[2:]), image.reshape(b * v, *image.shape[2:]), normalize=True)
        return self.cfg.weight * loss.mean()


# ---------------------------------------------------------------------------
# SSIM structure term of the pose refinement (src/evaluation/pose_evaluator.py:128-133):
# `1 - structure` of src/loss/loss_ssim.py::ssim(target, pred, data_range=1.0, win_size=11, retrun_seprate=True).
# ---------------------------------------------------------------------------
SSIM_WIN, SSIM_SIGMA = 11, 1.5
SSIM_C3 = 0.5 * (0.03 * 1.0) ** 2                 # C2 / 2, C2 = (K2 data_range)^2
SSIM_EPS2 = torch.finfo(torch.float32).eps ** 2
SSIM_STRUCTURE_MAX = 0.98


def ssim_window() -> Tensor:
    """`_fspecial_gauss_1d(11, 1.5)` (loss_ssim.py:12-26): formed and normalised in fp32, whatever the images' dtype"""
    coords = torch.arange(SSIM_WIN, dtype=torch.float)
    coords -= SSIM_WIN // 2
    g = torch.exp(-(coords ** 2) / (2 * SSIM_SIGMA ** 2))
    g /= g.sum()
    return g


def ssim_structure_map(target: Tensor, pred: Tensor, details: bool = False):
    """the plain expression of loss_ssim.py:80-124 for (N, C, H, W): the structure map (N, C, H-10, W-10) after its 0.98 clamp.
    `details`: also the quantities the branches switch on (raw map, |sigma12|, sqrt(sigma1^2 sigma2^2), the unclamped variances)."""
    n, c, h, w = pred.shape
    win = ssim_window().to(pred.device, pred.dtype)

    def filt(t):                                   # valid, separable: height first, then width (gaussian_filter's order)
        t = F.conv2d(t.reshape(n * c, 1, h, w), win.view(1, 1, -1, 1))
        return F.conv2d(t, win.view(1, 1, 1, -1)).reshape(n, c, h - SSIM_WIN + 1, w - SSIM_WIN + 1)

    x, y = target.to(pred.dtype), pred
    mu1, mu2 = filt(x), filt(y)
    raw1, raw2 = filt(x * x) - mu1.pow(2), filt(y * y) - mu2.pow(2)
    raw12 = filt(x * y) - mu1 * mu2
    s1, s2 = raw1.clamp(min=SSIM_EPS2), raw2.clamp(min=SSIM_EPS2)
    cap = torch.sqrt(s1 * s2)
    s12 = torch.sign(raw12) * torch.minimum(cap, raw12.abs())
    raw = (s12 + SSIM_C3) / (torch.sqrt(s1) * torch.sqrt(s2) + SSIM_C3)
    out = raw.clamp(max=SSIM_STRUCTURE_MAX)
    return (out, raw, raw12.abs(), cap, raw1, raw2) if details else out


def _structure_expression(target: Tensor, pred: Tensor) -> Tensor:
    """per-image structure (N,): mean over the pixels, then the channels"""
    return ssim_structure_map(target, pred).flatten(2).mean(-1).mean(1)


_SSIM_WINDOW_C = None


def _window_c():
    import ctypes as C
    global _SSIM_WINDOW_C
    if _SSIM_WINDOW_C is None:
        _SSIM_WINDOW_C = (C.c_float * SSIM_WIN)(*ssim_window().tolist())
    return _SSIM_WINDOW_C


class _SsimStructureHip(torch.autograd.Function):
    """per-image structure (N,) on libgsr_hip.so (include/gsr.h gsr_ssim_structure_fwd / _bwd): the pass + an ordered fold; when `pred`
    needs a gradient the pass also leaves the three adjoint maps the one-launch backward filters.  The target is ground truth."""

    @staticmethod
    def forward(ctx, pred, target):
        import ctypes as C
        from . import _lib
        lib = _lib.load()
        pred, target = pred.contiguous(), target.contiguous()
        n, c, h, w = pred.shape
        dev = pred.device
        need = ctx.needs_input_grad[0]
        maps = torch.empty((3, n * c * (h - SSIM_WIN + 1) * (w - SSIM_WIN + 1)), dtype=torch.float32, device=dev) if need else None
        scratch = torch.empty(lib.gsr_ssim_structure_scratch_bytes(n, c, h, w), dtype=torch.uint8, device=dev)
        out = torch.empty(n, dtype=torch.float32, device=dev)
        _lib.check(lib.gsr_ssim_structure_fwd(target.data_ptr(), pred.data_ptr(), n, c, h, w, _window_c(), out.data_ptr(),
                                              maps.data_ptr() if need else None, scratch.data_ptr(),
                                              C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)), "gsr_ssim_structure_fwd")
        if need:
            ctx.save_for_backward(pred, target, maps)
        return out

    @staticmethod
    def backward(ctx, g):
        import ctypes as C
        from . import _lib
        pred, target, maps = ctx.saved_tensors
        n, c, h, w = pred.shape
        grad = torch.empty_like(pred)
        g = g.contiguous().float()
        _lib.check(_lib.load().gsr_ssim_structure_bwd(target.data_ptr(), pred.data_ptr(), maps.data_ptr(), g.data_ptr(), n, c, h, w, _window_c(),
                                                      grad.data_ptr(), C.c_void_p(torch.cuda.current_stream(pred.device).cuda_stream)),
                   "gsr_ssim_structure_bwd")
        return grad, None


def ssim_structure_per_image(target: Tensor, pred: Tensor) -> Tensor:
    """structure (N,) of (N, C, H, W) images, H, W >= 11; differentiable with respect to `pred`.  fp32 device tensors with a ground-truth
    target go through the HIP kernels (and raise if libgsr_hip.so is missing); anything else is the plain torch expression."""
    if pred.dim() != 4 or pred.shape != target.shape:
        raise ValueError(f"ssim_structure takes two (N, C, H, W) tensors of one shape, got {tuple(target.shape)} and {tuple(pred.shape)}")
    if min(pred.shape[-2:]) < SSIM_WIN:
        raise ValueError("ssim_structure: the 11 x 11 window needs height and width >= 11")
    if pred.is_cuda and target.is_cuda and pred.dtype == torch.float32 and target.dtype == torch.float32 and not target.requires_grad \
            and pred.numel() > 0:
        return _SsimStructureHip.apply(pred, target)
    return _structure_expression(target, pred)


def ssim_structure(target: Tensor, pred: Tensor) -> Tensor:
    """the `structure` scalar of `ssim(target, pred, size_average=True, data_range=1.0, retrun_seprate=True, win_size=11)`"""
    return ssim_structure_per_image(target, pred).mean()


class LossSsimStructure(nn.Module):
    """`(1 - structure) * weight` of the rendered views against `batch["target"]["image"]` (pose_evaluator.py:128-133), with the interface
    of the other losses so that it drops into `evaluation.align_target_poses`"""

    def __init__(self, weight: float = 1.0):
        super().__init__()
        self.weight = weight

    def forward(self, prediction, batch, gaussians=None, global_step: int = 0) -> Tensor:
        image = batch["target"]["image"]
        b, v = image.shape[:2]
        return self.weight * (1 - ssim_structure(image.reshape(b * v, *image.shape[2:]), prediction.color.reshape(b * v, *image.shape[2:])))


# ---------------------------------------------------------------------------
# Point-map distillation loss (src/loss/loss_point.py:188-254 `Regr3D`, src/geometry/ptc_geometry.py:270-328 `normalize_pointcloud`):
# the student's means against the frozen teacher's point maps.
# One deliberate deviation from the reference, on every path: a view whose valid set is empty contributes 0 with a zero gradient (the
# reference returns NaN, the mean of an empty tensor).
# ---------------------------------------------------------------------------
REGR3D_QUANTILES = (0.002, 0.998)
REGR3D_CONF_MIN = 3


def _norm_factor(pts1: Tensor, pts2: Tensor, norm_mode: str, valid1: Tensor, valid2: Tensor):
    """the per-image scale of `normalize_pointcloud`, jointly over both views, and the (possibly warped) points"""
    how, dis_mode = norm_mode.split("_")
    b = pts1.shape[0]
    if how == "avg":
        zero = torch.zeros_like(pts1[..., :1])
        both = torch.cat((torch.where(valid1.unsqueeze(-1), pts1, zero).reshape(b, -1, 3), torch.where(valid2.unsqueeze(-1), pts2, zero).reshape(b, -1, 3)), dim=1)
        nnz = valid1.reshape(b, -1).sum(1) + valid2.reshape(b, -1).sum(1)
        dis = both.norm(dim=-1)
        if dis_mode == "log1p":
            dis = torch.log1p(dis)
        elif dis_mode == "warp-log1p":
            log_dis = torch.log1p(dis)
            warp = log_dis / dis.clip(min=1e-8)
            n1 = pts1[0].numel() // 3
            pts1 = pts1 * warp[:, :n1].reshape(pts1.shape[:-1]).unsqueeze(-1)
            pts2 = pts2 * warp[:, n1:].reshape(pts2.shape[:-1]).unsqueeze(-1)
            dis = log_dis
        elif dis_mode != "dis":
            raise ValueError(f"bad dis_mode {dis_mode!r}")
        factor = dis.sum(dim=1) / (nnz.to(dis.dtype) + 1e-8)
    else:
        nan = torch.full_like(pts1[..., :1], float("nan"))
        both = torch.cat((torch.where(valid1.unsqueeze(-1), pts1, nan).reshape(b, -1, 3), torch.where(valid2.unsqueeze(-1), pts2, nan).reshape(b, -1, 3)), dim=1)
        dis = both.norm(dim=-1)
        if how == "median":
            factor = dis.nanmedian(dim=1).values.detach()
        elif how == "sqrt":
            factor = dis.sqrt().nanmean(dim=1) ** 2
        else:
            raise ValueError(f"bad norm_mode {norm_mode!r}")
    return pts1, pts2, factor.clip(min=1e-8).reshape(b, *([1] * (pts1.dim() - 1)))


def normalize_pointcloud(pts1: Tensor, pts2: Tensor, norm_mode: str, valid1: Tensor, valid2: Tensor):
    pts1, pts2, f = _norm_factor(pts1, pts2, norm_mode, valid1, valid2)
    return pts1 / f, pts2 / f


def regr3d_valid_masks(gt_pts1: Tensor, gt_pts2: Tensor, conf1: Tensor, conf2: Tensor, dist_clip=None):
    """the valid sets of Regr3D: |gt| inside its per-image [0.2 %, 99.8 %] quantiles and confidence >= 3, or |gt| <= dist_clip"""
    dis1, dis2 = gt_pts1.norm(dim=-1), gt_pts2.norm(dim=-1)
    if dist_clip is not None:
        return dis1 <= dist_clip, dis2 <= dist_clip, None
    b = dis1.shape[0]
    q = torch.tensor(REGR3D_QUANTILES, device=dis1.device, dtype=dis1.dtype)
    shape = (b,) + (1,) * (dis1.dim() - 1)
    q1, q2 = torch.quantile(dis1.reshape(b, -1), q, dim=1), torch.quantile(dis2.reshape(b, -1), q, dim=1)
    valid1 = (dis1 >= q1[0].view(shape)) & (dis1 <= q1[1].view(shape)) & (conf1 >= REGR3D_CONF_MIN)
    valid2 = (dis2 >= q2[0].view(shape)) & (dis2 <= q2[1].view(shape)) & (conf2 >= REGR3D_CONF_MIN)
    return valid1, valid2, torch.stack((q1.t(), q2.t()))           # quantiles (2, B, 2)


def regr3d_expression(gt_pts1: Tensor, gt_pts2: Tensor, pr_pts1: Tensor, pr_pts2: Tensor, conf1: Tensor, conf2: Tensor,
                      norm_mode="avg_dis", gt_scale: bool = False, dist_clip=None, disable_view1: bool = False) -> Tensor:
    """`Regr3D.forward` as plain torch ops in the inputs' dtype: the CPU path and, in float64, the yardstick of the kernels"""
    valid1, valid2, _ = regr3d_valid_masks(gt_pts1, gt_pts2, conf1, conf2, dist_clip)
    if norm_mode:
        pr_pts1, pr_pts2 = normalize_pointcloud(pr_pts1, pr_pts2, norm_mode, valid1, valid2)
        if not gt_scale:
            gt_pts1, gt_pts2 = normalize_pointcloud(gt_pts1, gt_pts2, norm_mode, valid1, valid2)
    mean = lambda t: t.mean() if t.numel() else t.sum()           # (empty valid set: 0, see above)
    loss2 = mean(torch.norm(pr_pts2 - gt_pts2, dim=-1)[valid2])
    if disable_view1:
        return loss2
    return mean(torch.norm(pr_pts1 - gt_pts1, dim=-1)[valid1]) + loss2


class Regr3D(nn.Module):
    """`Regr3D(norm_mode, alpha, gt_scale)` with the reference's forward signature.  fp32 device tensors with norm_mode None / 'avg_dis' run
    on the HIP kernels (points.regr3d_hip: exact radix selection instead of torch.quantile's sorts, one fused mask / normalise / distance
    pass each way; raises if libgsr_hip.so is missing); everything else -- CPU tensors, other dtypes, gt_scale, the other norm modes, none
    of which a training wrapper uses -- is `regr3d_expression`."""

    def __init__(self, norm_mode="avg_dis", alpha: float = 0.2, gt_scale: bool = False):
        super().__init__()
        self.norm_mode, self.alpha, self.gt_scale = norm_mode, alpha, gt_scale

    def forward(self, gt_pts1, gt_pts2, pr_pts1, pr_pts2, conf1=None, conf2=None, dist_clip=None, disable_view1=False, details=None) -> Tensor:
        from . import points
        if (self.norm_mode in (None, "avg_dis") and not (self.norm_mode and self.gt_scale) and (dist_clip is None or dist_clip > 0)
                and points.regr3d_hip_ok(gt_pts1, gt_pts2, pr_pts1, pr_pts2, conf1, conf2)):
            return points.regr3d_hip(gt_pts1, gt_pts2, pr_pts1, pr_pts2, conf1, conf2, bool(self.norm_mode), disable_view1, dist_clip, details)
        return regr3d_expression(gt_pts1, gt_pts2, pr_pts1, pr_pts2, conf1, conf2, self.norm_mode, self.gt_scale, dist_clip, disable_view1)


# ---------------------------------------------------------------------------
# AdaAttN loss (src/loss/loss_adaattn.py:61-191, AdaAttN of src/model/encoder/stylizer/stylizer.py:23-73, NormalizedVGG of
# stylizer/vgg.py:5-92): L1 between the prediction's VGG features and the target's features re-styled by attention-weighted style
# statistics, plus lam x the MSE of spatial feature statistics against the style's.  The stylised target depends on the target and the
# style only: it is computed without a graph, on the kernels of csrc/vit_adaattn.hip for device tensors.
# ---------------------------------------------------------------------------
CALLS.update({"adaattn_hip_stats": 0, "adaattn_expr_stats": 0, "adaattn_hip_l1": 0})
ADAATTN_MAX_D, ADAATTN_MAX_C = 448, 256        # what vit_adaattn_stats takes (VGG layers 1 - 3); beyond it: the expression
# make_vgg() as (kind, c_in, c_out): every 3 x 3 convolution is [ReflectionPad2d(1), Conv2d, ReLU] (three Sequential indices), the 1 x 1
# input convolution and the pools take one index each; "end": a slice ends after the ReLU of conv{k}_1
_NVGG_OPS = (("c1", 3, 3), ("c3", 3, 64), "end", ("c3", 64, 64), "pool", ("c3", 64, 128), "end", ("c3", 128, 128), "pool", ("c3", 128, 256), "end",
             ("c3", 256, 256), ("c3", 256, 256), ("c3", 256, 256), "pool", ("c3", 256, 512), "end",
             ("c3", 512, 512), ("c3", 512, 512), ("c3", 512, 512), "pool", ("c3", 512, 512), "end")
_NVGG_SLICE_ENDS = (4, 11, 18, 31, 44)


class NormalizedVGG(nn.Module):
    """relu1_1 .. relu{depth}_1 of the "normalised" VGG19 (a 1 x 1 input convolution, reflection padding in front of every 3 x 3 convolution,
    max-pooling) on images in [0, 1] without ImageNet normalisation.  Parameter names are the reference's: `slice{k}.{N}.weight / .bias`, N the
    index in its nn.Sequential.  Frozen.  Only the slices up to `depth` exist and run (the reference always runs all five and so refuses
    images under 32 pixels a side).  On the GPU the eligible convolutions run on Conv2dX6: a reflect-padded 3 x 3 convolution is the
    zero-padded convolution of the reflect-padded input with one border pixel cropped."""

    def __init__(self, depth: int = 5):
        super().__init__()
        assert 1 <= depth <= 5, depth
        self.depth = depth
        self.all_keys = []                                                   # the bare Sequential's keys of all five slices, in order
        idx, k, block = 0, 1, nn.Sequential()
        for op in _NVGG_OPS:
            if op == "end":
                if k <= depth:
                    setattr(self, f"slice{k}", block)
                k, block = k + 1, nn.Sequential()
            elif op == "pool":
                idx += 1
            else:
                kind, ci, co = op
                idx += kind == "c3"                                          # its ReflectionPad2d
                if k <= depth:
                    block.add_module(str(idx), nn.Conv2d(ci, co, 1) if kind == "c1" else Conv2dX6(ci, co, 3, padding=1))
                self.all_keys += [f"{idx}.weight", f"{idx}.bias"]
                idx += 1 if kind == "c1" else 2                              # the convolution (and its ReLU)
        assert idx == _NVGG_SLICE_ENDS[-1]
        self.requires_grad_(False)

    def load_normalised_vgg(self, state_dict: dict):
        """`vgg_normalised.pth`: the state dict of the bare nn.Sequential (`0.weight`, `2.weight`, `5.weight`, ...).  Strict: its keys must be
        exactly the 17 convolutions' weights and biases; those of slices beyond `depth` are checked by name and not kept."""
        _same_keys(set(state_dict), set(self.all_keys), "vgg_normalised")
        sd = {}
        for key, val in state_dict.items():
            k = 1 + sum(int(key.split(".")[0]) >= e for e in _NVGG_SLICE_ENDS)
            if k <= self.depth:
                sd[f"slice{k}.{key}"] = val
        return self.load_state_dict(sd, strict=True)

    @staticmethod
    def _conv3_relu(m, x: Tensor) -> Tensor:
        xp = F.pad(x, (1, 1, 1, 1), mode="reflect")
        # not in "bf16x3": its products leave out the 2^-16-level terms, and the unscaled AdaAttN logits (sums of hundreds of feature products in
        # front of an exp) need features of fp32 quality; that mode keeps the library's fp32 convolution here
        if vit_ops.LINEAR_MODE != "bf16x3" and m._x6_ok(xp):
            return torch.relu(m(xp)[..., 1:-1, 1:-1])
        return torch.relu(F.conv2d(xp, m.weight, m.bias))

    def forward(self, x: Tensor) -> list:
        feats = []
        for k in range(1, self.depth + 1):
            convs = list(getattr(self, f"slice{k}"))
            for m in convs[:-1]:                                             # slice 1: the 1 x 1 input map; later slices: conv{k-1}_2 ..
                x = m(x) if k == 1 else self._conv3_relu(m, x)
            if k > 1:
                x = vit_ops.maxpool2x2(x)
            x = self._conv3_relu(convs[-1], x)
            feats.append(x)
        return feats


def _adaattn_qk(feats: list, upto: int) -> list:
    """the cumulative query / key stacks of VGGContentLoss: q_0 = f_0, q_i = cat(bilinear(q_{i-1} -> size of f_i), f_i) -- relu1_1 is
    resampled once per level, not once by the total factor"""
    q, out = feats[0], [feats[0]]
    for f in feats[1:upto]:
        q = torch.cat([F.interpolate(q, size=f.shape[-2:], mode="bilinear", align_corners=False), f], 1)
        out.append(q)
    return out


def adaattn_stats_expression(q_hat: Tensor, k_hat: Tensor, s: Tensor, style_index: Tensor | None = None):
    """AdaAttN.forward's statistics as plain torch ops: q_hat (Bq, D, Nq), k_hat (Bs, D, M), s (Bs, C, M) -> mean, std (Bq, C, Nq)"""
    if style_index is not None:
        k_hat, s = k_hat[style_index.to(k_hat.device, torch.long)], s[style_index.to(s.device, torch.long)]
    attn = F.softmax(torch.bmm(q_hat.transpose(2, 1), k_hat), -1)
    st = s.transpose(2, 1)
    mean = torch.bmm(attn, st)
    var = F.relu(torch.bmm(attn, st ** 2) - mean ** 2)
    return mean.transpose(2, 1), torch.sqrt(var).transpose(2, 1)


_ADAATTN_INDEX: dict = {}      # (index values, device) -> (host int32 tensor, device int32 tensor)


def _adaattn_index(style_index, bq: int, bs: int, dev):
    if style_index is None:
        vals = tuple(range(bq))
    else:
        vals = tuple(int(i) for i in style_index.detach().cpu().reshape(-1).tolist())      # (a device index is read back: pass a CPU tensor)
    key = (vals, str(dev))
    if key not in _ADAATTN_INDEX:
        if len(_ADAATTN_INDEX) > 64:
            _ADAATTN_INDEX.clear()
        host = torch.tensor(vals, dtype=torch.int32)
        _ADAATTN_INDEX[key] = (host, host.to(dev))
    return _ADAATTN_INDEX[key]


def adaattn_stats(q_hat: Tensor, k_hat: Tensor, s: Tensor, style_index: Tensor | None = None):
    """(mean, std), each (Bq, C, Nq): the attention-weighted mean and standard deviation of the style features s (Bs, C, M) under
    softmax_m(q_hat^T k_hat) (unscaled), q_hat (Bq, D, Nq) and k_hat (Bs, D, M) instance-normalised; image b uses style row style_index[b]
    (None: Bq == Bs, row b).  Forward only.  fp32 device tensors with D % 64 == 0, D <= 448, C % 64 == 0, C <= 256 run on vit_adaattn_stats
    (and raise if libvit_hip.so is missing); anything else is `adaattn_stats_expression`.  CALLS counts the route."""
    if q_hat.dim() != 3 or k_hat.dim() != 3 or s.dim() != 3 or q_hat.shape[1] != k_hat.shape[1] or k_hat.shape[0] != s.shape[0] \
            or k_hat.shape[2] != s.shape[2] or q_hat.shape[2] < 1 or s.shape[2] < 1:
        raise ValueError(f"adaattn_stats: q_hat (Bq, D, Nq), k_hat (Bs, D, M), s (Bs, C, M), got {tuple(q_hat.shape)}, {tuple(k_hat.shape)}, {tuple(s.shape)}")
    (bq, d, nq), (bs, c, m) = q_hat.shape, s.shape
    if (style_index is None and bq != bs) or (style_index is not None and style_index.numel() != bq):
        raise ValueError(f"adaattn_stats: {bq} images and {bs} styles need a style_index of {bq} entries")
    if all(t.is_cuda and t.dtype == torch.float32 for t in (q_hat, k_hat, s)) and d % 64 == 0 and d <= ADAATTN_MAX_D \
            and c % 64 == 0 and c <= ADAATTN_MAX_C and bq <= 65535:
        host, devi = _adaattn_index(style_index, bq, bs, q_hat.device)
        q_hat, k_hat, s = (vit_ops._aligned(t.detach()) for t in (q_hat, k_hat, s))
        mean, std = torch.empty((bq, c, nq), dtype=torch.float32, device=s.device), torch.empty((bq, c, nq), dtype=torch.float32, device=s.device)
        CALLS["adaattn_hip_stats"] += 1
        vit_ops._check(vit_ops.load().vit_adaattn_stats(q_hat.data_ptr(), k_hat.data_ptr(), s.data_ptr(), host.data_ptr(), devi.data_ptr(), bq, bs,
                                                        d, c, nq, m, mean.data_ptr(), std.data_ptr(), vit_ops._stream(s.device)), "vit_adaattn_stats")
        return mean, std
    CALLS["adaattn_expr_stats"] += 1
    return adaattn_stats_expression(q_hat, k_hat, s, style_index)


class _AdaAttnL1Hip(torch.autograd.Function):
    """mean |p - (instance_norm(c) std + mean)| on vit_adaattn_l1: the pass writes sign(p - cs) / numel beside the loss, the backward is one
    scale by the upstream gradient.  c, mean and std are ground truth."""

    @staticmethod
    def forward(ctx, p, c, mean, std, want_cs):
        lib = vit_ops.load()
        p, c, mean, std = (vit_ops._aligned(t) for t in (p, c, mean, std))
        b, ch, n = p.shape
        dev = p.device
        scratch = torch.empty(lib.vit_adaattn_l1_scratch_bytes(b, ch) // 8, dtype=torch.float64, device=dev)
        loss = torch.empty((), dtype=torch.float32, device=dev)
        grad = torch.empty_like(p)
        cs = torch.empty_like(p) if want_cs else None
        CALLS["adaattn_hip_l1"] += 1
        vit_ops._check(lib.vit_adaattn_l1(p.data_ptr(), c.data_ptr(), mean.data_ptr(), std.data_ptr(), b, ch, n, scratch.data_ptr(), loss.data_ptr(),
                                          grad.data_ptr(), cs.data_ptr() if want_cs else None, vit_ops._stream(dev)), "vit_adaattn_l1")
        ctx.save_for_backward(grad)
        ctx.mark_non_differentiable(grad)
        if want_cs:
            ctx.mark_non_differentiable(cs)
            return loss, grad, cs
        return loss, grad, None

    @staticmethod
    def backward(ctx, g, _g_grad, _g_cs):
        (grad,) = ctx.saved_tensors
        return grad * g, None, None, None, None


def adaattn_l1(p: Tensor, c: Tensor, mean: Tensor, std: Tensor, details: dict | None = None) -> Tensor:
    """the content term of one layer: mean |p - cs|, cs = instance_norm(c) * std + mean (per (image, channel) over the positions, biased
    variance, eps 1e-5), all (B, C, N).  fp32 device tensors with ground-truth c / mean / std go through vit_adaattn_l1; anything else is
    the plain expression.  `details` receives `cs` and `feature_grad` = sign(p - cs) / numel."""
    if p.dim() != 3 or not (p.shape == c.shape == mean.shape == std.shape):
        raise ValueError(f"adaattn_l1: four (B, C, N) tensors of one shape, got {[tuple(t.shape) for t in (p, c, mean, std)]}")
    if all(t.is_cuda and t.dtype == torch.float32 for t in (p, c, mean, std)) and not (c.requires_grad or mean.requires_grad or std.requires_grad) \
            and p.numel() > 0:
        loss, grad, cs = _AdaAttnL1Hip.apply(p, c, mean, std, details is not None)
        if details is not None:
            details["cs"], details["feature_grad"] = cs, grad
        return loss
    # (one position: the normalised value is 0, as on the kernel; F.instance_norm refuses a single spatial element)
    cs = (torch.zeros_like(c) if c.shape[-1] == 1 else F.instance_norm(c)) * std + mean
    if details is not None:
        details["cs"], details["feature_grad"] = cs.detach(), torch.sign(p.detach() - cs.detach()) / p.numel()
    return (p - cs).abs().mean()


def _gram(x: Tensor) -> Tensor:
    b, c, h, w = x.shape
    f = x.reshape(b, c, h * w)
    return torch.bmm(f, f.transpose(2, 1)) / (c * h * w)


def adaattn_style_term(pred_feats: list, style_feats: list, layers, stats, style_index: Tensor | None = None) -> Tensor:
    """VGGStyleLoss (MSE, mean): spatial mean / unbiased std / Gram matrix of the prediction's features against the style's.  The style's
    statistics are formed once per style image and repeated per view (identical images have identical statistics)."""
    rep = (lambda t: t) if style_index is None else (lambda t: t[style_index.to(t.device, torch.long)])
    loss = 0
    for l in layers:
        p, s = pred_feats[l - 1], style_feats[l - 1]
        if "mean" in stats:
            loss = loss + F.mse_loss(p.mean((-2, -1)), rep(s.mean((-2, -1))))
        if "std" in stats:
            loss = loss + F.mse_loss(p.std((-2, -1)), rep(s.std((-2, -1))))
        if "gram" in stats:
            loss = loss + F.mse_loss(_gram(p), rep(_gram(s)))
    return loss


def adaattn_expression(pred_feats: list, content_feats: list, style_feats: list, lam: float = 0.3, content_loss_layers=(3,),
                       style_loss_layers=(2, 3), style_loss_stats=("mean", "std"), style_index: Tensor | None = None,
                       details: dict | None = None) -> Tensor:
    """`LossAdaAttN.forward` after its three VGG passes, as plain torch ops in the inputs' dtype: the CPU path and, in float64, the yardstick
    of the kernels.  The feature lists hold relu1_1 .. of the prediction (b v images), the target (b v) and the style (one per style image;
    `style_index` (b v,) maps an image to its style, None: one style per image)."""
    depth = max(content_loss_layers)
    with torch.no_grad():
        qs, ks = _adaattn_qk(content_feats, depth), _adaattn_qk(style_feats, depth)
    content = 0
    for l in sorted(content_loss_layers):
        with torch.no_grad():
            mean, std = adaattn_stats_expression(F.instance_norm(qs[l - 1].flatten(2)), F.instance_norm(ks[l - 1].flatten(2)),
                                                 style_feats[l - 1].flatten(2), style_index)
        cs = (F.instance_norm(content_feats[l - 1].flatten(2)) * std + mean).detach()
        p = pred_feats[l - 1].flatten(2)
        content = content + (p - cs).abs().mean()
        if details is not None:
            details[f"cs{l}"], details[f"feature_grad{l}"] = cs, torch.sign(p.detach() - cs) / p.numel()
    style = adaattn_style_term(pred_feats, style_feats, style_loss_layers, style_loss_stats, style_index)
    if details is not None:
        details["content"], details["style"] = content.detach(), style.detach()
    return content + lam * style


@dataclass
class LossAdaAttNCfg:
    lam: float = 0.3
    content_loss_layers: tuple = (3,)
    style_loss_layers: tuple = (2, 3)
    style_loss_stats: tuple = ("mean", "std")


class LossAdaAttN(nn.Module):
    """content + lam * style of loss_adaattn.py on `prediction.color`, `batch["target"]["image"]` (b, v, 3, H, W) and
    `batch["style"]["image"]` (b, 3, h, w), all in [0, 1].  The target and the style run through the VGG without a graph and the style once
    per style image, not per view.  fp32 device tensors: the stylised target's statistics on vit_adaattn_stats (layers 1 - 3; 4 - 5 on the
    expression), the L1 and its gradient on vit_adaattn_l1; the style term's small statistics stay framework ops (they need autograd).
    `details` (a dict) receives `content`, `style` and per content layer l `cs{l}` and `feature_grad{l}`."""

    def __init__(self, cfg: LossAdaAttNCfg = LossAdaAttNCfg(), vgg: NormalizedVGG | None = None):
        super().__init__()
        self.cfg = cfg
        layers = [*cfg.content_loss_layers, *cfg.style_loss_layers]
        if not cfg.content_loss_layers or not all(l in (1, 2, 3, 4, 5) for l in layers):
            raise ValueError(f"LossAdaAttN: VGG layers are 1 .. 5 and there is at least one content layer, got {cfg}")
        if not all(s in ("mean", "std", "gram") for s in cfg.style_loss_stats):
            raise ValueError(f"LossAdaAttN: style statistics are 'mean', 'std', 'gram', got {cfg.style_loss_stats}")
        self.vgg = (vgg or NormalizedVGG(depth=max(layers))).eval()
        if self.vgg.depth < max(layers):
            raise ValueError(f"LossAdaAttN: the VGG ends at relu{self.vgg.depth}_1, the configuration needs relu{max(layers)}_1")
        for p in self.vgg.parameters():                                     # convert_to_buffer(..., persistent=False)
            p.requires_grad_(False)

    def forward(self, prediction, batch, gaussians=None, global_step: int = 0, details: dict | None = None) -> Tensor:
        image, style = batch["target"]["image"], batch["style"]["image"]
        b, v = image.shape[:2]
        if style.shape[0] != b:
            raise ValueError(f"LossAdaAttN: one style image per scene, got {tuple(style.shape)} for {b} scenes")
        cfg = self.cfg
        index = torch.arange(b, dtype=torch.int32).repeat_interleave(v)
        fp = self.vgg(prediction.color.reshape(b * v, *image.shape[2:]))
        with torch.no_grad():
            fc, fs = self.vgg(image.reshape(b * v, *image.shape[2:])), self.vgg(style)
        if not (image.is_cuda and image.dtype == torch.float32 and style.dtype == torch.float32 and prediction.color.dtype == torch.float32):
            return adaattn_expression(fp, fc, fs, cfg.lam, cfg.content_loss_layers, cfg.style_loss_layers, cfg.style_loss_stats, index, details)
        depth = max(cfg.content_loss_layers)
        with torch.no_grad():
            qs, ks = _adaattn_qk(fc, depth), _adaattn_qk(fs, depth)
        content = 0
        for l in sorted(cfg.content_loss_layers):
            with torch.no_grad():
                mean, std = adaattn_stats(F.instance_norm(qs[l - 1].flatten(2)), F.instance_norm(ks[l - 1].flatten(2)), fs[l - 1].flatten(2), index)
            d = {} if details is not None else None
            content = content + adaattn_l1(fp[l - 1].flatten(2), fc[l - 1].flatten(2), mean, std, d)
            if details is not None:
                details[f"cs{l}"], details[f"feature_grad{l}"] = d["cs"], d["feature_grad"]
        style_term = adaattn_style_term(fp, fs, cfg.style_loss_layers, cfg.style_loss_stats, index)
        if details is not None:
            details["content"], details["style"] = content.detach(), style_term.detach()
        return content + cfg.lam * style_term


def get_losses(cfgs) -> list:
    """the reference's loss registry (src/loss/__init__.py): this module's cfg dataclasses -> their modules, in order: mse, lpips, style, depth
    and adaattn."""
    table = {LossMseCfg: LossMse, LossLpipsCfg: LossLpips, LossStyleCfg: LossStyle, LossDepthCfg: LossDepth, LossAdaAttNCfg: LossAdaAttN}
    out = []
    for cfg in cfgs:
        if type(cfg) not in table:
            raise NotImplementedError(f"get_losses: no loss for {cfg!r}: an entry is one of this module's cfg dataclasses "
                                      "(LossMseCfg, LossLpipsCfg, LossStyleCfg, LossDepthCfg, LossAdaAttNCfg; adaattn is LossAdaAttNCfg, not a dict)")
        out.append(table[type(cfg)](cfg))
    return out
