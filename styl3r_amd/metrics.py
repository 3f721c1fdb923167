"""Image scores of the test step: `compute_psnr`, `compute_ssim`, `compute_lpips` (src/evaluation/metrics.py:11-52), same signatures and
`(batch,)` results.

fp32 device images go through libgsr_hip.so's `gsr_image_scores` (csrc/gsr_ssim.hip): one pass over both images yields SSIM and the
clipped mean squared error PSNR is formed from, so `image_scores` returns both from one launch.  Anything else (CPU tensors, other
dtypes) takes the plain float64 expression of the same formulas, as `losses.mse_loss` does.

SSIM is what the reference gets from `skimage.metrics.structural_similarity(gt, hat, win_size=11, gaussian_weights=True, channel_axis=0,
data_range=1.0)`: the separable Gaussian window of sigma 1.5 and radius 5, sample covariance (x 121/120), C1 = 1e-4, C2 = 9e-4, the map
averaged over the pixels left after skimage's crop of 5 from every edge and then over the channels; the inputs are not clipped.  Every
kept pixel's window lies inside the image, so the valid filter of the interior is exact and skimage's boundary mode never enters.

`compute_pose_error` (src/evaluation/metrics.py:87-99) and `pose_auc` (src/misc/cam_utils.py:181-193) are the relative-pose scores.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F
from torch import Tensor

from .losses import LPIPS

WIN_RADIUS, WIN_SIGMA = 5, 1.5           # int(truncate 3.5 * sigma 1.5 + 0.5) = 5: an 11 x 11 window
SSIM_C1, SSIM_C2 = 1e-4, 9e-4            # (K1 data_range)^2, (K2 data_range)^2 with K1 = 0.01, K2 = 0.03, data_range = 1
COV_NORM = 121.0 / 120.0                 # use_sample_covariance: NP / (NP - 1), NP = 11^2


def gaussian_window(dtype=torch.float64) -> Tensor:
    """scipy.ndimage's 1-D Gaussian of sigma 1.5 and radius 5, normalised to sum 1 (11 taps)"""
    x = torch.arange(-WIN_RADIUS, WIN_RADIUS + 1, dtype=torch.float64)
    w = torch.exp(-0.5 / WIN_SIGMA ** 2 * x * x)
    return (w / w.sum()).to(dtype)


def _check_pair(ground_truth: Tensor, predicted: Tensor, need_window: bool) -> None:
    if ground_truth.dim() != 4 or ground_truth.shape != predicted.shape:
        raise ValueError(f"image scores take two (batch, channel, height, width) tensors of one shape, got {tuple(ground_truth.shape)} "
                         f"and {tuple(predicted.shape)}")
    if need_window and min(ground_truth.shape[-2:]) < 2 * WIN_RADIUS + 1:
        raise ValueError("win_size exceeds image extent: SSIM needs height and width >= 11")


def _on_kernel(ground_truth: Tensor, predicted: Tensor) -> bool:
    return (ground_truth.is_cuda and predicted.is_cuda and ground_truth.dtype == torch.float32 and predicted.dtype == torch.float32
            and ground_truth.numel() > 0)


def _scores_hip(ground_truth: Tensor, predicted: Tensor):
    """(ssim (N,), mse (N,)) fp32 from gsr_image_scores"""
    import ctypes as C
    from . import _lib
    lib = _lib.load()
    gt, pred = ground_truth.detach().contiguous(), predicted.detach().contiguous()
    n, c, h, w = gt.shape
    dev = gt.device
    scratch = torch.empty(lib.gsr_image_scores_scratch_bytes(n, c, h, w), dtype=torch.uint8, device=dev)
    ssim = torch.empty(n, dtype=torch.float32, device=dev)
    mse = torch.empty(n, dtype=torch.float32, device=dev)
    _lib.check(lib.gsr_image_scores(gt.data_ptr(), pred.data_ptr(), n, c, h, w, ssim.data_ptr(), mse.data_ptr(), scratch.data_ptr(),
                                    C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)), "gsr_image_scores")
    return ssim, mse


def _filter_valid(t: Tensor, w: Tensor) -> Tensor:
    """separable 11 x 11 Gaussian filter of (N, C, H, W), only where the window lies inside: (N, C, H - 10, W - 10)"""
    n, c, h, wd = t.shape
    x = t.reshape(n * c, 1, h, wd)
    x = F.conv2d(x, w.view(1, 1, 1, -1))
    x = F.conv2d(x, w.view(1, 1, -1, 1))
    return x.reshape(n, c, h - 2 * WIN_RADIUS, wd - 2 * WIN_RADIUS)


def _ssim_expression(ground_truth: Tensor, predicted: Tensor) -> Tensor:
    x, y = ground_truth.detach().double(), predicted.detach().double()
    w = gaussian_window(torch.float64).to(x.device)
    ux, uy = _filter_valid(x, w), _filter_valid(y, w)
    vx = COV_NORM * (_filter_valid(x * x, w) - ux * ux)
    vy = COV_NORM * (_filter_valid(y * y, w) - uy * uy)
    vxy = COV_NORM * (_filter_valid(x * y, w) - ux * uy)
    s = ((2 * ux * uy + SSIM_C1) * (2 * vxy + SSIM_C2)) / ((ux * ux + uy * uy + SSIM_C1) * (vx + vy + SSIM_C2))
    return s.mean(dim=(2, 3)).mean(dim=1)


def _mse_expression(ground_truth: Tensor, predicted: Tensor) -> Tensor:
    return ((ground_truth.detach().double().clip(0, 1) - predicted.detach().double().clip(0, 1)) ** 2).flatten(1).mean(dim=1)


def _psnr(mse: Tensor) -> Tensor:
    return -10 * mse.log10()                 # +inf for identical images


@torch.no_grad()
def image_scores(ground_truth: Tensor, predicted: Tensor):
    """(psnr (batch,), ssim (batch,)) of (batch, channel, height, width) images; one kernel pass for fp32 device images"""
    _check_pair(ground_truth, predicted, need_window=True)
    if _on_kernel(ground_truth, predicted):
        ssim, mse = _scores_hip(ground_truth, predicted)
        return _psnr(mse), ssim
    dt = predicted.dtype
    return _psnr(_mse_expression(ground_truth, predicted)).to(dt), _ssim_expression(ground_truth, predicted).to(dt)


@torch.no_grad()
def compute_psnr(ground_truth: Tensor, predicted: Tensor) -> Tensor:
    """src/evaluation/metrics.py:11-20.  The kernel is the SSIM pass, whose window needs 11 x 11 pixels: smaller images take the expression."""
    _check_pair(ground_truth, predicted, need_window=False)
    if _on_kernel(ground_truth, predicted) and min(ground_truth.shape[-2:]) >= 2 * WIN_RADIUS + 1:
        return _psnr(_scores_hip(ground_truth, predicted)[1])
    return _psnr(_mse_expression(ground_truth, predicted)).to(predicted.dtype)


@torch.no_grad()
def compute_ssim(ground_truth: Tensor, predicted: Tensor) -> Tensor:
    """src/evaluation/metrics.py:38-52 (skimage structural_similarity per image, see the module docstring)"""
    return image_scores(ground_truth, predicted)[1]


_LPIPS: dict = {}


def get_lpips(device) -> LPIPS:
    """one LPIPS-VGG module per device, in eval mode (metrics.py:23-25).  It starts with random weights (`weights_loaded` False), so its
    scores mean nothing until `LPIPS.load_lpips_weights(lin_sd, vgg16_sd)` has been called on it."""
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    if device not in _LPIPS:
        _LPIPS[device] = LPIPS().to(device).eval().requires_grad_(False)
    return _LPIPS[device]


@torch.no_grad()
def compute_lpips(ground_truth: Tensor, predicted: Tensor, lpips: LPIPS | None = None) -> Tensor:
    """src/evaluation/metrics.py:28-35: LPIPS(ground_truth, predicted, normalize=True) per image -> (batch,).  On the HIP route (losses.LPIPS)
    for fp32 device images; `lpips` defaults to the module of `get_lpips(predicted.device)`."""
    _check_pair(ground_truth, predicted, need_window=False)
    module = lpips if lpips is not None else get_lpips(predicted.device)
    return module.forward(ground_truth, predicted, normalize=True)[:, 0, 0, 0]



# ---- relative camera pose (src/evaluation/metrics.py:70-99, src/misc/cam_utils.py:181-193) --------------------------------------------
@torch.no_grad()
def compute_pose_error(pose_gt: Tensor, pose_pred: Tensor):
    """(error_t, error_t_scale, error_R) of camera-to-world poses (..., 4, 4): the angle between the translations in degrees, folded to
    min(e, 180 - e) (the sign ambiguity of an essential-matrix estimate), the norm of their difference, and the rotation angle of
    R_pred^T R_gt in degrees.  Any leading batch dimensions; the results have their shape."""
    R_gt, t_gt = pose_gt[..., :3, :3], pose_gt[..., :3, 3]
    R, t = pose_pred[..., :3, :3], pose_pred[..., :3, 3]
    cos_t = ((t * t_gt).sum(-1) / (t.norm(dim=-1) * t_gt.norm(dim=-1))).clamp(-1.0, 1.0)
    error_t = torch.rad2deg(torch.acos(cos_t))
    error_t = torch.minimum(error_t, 180 - error_t)
    error_t_scale = (t - t_gt).norm(dim=-1)
    cos_r = (((R * R_gt).sum(dim=(-2, -1)) - 1) / 2).clamp(-1.0, 1.0)          # trace(R^T R_gt) = sum_ij R_ij R_gt_ij
    error_R = torch.rad2deg(torch.abs(torch.acos(cos_r)))
    return error_t, error_t_scale, error_R


def pose_auc(errors, thresholds):
    """area under the recall-over-error curve up to each threshold, divided by the threshold (the pose-AUC of the NoPoSplat tables)"""
    import numpy as np
    e = np.sort(np.asarray(errors, dtype=np.float64).reshape(-1))
    recall = (np.arange(len(e)) + 1) / len(e)
    e, recall = np.r_[0.0, e], np.r_[0.0, recall]
    aucs = []
    for t in thresholds:
        last = np.searchsorted(e, t)
        r, x = np.r_[recall[:last], recall[last - 1]], np.r_[e[:last], t]
        aucs.append(float(np.sum(0.5 * (r[1:] + r[:-1]) * np.diff(x)) / t))
    return aucs
