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

from typing import NamedTuple, Optional

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


# ---- multi-view consistency of rendered sets (csrc/gsr_consistency.hip) -----------------------------------------------------------------
# The one objective number the stylization literature reports for a stylized scene (StyleRF, StyleGaussian, Styl3R): frame t of a
# fly-through is warped onto frame t + gap, pixels not visible in both are masked out, RMSE and LPIPS are taken over the rest; short
# range is the neighbouring frame, long range seven frames on.  Those works warp with an optical-flow network.  Here the warp is
# GEOMETRIC: every set `decoder.forward_styles` renders shares one geometry, and the pass returns the depth map the sets share next to
# the exact cameras.  The numbers are comparable between runs of this package, not with the papers' tables.
SHORT_RANGE_GAP, LONG_RANGE_GAP = 1, 7     # the literature's convention; defaults of `compute_consistency`, not constants of the kernel
CALLS = {"consistency_hip": 0, "consistency_expression": 0}     # calls of gsr_warp_consistency (one per chunk of sets) / of the expression


class ConsistencyResult(NamedTuple):
    rmse: Tensor                 # (S,P) float64: sqrt(sse / (3 count)), NaN where count == 0
    count: Tensor                # (P,) int32: valid pixels of the pair
    valid: Tensor                # (P,) float64: count / (H W)
    mask: Tensor                 # (P,H,W) bool
    warped: Optional[Tensor]     # (S,P,3,H,W) fp32, 0 at invalid pixels; None unless asked for
    sse: Tensor                  # (S,P) float64: the sum over valid pixels and channels of (warped - dst)^2


def consistency_pairs(num_frames: int, gap: int) -> Tensor:
    """int64 (max(num_frames - gap, 0), 2): rows (t, t + gap) = (src, dst), frame t warped onto frame t + gap"""
    if gap < 0 or num_frames < 0:
        raise ValueError(f"consistency_pairs: num_frames {num_frames} and gap {gap} must not be negative")
    t = torch.arange(max(num_frames - gap, 0), dtype=torch.int64)
    return torch.stack([t, t + gap], dim=1)


def _check_consistency(images: Tensor, depth: Tensor, extrinsics: Tensor, intrinsics: Tensor, pairs: Tensor, depth_tol: float):
    """shape / dtype refusals shared by both routes; returns images as (S,V,3,H,W)"""
    if images.dim() == 4:
        images = images[None]
    if images.dim() != 5 or images.shape[2] != 3 or images.shape[0] < 1:
        raise ValueError(f"warp_consistency: images are (S,V,3,H,W) or (V,3,H,W), got {tuple(images.shape)}")
    V, H, W = images.shape[1], images.shape[3], images.shape[4]
    if tuple(depth.shape) != (V, H, W):
        raise ValueError(f"warp_consistency: depth is (V,H,W) = {(V, H, W)}, the map the sets share, got {tuple(depth.shape)}")
    if tuple(extrinsics.shape) != (V, 4, 4) or tuple(intrinsics.shape) != (V, 3, 3):
        raise ValueError(f"warp_consistency: cameras are (V,4,4) c2w and (V,3,3) normalised intrinsics with V = {V}, got "
                         f"{tuple(extrinsics.shape)} and {tuple(intrinsics.shape)}")
    if H < 2 or W < 2:
        raise ValueError(f"warp_consistency: a bilinear tap needs height and width >= 2, got {H} x {W}")
    if pairs.dim() != 2 or pairs.shape[1] != 2 or pairs.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"warp_consistency: pairs are integer (P,2) rows (src, dst), got {pairs.dtype} {tuple(pairs.shape)}")
    if not (images.is_floating_point() and depth.is_floating_point() and extrinsics.is_floating_point() and intrinsics.is_floating_point()):
        raise ValueError("warp_consistency: images, depth and cameras are floating-point tensors")
    if not depth_tol >= 0:
        raise ValueError(f"warp_consistency: depth_tol is a relative slack >= 0, got {depth_tol}")
    return images


def _consistency_result(sse: Tensor, count: Tensor, mask: Tensor, warped, H: int, W: int) -> ConsistencyResult:
    rmse = (sse / (3.0 * count.to(torch.float64))).sqrt()                      # 0 / 0 = NaN where nothing is visible in both
    valid = count.to(torch.float64) / torch.tensor(float(H * W), dtype=torch.float64, device=count.device)     # (a tensor divisor: a true division on every device)
    return ConsistencyResult(rmse, count, valid, mask, warped, sse)


@torch.no_grad()
def warp_consistency_expression(images: Tensor, depth: Tensor, extrinsics: Tensor, intrinsics: Tensor, pairs: Tensor, *,
                                depth_tol: float = 0.05, return_warped: bool = False) -> ConsistencyResult:
    """The float64 restatement of `gsr_warp_consistency` (include/gsr.h states the formulas): the CPU path and the yardstick of the
    kernel.  Written element-wise, in the kernel's operation order -- no `@`, `einsum` or `grid_sample`, whose BLAS / interpolation
    kernels may fuse multiply-adds -- so the mask is the same set of IEEE operations on both sides; the sums over pixels are
    `torch.sum`, whose order differs from the kernel's (relative 3 H W 2^-52).  Works on any device."""
    images = _check_consistency(images, depth, extrinsics, intrinsics, pairs, depth_tol)
    CALLS["consistency_expression"] += 1
    S, V, _, H, W = images.shape
    P = pairs.shape[0]
    dev, f64 = depth.device, torch.float64
    img = images.detach().to(f64).reshape(S, V, 3, H * W)
    dep = depth.detach().to(f64).reshape(V, H * W)
    E, Kd = extrinsics.detach().to(dev, f64), intrinsics.detach().to(dev, f64)
    src, dst = pairs[:, 0].to(dev, torch.int64), pairs[:, 1].to(dev, torch.int64)
    pair_ok = (src >= 0) & (src < V) & (dst >= 0) & (dst < V)
    vi, vj = src.clamp(0, V - 1), dst.clamp(0, V - 1)
    e = lambda M, v, r, c: M[v, r, c][:, None, None]                           # one camera entry per pair, broadcast over (H, W)
    xs = torch.arange(W, dtype=f64, device=dev)[None, None, :]
    ys = torch.arange(H, dtype=f64, device=dev)[None, :, None]
    d = dep[vj].reshape(P, H, W)
    ok = pair_ok[:, None, None] & torch.isfinite(d) & (d > 0)
    # (divisors are device tensors: a Python scalar divisor is turned into a multiplication by its reciprocal on the GPU)
    u, v = (xs + 0.5) / torch.tensor(float(W), dtype=f64, device=dev), (ys + 0.5) / torch.tensor(float(H), dtype=f64, device=dev)
    xc = ((u - e(Kd, vj, 0, 2)) / e(Kd, vj, 0, 0)) * d
    yc = ((v - e(Kd, vj, 1, 2)) / e(Kd, vj, 1, 1)) * d
    wx = ((e(E, vj, 0, 0) * xc + e(E, vj, 0, 1) * yc) + e(E, vj, 0, 2) * d) + e(E, vj, 0, 3)
    wy = ((e(E, vj, 1, 0) * xc + e(E, vj, 1, 1) * yc) + e(E, vj, 1, 2) * d) + e(E, vj, 1, 3)
    wz = ((e(E, vj, 2, 0) * xc + e(E, vj, 2, 1) * yc) + e(E, vj, 2, 2) * d) + e(E, vj, 2, 3)
    dx, dy, dz = wx - e(E, vi, 0, 3), wy - e(E, vi, 1, 3), wz - e(E, vi, 2, 3)
    sx = (e(E, vi, 0, 0) * dx + e(E, vi, 1, 0) * dy) + e(E, vi, 2, 0) * dz      # R_i^T: the columns
    sy = (e(E, vi, 0, 1) * dx + e(E, vi, 1, 1) * dy) + e(E, vi, 2, 1) * dz
    z = (e(E, vi, 0, 2) * dx + e(E, vi, 1, 2) * dy) + e(E, vi, 2, 2) * dz
    ok = ok & (z > 0)
    px = ((e(Kd, vi, 0, 0) * sx) / z + e(Kd, vi, 0, 2)) * float(W) - 0.5
    py = ((e(Kd, vi, 1, 1) * sy) / z + e(Kd, vi, 1, 2)) * float(H) - 0.5
    ok = ok & (px >= 0) & (px <= float(W - 1)) & (py >= 0) & (py <= float(H - 1))
    zero = torch.zeros((), dtype=f64, device=dev)
    px, py = torch.where(ok, px, zero), torch.where(ok, py, zero)
    fx0, fy0 = px.floor().clamp(max=float(W - 2)), py.floor().clamp(max=float(H - 2))
    ax, ay = px - fx0, py - fy0
    w00, w01, w10, w11 = (1.0 - ax) * (1.0 - ay), ax * (1.0 - ay), (1.0 - ax) * ay, ax * ay
    t00 = (fy0.to(torch.int64) * W + fx0.to(torch.int64)).reshape(P, H * W)
    taps = (t00, t00 + 1, t00 + W, t00 + W + 1)
    bilinear = lambda q: ((w00 * q[0] + w01 * q[1]) + w10 * q[2]) + w11 * q[3]
    dsrc = dep[vi]
    dt = [torch.gather(dsrc, 1, t).reshape(P, H, W) for t in taps]
    for q in dt:
        ok = ok & torch.isfinite(q) & (q > 0)
    dt = [torch.where(ok, q, zero) for q in dt]
    D = bilinear(dt)
    ok = ok & ((z - D).abs() <= depth_tol * D)
    count = ok.sum(dim=(1, 2)).to(torch.int32)
    sse = torch.empty((S, P), dtype=f64, device=dev)
    warped = torch.empty((S, P, 3, H, W), dtype=torch.float32, device=dev) if return_warped else None
    for s in range(S):                                                          # (one set at a time: the taps of all sets at once are S x the memory)
        isrc = img[s][vi]                                                       # (P,3,HW)
        q = [torch.gather(isrc, 2, t[:, None, :].expand(P, 3, H * W)).reshape(P, 3, H, W) for t in taps]
        w = (((w00[:, None] * q[0] + w01[:, None] * q[1]) + w10[:, None] * q[2]) + w11[:, None] * q[3]).to(torch.float32)
        w = torch.where(ok[:, None], w, torch.zeros((), dtype=torch.float32, device=dev))
        diff = w.to(f64) - img[s][vj].reshape(P, 3, H, W)
        sq = diff * diff
        per_pixel = torch.where(ok, (sq[:, 0] + sq[:, 1]) + sq[:, 2], zero)
        sse[s] = per_pixel.sum(dim=(1, 2))
        if return_warped:
            warped[s] = w
    return _consistency_result(sse, count, ok, warped, H, W)


def _consistency_on_kernel(images: Tensor, depth: Tensor, extrinsics: Tensor, intrinsics: Tensor, pairs: Tensor) -> bool:
    return (images.is_cuda and depth.is_cuda and extrinsics.is_cuda and intrinsics.is_cuda and images.dtype == torch.float32
            and depth.dtype == torch.float32 and pairs.shape[0] > 0 and max(images.shape[-2:]) <= 16384)


@torch.no_grad()
def warp_consistency(images: Tensor, depth: Tensor, extrinsics: Tensor, intrinsics: Tensor, pairs: Tensor, *, depth_tol: float = 0.05,
                     return_warped: bool = False) -> ConsistencyResult:
    """Warp view pairs[p][0] onto view pairs[p][1] through the depth map and the cameras and compare where the point is seen by both.
      images      (S,V,3,H,W), or (V,3,H,W) for one set: colour sets rendered over ONE geometry, in [0, 1]
      depth       (V,H,W): the depth the sets share -- `DecoderOutput.depth`, the alpha-composited camera-space z of the rasterizer
                  (sum of w_k z_k over the composited splats, 0 where nothing was hit), IN THE UNITS OF THE CAMERAS' TRANSLATIONS.  A decoder
                  with `make_scale_invariant` renders z / near: multiply by near first (`evaluation.consistency_step` does)
      extrinsics  (V,4,4) camera-to-world with orthonormal rotations; intrinsics (V,3,3) normalised; pairs integer (P,2) rows (src, dst)
      depth_tol   the relative slack of the occlusion test |z - D| <= depth_tol * D.  The depth is alpha-composited, so at edges and on
                  semi-transparent surfaces it is a blend of surfaces: this slack is what absorbs that.  A parameter, not tuned here
    fp32 device images and depth go through `gsr_warp_consistency` (two launches per chunk of `GSR_CONSISTENCY_MAX_SETS` sets; the cameras
    are converted to float64 on the device); anything else is `warp_consistency_expression`.  `CALLS` counts the route."""
    images = _check_consistency(images, depth, extrinsics, intrinsics, pairs, depth_tol)
    if not _consistency_on_kernel(images, depth, extrinsics, intrinsics, pairs):
        return warp_consistency_expression(images, depth, extrinsics, intrinsics, pairs, depth_tol=depth_tol, return_warped=return_warped)
    import ctypes as C
    from . import _lib
    lib = _lib.load()
    S, V, _, H, W = images.shape
    P = pairs.shape[0]
    dev = depth.device
    img, dep = images.detach().contiguous(), depth.detach().contiguous()
    c2w, K = extrinsics.detach().to(dev, torch.float64).contiguous(), intrinsics.detach().to(dev, torch.float64).contiguous()
    pr = pairs.to(dev, torch.int32).contiguous()
    cap = _lib.GSR_CONSISTENCY_MAX_SETS
    scratch_bytes = lib.gsr_warp_consistency_scratch_bytes(P, min(S, cap), H, W)
    if not scratch_bytes:
        raise ValueError(f"warp_consistency: gsr_warp_consistency refuses P = {P}, H = {H}, W = {W}")
    scratch = torch.empty(scratch_bytes, dtype=torch.uint8, device=dev)
    mask = torch.empty((P, H, W), dtype=torch.uint8, device=dev)
    count = torch.empty(P, dtype=torch.int32, device=dev)
    sse = torch.empty((S, P), dtype=torch.float64, device=dev)
    warped = torch.empty((S, P, 3, H, W), dtype=torch.float32, device=dev) if return_warped else None
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    for s0 in range(0, S, cap):                                               # (mask and count come out the same from every chunk)
        n = min(cap, S - s0)
        chunk_sse = sse[s0:s0 + n]                                            # (contiguous rows)
        _lib.check(lib.gsr_warp_consistency(img[s0:s0 + n].data_ptr(), dep.data_ptr(), c2w.data_ptr(), K.data_ptr(), pr.data_ptr(), n, V, P, H, W,
                                            float(depth_tol), warped[s0:s0 + n].data_ptr() if return_warped else None, mask.data_ptr(),
                                            count.data_ptr(), chunk_sse.data_ptr(), scratch.data_ptr(), scratch_bytes, stream),
                   "gsr_warp_consistency")
        CALLS["consistency_hip"] += 1
    return _consistency_result(sse, count, mask.bool(), warped, H, W)


@torch.no_grad()
def compute_consistency(images: Tensor, depth: Tensor, extrinsics: Tensor, intrinsics: Tensor, *, gaps=(SHORT_RANGE_GAP, LONG_RANGE_GAP),
                        lpips: Optional[LPIPS] = None, depth_tol: float = 0.05, lpips_batch: int = 32) -> list:
    """Short- and long-range consistency of the frames of one fly-through: frame t against frame t + gaps[0] ("short") and t + gaps[1]
    ("long"), both ranges in ONE `warp_consistency` call.  images (S,F,3,H,W) or (F,3,H,W), depth (F,H,W), cameras (F,4,4) / (F,3,3) as
    `warp_consistency` takes them.  Returns one dict per set: "short_rmse", "long_rmse", "short_valid", "long_valid" -- floats, each the
    mean over the range's pairs with count > 0 (NaN when there is none) -- and, when an `LPIPS` module is passed, "short_lpips" /
    "long_lpips" from `compute_lpips(warped * mask, dst * mask)`, the masked-image convention of StyleRF and its successors, through the
    existing LPIPS kernels, `lpips_batch` images at a time."""
    if len(gaps) != 2:
        raise ValueError(f"compute_consistency: gaps are (short, long), got {gaps!r}")
    images5 = images[None] if images.dim() == 4 else images
    S, F = images5.shape[:2]
    ranges = [consistency_pairs(F, int(g)) for g in gaps]
    pairs = torch.cat(ranges)
    names = ("short", "long")
    nan = float("nan")
    if pairs.shape[0] == 0:
        _check_consistency(images5, depth, extrinsics, intrinsics, pairs, depth_tol)
        keys = [f"{n}_{k}" for n in names for k in (("rmse", "valid", "lpips") if lpips is not None else ("rmse", "valid"))]
        return [dict.fromkeys(keys, nan) for _ in range(S)]
    res = warp_consistency(images5, depth, extrinsics, intrinsics, pairs, depth_tol=depth_tol, return_warped=lpips is not None)
    P = pairs.shape[0]
    lp = None
    if lpips is not None:
        H, W = images5.shape[-2:]
        m = res.mask[None, :, None].to(res.warped.dtype)                       # (1,P,1,H,W)
        dst_index = pairs[:, 1].to(images5.device)
        a = (images5.detach()[:, dst_index].to(res.warped.dtype) * m).reshape(S * P, 3, H, W)
        b = (res.warped * m).reshape(S * P, 3, H, W)
        lp = torch.cat([compute_lpips(b[k:k + lpips_batch], a[k:k + lpips_batch], lpips) for k in range(0, S * P, lpips_batch)])
        lp = lp.reshape(S, P).to(torch.float64)
    seen = res.count > 0                                                        # (P,)
    out = [dict() for _ in range(S)]
    lo = 0
    for name, rng in zip(names, ranges):
        hi = lo + rng.shape[0]
        keep = seen[lo:hi]
        n = keep.sum().to(torch.float64)                                        # 0 pairs: 0 / 0 = NaN
        mean = lambda t: (torch.where(keep, t, torch.zeros((), dtype=t.dtype, device=t.device)).sum(dim=-1) / n).tolist()
        rmse, valid = mean(res.rmse[:, lo:hi]), mean(res.valid[None, lo:hi])[0]
        lpm = mean(lp[:, lo:hi]) if lp is not None else None
        for s in range(S):
            out[s][f"{name}_rmse"], out[s][f"{name}_valid"] = rmse[s], valid
            if lpm is not None:
                out[s][f"{name}_lpips"] = lpm[s]
        lo = hi
    return out
