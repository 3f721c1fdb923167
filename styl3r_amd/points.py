"""Bindings of csrc/gsr_points.hip (include/gsr.h): the teacher head's post-processing and the Regr3D point loss on libgsr_hip.so.
Device fp32 tensors only -- the callers (`encoder.PixelwiseTaskWithDPT`, `losses.Regr3D`) keep the plain torch expression for everything
else.  A missing library raises."""
from __future__ import annotations

import ctypes as C
from typing import Optional

import torch
from torch import Tensor

from . import _lib


def _stream(dev) -> C.c_void_p:
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def pointmap_post_expression(raw: Tensor) -> dict:
    """heads/postprocess.py:10-19 with depth mode ('exp', -inf, inf) and conf mode ('exp', 1, inf): raw (P,4,H,W) ->
    pts3d (P,H,W,3) = unit direction x expm1(norm), conf (P,H,W) = 1 + exp(raw[:, 3])"""
    f = raw.permute(0, 2, 3, 1)
    xyz = f[..., :3]
    d = xyz.norm(dim=-1, keepdim=True)
    return {"pts3d": xyz / d.clip(min=1e-8) * d.expm1(), "conf": 1 + f[..., 3].exp()}


def pointmap_post(raw: Tensor) -> dict:
    """`pointmap_post_expression` in one pass (gsr_pointmap_post) for a device fp32 head output that needs no gradient (the teacher is frozen)"""
    if not (raw.is_cuda and raw.dtype == torch.float32 and not (raw.requires_grad and torch.is_grad_enabled())):
        return pointmap_post_expression(raw)
    raw = raw.contiguous()
    P, ch, H, W = raw.shape
    assert ch == 4, "pointmap_post takes the 4-channel (xyz, confidence) head output"
    pts = torch.empty((P, H, W, 3), dtype=torch.float32, device=raw.device)
    conf = torch.empty((P, H, W), dtype=torch.float32, device=raw.device)
    _lib.check(_lib.load().gsr_pointmap_post(raw.data_ptr(), P, H, W, pts.data_ptr(), conf.data_ptr(), _stream(raw.device)), "gsr_pointmap_post")
    return {"pts3d": pts, "conf": conf}


def _image_block_contiguous(t: Tensor) -> bool:
    """(B, ..., 3) whose per-image block is packed: what means[:, k] of a (b,v,h,w,1,3) tensor is"""
    return t[0].is_contiguous() and (t.shape[0] == 1 or t.stride(0) >= t[0].numel())


class _Regr3DHip(torch.autograd.Function):
    """Regr3D on gsr_regr3d_fwd / _bwd.  pr1 / pr2 are read through their batch stride (no copy of means[:, k]); the teacher side is
    ground truth.  `details`: a dict that receives status (2,B,2) int32, quantiles (2,B,2) and valid (2,B,N) uint8, or None."""

    @staticmethod
    def forward(ctx, pr1, pr2, gt1, gt2, conf1, conf2, norm, disable_view1, dist_clip, details):
        lib = _lib.load()
        B = gt1.shape[0]
        N = gt1[0].numel() // 3
        pr1 = pr1 if _image_block_contiguous(pr1) else pr1.contiguous()
        pr2 = pr2 if _image_block_contiguous(pr2) else pr2.contiguous()
        gt1, gt2, conf1, conf2 = gt1.contiguous(), gt2.contiguous(), conf1.contiguous(), conf2.contiguous()
        dev = gt1.device
        scratch = torch.empty(lib.gsr_regr3d_scratch_bytes(B, N), dtype=torch.uint8, device=dev)
        loss = torch.empty((), dtype=torch.float32, device=dev)
        status = torch.empty((2, B, 2), dtype=torch.int32, device=dev)
        quant = torch.empty((2, B, 2), dtype=torch.float32, device=dev) if details is not None else None
        valid = torch.empty((2, B, N), dtype=torch.uint8, device=dev) if details is not None else None
        s1 = pr1.stride(0) if B > 1 else 3 * N
        s2 = pr2.stride(0) if B > 1 else 3 * N
        _lib.check(lib.gsr_regr3d_fwd(gt1.data_ptr(), gt2.data_ptr(), conf1.data_ptr(), conf2.data_ptr(), pr1.data_ptr(), pr2.data_ptr(), s1, s2,
                                      B, N, int(norm), int(bool(disable_view1)), float(dist_clip or 0.0), scratch.data_ptr(), loss.data_ptr(),
                                      status.data_ptr(), quant.data_ptr() if quant is not None else None,
                                      valid.data_ptr() if valid is not None else None, _stream(dev)), "gsr_regr3d_fwd")
        if details is not None:
            details.update(status=status, quantiles=quant, valid=valid)
        ctx.save_for_backward(pr1, pr2, gt1, gt2, scratch)
        ctx.cfg = (B, N, s1, s2, int(norm), int(bool(disable_view1)))
        return loss

    @staticmethod
    def backward(ctx, g):
        pr1, pr2, gt1, gt2, scratch = ctx.saved_tensors
        B, N, s1, s2, norm, dv1 = ctx.cfg
        d1 = torch.empty((B,) + tuple(pr1.shape[1:]), dtype=torch.float32, device=pr1.device)
        d2 = torch.empty((B,) + tuple(pr2.shape[1:]), dtype=torch.float32, device=pr2.device)
        g = g.contiguous().float()
        _lib.check(_lib.load().gsr_regr3d_bwd(gt1.data_ptr(), gt2.data_ptr(), pr1.data_ptr(), pr2.data_ptr(), s1, s2, B, N, norm, dv1, g.data_ptr(),
                                              scratch.data_ptr(), d1.data_ptr(), d2.data_ptr(), _stream(pr1.device)), "gsr_regr3d_bwd")
        return d1, d2, None, None, None, None, None, None, None, None


def regr3d_hip_ok(gt1: Tensor, gt2: Tensor, pr1: Tensor, pr2: Tensor, conf1: Tensor, conf2: Tensor) -> bool:
    ts = (gt1, gt2, pr1, pr2, conf1, conf2)
    return (all(t.is_cuda and t.dtype == torch.float32 for t in ts) and not any(t.requires_grad for t in (gt1, gt2, conf1, conf2))
            and gt1.dim() >= 3 and gt1.shape == gt2.shape == pr1.shape == pr2.shape and gt1.shape[-1] == 3
            and conf1.shape == conf2.shape == gt1.shape[:-1] and gt1.shape[0] >= 1 and gt1[0].numel() >= 6)


def regr3d_hip(gt1: Tensor, gt2: Tensor, pr1: Tensor, pr2: Tensor, conf1: Tensor, conf2: Tensor, norm: bool, disable_view1: bool = False,
               dist_clip: Optional[float] = None, details: Optional[dict] = None) -> Tensor:
    if dist_clip is not None and not dist_clip > 0:
        raise ValueError("Regr3D on the kernels: dist_clip must be positive")
    return _Regr3DHip.apply(pr1, pr2, gt1, gt2, conf1, conf2, norm, disable_view1, dist_clip, details)
