"""Cameras of the fly-through videos: src/visualization/camera_trajectory/{interpolation,wobble}.py and the three trajectories of the
wrapper (model_wrapper_style.py:632-727: interpolation, wobble, exaggerated interpolation).

Device fp32 tensors go through ONE `gsr_trajectory` launch (csrc/gsr_outputs.hip): no Euler round trip through the host.  CPU tensors
take the float64 restatement below (torch only, no scipy) -- the yardstick of the kernel's tests.  Both compute in float64 to the end
and round once to float32; the reference rounds the pivot parameters to float32 before its last step, so it sits a few float32 ulps
of the pose's scale away from either.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Optional

import torch
from torch import Tensor

from . import _lib

TAU = 2 * math.pi


# ---- float64 restatement (host) ----
def _parallel(a: Tensor, b: Tensor, eps: float) -> Tensor:
    return ((a * b).sum(-1).abs() - 1).abs() < eps


def _frame(y: Tensor, z: Tensor) -> Tensor:
    """generate_coordinate_frame: columns [y x z, y, z]"""
    return torch.stack([torch.linalg.cross(y, z), y, z], dim=-1)


def _intersect_rays(oa: Tensor, a: Tensor, ob: Tensor, b: Tensor) -> Tensor:
    eye = torch.eye(3, dtype=oa.dtype)
    na = a[..., :, None] * a[..., None, :] - eye
    nb = b[..., :, None] * b[..., None, :] - eye
    rhs = (na @ oa[..., None] + nb @ ob[..., None])
    return torch.linalg.solve(na + nb, rhs)[..., 0]


def _euler_yz(m: Tensor):
    """Y and Z angles of the intrinsic "YXZ" decomposition m = Ry Rx Rz; at gimbal lock the third angle is 0 (scipy's rule)"""
    lock = m[..., 1, 0] ** 2 + m[..., 1, 1] ** 2 < 1e-24
    ay = torch.atan2(m[..., 0, 2], m[..., 2, 2])
    az = torch.atan2(m[..., 1, 0], m[..., 1, 1])
    ay_lock = torch.where(m[..., 1, 2] < 0, torch.atan2(m[..., 0, 1], m[..., 0, 0]), torch.atan2(-m[..., 0, 1], m[..., 0, 0]))
    return torch.where(lock, ay_lock, ay), torch.where(lock, torch.zeros_like(az), az)


def _pivot_params(e: Tensor, frame: Tensor, pivot: Tensor):
    tf = _frame(frame[..., :, 1], e[..., :3, 2])
    tr = (tf.transpose(-1, -2) @ (pivot - e[..., :3, 3])[..., None])[..., 0]
    ay, az = _euler_yz(frame.transpose(-1, -2) @ e[..., :3, :3])
    return tr, ay, az


def _circular(a: Tensor, b: Tensor, t: Tensor) -> Tensor:
    a, b = a % TAU, b % TAU
    d, al, ar = (b - a).abs(), a - TAU, a + TAU
    dl, dr = (b - al).abs(), (b - ar).abs()
    use_d = (d < dl) & (d < dr)
    use_l = (dl < dr) & ~use_d
    a0 = torch.where(use_d, a, torch.where(use_l, al, ar))
    return a0 + (b - a0) * t


def _interpolate_extrinsics_f64(initial: Tensor, final: Tensor, t: Tensor, eps: float) -> Tensor:
    """(*batch,4,4) x2, (F) -> float64 (*batch,F,4,4)"""
    A, B = torch.broadcast_tensors(initial.double(), final.double())
    t = t.double()
    a, b, oa, ob = A[..., :3, 2], B[..., :3, 2], A[..., :3, 3], B[..., :3, 3]
    par = _parallel(a, b, eps)
    pivot = 0.5 * (oa + ob)
    if (~par).any():
        pivot = pivot.clone()
        pivot[~par] = _intersect_rays(oa[~par], a[~par], ob[~par], b[~par])
    b2 = b.clone()
    b2[_parallel(a, b2, eps)] = torch.tensor([0.0, 0.0, 1.0], dtype=torch.float64)
    b2[_parallel(a, b2, eps)] = torch.tensor([0.0, 1.0, 0.0], dtype=torch.float64)
    y = torch.linalg.cross(a, b2)
    y = y / y.norm(dim=-1, keepdim=True)
    frame = _frame(y, a)
    ta, ya, za = _pivot_params(A, frame, pivot)
    tb, yb, zb = _pivot_params(B, frame, pivot)
    tr = ta[..., None, :] + (tb - ta)[..., None, :] * t[:, None]
    ay = _circular(ya[..., None], yb[..., None], t)
    az = _circular(za[..., None], zb[..., None], t)
    cy, sy, cz, sz, zero = ay.cos(), ay.sin(), az.cos(), az.sin(), torch.zeros_like(ay)
    euler = torch.stack([torch.stack([cy * cz, -cy * sz, sy], -1), torch.stack([sz, cz, zero], -1),
                         torch.stack([-sy * cz, sy * sz, cy], -1)], -2)
    rot = frame[..., None, :, :] @ euler
    tf = _frame(y[..., None, :].expand(rot.shape[:-2] + (3,)), rot[..., :, 2])
    origin = pivot[..., None, :] - (tf @ tr[..., None])[..., 0]
    out = torch.eye(4, dtype=torch.float64).expand(rot.shape[:-2] + (4, 4)).clone()
    out[..., :3, :3] = rot
    out[..., :3, 3] = origin
    return out


def _wobble_f64(c2w: Tensor, radius: Tensor, t: Tensor, num_rotations: int, scale_radius_with_t: bool) -> Tensor:
    """float64 (*batch,F,4,4) right-multiplied by the wobble transform; radius (*batch), t (F) as the caller holds them"""
    t = t.double()
    r = radius.double()[..., None] * (t if scale_radius_with_t else torch.ones_like(t))
    tx, ty = torch.sin(TAU * num_rotations * t) * r, -torch.cos(TAU * num_rotations * t) * r
    out = c2w.clone()
    out[..., :3, 3] = c2w[..., :3, 3] + c2w[..., :3, 0] * tx[..., None] + c2w[..., :3, 1] * ty[..., None]
    return out


# ---- device path ----
def _stream(dev) -> C.c_void_p:
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _is_hip(*ts: Tensor) -> bool:
    return all(x.is_cuda for x in ts)


def trajectory_hip(c2w_a: Tensor, c2w_b: Tensor, K_a: Tensor, K_b: Tensor, t: Tensor, *, t_scale: float = 1.0, t_shift: float = 0.0,
                   eps: float = 1e-4, hold_a: bool = False, wobble_factor: float = 0.0, wobble_rotations: int = 1,
                   wobble_scale_with_t: bool = True, wobble_radius: Optional[Tensor] = None):
    """`gsr_trajectory` (include/gsr.h): (P,4,4) x2, (P,3,3) x2, (F) device tensors -> c2w (P,F,4,4), K (P,F,3,3), one launch"""
    if not _is_hip(c2w_a, c2w_b, K_a, K_b, t):
        raise RuntimeError("trajectory_hip needs tensors on an MI355X (HIP) device; CPU tensors go through the functions of this module")
    f = lambda x: x.detach().contiguous().float()
    a, b, ka, kb, t = f(c2w_a), f(c2w_b), f(K_a), f(K_b), f(t)
    P, F = a.shape[0], t.shape[0]
    assert a.shape == b.shape == (P, 4, 4) and ka.shape == kb.shape == (P, 3, 3) and t.dim() == 1
    rad = None if wobble_radius is None else f(wobble_radius).reshape(P)
    c2w = torch.empty((P, F, 4, 4), dtype=torch.float32, device=a.device)
    K = torch.empty((P, F, 3, 3), dtype=torch.float32, device=a.device)
    _lib.check(_lib.load().gsr_trajectory(a.data_ptr(), b.data_ptr(), ka.data_ptr(), kb.data_ptr(), t.data_ptr(), P, F, float(t_scale),
                                          float(t_shift), float(eps), int(bool(hold_a)), float(wobble_factor), int(wobble_rotations),
                                          int(bool(wobble_scale_with_t)), rad.data_ptr() if rad is not None else None, c2w.data_ptr(),
                                          K.data_ptr(), _stream(a.device)), "gsr_trajectory")
    return c2w, K


def _pairs(x: Tensor, y: Tensor, n: int):
    x, y = torch.broadcast_tensors(x, y)
    return x.shape[:-2], x.reshape(-1, n, n), y.reshape(-1, n, n)


# ---- the reference's functions ----
@torch.no_grad()
def interpolate_extrinsics(initial: Tensor, final: Tensor, t: Tensor, eps: float = 1e-4) -> Tensor:
    """interpolation.py:207-255: (*batch,4,4) x2, (F) -> fp32 (*batch,F,4,4), rotating about the focus point of the two look rays"""
    if _is_hip(initial, final, t):
        batch, a, b = _pairs(initial, final, 4)
        eye = torch.eye(3, dtype=torch.float32, device=a.device).expand(a.shape[0], 3, 3)
        return trajectory_hip(a, b, eye, eye, t, eps=eps)[0].reshape(*batch, t.shape[0], 4, 4)
    return _interpolate_extrinsics_f64(initial, final, t, eps).float()


def interpolate_intrinsics(initial: Tensor, final: Tensor, t: Tensor) -> Tensor:
    """interpolation.py:8-16 (plain fp32 expression on either device; the kernel forms the same bits for `trajectory_cameras`)"""
    return initial[..., None, :, :] + (final - initial)[..., None, :, :] * t[:, None, None]


@torch.no_grad()
def generate_wobble_transformation(radius: Tensor, t: Tensor, num_rotations: int = 1, scale_radius_with_t: bool = True) -> Tensor:
    """wobble.py:7-22: radius (*batch), t (F) -> fp32 (*batch,F,4,4) translations in the image plane"""
    batch = radius.shape
    if _is_hip(radius, t):
        n = max(radius.numel(), 1)
        eye4 = torch.eye(4, dtype=torch.float32, device=t.device).expand(n, 4, 4)
        eye3 = torch.eye(3, dtype=torch.float32, device=t.device).expand(n, 3, 3)
        tf = trajectory_hip(eye4, eye4, eye3, eye3, t, hold_a=True, wobble_factor=1.0, wobble_rotations=num_rotations,
                            wobble_scale_with_t=scale_radius_with_t, wobble_radius=radius.reshape(n))[0]
        return tf.reshape(*batch, t.shape[0], 4, 4)
    eye = torch.eye(4, dtype=torch.float64).expand(*batch, t.shape[0], 4, 4)
    return _wobble_f64(eye, radius, t, num_rotations, scale_radius_with_t).float()


@torch.no_grad()
def generate_wobble(extrinsics: Tensor, radius: Tensor, t: Tensor) -> Tensor:
    """wobble.py:25-32: extrinsics (*batch,4,4) @ the wobble transform -> fp32 (*batch,F,4,4)"""
    batch = extrinsics.shape[:-2]
    radius = radius.expand(batch)
    if _is_hip(extrinsics, radius, t):
        e = extrinsics.reshape(-1, 4, 4)
        eye3 = torch.eye(3, dtype=torch.float32, device=t.device).expand(e.shape[0], 3, 3)
        out = trajectory_hip(e, e, eye3, eye3, t, hold_a=True, wobble_factor=1.0, wobble_radius=radius.reshape(-1))[0]
        return out.reshape(*batch, t.shape[0], 4, 4)
    e = extrinsics.double()[..., None, :, :].expand(*batch, t.shape[0], 4, 4)
    return _wobble_f64(e, radius, t, 1, True).float()


def smooth_time(num_frames: int, smooth: bool = True, device=None) -> Tensor:
    """render_video_generic's frame times: linspace(0, 1, num_frames), eased by (cos(pi (t + 1)) + 1) / 2"""
    t = torch.linspace(0, 1, num_frames, dtype=torch.float32, device=device)
    return (torch.cos(torch.pi * (t + 1)) + 1) / 2 if smooth else t


KINDS = {  # kind: (default num_frames, smooth, loop_reverse)
    "interpolation": (60, True, True), "wobble": (60, True, True), "interpolation_exaggerated": (300, False, False)}


@torch.no_grad()
def trajectory_cameras(context: dict, target: Optional[dict] = None, kind: str = "interpolation", num_frames: Optional[int] = None,
                       smooth: Optional[bool] = None):
    """The cameras of one of the wrapper's videos (model_wrapper_style.py:632-727) for a batch of b scenes:
    (extrinsics (b,F,4,4), intrinsics (b,F,3,3), near (b,F), far (b,F)).  The second endpoint is context view 1 when there are two
    context views, otherwise target view 0; wobble: radius 0.25 |o_a - o_b| scaled by t around context view 0; exaggerated: t * 5 - 2
    with a wobble of radius 0.5 |o_a - o_b| and 5 rotations.  near / far are context view 0's for every frame."""
    if kind not in KINDS:
        raise ValueError(f"unknown trajectory kind {kind!r}: one of {sorted(KINDS)}")
    frames, ease, _ = KINDS[kind]
    num_frames = frames if num_frames is None else num_frames
    ease = ease if smooth is None else smooth
    ext, intr = context["extrinsics"], context["intrinsics"]
    b, v = ext.shape[:2]
    if v == 2:
        ext_b, intr_b = ext[:, 1], intr[:, 1]
    else:
        if target is None:
            raise ValueError("with other than two context views the trajectory ends at target view 0: pass `target`")
        ext_b, intr_b = target["extrinsics"][:, 0], target["intrinsics"][:, 0]
    if kind != "interpolation" and v != 2:
        raise ValueError(f"the {kind} video takes its radius from two context views")
    ext_a, intr_a = ext[:, 0], intr[:, 0]
    t = smooth_time(num_frames, ease, device=ext.device)
    if _is_hip(ext, intr):
        opts = {"interpolation": {}, "wobble": dict(hold_a=True, wobble_factor=0.25),
                "interpolation_exaggerated": dict(t_scale=5.0, t_shift=-2.0, wobble_factor=0.5, wobble_rotations=5, wobble_scale_with_t=False)}[kind]
        c2w, K = trajectory_hip(ext_a, ext_b, intr_a, intr_b, t, **opts)
    else:
        delta = (ext_a[:, :3, 3].double() - ext_b[:, :3, 3].double()).norm(dim=-1)
        if kind == "interpolation":
            c2w, K = _interpolate_extrinsics_f64(ext_a, ext_b, t, 1e-4), interpolate_intrinsics(intr_a, intr_b, t)
        elif kind == "wobble":
            c2w = _wobble_f64(ext_a.double()[:, None].expand(b, num_frames, 4, 4), delta * 0.25, t, 1, True)
            K = intr_a[:, None].expand(b, num_frames, 3, 3).clone()
        else:
            tm = t * 5 - 2
            c2w = _wobble_f64(_interpolate_extrinsics_f64(ext_a, ext_b, tm, 1e-4), delta * 0.5, t, 5, False)
            K = interpolate_intrinsics(intr_a, intr_b, tm)
        c2w = c2w.float()
    near = context["near"][:, :1].expand(b, num_frames)
    far = context["far"][:, :1].expand(b, num_frames)
    return c2w, K, near, far
