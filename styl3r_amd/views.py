"""View selection: which frames of a scene become context and target views.

Three parts, with the reference's names and semantics:

  view_overlap              the share of one view's pixel rays whose segment [0, inf), projected into another view, crosses that image
                            (src/geometry/epipolar_lines.py::project_rays on get_world_rays of sample_image_grid) -- for MANY pairs in
                            one call.  Device cameras go through `gsr_view_overlap` (csrc/gsr_views.hip); CPU cameras through the
                            float64 torch restatement below (`overlap_counts_torch`), which is also what the GPU tests hold the kernel to.
  EvaluationIndexGenerator  src/evaluation/evaluation_index_generator.py: `add_scene` is its test_step on cameras alone.  All candidate
                            partners of a context frame go out in ONE view_overlap call and come back in one read-back; the host then
                            replays the reference's walk, quirks included.
  the samplers              src/dataset/view_sampler/: bounded, evaluation, arbitrary, all, `add_additional_context_index` and
                            `get_view_sampler`, drawing from torch's global CPU generator in the reference's call order.

The overlap arithmetic (both paths, float64, every product and sum rounded once in the order written here):
  pixel      x = (col + 0.5) / W, y = (row + 0.5) / H in fp32, then widened
  ray        K^-1 (x, y, 1), normalised, rotated by the camera-to-world matrix; the origin is its translation column
  into b     world-to-camera of b (the 4 x 4 inverse by 2 x 2 minors, the 3 x 3 by cofactors -- no solver library)
  frame      the four lines x = 0, x = 1, y = 0, y = 1: t = (c oz - os) / (ds - c dz) with c = (value - cs) / fs, the other coordinate
             co + fo (oo (c dz - ds) + do (os - c oz)) / (dz os - ds oz); no guard against zero denominators
  valid      other coordinate in [-1e-6, 1 + 1e-6], z(t) > -1e-6, t > -1e-6
  min / max  invalid t become +inf / -inf, the first index of the extreme wins, the flag of THAT entry is the result
  zero       the origin (the direction if |origin| < 1e-6) over z + 2^-23, NaN -> 0, +-inf -> +-1e8, through K; in bounds and
             z > -1e-6; false if origin z < 1e-6 away from the camera
  infinity   the direction, the same way
  overlaps   (zero | frame-min) and (infinity | frame-max)
Previews (the reference's save_previews) are not built.
"""
from __future__ import annotations

import ctypes as C
import json
from dataclasses import asdict, dataclass
from pathlib import Path
from typing import Optional, Union

import torch
from torch import Tensor

from . import _lib

_EPS = 1e-6
_Z_EPS = 1.1920928955078125e-07           # torch.finfo(torch.float32).eps
_BIG = 1e8
_MAX_RAYS = 1 << 24                        # float32(count) and float32(H W) stay exact
_CHUNK_RAYS = 1 << 21                      # rays per slice of the torch restatement (a few dozen float64 temporaries each)


# ---- the float64 restatement ----
def _inverse3(m: Tensor) -> Tensor:
    a, b, c, d, e, f, g, h, i = (m[..., r, s] for r in range(3) for s in range(3))
    c00, c01, c02 = e * i - f * h, c * h - b * i, b * f - c * e
    c10, c11, c12 = f * g - d * i, a * i - c * g, c * d - a * f
    c20, c21, c22 = d * h - e * g, b * g - a * h, a * e - b * d
    det = (a * c00 + b * c10) + c * c20
    return torch.stack([c00, c01, c02, c10, c11, c12, c20, c21, c22], -1).div(det[..., None]).reshape(*m.shape)


def _inverse4(m: Tensor) -> Tensor:
    """general 4 x 4 inverse: the adjugate from the 2 x 2 minors of the upper (s) and the lower (c) row pair, over the determinant"""
    A = lambda r, c: m[..., r, c]
    s0, s1, s2 = A(0, 0) * A(1, 1) - A(1, 0) * A(0, 1), A(0, 0) * A(1, 2) - A(1, 0) * A(0, 2), A(0, 0) * A(1, 3) - A(1, 0) * A(0, 3)
    s3, s4, s5 = A(0, 1) * A(1, 2) - A(1, 1) * A(0, 2), A(0, 1) * A(1, 3) - A(1, 1) * A(0, 3), A(0, 2) * A(1, 3) - A(1, 2) * A(0, 3)
    c5, c4, c3 = A(2, 2) * A(3, 3) - A(3, 2) * A(2, 3), A(2, 1) * A(3, 3) - A(3, 1) * A(2, 3), A(2, 1) * A(3, 2) - A(3, 1) * A(2, 2)
    c2, c1, c0 = A(2, 0) * A(3, 3) - A(3, 0) * A(2, 3), A(2, 0) * A(3, 2) - A(3, 0) * A(2, 2), A(2, 0) * A(3, 1) - A(3, 0) * A(2, 1)
    det = ((((s0 * c5 - s1 * c4) + s2 * c3) + s3 * c2) - s4 * c1) + s5 * c0
    adj = [(A(1, 1) * c5 - A(1, 2) * c4) + A(1, 3) * c3, (A(0, 2) * c4 - A(0, 1) * c5) - A(0, 3) * c3,
           (A(3, 1) * s5 - A(3, 2) * s4) + A(3, 3) * s3, (A(2, 2) * s4 - A(2, 1) * s5) - A(2, 3) * s3,
           (A(1, 2) * c2 - A(1, 0) * c5) - A(1, 3) * c1, (A(0, 0) * c5 - A(0, 2) * c2) + A(0, 3) * c1,
           (A(3, 2) * s2 - A(3, 0) * s5) - A(3, 3) * s1, (A(2, 0) * s5 - A(2, 2) * s2) + A(2, 3) * s1,
           (A(1, 0) * c4 - A(1, 1) * c2) + A(1, 3) * c0, (A(0, 1) * c2 - A(0, 0) * c4) - A(0, 3) * c0,
           (A(3, 0) * s4 - A(3, 1) * s2) + A(3, 3) * s0, (A(2, 1) * s2 - A(2, 0) * s4) - A(2, 3) * s0,
           (A(1, 1) * c1 - A(1, 0) * c3) - A(1, 2) * c0, (A(0, 0) * c3 - A(0, 1) * c1) + A(0, 2) * c0,
           (A(3, 1) * s1 - A(3, 0) * s3) - A(3, 2) * s0, (A(2, 0) * s3 - A(2, 1) * s1) + A(2, 2) * s0]
    return torch.stack(adj, -1).div(det[..., None]).reshape(*m.shape)


def _in01(v: Tensor) -> Tensor:
    return (v >= -_EPS) & (v <= 1 + _EPS)


def _point_valid(K, px, py, pz) -> Tensor:
    den = pz + _Z_EPS
    qx, qy, qz = ((p / den).nan_to_num(nan=0.0, posinf=_BIG, neginf=-_BIG) for p in (px, py, pz))
    x = (K[0] * qx + K[1] * qy) + K[2] * qz
    y = (K[3] * qx + K[4] * qy) + K[5] * qz
    return _in01(x) & _in01(y) & (pz > -_EPS)


def _frame_hit(fs, fo, cs, co, value, os_, oo, oz, ds, dn, dz):
    c = (value - cs) / fs
    t = (c * oz - os_) / (ds - c * dz)
    other = co + (fo * (oo * (c * dz - ds) + dn * (os_ - c * oz))) / (dz * os_ - ds * oz)
    return t, _in01(other) & (oz + t * dz > -_EPS) & (t > -_EPS)


def _directed_counts(Ki, E, M, K, x, y) -> Tensor:
    """Ki, E: source views' inverse intrinsics (D,9) / camera-to-world (D,16); M, K: destination views' world-to-camera (D,16) /
    intrinsics (D,9); x, y (R,) float64 pixel coordinates -> (D,) int64 counts of overlapping rays"""
    Ki, E, M, K = (t.t()[:, :, None] for t in (Ki, E, M, K))                 # [entry] -> (D,1)
    wx, wy, wz = E[3], E[7], E[11]
    ox = ((M[0] * wx + M[1] * wy) + M[2] * wz) + M[3]
    oy = ((M[4] * wx + M[5] * wy) + M[6] * wz) + M[7]
    oz = ((M[8] * wx + M[9] * wy) + M[10] * wz) + M[11]
    at_camera = ((ox * ox + oy * oy) + oz * oz).sqrt() < _EPS
    depth_zero = oz < _EPS
    cx, cy, cz = (Ki[0] * x + Ki[1] * y) + Ki[2], (Ki[3] * x + Ki[4] * y) + Ki[5], (Ki[6] * x + Ki[7] * y) + Ki[8]
    length = ((cx * cx + cy * cy) + cz * cz).sqrt()
    cx, cy, cz = cx / length, cy / length, cz / length
    ux, uy, uz = (E[0] * cx + E[1] * cy) + E[2] * cz, (E[4] * cx + E[5] * cy) + E[6] * cz, (E[8] * cx + E[9] * cy) + E[10] * cz
    dx, dy, dz = (M[0] * ux + M[1] * uy) + M[2] * uz, (M[4] * ux + M[5] * uy) + M[6] * uz, (M[8] * ux + M[9] * uy) + M[10] * uz
    hits = [_frame_hit(K[0], K[4], K[2], K[5], 0.0, ox, oy, oz, dx, dy, dz), _frame_hit(K[0], K[4], K[2], K[5], 1.0, ox, oy, oz, dx, dy, dz),
            _frame_hit(K[4], K[0], K[5], K[2], 0.0, oy, ox, oz, dy, dx, dz), _frame_hit(K[4], K[0], K[5], K[2], 1.0, oy, ox, oz, dy, dx, dz)]
    inf = torch.full_like(dx, float("inf"))
    t0, v0 = hits[0]
    lo, hi = torch.where(v0, t0, inf), torch.where(v0, t0, -inf)
    lo_valid, hi_valid = v0.clone(), v0.clone()
    for t, v in hits[1:]:
        tl, th = torch.where(v, t, inf), torch.where(v, t, -inf)
        less, more = tl < lo, th > hi                                        # strict: the first index keeps a tie
        lo, lo_valid = torch.where(less, tl, lo), torch.where(less, v, lo_valid)
        hi, hi_valid = torch.where(more, th, hi), torch.where(more, v, hi_valid)
    zero_valid = _point_valid(K, torch.where(at_camera, dx, ox), torch.where(at_camera, dy, oy), torch.where(at_camera, dz, oz))
    zero_valid = zero_valid & ~(depth_zero & ~at_camera)
    inf_valid = _point_valid(K, dx, dy, dz)
    return ((zero_valid | lo_valid) & (inf_valid | hi_valid)).sum(-1)


def pixel_coordinates(H: int, W: int, device):
    """sample_image_grid's coordinates, (xs (W,), ys (H,)) float64 on `device`: (idx + 0.5) / length by an fp32 division, then widened.
    Formed on the HOST whatever the device: a device's own fp32 division need not round correctly (one ulp off at W = 640, which moves
    rays), the kernel's and the reference's CPU division do."""
    xs = ((torch.arange(W) + 0.5) / W).to(device, torch.float64)
    ys = ((torch.arange(H) + 0.5) / H).to(device, torch.float64)
    return xs, ys


def overlap_counts_torch(extrinsics: Tensor, intrinsics: Tensor, pairs: Tensor, image_shape) -> Tensor:
    """the batched float64 restatement on the tensors' own device: (P,2) int32 counts (every pair index must be valid)"""
    H, W = (int(s) for s in image_shape)
    dev = extrinsics.device
    E = extrinsics.detach().to(torch.float64)
    K = intrinsics.detach().to(torch.float64)
    V = E.shape[0]
    Ki, M = _inverse3(K).reshape(V, 9), _inverse4(E).reshape(V, 16)
    E, K = E.reshape(V, 16), K.reshape(V, 9)
    xs, ys = pixel_coordinates(H, W, dev)
    x, y = xs.repeat(H), ys.repeat_interleave(W)
    pairs = pairs.to(dev, torch.int64)
    src, dst = pairs.reshape(-1), pairs.flip(-1).reshape(-1)                # direction 2 p + d: pairs[p][d] -> pairs[p][1 - d]
    D = src.numel()
    counts = torch.zeros(D, dtype=torch.int64, device=dev)
    rays = max(1, _CHUNK_RAYS // min(H * W, _CHUNK_RAYS))                   # directions per slice
    step_r = min(H * W, _CHUNK_RAYS)
    for d0 in range(0, D, rays):
        s, t = src[d0:d0 + rays], dst[d0:d0 + rays]
        for r0 in range(0, H * W, step_r):
            counts[d0:d0 + rays] += _directed_counts(Ki[s], E[s], M[t], K[t], x[r0:r0 + step_r], y[r0:r0 + step_r])
    return counts.to(torch.int32).reshape(-1, 2)


# ---- view_overlap ----
def _stream(dev) -> C.c_void_p:
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _check_cameras(extrinsics: Tensor, intrinsics: Tensor, image_shape):
    H, W = (int(s) for s in image_shape)
    if extrinsics.dim() != 3 or extrinsics.shape[1:] != (4, 4) or intrinsics.shape != (extrinsics.shape[0], 3, 3):
        raise ValueError(f"expected extrinsics (V,4,4) and intrinsics (V,3,3), got {tuple(extrinsics.shape)} and {tuple(intrinsics.shape)}")
    if extrinsics.shape[0] < 1 or H < 1 or W < 1 or H * W > _MAX_RAYS:
        raise ValueError(f"no views, or an image of {H} x {W}: H W must lie in 1 .. 2^24")
    if intrinsics.device != extrinsics.device:
        raise ValueError("extrinsics and intrinsics live on different devices")
    return H, W


def view_overlap_device(extrinsics: Tensor, intrinsics: Tensor, pairs: Tensor, image_shape) -> Tensor:
    """the kernel as it is: fp32 device cameras, int32 DEVICE pairs (P,2), nothing validated on the host -> device counts (P,2) int32
    (-1, -1 for a pair outside [0, V)).  No host sync."""
    H, W = _check_cameras(extrinsics, intrinsics, image_shape)
    if not extrinsics.is_cuda or not pairs.is_cuda or pairs.dtype != torch.int32 or pairs.dim() != 2 or pairs.shape[1] != 2:
        raise RuntimeError("view_overlap_device takes device cameras and an int32 (P,2) device tensor of pairs")
    lib, dev, V, P = _lib.load(), extrinsics.device, extrinsics.shape[0], pairs.shape[0]
    E = extrinsics.detach().to(torch.float32).contiguous()
    K = intrinsics.detach().to(torch.float32).contiguous()
    pairs = pairs.contiguous()
    need = lib.gsr_view_overlap_scratch_bytes(V, P)
    scratch = torch.empty(max(need, 8) // 8, dtype=torch.float64, device=dev)
    counts = torch.empty(P, 2, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(lib.gsr_view_overlap(E.data_ptr(), K.data_ptr(), V, pairs.data_ptr(), P, H, W, scratch.data_ptr(), scratch.numel() * 8,
                                        counts.data_ptr(), _stream(dev)), "gsr_view_overlap")
    return counts


def overlap_counts(extrinsics: Tensor, intrinsics: Tensor, pairs, image_shape) -> Tensor:
    """the counts of `view_overlap` alone, on the cameras' device: pairs checked on the host, then the kernel (device cameras) or the
    float64 restatement (CPU cameras)"""
    H, W = _check_cameras(extrinsics, intrinsics, image_shape)
    p = torch.as_tensor(pairs).detach().cpu()
    if p.dim() != 2 or p.shape[1] != 2 or p.shape[0] < 1 or p.is_floating_point() or p.dtype == torch.bool:
        raise ValueError(f"pairs must be an integer (P,2) array with P >= 1, got {tuple(p.shape)} {p.dtype}")
    V = extrinsics.shape[0]
    if int(p.min()) < 0 or int(p.max()) >= V:
        raise IndexError(f"a pair names a view outside [0, {V})")
    if extrinsics.is_cuda:
        return view_overlap_device(extrinsics, intrinsics, p.to(torch.int32).to(extrinsics.device), (H, W))
    return overlap_counts_torch(extrinsics.to(torch.float32), intrinsics.to(torch.float32), p, (H, W))


def overlap_ratio(counts: Tensor, image_shape) -> Tensor:
    """count / (H W) in float64, rounded once more to fp32: two integers below 2^24 divide to the same fp32 either way (53 >= 2 * 24 + 2
    bits make the double rounding harmless), and the result does not depend on how a device rounds its fp32 division"""
    return (counts.to(torch.float64) / float(int(image_shape[0]) * int(image_shape[1]))).to(torch.float32)


def view_overlap(extrinsics: Tensor, intrinsics: Tensor, pairs, image_shape):
    """extrinsics (V,4,4) camera-to-world, intrinsics (V,3,3) normalised, pairs (P,2) integers, image_shape (H, W)
    -> (counts int32 (P,2), overlap fp32 (P,2)) on the cameras' device.  counts[p][0]: rays of view pairs[p][0] that overlap the image
    of view pairs[p][1]; counts[p][1]: the other way.  overlap = count / (H W) rounded to fp32, the reference's
    overlaps_image.float().mean() bit for bit.  Pair indices are checked on the host before anything is uploaded."""
    counts = overlap_counts(extrinsics, intrinsics, pairs, image_shape)
    return counts, overlap_ratio(counts, image_shape)


# ---- the evaluation index ----
@dataclass
class EvaluationIndexGeneratorCfg:
    num_target_views: int
    min_distance: int
    max_distance: int
    min_overlap: float
    max_overlap: float
    output_path: Path
    save_previews: bool
    seed: int


@dataclass
class IndexEntry:
    context: tuple
    target: tuple
    overlap: Optional[Union[str, float]] = None      # "small" / "medium" / "large", or the ratio itself


def _index_to_json(index: dict) -> dict:
    return {k: None if v is None else asdict(v) for k, v in index.items()}


def load_index(path) -> dict:
    """an evaluation_index.json -> {scene: IndexEntry | None}, context and target as tuples"""
    with Path(path).open("r") as f:
        raw = json.load(f)
    return {k: None if v is None else IndexEntry(tuple(v["context"]), tuple(v["target"]), v.get("overlap")) for k, v in raw.items()}


class EvaluationIndexGenerator:
    """The reference's generator without its LightningModule: `add_scene` per scene, then `save_index`.  ONE torch.Generator seeded from
    cfg.seed lives across scenes and is consumed as the reference consumes it: randperm(v), then per success one randint for the choice
    and randint draws of the targets until they are distinct."""

    def __init__(self, cfg: EvaluationIndexGeneratorCfg) -> None:
        if cfg.save_previews:
            raise NotImplementedError("previews are not built (their labels need a font the package does not have)")
        self.cfg = cfg
        self.generator = torch.Generator()
        self.generator.manual_seed(cfg.seed)
        self.index: dict = {}

    def candidates(self, context: int, v: int) -> list:
        """the frames the reference's walk can reach from `context`, in its order: forwards, then backwards, from min_distance on, up
        to the end of the scene or distance max_distance + 1 (that frame is still evaluated before the walk breaks)"""
        out = []
        last = max(self.cfg.min_distance, self.cfg.max_distance + 1)
        for step in (1, -1):
            out.append([context + step * d for d in range(self.cfg.min_distance, last + 1) if 0 <= context + step * d < v])
        return out

    def add_scene(self, scene: str, extrinsics: Tensor, intrinsics: Tensor, image_shape) -> Optional[IndexEntry]:
        cfg, v = self.cfg, extrinsics.shape[0]
        entry = None
        for context in torch.randperm(v, generator=self.generator).tolist():
            walks = self.candidates(context, v)
            frames = walks[0] + walks[1]
            if not frames:
                continue
            # one call and one read-back per context frame: the counts come back, the quotient is formed on the host
            overlap = overlap_ratio(overlap_counts(extrinsics, intrinsics, [(context, f) for f in frames], image_shape).cpu(), image_shape)
            # [p][0]: the context's rays in the partner (the reference's overlap_b), [p][1]: the partner's in the context (overlap_a)
            both = torch.minimum(overlap[:, 1], overlap[:, 0])
            accept = ((both >= cfg.min_overlap) & (both <= cfg.max_overlap)).tolist()      # fp32 against the Python float, as torch compares
            low = (both < cfg.min_overlap).tolist()
            valid, p = [], 0
            for walk in walks:
                for k, frame in enumerate(walk):
                    if accept[p + k]:
                        valid.append(frame)
                    if low[p + k] or abs(frame - context) > cfg.max_distance:
                        break
                p += len(walk)
            if not valid:
                continue
            chosen = valid[int(torch.randint(0, len(valid), size=tuple(), generator=self.generator))]
            left, right = min(chosen, context), max(chosen, context)
            if right - left + 1 < cfg.num_target_views:
                raise ValueError(f"{cfg.num_target_views} distinct targets do not fit between frames {left} and {right}")
            while True:
                targets = torch.randint(left, right + 1, (cfg.num_target_views,), generator=self.generator).tolist()
                if len(set(targets)) == len(targets):
                    break
            entry = IndexEntry(context=(left, right), target=tuple(sorted(targets)))
            break
        self.index[scene] = entry
        return entry

    def save_index(self, path=None) -> Path:
        """the reference's layout: {scene: null | {"context": [l, r], "target": [...], "overlap": null}}; default path
        cfg.output_path / "evaluation_index.json" """
        path = Path(self.cfg.output_path) / "evaluation_index.json" if path is None else Path(path)
        path.parent.mkdir(exist_ok=True, parents=True)
        with path.open("w") as f:
            json.dump(_index_to_json(self.index), f)
        return path

    load_index = staticmethod(load_index)


# ---- the view samplers ----
class StepTracker:
    """what the samplers ask of a step tracker: get_step().  Any object with that method serves."""

    def __init__(self, step: int = 0) -> None:
        self.step = int(step)

    def set_step(self, step: int) -> None:
        self.step = int(step)

    def get_step(self) -> int:
        return self.step


def add_additional_context_index(indices: Tensor, number_of_context_views: int) -> Tensor:
    """(left, right) -> number_of_context_views indices spread evenly between them (fp32 linspace, truncated)"""
    left, right = indices.unbind(dim=-1)
    return torch.linspace(left.item(), right.item(), number_of_context_views).long()


def _dummy_overlap(device) -> Tensor:
    return torch.tensor([0.5], dtype=torch.float32, device=device)


class ViewSampler:
    def __init__(self, cfg, stage: str, is_overfitting: bool, cameras_are_circular: bool, step_tracker=None) -> None:
        self.cfg = cfg
        self.stage = stage
        self.is_overfitting = is_overfitting
        self.cameras_are_circular = cameras_are_circular
        self.step_tracker = step_tracker

    def sample(self, scene: str, extrinsics: Tensor, intrinsics: Tensor, device=torch.device("cpu")):
        """-> (context indices int64, target indices int64, overlap fp32 (1,))"""
        raise NotImplementedError

    @property
    def global_step(self) -> int:
        return 0 if self.step_tracker is None else self.step_tracker.get_step()


@dataclass
class ViewSamplerBoundedCfg:
    name: str                      # "bounded"
    num_context_views: int
    num_target_views: int
    min_distance_between_context_views: int
    max_distance_between_context_views: int
    min_distance_to_context_views: int
    warm_up_steps: int
    initial_min_distance_between_context_views: int
    initial_max_distance_between_context_views: int


class ViewSamplerBounded(ViewSampler):
    def schedule(self, initial: int, final: int) -> int:
        fraction = self.global_step / self.cfg.warm_up_steps
        return min(initial + int((final - initial) * fraction), final)

    def gap_range(self, num_views: int):
        """(min_gap, max_gap) between the outer context views at the current step"""
        cfg = self.cfg
        if self.stage == "test":                                  # the full gap, always
            lo = hi = cfg.max_distance_between_context_views
        elif cfg.warm_up_steps > 0:
            hi = self.schedule(cfg.initial_max_distance_between_context_views, cfg.max_distance_between_context_views)
            lo = self.schedule(cfg.initial_min_distance_between_context_views, cfg.min_distance_between_context_views)
        else:
            lo, hi = cfg.min_distance_between_context_views, cfg.max_distance_between_context_views
        if not self.cameras_are_circular:
            hi = min(num_views - 1, hi)
        return max(2 * cfg.min_distance_to_context_views, lo), hi

    def sample(self, scene: str, extrinsics: Tensor, intrinsics: Tensor, device=torch.device("cpu")):
        cfg, num_views = self.cfg, extrinsics.shape[0]
        min_gap, max_gap = self.gap_range(num_views)
        if max_gap < min_gap:
            raise ValueError("Example does not have enough frames!")
        # draws, in order: the gap, the left view, the targets (not when testing), the extra context views
        gap = torch.randint(min_gap, max_gap + 1, size=tuple(), device=device).item()
        left = torch.randint(num_views if self.cameras_are_circular else num_views - gap, size=tuple(), device=device).item()
        if self.stage == "test":
            left = 0
        right = left + gap
        if self.is_overfitting:
            left, right = 0, max_gap
        if self.stage == "test":
            target = torch.arange(left, right + 1, device=device)
        else:
            target = torch.randint(left + cfg.min_distance_to_context_views, right + 1 - cfg.min_distance_to_context_views,
                                   size=(cfg.num_target_views,), device=device)
        if self.cameras_are_circular:
            target %= num_views
            right %= num_views
        extra = []
        if cfg.num_context_views > 2:
            wanted = cfg.num_context_views - 2
            while len(set(extra)) != wanted:
                extra = torch.randint(left + 1, right, (wanted,)).tolist()
        return torch.tensor((left, *extra, right)), target, _dummy_overlap(device)

    @property
    def num_context_views(self) -> int:
        return self.cfg.num_context_views

    @property
    def num_target_views(self) -> int:
        return self.cfg.num_target_views


@dataclass
class ViewSamplerArbitraryCfg:
    name: str                      # "arbitrary"
    num_context_views: int
    num_target_views: int
    context_views: Optional[list]
    target_views: Optional[list]


class ViewSamplerArbitrary(ViewSampler):
    def sample(self, scene: str, extrinsics: Tensor, intrinsics: Tensor, device=torch.device("cpu")):
        cfg, num_views = self.cfg, extrinsics.shape[0]
        # both draws are made even when the views are fixed: the generator moves as the reference's does
        context = torch.randint(0, num_views, size=(cfg.num_context_views,), device=device)
        if cfg.context_views is not None:
            context = torch.tensor(cfg.context_views, dtype=torch.int64, device=device)
            if cfg.num_context_views >= 3 and len(cfg.context_views) == 2:
                context = add_additional_context_index(context, cfg.num_context_views)
            else:
                assert len(cfg.context_views) == cfg.num_context_views
        target = torch.randint(0, num_views, size=(cfg.num_target_views,), device=device)
        if cfg.target_views is not None:
            assert len(cfg.target_views) == cfg.num_target_views
            target = torch.tensor(cfg.target_views, dtype=torch.int64, device=device)
        return context, target, _dummy_overlap(device)

    @property
    def num_context_views(self) -> int:
        return self.cfg.num_context_views

    @property
    def num_target_views(self) -> int:
        return self.cfg.num_target_views


@dataclass
class ViewSamplerAllCfg:
    name: str                      # "all"


class ViewSamplerAll(ViewSampler):
    """every frame is context and target.  (The reference's returns two values, which its own loader cannot unpack; here the
    placeholder overlap of the other samplers comes third.)"""

    def sample(self, scene: str, extrinsics: Tensor, intrinsics: Tensor, device=torch.device("cpu")):
        frames = torch.arange(extrinsics.shape[0], device=device)
        return frames, frames, _dummy_overlap(device)

    @property
    def num_context_views(self) -> int:
        return 0

    @property
    def num_target_views(self) -> int:
        return 0


@dataclass
class ViewSamplerEvaluationCfg:
    name: str                      # "evaluation"
    index_path: Path
    num_context_views: int


class ViewSamplerEvaluation(ViewSampler):
    def __init__(self, cfg, stage: str, is_overfitting: bool, cameras_are_circular: bool, step_tracker=None) -> None:
        super().__init__(cfg, stage, is_overfitting, cameras_are_circular, step_tracker)
        self.index = load_index(cfg.index_path)

    def sample(self, scene: str, extrinsics: Tensor, intrinsics: Tensor, device=torch.device("cpu")):
        entry = self.index.get(scene)
        if entry is None:
            raise ValueError(f"No indices available for scene {scene}.")
        context = torch.tensor(entry.context, dtype=torch.int64, device=device)
        target = torch.tensor(entry.target, dtype=torch.int64, device=device)
        ratio = entry.overlap if isinstance(entry.overlap, float) else 0.75 if entry.overlap == "large" else 0.25
        v = self.num_context_views
        if v >= 3 and v > len(context):                             # a two-view index serving more context views
            context = add_additional_context_index(context, v)
        return context, target, torch.tensor([ratio], dtype=torch.float32, device=device)

    @property
    def num_context_views(self) -> int:
        return self.cfg.num_context_views

    @property
    def num_target_views(self) -> int:
        return 0


VIEW_SAMPLERS = {"all": ViewSamplerAll, "arbitrary": ViewSamplerArbitrary, "bounded": ViewSamplerBounded, "evaluation": ViewSamplerEvaluation}


def get_view_sampler(cfg, stage: str, overfit: bool, cameras_are_circular: bool, step_tracker=None) -> ViewSampler:
    return VIEW_SAMPLERS[cfg.name](cfg, stage, overfit, cameras_are_circular, step_tracker)
