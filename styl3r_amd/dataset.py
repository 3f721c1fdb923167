"""The step in front of styl3r_amd.inputs: the datasets' `.torch` chunks and their JPEG frames.

  decode_jpeg     JPEG streams of one picture size -> uint8 (n,H,W,3), the bytes PIL gives (libjpeg-turbo, JDCT_ISLOW, fancy upsampling)
                  bit for bit.  The Huffman stage runs on the host (`gsr_jpeg_entropy`, C++, threaded over images, GIL released); the
                  rest -- dequantisation, IDCT, chroma upsampling, colour -- is `gsr_jpeg_pixels` (csrc/gsr_jpeg.hip) for a device
                  target and a numpy restatement of the same integers for a CPU target (include/gsr.h has the rules).
  read_chunk      one `.torch` chunk -> its list of example dicts
  ChunkDataset    the reference's DatasetRE10kStyle.__iter__ (src/dataset/dataset_re10k_style.py:93-213) on these pieces: it decodes only
                  the frames the sampler picked, all of them in one call
  iter_batches    collated batches, the host half (chunk read, sampling, entropy stage) one batch ahead on a background thread

A stream outside the fast path, or one the entropy stage calls corrupt, goes to PIL: what PIL returns is used and what it raises is
raised, so the behaviour of the reference's loader is kept in every case.  CALLS counts the routes.
"""
from __future__ import annotations

import ctypes as C
import json
import queue
import threading
from dataclasses import dataclass, field
from io import BytesIO
from pathlib import Path
from typing import Optional, Sequence

import numpy as np
import torch
from torch import Tensor

from . import _lib
from . import inputs
from .inputs import SkipExample

CALLS = {"jpeg_hip": 0, "jpeg_host": 0, "jpeg_fallback": 0}     # images decoded on the device / by the numpy restatement / by PIL


# ---- the numpy restatement of csrc/gsr_jpeg.hip ----
def _idct8(x: np.ndarray, shift: int) -> np.ndarray:
    """one pass of the "islow" IDCT along the LAST axis of int64 (..., 8), outputs descaled by `shift` with rounding"""
    i = [x[..., k] for k in range(8)]
    z1 = (i[2] + i[6]) * 4433
    tmp2 = z1 + i[6] * -15137
    tmp3 = z1 + i[2] * 6270
    tmp0 = (i[0] + i[4]) * 8192
    tmp1 = (i[0] - i[4]) * 8192
    tmp10, tmp13, tmp11, tmp12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
    tmp0, tmp1, tmp2, tmp3 = i[7], i[5], i[3], i[1]
    z1, z2, z3, z4 = tmp0 + tmp3, tmp1 + tmp2, tmp0 + tmp2, tmp1 + tmp3
    z5 = (z3 + z4) * 9633
    tmp0, tmp1, tmp2, tmp3 = tmp0 * 2446, tmp1 * 16819, tmp2 * 25172, tmp3 * 12299
    z1, z2 = z1 * -7373, z2 * -20995
    z3, z4 = z3 * -16069 + z5, z4 * -3196 + z5
    tmp0, tmp1, tmp2, tmp3 = tmp0 + z1 + z3, tmp1 + z2 + z4, tmp2 + z2 + z3, tmp3 + z1 + z4
    r = 1 << (shift - 1)
    out = [tmp10 + tmp3, tmp11 + tmp2, tmp12 + tmp1, tmp13 + tmp0, tmp13 - tmp0, tmp12 - tmp1, tmp11 - tmp2, tmp10 - tmp3]
    return np.stack([(o + r) >> shift for o in out], axis=-1)


def _plane_host(coefs: np.ndarray, quant: np.ndarray, bw: int, bh: int) -> np.ndarray:
    """int16 (bw * bh * 64) coefficient blocks + uint16 (64) table -> the component's byte plane int32 (bh * 8, bw * 8)"""
    d = coefs.reshape(-1, 8, 8).astype(np.int64) * quant.reshape(1, 8, 8).astype(np.int64)
    ws = _idct8(d.transpose(0, 2, 1), 11).transpose(0, 2, 1)          # pass 1: along the columns
    v = _idct8(ws, 18)                                                 # pass 2: along the rows
    s = v & 1023
    s = np.where(s >= 512, s - 1024, s)
    px = np.clip(s + 128, 0, 255).astype(np.int32)
    return px.reshape(bh, bw, 8, 8).transpose(0, 2, 1, 3).reshape(bh * 8, bw * 8)


def _h2v1(p: np.ndarray, cw: int) -> np.ndarray:
    """(rows, >= cw) -> (rows, 2 cw): the triangle filter along the last axis, replication when cw <= 2"""
    p = p[:, :cw]
    if cw <= 2:
        return np.repeat(p, 2, axis=1)
    out = np.empty((p.shape[0], 2 * cw), np.int32)
    out[:, 0] = p[:, 0]
    out[:, 2::2] = (3 * p[:, 1:] + p[:, :-1] + 1) >> 2
    out[:, 1:-1:2] = (3 * p[:, :-1] + p[:, 1:] + 2) >> 2
    out[:, -1] = p[:, -1]
    return out


def _h2v2(p: np.ndarray, cw: int, ch: int) -> np.ndarray:
    """(>= ch, >= cw) -> (2 ch, 2 cw)"""
    p = p[:ch, :cw]
    if cw <= 2:
        return np.repeat(np.repeat(p, 2, axis=0), 2, axis=1)
    rows = np.arange(ch)
    above, below = p[np.maximum(rows - 1, 0)], p[np.minimum(rows + 1, ch - 1)]
    cs = np.empty((2 * ch, cw), np.int32)
    cs[0::2] = 3 * p + above
    cs[1::2] = 3 * p + below
    out = np.empty((2 * ch, 2 * cw), np.int32)
    out[:, 0] = (4 * cs[:, 0] + 8) >> 4
    out[:, 2::2] = (3 * cs[:, 1:] + cs[:, :-1] + 8) >> 4
    out[:, 1:-1:2] = (3 * cs[:, :-1] + cs[:, 1:] + 7) >> 4
    out[:, -1] = (4 * cs[:, -1] + 7) >> 4
    return out


def pixels_host(coefs: np.ndarray, desc, H: int, W: int) -> np.ndarray:
    """the device stage in numpy, one image: int16 coefficient buffer + its GsrJpegDesc -> uint8 (H,W,3); zeros if not decoded"""
    if desc.sampling < 0:
        return np.zeros((H, W, 3), np.uint8)
    planes, at = [], int(desc.coef_offset)
    for c in range(desc.ncomp):
        bw, bh = desc.bw[c], desc.bh[c]
        n = bw * bh * 64
        planes.append(_plane_host(coefs[at:at + n], np.ctypeslib.as_array(desc.quant[c]), bw, bh))
        at += n
    Y = planes[0][:H, :W]
    if desc.sampling == _lib.GSR_JPEG_GRAY:
        return np.repeat(Y[..., None], 3, axis=-1).astype(np.uint8)
    cw, ch = (W + 1) // 2, (H + 1) // 2
    if desc.sampling == _lib.GSR_JPEG_444:
        cb, cr = planes[1], planes[2]
    elif desc.sampling == _lib.GSR_JPEG_422:
        cb, cr = _h2v1(planes[1][:H], cw), _h2v1(planes[2][:H], cw)
    else:
        cb, cr = _h2v2(planes[1], cw, ch), _h2v2(planes[2], cw, ch)
    cb, cr = cb[:H, :W] - 128, cr[:H, :W] - 128
    R = Y + ((91881 * cr + 32768) >> 16)
    G = Y + ((-22554 * cb + 32768 - 46802 * cr) >> 16)
    B = Y + ((116130 * cb + 32768) >> 16)
    return np.clip(np.stack([R, G, B], axis=-1), 0, 255).astype(np.uint8)


# ---- decode_jpeg ----
def _as_bytes(blob) -> bytes:
    if isinstance(blob, Tensor):
        return blob.detach().cpu().contiguous().numpy().tobytes()
    if isinstance(blob, np.ndarray):
        return blob.tobytes()
    return bytes(blob)


def jpeg_probe(blob):
    """-> (status, GsrJpegInfo) of one stream: GSR_OK (0), _lib.GSR_JPEG_UNSUPPORTED or _lib.GSR_JPEG_CORRUPT"""
    data = _as_bytes(blob)
    info = _lib.GsrJpegInfo()
    rc = _lib.load().gsr_jpeg_probe(data, len(data), C.byref(info))
    if rc < 0:
        _lib.check(rc, "gsr_jpeg_probe")
    return rc, info


def _pil_rgb(data: bytes) -> np.ndarray:
    from PIL import Image
    return np.array(Image.open(BytesIO(data)).convert("RGB"))


def _threads(threads, n: int) -> int:
    return max(1, min(8, n) if threads is None else int(threads))


@dataclass
class EntropyResult:
    """the host half of `decode_jpeg`: what the background thread of `iter_batches` hands to the consumer"""
    blobs: list
    H: int
    W: int
    coefs: Optional[Tensor]            # int16, the used prefix of the (pinned) coefficient buffer; None when no image took the fast path
    desc: object                       # (GsrJpegDesc * n)
    status: np.ndarray                 # int32 (n)
    fallback: dict = field(default_factory=dict)      # image -> uint8 (H,W,3) from PIL


def jpeg_entropy(blobs: Sequence, threads=None, pin: bool = False) -> EntropyResult:
    """Host half: sizes from the markers, `gsr_jpeg_entropy` over all streams, PIL for the images it does not take.  ValueError for
    pictures of different sizes; whatever PIL raises for a stream it cannot read."""
    lib = _lib.load()
    blobs = [_as_bytes(b) for b in blobs]
    n = len(blobs)
    if n == 0:
        raise ValueError("decode_jpeg: no streams")
    sizes, fallback = [], {}
    for i, data in enumerate(blobs):
        info = _lib.GsrJpegInfo()
        rc = lib.gsr_jpeg_probe(data, len(data), C.byref(info))
        if rc == 0:
            sizes.append((info.height, info.width))
        else:
            fallback[i] = _pil_rgb(data)                      # raises what the reference's loader raises
            sizes.append(tuple(fallback[i].shape[:2]))
    if len(set(sizes)) != 1:
        raise ValueError(f"decode_jpeg: the pictures of one call share a size; got (H, W) = {sorted(set(sizes))}")
    H, W = sizes[0]
    desc = (_lib.GsrJpegDesc * n)()
    status = np.full(n, _lib.GSR_JPEG_UNSUPPORTED, np.int32)
    coefs = None
    if len(fallback) < n:
        nbytes = lib.gsr_jpeg_coef_bytes(n, H, W)
        if nbytes == 0:
            raise ValueError(f"decode_jpeg: bad dimensions n {n}, {H} x {W}")
        coefs = torch.empty(nbytes // 2, dtype=torch.int16, pin_memory=pin)
        ptrs = (C.c_void_p * n)(*[C.cast(C.c_char_p(b), C.c_void_p) for b in blobs])
        lens = (C.c_size_t * n)(*[len(b) for b in blobs])
        _lib.check(lib.gsr_jpeg_entropy(ptrs, lens, n, H, W, coefs.data_ptr(), C.addressof(desc), status.ctypes.data, _threads(threads, n)),
                   "gsr_jpeg_entropy")
        used = max(int(d.coef_offset + d.coef_count) for d in desc)
        coefs = coefs[:used] if used else None
    for i in range(n):
        if status[i] != 0 and i not in fallback:
            fallback[i] = _pil_rgb(blobs[i])
            if fallback[i].shape[:2] != (H, W):
                raise ValueError(f"decode_jpeg: the pictures of one call share a size; got (H, W) = {[(H, W), fallback[i].shape[:2]]}")
    return EntropyResult(blobs, H, W, coefs, desc, status, fallback)


def _stream(dev) -> C.c_void_p:
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def jpeg_pixels(res: EntropyResult, device=None) -> Tensor:
    """Second half: uint8 (n,H,W,3) on `device` (None: CPU).  Every upload and launch is ordered on the device's current stream."""
    n, H, W = len(res.blobs), res.H, res.W
    dev = torch.device("cpu") if device is None else torch.device(device)
    CALLS["jpeg_fallback"] += len(res.fallback)
    if dev.type == "cpu":
        out = np.empty((n, H, W, 3), np.uint8)
        coefs = res.coefs.numpy() if res.coefs is not None else None
        for i in range(n):
            out[i] = res.fallback[i] if i in res.fallback else pixels_host(coefs, res.desc[i], H, W)
        CALLS["jpeg_host"] += n - len(res.fallback)
        return torch.from_numpy(out)
    if res.coefs is None:
        return torch.from_numpy(np.stack([res.fallback[i] for i in range(n)])).to(dev)
    lib = _lib.load()
    coefs = res.coefs.to(dev, non_blocking=True)
    desc = torch.frombuffer(res.desc, dtype=torch.uint8).to(dev, non_blocking=True)
    nbytes = lib.gsr_jpeg_scratch_bytes(n, H, W)
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    out = torch.empty((n, H, W, 3), dtype=torch.uint8, device=dev)
    _lib.check(lib.gsr_jpeg_pixels(coefs.data_ptr(), desc.data_ptr(), n, H, W, scratch.data_ptr(), nbytes, out.data_ptr(), _stream(dev)),
               "gsr_jpeg_pixels")
    for i, img in res.fallback.items():
        out[i] = torch.from_numpy(img).to(dev)
    CALLS["jpeg_hip"] += n - len(res.fallback)
    return out


def decode_jpeg(blobs: Sequence, device=None, threads=None) -> Tensor:
    """JPEG streams (`bytes` or 1-D uint8 tensors) of ONE picture size -> uint8 (n,H,W,3) on `device` (None: CPU), the bytes of
    `PIL.Image.open(...).convert("RGB")`.  Device target: entropy stage into a pinned buffer, one upload, `gsr_jpeg_pixels`.  Pictures
    of different sizes: ValueError naming them.  `threads`: workers of the entropy stage, default min(8, n)."""
    dev = None if device is None else torch.device(device)
    on_gpu = dev is not None and dev.type != "cpu"
    return jpeg_pixels(jpeg_entropy(blobs, threads, pin=on_gpu), dev)


# ---- chunks ----
def read_chunk(path) -> list:
    """one `.torch` chunk: a list of dicts with "key" (scene name), "cameras" (n,18) float32, "images" (n 1-D uint8 tensors: JPEG bytes)
    and whatever else the converter stored"""
    return torch.load(str(path), weights_only=True)


@dataclass
class DatasetRE10kStyleCfg:
    """the reference's DatasetRE10kStyleCfg (+ DatasetCfgCommon), field for field"""
    name: str
    roots: list
    baseline_min: float
    baseline_max: float
    max_fov: float
    make_baseline_1: bool
    augment: bool
    relative_pose: bool
    skip_bad_shape: bool
    style_root: Path
    specified_style_image_path: Optional[Path] = None
    original_image_shape: tuple = (360, 640)
    input_image_shape: tuple = (256, 256)
    background_color: tuple = (0.0, 0.0, 0.0)
    cameras_are_circular: bool = False
    overfit_to_scene: Optional[str] = None
    view_sampler: object = None

    def input_cfg(self, near: float, far: float) -> inputs.InputCfg:
        return inputs.InputCfg(tuple(self.input_image_shape), self.make_baseline_1, self.baseline_min, self.baseline_max, self.relative_pose,
                               self.max_fov, near, far, self.augment)


@dataclass
class _Pending:
    """an example whose host half is done: cameras, picked frames through the entropy stage, the style picture's bytes"""
    scene: str
    intrinsics: Tensor
    extrinsics: Tensor
    context: Tensor
    target: Tensor
    flip: bool
    frames: EntropyResult
    style: Tensor


class ChunkDataset:
    """`DatasetRE10kStyle(cfg, stage, view_sampler)` of the reference as an iterable of example dicts on `device` (None: CPU).  The random
    draws -- the two `torch.randperm` shuffles, the sampler's, the augmentation's -- come from torch's global CPU generator in the
    reference's order: a seeded run visits the same scenes, frames and flips.  Only the frames the sampler picked are decoded, context
    and target in ONE `decode_jpeg` call.  A skipped example is skipped here too: too few frames, field of view, baseline, a frame index
    outside the scene (IndexError), a picture PIL cannot read (OSError), a shape other than cfg.original_image_shape."""
    near: float = 0.1
    far: float = 100.0

    def __init__(self, cfg: DatasetRE10kStyleCfg, stage: str, view_sampler, device=None) -> None:
        self.cfg, self.stage, self.view_sampler = cfg, stage, view_sampler
        self.device = None if device is None else torch.device(device)
        self.chunks = []
        for root in cfg.roots:
            root = Path(root) / self.data_stage
            self.chunks.extend(sorted(p for p in root.iterdir() if p.suffix == ".torch"))
        if cfg.overfit_to_scene is not None:
            self.chunks = [self.index[cfg.overfit_to_scene]] * len(self.chunks)
        with open(Path(cfg.style_root) / "train" / "scene_style_mapping_all.json") as f:
            self.scene_style_mapping = json.load(f)

    @property
    def data_stage(self) -> str:
        if self.cfg.overfit_to_scene is not None or self.stage == "val":
            return "test"
        return self.stage

    @property
    def index(self) -> dict:
        merged = {}
        for data_stage in (("test", "train") if self.cfg.overfit_to_scene is not None else (self.data_stage,)):
            for root in self.cfg.roots:
                with (Path(root) / data_stage / "index.json").open() as f:
                    index = {k: Path(root) / data_stage / v for k, v in json.load(f).items()}
                assert not (set(merged) & set(index)), "the datasets' scene keys must be unique"
                merged.update(index)
        return merged

    @staticmethod
    def shuffle(lst: list) -> list:
        return [lst[i] for i in torch.randperm(len(lst))]

    def read_style_image(self, scene: str) -> Tensor:
        """the style picture as uint8 (H,W,3) (PIL, as in the reference: style pictures are not JPEG frames of one size)"""
        path = self.cfg.specified_style_image_path
        if path is not None:
            if not Path(path).exists():
                raise FileNotFoundError(f"No image found for {path}")
        else:
            if scene not in self.scene_style_mapping:
                raise KeyError(f"{scene} is not found in scene_style_mapping!")
            path = Path(self.cfg.style_root) / "train" / self.scene_style_mapping[scene]
        from PIL import Image
        return torch.from_numpy(np.asarray(Image.open(path).convert("RGB")).copy())

    def pending(self):
        """the host half of `__iter__`: everything up to and including the entropy stage, no device call"""
        cfg = self.cfg
        icfg = cfg.input_cfg(self.near, self.far)
        pin = self.device is not None and self.device.type != "cpu"
        if self.stage in ("train", "val"):
            self.chunks = self.shuffle(self.chunks)
        for chunk_path in self.chunks:
            chunk = read_chunk(chunk_path)
            if cfg.overfit_to_scene is not None:
                item = [x for x in chunk if x["key"] == cfg.overfit_to_scene]
                assert len(item) == 1
                chunk = item * len(chunk)
            if self.stage in ("train", "val"):
                chunk = self.shuffle(chunk)
            for example in chunk:
                extrinsics, intrinsics = inputs.convert_poses(example["cameras"])
                scene = example["key"]
                try:
                    context, target = self.view_sampler.sample(scene, extrinsics, intrinsics)[:2]
                except ValueError:
                    continue                                     # not enough frames
                if (inputs.get_fov_deg(intrinsics.double().numpy()) > cfg.max_fov).any():
                    continue
                picked = torch.cat([context.reshape(-1), target.reshape(-1)]).tolist()
                try:
                    frames = jpeg_entropy([example["images"][i] for i in picked], pin=pin)
                except IndexError:
                    continue
                except OSError:
                    print(f"Skipped bad example {scene}.")
                    continue
                except ValueError as err:                        # pictures of different sizes inside one scene
                    if cfg.skip_bad_shape:
                        print(f"Skipped bad example {scene}. {err}")
                        continue
                    raise
                if cfg.skip_bad_shape and (frames.H, frames.W) != tuple(cfg.original_image_shape):
                    print(f"Skipped bad example {scene}. Shape was {(frames.H, frames.W)}.")
                    continue
                try:                                             # the baseline gate comes BEFORE the augmentation draw
                    inputs.prepare_cameras_f64(intrinsics, extrinsics, context.tolist(), target.tolist(), icfg, (frames.H, frames.W))
                except SkipExample as err:
                    print(f"Skipped {scene}: {err}")
                    continue
                style = self.read_style_image(scene)
                flip = bool(self.stage == "train" and cfg.augment and not (torch.rand(tuple()) < 0.5))
                yield _Pending(scene, intrinsics, extrinsics, context, target, flip, frames, style)

    def finish(self, p: _Pending) -> dict:
        """the device half: upload, `gsr_jpeg_pixels`, `prepare_example` -- on the caller's thread and current stream"""
        frames = jpeg_pixels(p.frames, self.device)
        return inputs.prepare_example(frames, p.intrinsics, p.extrinsics, p.context, p.target, p.style, self.cfg.input_cfg(self.near, self.far),
                                      stage=self.stage, flip=p.flip, scene=p.scene, device=self.device, preselected=True)

    def __iter__(self):
        for p in self.pending():
            yield self.finish(p)


_END = object()


def iter_batches(dataset: ChunkDataset, batch_size: int, prefetch: int = 1):
    """Collated batches of `batch_size` examples (the last one holds what is left, as a DataLoader's does).  prefetch >= 1: ONE
    background thread runs the host half -- chunk read, sampling, entropy decode into pinned buffers -- up to `prefetch` batches ahead;
    every upload and launch happens on the consumer's thread and current stream when the batch is taken.  prefetch = 0: inline.  The
    random draws are the producer's, in the same order either way."""
    if batch_size < 1 or prefetch < 0:
        raise ValueError(f"iter_batches: batch_size {batch_size}, prefetch {prefetch}")

    def groups():
        group = []
        for p in dataset.pending():
            group.append(p)
            if len(group) == batch_size:
                yield group
                group = []
        if group:
            yield group

    def finish(group):
        return inputs.collate([dataset.finish(p) for p in group])

    if prefetch == 0:
        for group in groups():
            yield finish(group)
        return
    q: "queue.Queue" = queue.Queue(maxsize=prefetch)
    stop = threading.Event()

    def put(item) -> bool:
        while not stop.is_set():
            try:
                q.put(item, timeout=0.1)
                return True
            except queue.Full:
                pass
        return False

    def produce():
        try:
            for group in groups():
                if not put(group):
                    return
            put(_END)
        except BaseException as err:                              # handed to the consumer, raised there
            put(err)

    worker = threading.Thread(target=produce, name="styl3r-chunk-prefetch", daemon=True)
    worker.start()
    try:
        while True:
            item = q.get()
            if item is _END:
                break
            if isinstance(item, BaseException):
                raise item
            yield finish(item)
    finally:
        stop.set()
        worker.join()
