"""Save and resume training: the writer half of the reference's `ModelCheckpoint(every_n_train_steps, save_top_k, save_weights_only)`
(src/main_style.py:80-90, config/main.yaml:40-44); `checkpoint.py` keeps the readers.

The save has a hot path.  `torch.save` of the device tensors (1 806 at full encoder size) is one blocking device-to-host copy per tensor and
then pickling while the train step waits (4.4 GB weights-only, 13.2 GB with the moments; measurements: DESIGN R27).  Here the state leaves the train stream in ONE launch: csrc/vit_snapshot.hip
gathers every tensor into one staging buffer and writes, per 64 KiB chunk, a partial checksum and a count of non-finite fp32 words.  After
that launch the train step goes on; one device-to-host copy on a side stream and a writer thread do the rest.

    checksum of a tensor = (S1, S2) mod 2^64 over its bytes read as little-endian 32-bit words w_i (the last word zero-extended):
        S1 = sum w_i            S2 = sum (i + 1) w_i
    position-sensitive (two swapped words change S2), integer-only, so the kernel's result equals the numpy restatement `checksum` bit for bit.
    It is stored in the file and recomputed by `load_checkpoint`: the file is verifiable after the PCIe hop and again at load.
    The non-finite count keeps a diverged step from replacing the last good file (`save_top_k: 1` would otherwise make that fatal).

File layout = the Lightning wrapper's: {"state_dict": {"encoder.<name>": tensor}, "global_step": n, "epoch": 0}, with `weights_only=False`
also "optimizer_states": [optimizer.state_dict()] and "lr_schedulers": [scheduler.state_dict()], and always
"styl3r_amd": {"format": 1, "checksums": {...}}.  `checkpoint.load_wrapper_checkpoint` / `load_pretrained_encoder` and the reference's
`torch.load(path)["state_dict"]` (main_style.py:190-192, infer_model_re10k.py:300-306) read these files as they are.  Lightning's own
`Trainer.fit(ckpt_path=...)` restore is NOT claimed: Lightning is not a dependency of this package and that path was never exercised
(it also expects "loops", "callbacks" and "pytorch-lightning_version" entries that are not written here).

`CALLS` counts the routes taken: "kernel" (tensors through vit_snapshot_pack), "numpy" (CPU tensors and what the kernel does not take),
"made_contiguous", "pack_launches", "table_reused"."""
from __future__ import annotations

import os
import queue
import threading
from dataclasses import dataclass
from pathlib import Path
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch
from torch import Tensor, nn

FORMAT = 1
ALIGN = 64                 # tensor starts in the staging buffer
_MASK = (1 << 64) - 1
_SNAP_FP32, _SNAP_VEC16, _SNAP_WORD = 1, 2, 4                                          # include/vit_ops.h VIT_SNAP_*
_CHUNK_DTYPE = np.dtype([("src", "<u8"), ("dst_off", "<u8"), ("nbytes", "<u4"), ("flags", "<u4")])        # VitSnapChunk
_PARTIAL_DTYPE = np.dtype([("s1", "<u8"), ("s2", "<u8"), ("nonfinite", "<u4"), ("reserved", "<u4")])      # VitSnapPartial
CALLS = {"kernel": 0, "numpy": 0, "made_contiguous": 0, "pack_launches": 0, "table_reused": 0}
PACK_EVENTS: Optional[list] = None      # tools/bench_checkpoint.py sets a list: (start, end) timing events right around every pack launch

_STAGING: Dict[torch.device, Tensor] = {}       # device -> uint8 staging buffer (grown on demand)
_PINNED: Dict[torch.device, Tensor] = {}        # device -> pinned host mirror
_SIDE: Dict[torch.device, "torch.cuda.Stream"] = {}
_TABLES: Dict[torch.device, tuple] = {}         # device -> (key, pinned host table, device table, first row / row count per tensor)
_LAST_COPY: Dict[torch.device, "torch.cuda.Event"] = {}       # the copy that last read _STAGING / wrote _PINNED


class ChecksumMismatch(RuntimeError):
    """`load_checkpoint(verify=True)`: a tensor's bytes do not give the checksum stored with it; `.key` names the first such entry"""

    def __init__(self, key: str, stored, found):
        super().__init__(f"checkpoint entry {key!r}: stored checksum {tuple(stored)} != recomputed {tuple(found)}")
        self.key = key


class NonFiniteCheckpoint(RuntimeError):
    """a snapshot with NaN / inf in an fp32 tensor was refused (nothing written, nothing pruned); `.key` / `.count`: the first such tensor"""

    def __init__(self, key: str, count: int, path=None):
        super().__init__(f"refused to write {path or 'the checkpoint'}: {key!r} holds {count} non-finite value(s)")
        self.key, self.count = key, count


# ---- the numpy restatement ---------------------------------------------------------------------------------------------------------------
def _as_bytes(buffer) -> np.ndarray:
    if isinstance(buffer, Tensor):
        t = buffer.detach()
        if t.device.type != "cpu":
            t = t.cpu()
        return t.contiguous().reshape(-1).view(torch.uint8).numpy()
    if isinstance(buffer, np.ndarray):
        return np.ascontiguousarray(buffer).reshape(-1).view(np.uint8)
    return np.frombuffer(buffer, dtype=np.uint8)


def _words(b: np.ndarray):
    """the little-endian 32-bit words of a byte array in blocks of 2^20, the last word zero-extended"""
    n = b.size
    whole = n & ~3
    block = 4 << 20
    for lo in range(0, whole, block):
        yield lo >> 2, b[lo:min(lo + block, whole)].view("<u4")
    if n & 3:
        last = np.zeros(4, np.uint8)
        last[:n & 3] = b[whole:]
        yield whole >> 2, last.view("<u4")


def checksum(buffer) -> Tuple[int, int]:
    """(S1, S2) of a tensor / array / bytes-like: S1 = sum w_i, S2 = sum (i + 1) w_i mod 2^64 over its little-endian 32-bit words, a final
    partial word zero-extended -- what csrc/vit_snapshot.hip computes chunk by chunk (uint64 arithmetic wraps, which IS the definition)."""
    s1 = s2 = 0
    with np.errstate(over="ignore"):
        for base, w in _words(_as_bytes(buffer)):
            w = w.astype(np.uint64)
            idx = np.arange(base + 1, base + 1 + w.size, dtype=np.uint64)
            s1 = (s1 + int(w.sum(dtype=np.uint64))) & _MASK
            s2 = (s2 + int((idx * w).sum(dtype=np.uint64))) & _MASK
    return s1, s2


def count_nonfinite(t: Tensor) -> int:
    """words whose fp32 exponent field is all ones; 0 for every other dtype (the kernel's rule)"""
    if t.dtype != torch.float32:
        return 0
    n = 0
    for _, w in _words(_as_bytes(t)):
        n += int(np.count_nonzero((w & np.uint32(0x7f800000)) == np.uint32(0x7f800000)))
    return n


# ---- snapshot ----------------------------------------------------------------------------------------------------------------------------
def _lib():
    from . import vit_ops
    return vit_ops.load()


def chunk_bytes() -> int:
    return int(_lib().vit_snapshot_chunk_bytes())


def _round_up(n: int, a: int) -> int:
    return -(-n // a) * a


def _build_table(items, chunk: int):
    """rows of VitSnapChunk for [(data_ptr, dst_off, nbytes, is_fp32)], and per tensor its first row and row count"""
    parts, first, counts, row = [], [], [], 0
    for ptr, off, nbytes, fp32 in items:
        k = -(-nbytes // chunk)
        rows = np.zeros(k, _CHUNK_DTYPE)
        lo = np.arange(k, dtype=np.uint64) * np.uint64(chunk)
        rows["src"] = np.uint64(ptr) + lo
        rows["dst_off"] = np.uint64(off) + lo
        rows["nbytes"] = np.minimum(np.uint64(nbytes) - lo, np.uint64(chunk)).astype(np.uint32) if k else 0
        rows["flags"] = (_SNAP_FP32 if fp32 else 0) | (_SNAP_VEC16 if ptr % 16 == 0 else _SNAP_WORD if ptr % 4 == 0 else 0)
        parts.append(rows); first.append(row); counts.append(k)
        row += k
    table = np.concatenate(parts) if parts else np.zeros(0, _CHUNK_DTYPE)
    return table, np.asarray(first, np.int64), np.asarray(counts, np.int64)


class Snapshot:
    """The state as it was in stream order when `snapshot()` was called.  `wait()` blocks until the bytes are on the host and returns
    {name: host tensor}; it also fills `tensors`, `checksums` {name: (S1, S2)} and `nonfinite` {name: count}.  The host tensors of device
    sources are views of ONE cached pinned buffer per device: they are valid until the next `snapshot()` of that device."""

    def __init__(self):
        self.tensors: Dict[str, Tensor] = {}
        self.checksums: Dict[str, Tuple[int, int]] = {}
        self.nonfinite: Dict[str, int] = {}
        self._names: List[str] = []
        self._host: Dict[str, Tensor] = {}          # numpy route: private host copies
        self._groups = []                            # kernel route, per device
        self._keep = []                              # temporaries the launch reads
        self._done = False

    def first_nonfinite(self) -> Optional[Tuple[str, int]]:
        self.wait()
        for name in self._names:
            if self.nonfinite[name]:
                return name, self.nonfinite[name]
        return None

    def wait(self) -> Dict[str, Tensor]:
        if self._done:
            return self.tensors
        chunk_words = None
        got = {}
        for g in self._groups:
            g["event"].synchronize()
            host = g["pinned"].numpy()
            if chunk_words is None:
                chunk_words = chunk_bytes() // 4
            partials = host[g["partials_off"]:g["partials_off"] + g["n_chunks"] * _PARTIAL_DTYPE.itemsize].view(_PARTIAL_DTYPE)
            with np.errstate(over="ignore"):
                for name, t_like, off, nbytes, first, k in g["entries"]:
                    p = partials[first:first + k]
                    base = np.arange(k, dtype=np.uint64) * np.uint64(chunk_words)
                    s1 = int(p["s1"].sum(dtype=np.uint64)) & _MASK
                    s2 = int((p["s2"] + base * p["s1"]).sum(dtype=np.uint64)) & _MASK
                    bad = int(p["nonfinite"].sum(dtype=np.uint64))
                    # a storage of exactly this tensor's bytes over the pinned memory: torch.save then writes one record per tensor
                    flat = torch.from_numpy(host[off:off + nbytes])
                    dtype, shape = t_like
                    got[name] = (flat.view(dtype).reshape(shape), (s1, s2), bad)
        for name, t in self._host.items():
            got[name] = (t, checksum(t), count_nonfinite(t))
        for name in self._names:
            self.tensors[name], self.checksums[name], self.nonfinite[name] = got[name]
        self._keep.clear()
        self._done = True
        return self.tensors


def _grown(cache, dev, need: int, **kw) -> Tensor:
    buf = cache.get(dev)
    if buf is None or buf.numel() < need:
        last = _LAST_COPY.get(dev)
        if last is not None:
            last.synchronize()                       # the buffer about to be dropped may still be in a copy
        cache[dev] = None
        buf = cache[dev] = torch.zeros(_round_up(need, 1 << 20), dtype=torch.uint8, **kw)
    return buf


def snapshot(tensors: Dict[str, Tensor], stream=None) -> Snapshot:
    """Capture `tensors` as they are in the order of `stream` (default: the current stream of each tensor's device).

    Device tensors: ONE launch of csrc/vit_snapshot.hip per device packs them into a cached staging buffer (tensor starts aligned to 64 bytes,
    the per-chunk partial records behind the data); the caller's stream is held for that launch only.  A side stream then waits for it and
    copies the staging buffer into a cached pinned host buffer in one asynchronous copy, with an event recorded that `Snapshot.wait()` waits
    for.  Writes to the sources issued after this call (the next optimizer step) are ordered behind the launch and do not show.
    CPU tensors, and tensors the kernel does not take (non-strided layouts), are copied at once and go through the numpy restatement, which
    gives the same bytes, checksums and counts; a non-contiguous device tensor is made contiguous first.
    One staging / pinned pair per device: a second `snapshot()` waits (on the stream, not the host) for the previous copy to have read the
    staging buffer, and overwrites the host views the previous `wait()` returned -- consume them first (`Checkpointer` does)."""
    snap = Snapshot()
    per_dev: Dict[torch.device, list] = {}
    for name, t in tensors.items():
        if not isinstance(t, Tensor):
            raise TypeError(f"snapshot: {name!r} is not a tensor")
        snap._names.append(name)
        t = t.detach()
        if t.device.type == "cuda" and t.layout == torch.strided and not t.is_complex() and not t.is_quantized:
            if not t.is_contiguous():
                t = t.contiguous()
                CALLS["made_contiguous"] += 1
            per_dev.setdefault(t.device, []).append((name, t))
            CALLS["kernel"] += 1
        else:
            if t.layout != torch.strided:
                t = t.to_dense()
            snap._host[name] = t.to("cpu", copy=True).contiguous()
            CALLS["numpy"] += 1
    if not per_dev:
        return snap
    lib = _lib()
    chunk = chunk_bytes()
    for dev, named in per_dev.items():
        with torch.cuda.device(dev):
            items, entries, off = [], [], 0
            for name, t in named:
                nbytes = t.numel() * t.element_size()
                items.append((t.data_ptr() if nbytes else 0, off, nbytes, t.dtype == torch.float32))
                entries.append([name, (t.dtype, tuple(t.shape)), off, nbytes])
                off = _round_up(off + nbytes, ALIGN)
            train = stream if stream is not None else torch.cuda.current_stream(dev)
            key = tuple(items)
            hit = _TABLES.get(dev)
            if hit is not None and hit[0] == key:
                _, _, dev_table, first, counts = hit
                CALLS["table_reused"] += 1
            else:
                table, first, counts = _build_table(items, chunk)
                pinned_table = torch.from_numpy(table.view(np.uint8).reshape(-1).copy()).pin_memory() if table.size else None
                with torch.cuda.stream(train):
                    dev_table = pinned_table.to(dev, non_blocking=True) if table.size else None
                _TABLES[dev] = (key, pinned_table, dev_table, first, counts)       # (the pinned copy stays alive for the transfer)
            n_chunks = int(counts.sum())
            for e, f, k in zip(entries, first, counts):
                e += [int(f), int(k)]
            partials_off = _round_up(off, ALIGN)
            total = partials_off + n_chunks * _PARTIAL_DTYPE.itemsize
            staging = _grown(_STAGING, dev, max(total, 1), device=dev)
            pinned = _grown(_PINNED, dev, max(total, 1), pin_memory=True)
            side = _SIDE.get(dev)
            if side is None:
                side = _SIDE[dev] = torch.cuda.Stream(dev)
            last = _LAST_COPY.get(dev)
            if last is not None:
                train.wait_event(last)               # the previous copy must have read the staging buffer
            if n_chunks:
                if n_chunks >= 1 << 31:
                    raise ValueError("snapshot: more than 2^31 chunks")
                from . import vit_ops
                timed = PACK_EVENTS is not None
                if timed:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(train)
                rc = lib.vit_snapshot_pack(dev_table.data_ptr(), n_chunks, staging.data_ptr(), staging.data_ptr() + partials_off, train.cuda_stream)
                vit_ops._check(rc, "vit_snapshot_pack")
                if timed:
                    e1.record(train)
                    PACK_EVENTS.append((e0, e1))
                CALLS["pack_launches"] += 1
            packed = torch.cuda.Event()
            packed.record(train)
            side.wait_event(packed)
            with torch.cuda.stream(side):
                pinned[:total].copy_(staging[:total], non_blocking=True)
            copied = torch.cuda.Event()
            copied.record(side)
            _LAST_COPY[dev] = copied
            snap._keep.extend(t for _, t in named)
            snap._groups.append({"event": copied, "pinned": pinned, "partials_off": partials_off, "n_chunks": n_chunks,
                                 "entries": [tuple(e) for e in entries]})
    return snap


# ---- files -------------------------------------------------------------------------------------------------------------------------------
def _flatten_optimizer(opt_sd: dict) -> Dict[str, Tensor]:
    return {f"optimizer_states/0/state/{i}/{k}": v for i, st in opt_sd["state"].items() for k, v in st.items() if isinstance(v, Tensor)}


def _collect(obj, weights_only: bool, global_step: Optional[int]):
    """(tensors to snapshot, the rest of the file's entries, is_writer).  A TrainStep's `state_dict()` is a collective in "rs_ag" mode:
    every rank gets here, rank 0 alone writes."""
    if isinstance(obj, nn.Module):
        sd = {"encoder": obj.state_dict(), "global_step": 0}
        writer = True
    else:
        sd = obj.state_dict(optimizer=not weights_only)
        writer = getattr(obj.reducer, "rank", 0) == 0
    tensors = {"state_dict/encoder." + k: v for k, v in sd["encoder"].items()}
    meta = {"global_step": int(sd["global_step"] if global_step is None else global_step), "epoch": 0}
    if not weights_only:
        if sd.get("optimizer") is None:
            raise ValueError("save_checkpoint(weights_only=False) needs a TrainStep (an encoder alone has no optimizer state)")
        tensors.update(_flatten_optimizer(sd["optimizer"]))
        meta["optimizer"] = sd["optimizer"]
        meta["scheduler"] = sd.get("scheduler")
    return tensors, meta, writer


class _Save:
    """one file: the snapshot (taken in the constructor, in stream order) and the deferred host work (`run`)"""

    def __init__(self, obj, path, weights_only: bool, global_step: Optional[int], refuse_nonfinite: bool):
        self.path = Path(path)
        self.refuse_nonfinite = refuse_nonfinite
        tensors, self.meta, self.writer = _collect(obj, weights_only, global_step)
        self.snap = snapshot(tensors) if self.writer else None
        self.error: Optional[BaseException] = None
        self.written = False
        self._thread: Optional[threading.Thread] = None

    def run(self):
        if not self.writer:
            return
        host = self.snap.wait()
        if self.refuse_nonfinite:
            bad = self.snap.first_nonfinite()
            if bad is not None:
                raise NonFiniteCheckpoint(bad[0].split("/", 1)[1] if bad[0].startswith("state_dict/") else bad[0], bad[1], self.path)
        ckpt = {"state_dict": {k[len("state_dict/"):]: v for k, v in host.items() if k.startswith("state_dict/")},
                "global_step": self.meta["global_step"], "epoch": 0}
        if "optimizer" in self.meta:
            opt = self.meta["optimizer"]
            state = {i: {k: (host[f"optimizer_states/0/state/{i}/{k}"] if isinstance(v, Tensor) else v) for k, v in st.items()}
                     for i, st in opt["state"].items()}
            ckpt["optimizer_states"] = [{"state": state, "param_groups": opt["param_groups"]}]
            ckpt["lr_schedulers"] = [self.meta["scheduler"]] if self.meta["scheduler"] is not None else []
        ckpt["styl3r_amd"] = {"format": FORMAT, "checksums": {k: [int(a), int(b)] for k, (a, b) in self.snap.checksums.items()}}
        self.path.parent.mkdir(parents=True, exist_ok=True)
        tmp = self.path.with_name(self.path.name + ".tmp")
        try:
            with open(tmp, "wb") as f:
                torch.save(ckpt, f)
                f.flush()
                os.fsync(f.fileno())
            os.replace(tmp, self.path)               # the final name never holds a partial file
        except BaseException:
            if tmp.exists():
                tmp.unlink()
            raise
        self.written = True

    def _guarded(self):
        try:
            self.run()
        except BaseException as e:                   # re-raised by wait()
            self.error = e

    def start(self):
        self._thread = threading.Thread(target=self._guarded, name="styl3r-checkpoint", daemon=True)
        self._thread.start()
        return self

    def wait(self):
        if self._thread is not None:
            self._thread.join()
            self._thread = None
        if self.error is not None:
            e, self.error = self.error, None
            raise e
        return self.path


def save_checkpoint(train_step_or_encoder, path, weights_only: bool = True, global_step: Optional[int] = None, block: bool = False):
    """Write a wrapper-layout checkpoint (module docstring) of a `train.TrainStep` or of an encoder alone (weights only).

    COLLECTIVE for a TrainStep on more than one rank in "rs_ag" mode (`TrainStep.state_dict`): call it on every rank; rank 0 alone snapshots
    and writes.  The snapshot is taken before this returns (one launch on the current stream, module docstring); with `block=False` the wait
    for the copy, the checksum fold, `torch.save` to `<path>.tmp`, flush, fsync and the rename happen on a thread and the returned handle's
    `wait()` joins it and re-raises its error; `block=True` does all of it before returning.  Returns the handle (`.path`, `.written`)."""
    job = _Save(train_step_or_encoder, path, weights_only, global_step, refuse_nonfinite=False)
    if block:
        job.run()
        return job
    return job.start()


def _resolve(ckpt: dict, key: str):
    node = ckpt
    for part in key.split("/"):
        if isinstance(node, (list, tuple)):
            node = node[int(part)]
        elif part in node:
            node = node[part]
        else:
            node = node[int(part)]                   # optimizer state: integer keys
    return node


def load_checkpoint(path, verify: bool = True, weights_only: bool = True) -> dict:
    """`torch.load(path, map_location="cpu")`; with `verify`, every checksum stored under "styl3r_amd" is recomputed from the loaded bytes and
    the first entry that differs raises `ChecksumMismatch` (`.key`: e.g. "state_dict/encoder.backbone.enc_norm.weight").  Files without that
    entry (the released `re10k_2v.ckpt`, any Lightning checkpoint) load unverified; pass `weights_only=False` for files that pickle more than
    tensors and plain containers."""
    ckpt = torch.load(str(path), map_location="cpu", weights_only=weights_only)
    own = ckpt.get("styl3r_amd") if isinstance(ckpt, dict) else None
    if verify and own is not None:
        if own.get("format") != FORMAT:
            raise ValueError(f"{path}: checkpoint format {own.get('format')!r}, this build reads {FORMAT}")
        for key, stored in own["checksums"].items():
            found = checksum(_resolve(ckpt, key))
            if tuple(int(x) for x in stored) != found:
                raise ChecksumMismatch(key, stored, found)
    return ckpt


def resume(train_step, ckpt) -> dict:
    """Load a checkpoint (a path or a loaded dict) into a `train.TrainStep`: the encoder always; the optimizer state, the scheduler state and
    `global_step` when the file has them (`weights_only=False` saves).  A weights-only file leaves the optimizer fresh and `global_step`
    where it is, like the reference's `state_dict`-only loading (main_style.py:190-192)."""
    if not isinstance(ckpt, dict):
        ckpt = load_checkpoint(ckpt)
    sd = {"encoder": {k[len("encoder."):]: v for k, v in ckpt["state_dict"].items() if k.startswith("encoder.")}}
    if ckpt.get("optimizer_states"):
        sd["optimizer"] = ckpt["optimizer_states"][0]
        sd["global_step"] = int(ckpt.get("global_step", 0))
        if ckpt.get("lr_schedulers"):
            sd["scheduler"] = ckpt["lr_schedulers"][0]
    train_step.load_state_dict(sd)
    return ckpt


# ---- policy ------------------------------------------------------------------------------------------------------------------------------
@dataclass
class CheckpointCfg:
    """config/main.yaml:40-44 `checkpointing:`"""
    every_n_train_steps: int = 5000
    save_top_k: int = 1
    save_weights_only: bool = True
    load: Optional[str] = None


class Checkpointer:
    """`ModelCheckpoint(dirpath, every_n_train_steps, save_top_k, save_weights_only, monitor="info/global_step", mode="max")` of
    main_style.py:80-90 with `CHECKPOINT_EQUALS_CHAR = '_'`: files `epoch_0-step_<n>.ckpt`, the `save_top_k` with the largest step are kept
    (-1: all, 0: none are written).  `after_step(train_step)` goes after every train step and returns after the pack launch and the enqueue of
    the copy; ONE writer thread drains the saves in order.  There is one staging buffer: a save that comes due while the previous one is
    still being written waits for it first.  `after_step` is a collective when `TrainStep.state_dict` is (rank 0 alone writes).
    `refuse_nonfinite`: a snapshot with NaN / inf in it writes nothing and prunes nothing; `wait()` / `close()` raise `NonFiniteCheckpoint`."""

    def __init__(self, cfg: CheckpointCfg, directory, refuse_nonfinite: bool = True):
        self.cfg, self.directory, self.refuse_nonfinite = cfg, Path(directory), refuse_nonfinite
        self.kept: List[Tuple[int, Path]] = []
        self._queue: "queue.Queue" = queue.Queue()
        self._errors: List[BaseException] = []
        self._thread: Optional[threading.Thread] = None

    def path_for(self, step: int) -> Path:
        return self.directory / f"epoch_0-step_{step}.ckpt"

    def restore(self, train_step):
        """`cfg.load`: resume `train_step` from that file, if one is named"""
        return resume(train_step, self.cfg.load) if self.cfg.load else None

    def _drain(self):
        while True:
            job = self._queue.get()
            try:
                if job is None:
                    return
                job.run()
                if job.written:
                    self._prune(job)
            except BaseException as e:
                self._errors.append(e)
            finally:
                self._queue.task_done()

    def _prune(self, job):
        self.kept = [(s, p) for s, p in self.kept if p != job.path] + [(job.meta["global_step"], job.path)]
        k = self.cfg.save_top_k
        if k > 0:
            self.kept.sort()
            while len(self.kept) > k:
                _, old = self.kept.pop(0)
                if old.exists():
                    old.unlink()

    def after_step(self, train_step) -> bool:
        n, k = self.cfg.every_n_train_steps, self.cfg.save_top_k
        step = int(train_step.global_step)
        if not n or n < 0 or k == 0 or step % n:
            return False
        self._queue.join()                           # one staging buffer: the save in flight first
        job = _Save(train_step, self.path_for(step), self.cfg.save_weights_only, step, self.refuse_nonfinite)
        if self._thread is None:
            self._thread = threading.Thread(target=self._drain, name="styl3r-checkpoint-writer", daemon=True)
            self._thread.start()
        self._queue.put(job)
        return True

    def wait(self):
        """block until every save started so far is on disk (or refused); re-raise the first error of the writer thread"""
        self._queue.join()
        if self._errors:
            e = self._errors[0]
            self._errors.clear()
            raise e

    def close(self):
        try:
            self.wait()
        finally:
            if self._thread is not None:
                self._queue.put(None)
                self._thread.join()
                self._thread = None
