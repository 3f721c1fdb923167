#!/usr/bin/env python
"""What a checkpoint costs the train step, at full encoder size: a synthetic state with the tensor sizes of the full encoder's `state_dict()`
(shapes from the module built on the meta device, random values on the GPU; `--moments` adds two fp32 moments and a step counter per
parameter, the `weights_only=False` file).  Four numbers, each the median and the spread of `--reps` repetitions, the two routes alternating:
  (a) how long `Checkpointer.after_step` holds the host (wall clock around the call) and the train stream (device events around it);
  (b) the kernel time of the pack (device events right around the one launch, warm chunk table), and the bytes it reads and writes over it;
  (c) wall time from the `after_step` call until the file is complete (`Checkpointer.wait()` returned: copy, fold, torch.save, fsync, rename);
  (d) the same file by the plain route -- `torch.save` of the wrapper-layout dict straight from the device tensors, blocking -- wall time.
Also checks that both files hold the same bytes per tensor.  One JSON line.
  python tools/bench_checkpoint.py [--reps 3] [--moments] [--dir DIR] [--scale 1.0]
`--scale` shrinks every tensor's leading dimension (rehearsals; a result taken with it says so).  There is no CPU measurement path."""
import argparse, json, shutil, sys, tempfile, time
from pathlib import Path
from types import SimpleNamespace
sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import torch
from styl3r_amd import checkpointing as ck

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=3); ap.add_argument("--moments", action="store_true"); ap.add_argument("--dir", default=None)
ap.add_argument("--scale", type=float, default=1.0); ap.add_argument("--pack-calls", type=int, default=10)
args = ap.parse_args()
assert torch.cuda.is_available(), "bench_checkpoint needs the MI355X"
dev = torch.device("cuda:0")

from styl3r_amd.encoder import EncoderNoPoSplatTokenStyle, EncoderNoPoSplatTokenStyleCfg
with torch.device("meta"):
    meta = EncoderNoPoSplatTokenStyle(EncoderNoPoSplatTokenStyleCfg(name="noposplat_token_style", stylized=False))
g = torch.Generator(dev).manual_seed(11)


def like(t):
    shape = list(t.shape)
    if args.scale != 1.0 and shape and shape[0] > 8:
        shape[0] = max(8, int(shape[0] * args.scale))
    if t.dtype.is_floating_point:
        return torch.randn(shape, device=dev, dtype=t.dtype, generator=g)
    return torch.zeros(shape, device=dev, dtype=t.dtype)


encoder_sd = {k: like(v) for k, v in meta.state_dict().items()}
param_names = [n for n, _ in meta.named_parameters()]
opt_sd = None
if args.moments:
    state = {i: {"step": torch.tensor(100.0, device=dev), "exp_avg": like(encoder_sd[n]), "exp_avg_sq": like(encoder_sd[n]).abs_()}
             for i, n in enumerate(param_names)}
    opt_sd = {"state": state, "param_groups": [{"lr": 2e-4, "betas": (0.9, 0.95), "eps": 1e-8, "weight_decay": 0.05, "params": list(range(len(param_names)))}]}


class SyntheticStep:
    """what Checkpointer needs of a train.TrainStep"""
    reducer = SimpleNamespace(rank=0)
    global_step = 0

    def state_dict(self, optimizer=True):
        return {"encoder": encoder_sd, "optimizer": opt_sd if optimizer else None, "scheduler": None, "global_step": self.global_step}


def wrapper_dict(step):
    d = {"state_dict": {"encoder." + k: v for k, v in encoder_sd.items()}, "global_step": step, "epoch": 0}
    if args.moments:
        d["optimizer_states"], d["lr_schedulers"] = [opt_sd], []
    return d


tensors = {"state_dict/encoder." + k: v for k, v in encoder_sd.items()}
if args.moments:
    tensors.update(ck._flatten_optimizer(opt_sd))
nbytes = sum(t.numel() * t.element_size() for t in tensors.values())
out_dir = Path(tempfile.mkdtemp(prefix="bench_ckpt_", dir=args.dir))
step = SyntheticStep()
saver = ck.Checkpointer(ck.CheckpointCfg(every_n_train_steps=1, save_top_k=1, save_weights_only=not args.moments), out_dir / "hip")
(out_dir / "plain").mkdir()
work = torch.randn(4096, 4096, device=dev)          # stands for the next train step: queued behind the pack on the train stream


def ours():
    step.global_step += 1
    torch.cuda.synchronize(dev)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    assert saver.after_step(step)
    e1.record()
    t1 = time.perf_counter()
    (work @ work).sum()                               # the train stream goes on while the copy and the writer run
    saver.wait()
    t2 = time.perf_counter()
    torch.cuda.synchronize(dev)
    return {"host_ms": (t1 - t0) * 1e3, "stream_ms": e0.elapsed_time(e1), "file_complete_ms": (t2 - t0) * 1e3}


def plain():
    torch.cuda.synchronize(dev)
    path = out_dir / "plain" / "plain.ckpt"
    t0 = time.perf_counter()
    torch.save(wrapper_dict(step.global_step), path)
    return {"file_complete_ms": (time.perf_counter() - t0) * 1e3}, path


def pack_only():
    """events right around the launch (checkpointing.PACK_EVENTS): events around `snapshot()` would count the host's way to the launch"""
    torch.cuda.synchronize(dev)
    ck.PACK_EVENTS = []
    ck.snapshot(tensors).wait()
    torch.cuda.synchronize(dev)
    (e0, e1), = ck.PACK_EVENTS
    ck.PACK_EVENTS = None
    return e0.elapsed_time(e1)


stats = lambda ts: {"median": round(sorted(ts)[len(ts) // 2], 3), "min": round(min(ts), 3), "max": round(max(ts), 3)}
n0 = ck.CALLS["pack_launches"]
ours(); plain()                                       # warm-up of both routes: code objects, pinned buffer, chunk table, page cache
assert ck.CALLS["pack_launches"] == n0 + 1 and ck.CALLS["numpy"] == 0, "the save did not take the kernel route"
a, d = [], []
for _ in range(args.reps):
    a.append(ours()); d.append(plain()[0])
# same bytes in both files
mine = ck.load_checkpoint(saver.path_for(step.global_step))
theirs = torch.load(str(out_dir / "plain" / "plain.ckpt"), map_location="cpu", weights_only=True)
same = all(torch.equal(mine["state_dict"][k].reshape(-1).view(torch.uint8), theirs["state_dict"][k].reshape(-1).view(torch.uint8)) for k in theirs["state_dict"])
sizes = {"hip": saver.path_for(step.global_step).stat().st_size, "plain": (out_dir / "plain" / "plain.ckpt").stat().st_size}
del mine, theirs
saver.close()
pack = [pack_only() for _ in range(args.pack_calls + 2)][2:]
pack_ms = stats(pack)
res = {"metric": "checkpoint save at full encoder size: one-launch snapshot + writer thread vs blocking torch.save of the device tensors",
       "moments": bool(args.moments), "scale": args.scale, "tensors": len(tensors), "state_GB": round(nbytes / 1e9, 3), "reps": args.reps,
       "a_after_step_host_ms": stats([x["host_ms"] for x in a]), "a_after_step_train_stream_ms": stats([x["stream_ms"] for x in a]),
       "b_pack_kernel_ms": pack_ms, "b_pack_TBps_read_plus_write": round(2 * nbytes / (pack_ms["median"] * 1e-3) / 1e12, 3),
       "c_file_complete_ms": stats([x["file_complete_ms"] for x in a]), "d_plain_torch_save_ms": stats([x["file_complete_ms"] for x in d]),
       "files_hold_the_same_bytes": bool(same), "file_bytes": sizes, "calls": dict(ck.CALLS)}
shutil.rmtree(out_dir, ignore_errors=True)
print(json.dumps(res))
