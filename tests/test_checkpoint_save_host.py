"""Saving and resuming, host side (styl3r_amd/checkpointing.py, TrainStep.state_dict / load_state_dict): the checksum's definition, the
wrapper file layout, corruption detection, the ModelCheckpoint policy, the non-finite refusal, bit-exact resume on the CPU and the sharded
("rs_ag") optimizer state on a world-2 gloo group.  No GPU: every tensor takes the numpy route.  All comparisons are bit-exact."""
import json
import os
import subprocess
import sys
import textwrap
from pathlib import Path

import numpy as np
import pytest
import torch

from tests.ckpt_utils import hand_batch, hand_train_step

ROOT = Path(__file__).resolve().parents[1]
M64 = (1 << 64) - 1


def definition(raw: bytes):
    """S1 = sum w_i, S2 = sum (i + 1) w_i mod 2^64 in Python integers"""
    raw = raw + b"\0" * (-len(raw) % 4)
    words = [int.from_bytes(raw[i:i + 4], "little") for i in range(0, len(raw), 4)]
    return sum(words) & M64, sum((i + 1) * w for i, w in enumerate(words)) & M64


def test_checksum_is_the_definition_and_is_position_sensitive():
    from styl3r_amd.checkpointing import checksum, count_nonfinite
    rng = np.random.default_rng(0)
    for n in (0, 1, 3, 4, 5, 7, 8, 64, 1001):
        raw = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        assert checksum(raw) == definition(raw), n
    big = np.full(300_000, 0xFFFFFFFF, np.uint32)                       # S2 wraps past 2^64; more than one block of the restatement
    big = np.concatenate([big] * 8)
    s1 = big.size * 0xFFFFFFFF
    assert checksum(big) == (s1 & M64, (0xFFFFFFFF * (big.size * (big.size + 1) // 2)) & M64)
    assert checksum(b"") == (0, 0)
    # a length that is no multiple of 4: the last word is zero-extended
    assert checksum(b"\x01\x02\x03\x04\x05") == (0x04030201 + 0x05, 0x04030201 + 2 * 0x05)
    assert checksum(b"\x01\x02\x03\x04\x05") == checksum(b"\x01\x02\x03\x04\x05\x00\x00\x00")
    t = torch.arange(40, dtype=torch.float32)
    base = checksum(t)
    assert base == definition(t.numpy().tobytes()) == checksum(t.numpy()) == checksum(t.reshape(5, 8))
    flipped = t.clone(); flipped.view(torch.int32)[17] ^= 1 << 9
    assert checksum(flipped)[0] != base[0] and checksum(flipped)[1] != base[1]
    swapped = t.clone(); swapped[[3, 30]] = swapped[[30, 3]]
    assert checksum(swapped)[0] == base[0] and checksum(swapped)[1] != base[1]
    assert checksum(torch.ones(3, dtype=torch.bfloat16)) == definition(b"\x80\x3f" * 3)
    assert checksum(torch.tensor(2.0)) == definition(np.float32(2).tobytes())           # 0-dim
    x = torch.tensor([float("inf"), float("-inf"), float("nan"), -0.0, 1e-45, 1.0, 3.4e38])
    assert count_nonfinite(x) == 3 and count_nonfinite(x.double()) == 0 and count_nonfinite(x.view(torch.int32)) == 0


def test_chunk_table_is_the_headers_struct_and_cuts_tensors_at_the_chunk_size():
    """no device needed: the records `checkpointing` packs are include/vit_ops.h's structs, tensors are cut at the library's chunk size with
    the alignment flags of their source, and bad arguments are refused before any launch"""
    import ctypes as C
    import re
    from styl3r_amd import checkpointing as ck, vit_ops
    vit_ops.build_library()
    lib = vit_ops.load()
    header = (ROOT / "include/vit_ops.h").read_text()
    for name, dtype, size in (("VitSnapChunk", ck._CHUNK_DTYPE, 24), ("VitSnapPartial", ck._PARTIAL_DTYPE, 24)):
        body = re.search(rf"typedef struct {name} \{{(.*?)\}} {name};", header, re.S).group(1)
        assert re.findall(r"\b(\w+);", body) == list(dtype.names) and dtype.itemsize == size, name
    flags = {n: int(re.search(rf"#define VIT_SNAP_{n} (\d+)", header).group(1)) for n in ("FP32", "VEC16", "WORD")}
    assert (flags["FP32"], flags["VEC16"], flags["WORD"]) == (ck._SNAP_FP32, ck._SNAP_VEC16, ck._SNAP_WORD)
    ch = ck.chunk_bytes()
    assert ch == lib.vit_snapshot_chunk_bytes() and ch % 64 == 0 and ch >= 4096
    items = [(4096, 0, 5, False), (8192 + 4, 64, 2 * ch + 3, True), (0, 2 * ch + 128, 0, True), (12289, 2 * ch + 128, ch, False)]
    table, first, counts = ck._build_table(items, ch)
    assert counts.tolist() == [1, 3, 0, 1] and first.tolist() == [0, 1, 4, 4] and len(table) == 5
    assert table["src"].tolist() == [4096, 8196, 8196 + ch, 8196 + 2 * ch, 12289]
    assert table["dst_off"].tolist() == [0, 64, 64 + ch, 64 + 2 * ch, 2 * ch + 128]
    assert table["nbytes"].tolist() == [5, ch, ch, 3, ch]
    assert table["flags"].tolist() == [ck._SNAP_VEC16, ck._SNAP_FP32 | ck._SNAP_WORD, ck._SNAP_FP32 | ck._SNAP_WORD, ck._SNAP_FP32 | ck._SNAP_WORD, 0]
    one = C.c_void_p(64)                                            # (validation only: nothing is dereferenced)
    assert lib.vit_snapshot_pack(None, 0, None, None, None) == 0
    assert lib.vit_snapshot_pack(None, 1, one, one, None) == -1 and lib.vit_snapshot_pack(one, -1, one, one, None) == -1
    assert lib.vit_snapshot_pack(one, 1, None, one, None) == -1 and lib.vit_snapshot_pack(one, 1, one, None, None) == -1
    assert lib.vit_snapshot_pack(one, 1, C.c_void_p(96), one, None) == -1 and lib.vit_snapshot_pack(one, 1, one, C.c_void_p(68), None) == -1


@pytest.fixture(scope="module")
def student_file(tmp_path_factory):
    from styl3r_amd.checkpointing import save_checkpoint
    from tests.test_distill_host import tiny_student
    enc = tiny_student()
    path = tmp_path_factory.mktemp("ckpt") / "student.ckpt"
    job = save_checkpoint(enc, path, global_step=123, block=True)
    assert job.written and not list(path.parent.glob("*.tmp"))
    return enc, path


def test_file_has_the_wrapper_layout_and_loads_into_a_fresh_encoder(student_file):
    from styl3r_amd.checkpoint import load_pretrained_encoder, load_wrapper_checkpoint
    from styl3r_amd.checkpointing import load_checkpoint
    from tests.test_distill_host import tiny_student
    enc, path = student_file
    ckpt = load_checkpoint(path)
    assert ckpt["global_step"] == 123 and ckpt["epoch"] == 0 and "optimizer_states" not in ckpt
    assert ckpt["styl3r_amd"]["format"] == 1
    want = enc.state_dict()
    assert set(ckpt["state_dict"]) == {"encoder." + k for k in want} and all(k.startswith("encoder.") for k in ckpt["state_dict"])
    assert set(ckpt["styl3r_amd"]["checksums"]) == {"state_dict/" + k for k in ckpt["state_dict"]}
    plain = torch.load(str(path), weights_only=True)["state_dict"]                   # the reference's way in (main_style.py:190-192)
    fresh = tiny_student()
    with torch.no_grad():
        for p in fresh.parameters():
            p.add_(1.0)
    res = load_wrapper_checkpoint(fresh, {"state_dict": plain}, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    for k, v in fresh.state_dict().items():
        assert v.dtype == want[k].dtype and torch.equal(v.view(torch.uint8) if v.dim() else v, want[k].view(torch.uint8) if v.dim() else want[k]), k
    again = tiny_student()
    missing, unexpected = load_pretrained_encoder(again, ckpt)
    assert not missing and not unexpected


def test_a_flipped_byte_in_the_file_is_found_and_named(student_file, tmp_path):
    from styl3r_amd.checkpointing import ChecksumMismatch, load_checkpoint
    enc, path = student_file
    raw = bytearray(path.read_bytes())
    sd = enc.state_dict()
    for key in sorted(sd, key=lambda k: -sd[k].numel()):             # the largest tensor whose bytes occur once in the file
        needle = sd[key].numpy().tobytes()
        at = bytes(raw).find(needle)
        if at > 0 and bytes(raw).find(needle, at + 1) < 0:
            break
    else:
        raise AssertionError("no tensor with unique bytes")
    assert len(needle) >= 4096
    raw[at + len(needle) // 2] ^= 0x10
    bad = tmp_path / "flipped.ckpt"
    bad.write_bytes(raw)
    with pytest.raises(ChecksumMismatch) as err:
        load_checkpoint(bad)
    assert err.value.key == "state_dict/encoder." + key and key in str(err.value)
    loaded = load_checkpoint(bad, verify=False)
    assert not torch.equal(loaded["state_dict"]["encoder." + key], enc.state_dict()[key])
    # a file without the entry (the released re10k_2v.ckpt, any foreign checkpoint) loads unverified
    foreign = tmp_path / "foreign.ckpt"
    torch.save({"state_dict": {"encoder.x": torch.ones(3)}, "global_step": 5}, foreign)
    assert load_checkpoint(foreign)["global_step"] == 5


def run_policy(tmp_path, top_k, steps=7, every=2):
    from styl3r_amd.checkpointing import CheckpointCfg, Checkpointer
    ts = hand_train_step()
    ck = Checkpointer(CheckpointCfg(every_n_train_steps=every, save_top_k=top_k), tmp_path)
    for i in range(steps):
        ts(hand_batch(seed=i))
        ck.after_step(ts)
    return ts, ck


def test_policy_keeps_the_top_k_largest_steps_and_leaves_no_partial_file(tmp_path):
    ts, ck = run_policy(tmp_path / "a", 2)
    ck.close()
    assert sorted(p.name for p in (tmp_path / "a").iterdir()) == ["epoch_0-step_4.ckpt", "epoch_0-step_6.ckpt"]
    from styl3r_amd.checkpointing import load_checkpoint
    newest = load_checkpoint(tmp_path / "a" / "epoch_0-step_6.ckpt")
    assert newest["global_step"] == 6 and "optimizer_states" not in newest              # save_weights_only=True is the default
    # `CheckpointCfg.load`: a fresh TrainStep takes the weights of that file
    from styl3r_amd.checkpointing import CheckpointCfg, Checkpointer
    fresh = hand_train_step()
    assert Checkpointer(CheckpointCfg(), tmp_path / "d").restore(fresh) is None
    Checkpointer(CheckpointCfg(load=str(tmp_path / "a" / "epoch_0-step_6.ckpt")), tmp_path / "d").restore(fresh)
    assert all(_beq(v, newest["state_dict"]["encoder." + k]) for k, v in fresh.encoder.state_dict().items()) and fresh.global_step == 0
    ts, ck = run_policy(tmp_path / "b", 0)
    ck.close()
    assert not (tmp_path / "b").exists() or not list((tmp_path / "b").iterdir())
    ts, ck = run_policy(tmp_path / "c", -1)
    ck.close()
    assert sorted(p.name for p in (tmp_path / "c").iterdir()) == [f"epoch_0-step_{n}.ckpt" for n in (2, 4, 6)]


def test_a_diverged_step_does_not_replace_the_last_good_file(tmp_path):
    from styl3r_amd.checkpointing import NonFiniteCheckpoint
    ts, ck = run_policy(tmp_path, 1, steps=2)
    ck.wait()
    good = tmp_path / "epoch_0-step_2.ckpt"
    before = good.read_bytes()
    with torch.no_grad():
        ts.encoder.backbone[1].weight[3, 5] = float("nan")
    ts.global_step = 4
    assert ck.after_step(ts)
    with pytest.raises(NonFiniteCheckpoint) as err:
        ck.wait()
    assert err.value.key == "encoder.backbone.1.weight" and err.value.count >= 1 and "backbone.1.weight" in str(err.value)
    ck.close()
    assert [p.name for p in tmp_path.iterdir()] == ["epoch_0-step_2.ckpt"] and good.read_bytes() == before


def _beq(x, y):
    """bit-equal (NaN payloads and signed zeros included)"""
    return x.dtype == y.dtype and x.shape == y.shape and torch.equal(x.detach().reshape(-1).view(torch.uint8), y.detach().reshape(-1).view(torch.uint8))


def _state_of(ts):
    opt = ts.optimizer.state_dict()
    return ([p.detach().clone() for p in ts.encoder.parameters()],
            [(i, k, v.clone() if torch.is_tensor(v) else v) for i, st in sorted(opt["state"].items()) for k, v in sorted(st.items())],
            [g["lr"] for g in opt["param_groups"]], ts.global_step, ts.scheduler.get_last_lr() if ts.scheduler is not None else None)


def _assert_same_state(a, b):
    pa, sa, la, ga, ra = a
    pb, sb, lb, gb, rb = b
    assert len(pa) == len(pb) and all(_beq(x, y) for x, y in zip(pa, pb))
    assert [(i, k) for i, k, _ in sa] == [(i, k) for i, k, _ in sb] and sa
    for (i, k, x), (_, _, y) in zip(sa, sb):
        assert _beq(x, y) if torch.is_tensor(x) else x == y, (i, k)
    assert la == lb and ga == gb and ra == rb


def test_resume_on_the_cpu_continues_bit_for_bit(tmp_path):
    """four steps straight == two steps, save (weights_only=False), fresh objects, resume, two more steps: parameters, moments, step
    counters, global_step and learning rates; a weights-only file resumes the weights and leaves a fresh optimizer"""
    from oracle.encoder_cpu import cpu_attention
    from styl3r_amd.checkpointing import load_checkpoint, resume, save_checkpoint
    from styl3r_amd.train import TrainStep
    from tests.test_distill_host import distill_batch, tiny_student, tiny_teacher
    teacher = tiny_teacher()
    batches = [distill_batch(b=1) for _ in range(4)]
    for i, b in enumerate(batches):
        b["context"]["image"] = b["context"]["image"] + 0.01 * i

    def make():
        return TrainStep(tiny_student(), None, distiller=teacher, distill_only=True, warm_up_steps=3, lr=1e-5)
    with cpu_attention():
        straight = make()
        for b in batches:
            straight(b)
        first = make()
        for b in batches[:2]:
            first(b)
        save_checkpoint(first, tmp_path / "full.ckpt", weights_only=False, block=True)
        save_checkpoint(first, tmp_path / "weights.ckpt", block=True)
        second = make()
        ckpt = resume(second, tmp_path / "full.ckpt")
        assert ckpt["global_step"] == 2 and second.global_step == 2 and len(ckpt["optimizer_states"]) == 1 and len(ckpt["lr_schedulers"]) == 1
        _assert_same_state(_state_of(first), _state_of(second))
        for b in batches[2:]:
            second(b)
    _assert_same_state(_state_of(straight), _state_of(second))
    assert second.global_step == 4 and all(torch.isfinite(p).all() for p in second.encoder.parameters())
    assert any(not _beq(x, y) for x, y in zip(first.encoder.parameters(), second.encoder.parameters()))         # it did train on
    third = make()
    resume(third, load_checkpoint(tmp_path / "weights.ckpt"))
    assert all(_beq(x, y) for x, y in zip(third.encoder.state_dict().values(), first.encoder.state_dict().values()))
    assert third.global_step == 0 and not third.optimizer.state_dict()["state"]


def test_train_step_state_dict_covers_frozen_weights_and_load_bumps_versions():
    ts = hand_train_step()
    ts(hand_batch())
    sd = ts.state_dict()
    assert set(sd) == {"encoder", "optimizer", "scheduler", "global_step"} and sd["global_step"] == 1
    assert set(sd["encoder"]) == set(ts.encoder.state_dict()) and "table" in sd["encoder"] and "scale" in sd["encoder"]
    assert ts.state_dict(optimizer=False)["optimizer"] is None
    other = hand_train_step()
    ids = [id(p) for p in other.encoder.parameters()]
    versions = [p._version for p in other.encoder.parameters()]
    other.load_state_dict(sd)
    assert ids == [id(p) for p in other.encoder.parameters()]                        # written in place
    assert all(p._version > v for p, v in zip(other.encoder.parameters(), versions))
    _assert_same_state(_state_of(ts), _state_of(other))


SHARDED_WORKER = textwrap.dedent("""
    import json, sys
    sys.path.insert(0, %r)
    import torch
    from styl3r_amd import dist_utils
    from styl3r_amd.checkpointing import load_checkpoint, resume, save_checkpoint
    from tests.ckpt_utils import hand_batch, hand_train_step
    rank, _, world = dist_utils.env_world()
    dist = dist_utils.init_distributed("gloo")
    out = sys.argv[1]

    def run(mode):
        ts = hand_train_step(dist=dist, dp_mode=mode, bucket_bytes=8 * 1024, clip=None)
        for i in range(3):
            ts(hand_batch(seed=10 * i + rank))                   # different data per rank
        job = save_checkpoint(ts, f"{out}/{mode}.ckpt", weights_only=False, block=True)      # a collective: every rank calls it
        dist.barrier()
        return ts, job
    ta, ja = run("all_reduce")
    tb, jb = run("rs_ag")
    fa, fb = load_checkpoint(f"{out}/all_reduce.ckpt"), load_checkpoint(f"{out}/rs_ag.ckpt")
    sa, sb = fa["optimizer_states"][0]["state"], fb["optimizer_states"][0]["state"]
    same_moments = sorted(sa) == sorted(sb) and all(torch.equal(sa[i][k], sb[i][k]) for i in sa for k in sa[i])
    same_weights = all(torch.equal(fa["state_dict"][k], fb["state_dict"][k]) for k in fa["state_dict"])
    # the ranges rank 0 does not own: filled by the consolidation, not zeros
    params = [p for g in tb.optimizer.param_groups for p in g["params"]]
    foreign_zero, foreign = 0, 0
    for i, p in enumerate(params):
        r = tb.reducer._range.get(id(p))
        mask = torch.ones(p.numel(), dtype=torch.bool)
        if r is not None:
            mask[r[0]:r[1]] = False
        if rank != 0:
            mask = ~mask
        v = sb[i]["exp_avg_sq"].reshape(-1)[mask]             # on rank 1: what rank 1 owns = what rank 0 does not
        foreign += v.numel(); foreign_zero += int((v == 0).sum())
    # back into both modes: one more step of the resumed objects == one more step of the original
    cont = {}
    for mode, orig in (("all_reduce", ta), ("rs_ag", tb)):
        fresh = hand_train_step(dist=dist, dp_mode=mode, bucket_bytes=8 * 1024, clip=None)
        resume(fresh, fb if mode == "rs_ag" else fa)
        orig(hand_batch(seed=77 + rank)); fresh(hand_batch(seed=77 + rank))
        orig.reducer.wait_params(); fresh.reducer.wait_params()
        cont[mode] = all(torch.equal(x, y) for x, y in zip(orig.encoder.parameters(), fresh.encoder.parameters())) and fresh.global_step == 4
    cross = hand_train_step(dist=dist, dp_mode="all_reduce", bucket_bytes=8 * 1024, clip=None)
    resume(cross, fb)                                          # the sharded run's file into the other mode
    cross_state = cross.optimizer.state_dict()["state"]
    cross_ok = all(torch.equal(cross_state[i][k], sb[i][k]) for i in sb for k in sb[i])
    print(json.dumps(dict(rank=rank, same_moments=same_moments, same_weights=same_weights, foreign=foreign, foreign_zero=foreign_zero,
                          writer=[ja.written, jb.written], cont=cont, cross_ok=cross_ok, n_state=len(sb),
                          kinds=[type(ta.optimizer).__name__, type(tb.optimizer).__name__])), flush=True)
    dist.barrier(); dist.destroy_process_group()
""") % str(ROOT)


def test_sharded_optimizer_state_is_saved_whole_and_loads_into_both_modes(tmp_path):
    script = tmp_path / "sharded.py"; script.write_text(SHARDED_WORKER)
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29581", WORLD_SIZE="2")
    procs = [subprocess.Popen([sys.executable, str(script), str(tmp_path)], env=dict(env, RANK=str(r), LOCAL_RANK=str(r)),
                              stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for r in range(2)]
    for r, p in enumerate(procs):
        o, e = p.communicate(timeout=180)
        assert p.returncode == 0, e[-3000:]
        d = json.loads(o.strip().splitlines()[-1])
        assert d["kinds"][1] == "ShardedAdamWTorch" and d["n_state"] >= 9, d
        assert d["same_moments"] and d["same_weights"], d
        assert d["foreign"] > 1000 and d["foreign_zero"] == 0, d
        assert d["writer"] == [r == 0, r == 0], d                                      # rank 0 alone writes
        assert d["cont"] == {"all_reduce": True, "rs_ag": True} and d["cross_ok"], d
    assert sorted(p.name for p in tmp_path.glob("*.ckpt")) == ["all_reduce.ckpt", "rs_ag.ckpt"]
