"""bench.py's plain run (the headline alone) and --dump-outputs (what the timed step computed, for comparing two builds)."""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]
import bench  # noqa: E402

NAMES = ("color", "depth", "loss_mse", "grad_means", "grad_covariances", "grad_harmonics", "grad_opacities")


def test_dump_outputs_writes_float32_and_samples_large_arrays_the_same_way(tmp_path):
    big = torch.arange(bench.DUMP_MAX_ELEMS + 8, dtype=torch.float64).reshape(-1, 4)
    small = torch.linspace(0, 1, 12).reshape(3, 4)
    for d in ("a", "b"):
        bench.dump_outputs(tmp_path / d, {"big": big, "small": small, "scalar": small.sum()})
    for name in ("big", "small", "scalar"):
        a, b = np.load(tmp_path / "a" / f"{name}.npy"), np.load(tmp_path / "b" / f"{name}.npy")
        assert a.dtype == np.float32 and np.array_equal(a, b)
    s = np.load(tmp_path / "a" / "big.npy")
    assert s.shape == (bench.DUMP_MAX_ELEMS,) and np.all(np.diff(s) > 0)      # distinct elements, in index order
    assert np.array_equal(np.load(tmp_path / "a" / "small.npy"), small.numpy())   # small arrays whole, shape kept


def test_dump_outputs_is_refused_on_the_dry_run():
    with pytest.raises(SystemExit):
        bench.parse(["--dry-cpu", "--dump-outputs", "x"])
    assert bench.parse([]).full is False


@pytest.mark.gpu
def test_plain_run_reports_the_headline_alone_and_dumps_the_last_step(tmp_path):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE")}
    p = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--prewarm-seconds", "0",
                        "--dump-outputs", str(tmp_path)], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    d = json.loads(p.stdout.strip().splitlines()[-1])
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup", "config"):
        assert k in d
    assert d["steps"] == 3 and d["warmup"] == 1 and d["ms_per_step"] > 0 and d["value"] > 0
    for k in ("roofline", "mse_stand_alone_kernels", "dropin_per_view", "train_step", "infer", "cpu_baseline"):
        assert k not in d, k                                                   # --full only
    files = sorted(tmp_path.glob("*.npy"))
    assert sorted(f.stem for f in files) == sorted(NAMES)
    assert sum(f.stat().st_size for f in files) <= 64 << 20
    out = {n: np.load(tmp_path / f"{n}.npy") for n in NAMES}
    for n, a in out.items():
        assert a.dtype == np.float32 and np.isfinite(a).all(), n
    V, G = 10 * 4, 256 * 256
    assert out["color"].size == bench.DUMP_MAX_ELEMS and out["grad_means"].shape == (10, G, 3) and out["grad_opacities"].shape == (10, G)
    assert out["loss_mse"].shape == () and out["loss_mse"] > 0 and V * 3 * 256 * 256 > bench.DUMP_MAX_ELEMS
    assert np.abs(out["grad_means"]).max() > 0 and np.abs(out["color"]).max() > 0
