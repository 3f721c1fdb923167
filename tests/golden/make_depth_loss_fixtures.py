"""Generates tests/golden/depth_loss_ref.npz from the REFERENCE's own `LossDepth` (src/loss/loss_depth.py:26-60), imported through
tests/golden/ref_stubs.install() as make_loss_fixtures.py does.  For each of the four configurations of tests/depth_loss_inputs.CONFIGS:
the reference's value and d loss / d depth evaluated in float64 on the fp32-rounded inputs, and its value evaluated in fp32 on the CPU.
The inputs (2, 3, 19, 37) come from tests/depth_loss_inputs.make_inputs with the first seed whose differences pass the sign condition.
    python tests/golden/make_depth_loss_fixtures.py
"""
import importlib
import sys
import types
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))
from tests.depth_loss_inputs import CONFIGS, make_inputs, sign_condition_holds, value_tolerance
from tests.golden.ref_stubs import install

install()
# ---- package shims for the loss module's imports (as in make_loss_fixtures.py) ----------------------------------------
sys.modules["src.dataset.types"] = types.ModuleType("src.dataset.types"); sys.modules["src.dataset.types"].BatchedExample = dict
importlib.import_module("src.model.types")
sys.modules["diff_gaussian_rasterization"] = types.ModuleType("diff_gaussian_rasterization")
dec = types.ModuleType("src.model.decoder.decoder")


class DecoderOutput:
    def __init__(self, color, depth=None):
        self.color, self.depth = color, depth


dec.DecoderOutput = DecoderOutput
sys.modules["src.model.decoder.decoder"] = dec
ld = importlib.import_module("src.loss.loss_depth")

WEIGHT = 0.25                                                          # config/loss/depth.yaml
SHAPE = (2, 3, 19, 37)
seed = next(s for s in range(100) if sign_condition_holds(*make_inputs(*SHAPE, s)))
depth, near, far, image = make_inputs(*SHAPE, seed)
out = dict(seed=np.array(seed), weight=np.array(WEIGHT), depth=depth.numpy(), near=near.numpy(), far=far.numpy(), image=image.numpy())
assert all(a.dtype == np.float32 for a in (out["depth"], out["near"], out["far"], out["image"]))
for tag, (sigma, second) in CONFIGS.items():
    loss = ld.LossDepth(ld.LossDepthCfgWrapper(ld.LossDepthCfg(weight=WEIGHT, sigma_image=sigma, use_second_derivative=second)))
    d = depth.double().requires_grad_(True)
    value = loss(DecoderOutput(None, d), {"target": {"near": near.double(), "far": far.double(), "image": image.double()}}, None, 0)
    value.backward()
    with torch.no_grad():
        value32 = loss(DecoderOutput(None, depth), {"target": {"near": near, "far": far, "image": image}}, None, 0)
    value = value.detach()
    err32, tol = abs(float(value32) - float(value)), value_tolerance(WEIGHT, sigma)
    assert value32.dtype == torch.float32 and err32 <= tol, (tag, err32, tol)       # the reference's own fp32 value stays inside the derived bound
    out.update({f"{tag}_value": np.array(float(value)), f"{tag}_grad": d.grad.numpy(), f"{tag}_value_fp32": np.array(float(value32), dtype=np.float32)})
    print(f"{tag:17s} value {float(value):.12f}  fp32 error {err32:.3e} (bound {tol:.3e})  max|grad| {float(d.grad.abs().max()):.4e}")
path = ROOT / "tests/golden/depth_loss_ref.npz"
np.savez_compressed(path, **out)
print("seed", seed, "bytes", path.stat().st_size)
assert path.stat().st_size < 200_000
