"""Generates tests/golden/pose_eval_ref.npz from the REFERENCE's own functions, on the CPU, data only:
  * `ssim(X, Y, data_range=1.0, size_average=True, win_size=11, retrun_seprate=True)`   src/loss/loss_ssim.py:129-189
    for two image pairs of 2 x 3 x 48 x 48 in float64 (the images are stored as float32 and evaluated as float64): the four returned
    scalars and the gradient of `1 - structure` with respect to the second image;
  * `compute_pose_error`   src/evaluation/metrics.py:87-99   for a handful of pose pairs;
  * `pose_auc`             src/misc/cam_utils.py:181-193     for an error list at thresholds 5 / 10 / 20.
cv2, lpips and skimage are not installed: they are stubbed in this process's sys.modules (the three functions above never call them).
    python tests/golden/make_pose_eval_fixtures.py
"""
import importlib
import sys
import types
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))
from tests.golden.ref_stubs import REF, install

install()
for name in ("cv2", "lpips", "skimage", "skimage.metrics"):
    sys.modules.setdefault(name, types.ModuleType(name))
sys.modules["lpips"].LPIPS = object
sys.modules["skimage.metrics"].structural_similarity = None
if not hasattr(np, "trapz"):
    np.trapz = np.trapezoid
sys.modules.setdefault("src.evaluation", types.ModuleType("src.evaluation")).__path__ = [REF + "/src/evaluation"]
ssim = importlib.import_module("src.loss.loss_ssim").ssim
compute_pose_error = importlib.import_module("src.evaluation.metrics").compute_pose_error
pose_auc = importlib.import_module("src.misc.cam_utils").pose_auc

g = torch.Generator().manual_seed(2024)
N, C, H = 2, 3, 48
ys, xs = torch.meshgrid(torch.arange(H) / H, torch.arange(H) / H, indexing="ij")
out = {}


def smooth(phase):
    return torch.stack([torch.stack([0.5 + 0.3 * torch.sin(6.28 * (1.0 + 0.5 * c) * xs + phase + n) * torch.cos(6.28 * (0.7 + 0.4 * n) * ys + c)
                                     for c in range(C)]) for n in range(N)])


# pair "smooth": a smooth field plus noise against a slightly different smooth field plus other noise
x = smooth(0.0) + 0.05 * torch.randn(N, C, H, H, generator=g)
y = smooth(0.15) + 0.05 * torch.randn(N, C, H, H, generator=g)
pairs = {"smooth": (x, y)}
# pair "flat": the left 20 columns black in both (variances below eps^2: the lower clamp), the right part almost identical in the
# first image (structure map above 0.98: the upper clamp) and clearly different in the second
x = smooth(0.3) + 0.05 * torch.randn(N, C, H, H, generator=g)
y = x + 0.002 * torch.randn(N, C, H, H, generator=g)
y[1] = smooth(0.9)[1] + 0.08 * torch.randn(C, H, H, generator=g)
x[..., :20] = 0.0
y[..., :20] = 0.0
pairs["flat"] = (x, y)
for tag, (x, y) in pairs.items():
    x32, y32 = x.float(), y.float()
    xd, yd = x32.double(), y32.double().requires_grad_(True)
    s, brightness, contrast, structure = ssim(xd, yd, data_range=1.0, size_average=True, win_size=11, retrun_seprate=True)
    (1 - structure).backward()
    out[f"{tag}_x"], out[f"{tag}_y"] = x32.numpy(), y32.numpy()
    out[f"{tag}_scalars"] = np.array([t.item() for t in (s, brightness, contrast, structure)])
    out[f"{tag}_grad"] = yd.grad.numpy()
    print(tag, out[f"{tag}_scalars"], "grad max", float(yd.grad.abs().max()))

# pose pairs: random rigid poses and perturbed copies (small and large rotations, a flipped translation)
def rigid(gen, rot_scale, trans_scale):
    w = rot_scale * torch.randn(3, generator=gen, dtype=torch.float64)
    Wm = torch.tensor([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]], dtype=torch.float64)
    T = torch.eye(4, dtype=torch.float64)
    T[:3, :3] = torch.linalg.matrix_exp(Wm)
    T[:3, 3] = trans_scale * torch.randn(3, generator=gen, dtype=torch.float64)
    return T


gt, pred, errs = [], [], []
for k, (rs, ts) in enumerate([(0.02, 0.05), (0.1, 0.2), (0.5, 1.0), (2.0, 1.0), (0.05, 0.02), (1.0, 3.0)]):
    a = rigid(g, 0.6, 1.0)
    b = rigid(g, rs, ts) @ a
    if k == 3:
        b[:3, 3] = -b[:3, 3]
    gt.append(a); pred.append(b)
    errs.append([float(e) for e in compute_pose_error(a, b)])
out["pose_gt"], out["pose_pred"], out["pose_errors"] = torch.stack(gt).numpy(), torch.stack(pred).numpy(), np.array(errs)
e = np.abs(np.random.default_rng(5).normal(0, 12, size=37))
e[3], e[11] = 5.0, 40.0
out["auc_errors"], out["auc_thresholds"] = e, np.array([5, 10, 20])
out["auc"] = np.array(pose_auc(e, [5, 10, 20]))
print("pose errors", np.array(errs).round(4).tolist(), "auc", out["auc"])
path = ROOT / "tests/golden/pose_eval_ref.npz"
np.savez_compressed(path, **out)
print("bytes", path.stat().st_size)
