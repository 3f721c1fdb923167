"""Generate tests/golden/dataset_tiny/: a tiny synthetic dataset tree in the layout the REFERENCE's DatasetRE10kStyle reads, and the
sequence of examples that class yields from it -- src/dataset/dataset_re10k_style.py::DatasetRE10kStyle.__iter__ with the bounded view
sampler, stage "train", torch.manual_seed(0) and (1).  Data only: two `.torch` chunks (three scenes each, 64 x 36 JPEG frames and
18-float camera rows), index.json, two style pictures with their mapping, and expected.json with (scene, context indices, target
indices, flip) per yielded example plus where the global generator stands afterwards.  The tests read the tree and nothing else.

    STYL3R_REFERENCE=<reference checkout> python tests/golden/make_dataset_fixtures.py        (needs einops and Pillow)

Own stubs: jaxtyping, torchvision.transforms (ToTensor: uint8 HWC -> float CHW / 255; CenterCrop; both restated), cv2 (imported by src/misc/cam_utils.py,
not used on this path), src.misc.step_tracker, and empty `src.*` packages so that no heavy __init__ runs.  The flip of an example is
observed by a wrapper around the module's apply_augmentation_shim (it returns the example itself when it does not flip).

The scenes show what they are there to show: "short" has too few frames for the sampler, "wide" fails the field-of-view gate, "still"
fails the baseline gate (all cameras in one place), so the recorded sequence skips all three -- and the generator draws the skipped
examples' samples all the same.
"""
import importlib
import json
import os
import sys
import types
from io import BytesIO
from pathlib import Path

import numpy as np
import torch
from PIL import Image

REF = os.environ.get("STYL3R_REFERENCE", "reference")
OUT = Path(__file__).resolve().parent / "dataset_tiny"
W, H = 64, 36
SAMPLER = dict(name="bounded", num_context_views=2, num_target_views=2, min_distance_between_context_views=3,
               max_distance_between_context_views=8, min_distance_to_context_views=0, warm_up_steps=0,
               initial_min_distance_between_context_views=3, initial_max_distance_between_context_views=8)
CFG = dict(name="re10k_style", baseline_min=1e-3, baseline_max=1e10, max_fov=100.0, make_baseline_1=True, augment=True, relative_pose=True,
           skip_bad_shape=True, specified_style_image_path=None, original_image_shape=[H, W], input_image_shape=[32, 32],
           background_color=[0.0, 0.0, 0.0], cameras_are_circular=False, overfit_to_scene=None)


def install():
    sys.path.insert(0, REF)
    jt = types.ModuleType("jaxtyping")

    class _Sub:
        def __class_getitem__(cls, item):
            return cls
    for n in ("Float", "Int64", "Bool", "UInt8", "Shaped", "Int"):
        setattr(jt, n, type(n, (_Sub,), {}))
    sys.modules["jaxtyping"] = jt
    tv, tf = types.ModuleType("torchvision"), types.ModuleType("torchvision.transforms")

    class ToTensor:
        def __call__(self, img):
            a = np.asarray(img)
            a = a[..., None] if a.ndim == 2 else a
            return torch.from_numpy(a.copy()).permute(2, 0, 1).float().div(255)

    class CenterCrop:
        def __init__(self, size):
            self.size = size

        def __call__(self, img):
            h, w = img.shape[-2:]
            top, left = int(round((h - self.size) / 2.0)), int(round((w - self.size) / 2.0))
            return img[..., top:top + self.size, left:left + self.size]
    tf.ToTensor, tf.CenterCrop = ToTensor, CenterCrop
    tf.RandomCrop = lambda size: None             # constructed by the reference, never called
    tv.transforms = tf
    sys.modules["torchvision"], sys.modules["torchvision.transforms"] = tv, tf
    try:
        import cv2  # noqa: F401
    except ImportError:
        sys.modules["cv2"] = types.ModuleType("cv2")
    for name in ("src", "src.misc", "src.dataset", "src.dataset.shims", "src.dataset.view_sampler", "src.geometry"):
        m = types.ModuleType(name)
        m.__path__ = [REF + "/" + name.replace(".", "/")]
        sys.modules[name] = m
    st = types.ModuleType("src.misc.step_tracker")
    st.StepTracker = type("StepTracker", (), {})
    sys.modules["src.misc.step_tracker"] = st
    sys.modules["src.dataset.view_sampler"].ViewSampler = importlib.import_module("src.dataset.view_sampler.view_sampler").ViewSampler
    sys.modules["src.dataset.view_sampler"].ViewSamplerCfg = None
    return (importlib.import_module("src.dataset.dataset_re10k_style"), importlib.import_module("src.dataset.view_sampler.view_sampler_bounded"))


def frame(rng, t, phase):
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    img = np.stack([128 + 90 * np.sin(0.11 * x + 0.07 * y + phase + 0.3 * t + c) for c in range(3)], -1) + rng.normal(0, 3, (H, W, 3))
    return np.clip(img, 0, 255).astype(np.uint8)


def scene(rng, key, n, fx=0.9, step=0.08, phase=0.0, sampling=2):
    images, cams = [], []
    for t in range(n):
        buf = BytesIO()
        Image.fromarray(frame(rng, t, phase)).save(buf, "JPEG", quality=85, subsampling=sampling)
        images.append(torch.from_numpy(np.frombuffer(buf.getvalue(), np.uint8).copy()))
        a = 0.02 * t
        w2c = np.array([[np.cos(a), 0, np.sin(a), -step * t], [0, 1, 0, 0.01 * t * (step > 0)], [-np.sin(a), 0, np.cos(a), 0.02 * t * (step > 0)]])
        cams.append(np.concatenate([[fx, fx * W / H, 0.5, 0.5, 0, 0], w2c.reshape(-1)]))
    return {"key": key, "url": "", "timestamps": torch.arange(n, dtype=torch.int64), "cameras": torch.tensor(np.array(cams), dtype=torch.float32),
            "images": images}


def main():
    ds_mod, vs_mod = install()
    rng = np.random.default_rng(5)
    root = OUT / "re10k"
    (root / "train").mkdir(parents=True, exist_ok=True)
    (OUT / "style" / "train").mkdir(parents=True, exist_ok=True)
    chunks = {"000000.torch": [scene(rng, "a0", 12, phase=0.0), scene(rng, "short", 3, phase=1.0), scene(rng, "a2", 12, phase=2.0, sampling=0)],
              "000001.torch": [scene(rng, "b0", 12, phase=3.0, sampling=1), scene(rng, "wide", 12, fx=0.3, phase=4.0),
                               scene(rng, "still", 12, step=0.0, phase=5.0)]}
    index, mapping = {}, {}
    for name, items in chunks.items():
        torch.save(items, root / "train" / name)
        for k, it in enumerate(items):
            index[it["key"]] = name
            mapping[it["key"]] = f"style_{(len(mapping)) % 2}.png"
    (root / "train" / "index.json").write_text(json.dumps(index, indent=1))
    (OUT / "style" / "train" / "scene_style_mapping_all.json").write_text(json.dumps(mapping, indent=1))
    for k, (sw, sh) in enumerate(((300, 272), (264, 290))):
        y, x = np.mgrid[0:sh, 0:sw].astype(np.float64)
        img = np.stack([128 + 100 * np.sin(0.03 * x * (c + 1) + 0.02 * y + k) for c in range(3)], -1)
        Image.fromarray(np.clip(img, 0, 255).astype(np.uint8)).save(OUT / "style" / "train" / f"style_{k}.png", optimize=True)

    cfg = ds_mod.DatasetRE10kStyleCfg(roots=[root], style_root=OUT / "style", view_sampler=None, **CFG)
    sampler = vs_mod.ViewSamplerBounded(vs_mod.ViewSamplerBoundedCfg(**SAMPLER), "train", False, False, None)
    flips = []
    real = ds_mod.apply_augmentation_shim

    def spy(example, *a, **k):
        res = real(example, *a, **k)
        flips.append(res is not example)
        return res
    ds_mod.apply_augmentation_shim = spy
    runs = []
    for seed in (0, 1):
        torch.manual_seed(seed)
        del flips[:]
        rec = []
        for ex in ds_mod.DatasetRE10kStyle(cfg, "train", sampler):
            rec.append({"scene": ex["scene"], "context": ex["context"]["index"].tolist(), "target": ex["target"]["index"].tolist(),
                        "flip": bool(flips[-1])})
        runs.append({"seed": seed, "examples": rec, "next": int(torch.randint(0, 1 << 30, tuple()))})
        assert {r["scene"] for r in rec} == {"a0", "a2", "b0"}, rec
    assert any(r["flip"] for run in runs for r in run["examples"]) and not all(r["flip"] for run in runs for r in run["examples"])
    (OUT / "expected.json").write_text(json.dumps({"cfg": CFG, "sampler": SAMPLER, "stage": "train", "runs": runs}, indent=1))
    size = sum(p.stat().st_size for p in OUT.rglob("*") if p.is_file())
    print("wrote", OUT, size, "bytes;", runs)


if __name__ == "__main__":
    main()
