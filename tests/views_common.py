"""What tests/test_views_host.py and tests/test_gpu_views.py share: the loaded fixture tests/golden/view_selection.npz, its case lists, and
the two checks both files run -- one on CPU tensors, the other with the cameras on the device."""
import json
from pathlib import Path

import numpy as np
import torch

from styl3r_amd import views as vw

ROOT = Path(__file__).resolve().parent.parent
G = np.load(ROOT / "tests/golden/view_selection.npz")
T = lambda k: torch.from_numpy(G[k])
OVERLAP_CASES = [str(k) for k in G["overlap_cases"]]
DEGENERATE_CASES = [str(k) for k in G["degenerate_cases"]]
INDEX_SCENES = [str(k) for k in G["index_scenes"]]
INDEX_CFG = json.loads(str(G["index_cfg"]))
INDEX_ENTRIES = json.loads(str(G["index_entries"]))
SAMPLER_CASES = json.loads(str(G["sampler_cases"]))


def overlap_case(key):
    """-> (extrinsics, intrinsics, pairs, (H, W)) of an overlap or a degenerate fixture case"""
    kind, rest = key.split("_", 1)
    H, W = (int(s) for s in key.rsplit("_", 1)[1].split("x"))
    if kind == "deg":
        return T("deg_E"), T("deg_K"), T(key + "_pairs"), (H, W)
    track = rest.split("_")[0]
    return T(f"track_{track}_E"), T(f"track_{track}_K"), T(key + "_pairs"), (H, W)


def check_overlap_case(key, device=None):
    E, K, pairs, shape = overlap_case(key)
    if device is not None:
        E, K = E.to(device), K.to(device)
    counts, overlap = vw.view_overlap(E, K, pairs, shape)
    assert counts.device == E.device and counts.dtype == torch.int32 and overlap.dtype == torch.float32
    got, want = counts.cpu().numpy(), G[key + "_counts"]
    if key + "_counts_f64" in G:
        assert np.array_equal(want, G[key + "_counts_f64"]), key          # the reference's fp32 and float64 runs: the no-tolerance condition
    assert np.array_equal(got, want), f"{key}: counts differ at pairs {pairs[(got != want).any(1)].tolist()}: {got[got != want]} against {want[got != want]}"
    assert np.array_equal(overlap.cpu().numpy().view(np.int32), G[key + "_means"].view(np.int32)), key


def index_generator():
    cfg = {k: v for k, v in INDEX_CFG.items() if k != "image_shape"}
    return vw.EvaluationIndexGenerator(vw.EvaluationIndexGeneratorCfg(output_path=Path("unused"), **cfg))


def check_index(device=None):
    gen = index_generator()
    for name in INDEX_SCENES:
        E, K = T(f"index_{name}_E"), T(f"index_{name}_K")
        if device is not None:
            E, K = E.to(device), K.to(device)
        entry = gen.add_scene(name, E, K, INDEX_CFG["image_shape"])
        want = INDEX_ENTRIES[name]
        if want is None:
            assert entry is None and gen.index[name] is None, name
        else:
            assert entry == vw.IndexEntry(tuple(want["context"]), tuple(want["target"]), want["overlap"]), (name, entry, want)
    return gen
