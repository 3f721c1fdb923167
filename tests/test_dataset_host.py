"""styl3r_amd.dataset on the CPU: read_chunk, ChunkDataset and iter_batches over the tiny dataset tree of tests/golden/dataset_tiny/
(written by tests/golden/make_dataset_fixtures.py, which also recorded what the reference's DatasetRE10kStyle yields from it for
seeds 0 and 1).  Needs the library (entropy stage, axis plans), no GPU."""
import json
import shutil
from io import BytesIO
from pathlib import Path

import numpy as np
import pytest
import torch

from styl3r_amd import dataset as ds
from styl3r_amd import inputs as si
from styl3r_amd import views

TINY = Path(__file__).resolve().parent / "golden" / "dataset_tiny"
EXPECTED = json.loads((TINY / "expected.json").read_text())


def make_cfg(root=TINY / "re10k", **over):
    kw = {k: v for k, v in EXPECTED["cfg"].items()}
    kw.update(over)
    return ds.DatasetRE10kStyleCfg(roots=[root], style_root=TINY / "style", **kw)


def make_dataset(cfg=None, device=None):
    sampler = views.ViewSamplerBounded(views.ViewSamplerBoundedCfg(**EXPECTED["sampler"]), "train", False, False, None)
    return ds.ChunkDataset(cfg or make_cfg(), EXPECTED["stage"], sampler, device=device)


def same_tree(a, b, path=""):
    """two example / batch dicts: same keys, tensors equal bit for bit, everything else equal"""
    assert type(a) is type(b), path
    if isinstance(a, dict):
        assert a.keys() == b.keys(), path
        for k in a:
            same_tree(a[k], b[k], f"{path}/{k}")
    elif isinstance(a, torch.Tensor):
        assert a.dtype == b.dtype and a.shape == b.shape, path
        a, b = a.cpu().contiguous(), b.cpu().contiguous()
        assert torch.equal(a.view(torch.uint8) if a.dtype != torch.int64 else a, b.view(torch.uint8) if b.dtype != torch.int64 else b), path
    else:
        assert a == b, path


def pil_frames(example, indices):
    from PIL import Image
    return torch.from_numpy(np.stack([np.asarray(Image.open(BytesIO(example["images"][i].numpy().tobytes())).convert("RGB")) for i in indices]))


def test_read_chunk():
    chunk = ds.read_chunk(TINY / "re10k" / "train" / "000000.torch")
    assert [x["key"] for x in chunk] == ["a0", "short", "a2"]
    assert chunk[0]["cameras"].shape == (12, 18) and chunk[0]["cameras"].dtype == torch.float32
    assert len(chunk[0]["images"]) == 12 and chunk[0]["images"][0].dtype == torch.uint8 and chunk[0]["images"][0].dim() == 1
    assert len(chunk[1]["images"]) == 3


@pytest.mark.parametrize("run", EXPECTED["runs"], ids=lambda r: f"seed{r['seed']}")
def test_chunk_dataset_visits_what_the_reference_visits(run):
    """scenes, context / target indices and flips of the reference's DatasetRE10kStyle for the same seed, the skipped scenes skipped, and
    the global generator left where the reference leaves it"""
    torch.manual_seed(run["seed"])
    dataset = make_dataset()
    got, examples = [], []
    for p in dataset.pending():
        got.append({"scene": p.scene, "context": p.context.tolist(), "target": p.target.tolist(), "flip": p.flip})
        examples.append(dataset.finish(p))
    assert got == run["examples"]
    assert int(torch.randint(0, 1 << 30, tuple())) == run["next"]
    for ex, want in zip(examples, run["examples"]):
        assert ex["scene"] == want["scene"] and ex["context"]["index"].tolist() == want["context"] and ex["target"]["index"].tolist() == want["target"]
        assert ex["context"]["image"].shape == (2, 3, 32, 32) and ex["style"]["image"].shape == (3, 256, 256)


def test_examples_equal_prepare_example_on_pillow_frames():
    """the whole example -- images, cameras, style -- bit for bit what `prepare_example` gives for ALL frames of the scene decoded by
    Pillow (the default, index-selecting path), which also shows preselected=True against the default path"""
    torch.manual_seed(0)
    dataset = make_dataset()
    chunks = {x["key"]: x for name in ("000000.torch", "000001.torch") for x in ds.read_chunk(TINY / "re10k" / "train" / name)}
    before = dict(ds.CALLS)
    n = 0
    for p in dataset.pending():
        ex = dataset.finish(p)
        raw = chunks[p.scene]
        frames = pil_frames(raw, range(len(raw["images"])))
        E, K = si.convert_poses(raw["cameras"])
        want = si.prepare_example(frames, K, E, p.context, p.target, dataset.read_style_image(p.scene), dataset.cfg.input_cfg(0.1, 100.0),
                                  stage="train", flip=p.flip, scene=p.scene)
        same_tree(ex, want)
        n += 1
    assert n == 3 and ds.CALLS["jpeg_fallback"] == before["jpeg_fallback"] and ds.CALLS["jpeg_host"] == before["jpeg_host"] + 4 * n


def test_preselected_equals_the_default_path_and_checks_the_count():
    raw = ds.read_chunk(TINY / "re10k" / "train" / "000001.torch")[0]
    frames = pil_frames(raw, range(12))
    E, K = si.convert_poses(raw["cameras"])
    cfg = make_cfg().input_cfg(0.1, 100.0)
    ci, ti = [2, 9], [3, 3, 7]
    for flip in (False, True):
        want = si.prepare_example(frames, K, E, ci, ti, None, cfg, stage="train", flip=flip, scene="b0")
        got = si.prepare_example(frames[ci + ti], K, E, ci, ti, None, cfg, stage="train", flip=flip, scene="b0", preselected=True)
        same_tree(got, want)
    with pytest.raises(ValueError):
        si.prepare_example(frames, K, E, ci, ti, None, cfg, stage="train", flip=False, preselected=True)


@pytest.mark.parametrize("batch_size", [1, 2])
def test_iter_batches_prefetch_gives_the_inline_batches(batch_size):
    batches = {}
    for prefetch in (0, 1, 2):
        torch.manual_seed(1)
        batches[prefetch] = list(ds.iter_batches(make_dataset(), batch_size, prefetch=prefetch))
    assert len(batches[0]) == (3 + batch_size - 1) // batch_size
    assert batches[0][0]["context"]["image"].shape == (batch_size, 2, 3, 32, 32) and len(batches[0][0]["scene"]) == batch_size
    for prefetch in (1, 2):
        assert len(batches[prefetch]) == len(batches[0])
        for a, b in zip(batches[prefetch], batches[0]):
            same_tree(a, b)
    with pytest.raises(ValueError):
        next(ds.iter_batches(make_dataset(), 0))


def test_iter_batches_hands_over_the_producers_exception():
    class Boom(ds.ChunkDataset):
        def pending(self):
            yield from list(super().pending())[:1]
            raise RuntimeError("boom")
    sampler = views.ViewSamplerBounded(views.ViewSamplerBoundedCfg(**EXPECTED["sampler"]), "train", False, False, None)
    torch.manual_seed(0)
    it = ds.iter_batches(Boom(make_cfg(), "train", sampler), 1, prefetch=1)
    next(it)
    with pytest.raises(RuntimeError, match="boom"):
        next(it)


def test_a_corrupt_frame_skips_its_example_only(tmp_path):
    """frame 9 of scene b0 truncated: seed 0 picks it for its last example (context [4, 9]) and loses that example alone, as the
    reference's loader does on Pillow's OSError; the two examples in front of it are the recorded ones"""
    root = tmp_path / "re10k"
    shutil.copytree(TINY / "re10k", root)
    chunk = ds.read_chunk(root / "train" / "000001.torch")
    assert chunk[0]["key"] == "b0"
    blob = chunk[0]["images"][9]
    chunk[0]["images"][9] = blob[:int(len(blob) * 0.6)].clone()
    torch.save(chunk, root / "train" / "000001.torch")
    run = EXPECTED["runs"][0]
    assert run["examples"][-1]["scene"] == "b0" and 9 in run["examples"][-1]["context"]
    torch.manual_seed(0)
    got = [(ex["scene"], ex["context"]["index"].tolist(), ex["target"]["index"].tolist()) for ex in make_dataset(make_cfg(root))]
    assert got == [(r["scene"], r["context"], r["target"]) for r in run["examples"][:-1]]
    with pytest.raises(OSError):
        ds.decode_jpeg([chunk[0]["images"][9]])


def test_bad_shape_and_missing_style_entries():
    torch.manual_seed(0)
    assert list(make_dataset(make_cfg(original_image_shape=[36, 48]))) == []                     # every picture has the wrong shape
    torch.manual_seed(0)
    assert len(list(make_dataset(make_cfg(original_image_shape=[36, 48], skip_bad_shape=False)))) == 3
    dataset = make_dataset()
    with pytest.raises(KeyError):
        dataset.read_style_image("nowhere")
    with pytest.raises(FileNotFoundError):
        make_dataset(make_cfg(specified_style_image_path=TINY / "style" / "train" / "absent.png")).read_style_image("a0")
    one = make_dataset(make_cfg(specified_style_image_path=TINY / "style" / "train" / "style_1.png"))
    assert torch.equal(one.read_style_image("a0"), one.read_style_image("b0"))
