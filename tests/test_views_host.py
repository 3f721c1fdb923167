"""CPU: styl3r_amd/views.py on CPU tensors -- the float64 restatement of the view overlap, the evaluation-index generator and the view
samplers -- against what the reference's own functions returned for the same cameras and seeds (tests/golden/view_selection.npz,
written by tests/golden/make_view_fixtures.py), `inputs.example_from_scene`, and the C ABI of csrc/gsr_views.hip as far as it goes
without a device.  Counts are compared as integers and overlaps bit for bit: the generator refuses to write a pair on which the
reference's fp32 and float64 runs disagree by a ray, so there is no tolerance in this file.  This path is the yardstick of
tests/test_gpu_views.py."""
import ctypes as C
import json
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from styl3r_amd import _lib
from styl3r_amd import inputs as si
from styl3r_amd import views as vw

from tests.views_common import (DEGENERATE_CASES, G, INDEX_CFG, INDEX_ENTRIES, INDEX_SCENES, OVERLAP_CASES, ROOT, SAMPLER_CASES, T, check_index,
                                check_overlap_case, index_generator, overlap_case)


@pytest.mark.parametrize("key", OVERLAP_CASES + DEGENERATE_CASES)
def test_host_overlap_equals_the_reference_counts_and_mean_bits(key):
    check_overlap_case(key)


def test_overlap_fixture_spans_zero_to_one_and_its_own_conditions():
    lo, hi = 1.0, 0.0
    for key in OVERLAP_CASES:
        m = G[key + "_means"]
        lo, hi = min(lo, float(m.min())), max(hi, float(m.max()))
    assert lo < 0.05 and hi > 0.95
    assert sum(e is None for e in INDEX_ENTRIES.values()) == 1
    assert any(e and e["context"][1] - e["context"][0] == INDEX_CFG["max_distance"] + 1 for e in INDEX_ENTRIES.values())


def test_view_overlap_checks_its_arguments_on_the_host():
    E, K = T("deg_E"), T("deg_K")
    with pytest.raises(IndexError):
        vw.view_overlap(E, K, [(0, 4)], (5, 7))
    with pytest.raises(IndexError):
        vw.view_overlap(E, K, [(-1, 0)], (5, 7))
    with pytest.raises(ValueError):
        vw.view_overlap(E, K, [(0.0, 1.0)], (5, 7))
    with pytest.raises(ValueError):
        vw.view_overlap(E, K, [(0, 1, 2)], (5, 7))
    with pytest.raises(ValueError):
        vw.view_overlap(E, K, [(0, 1)], (4097, 4096))
    with pytest.raises(ValueError):
        vw.view_overlap(E, K[:3], [(0, 1)], (5, 7))


def test_host_overlap_is_the_same_in_slices():
    """the restatement cuts directions and rays into slices of _CHUNK_RAYS: any cut gives the same counts"""
    E, K, pairs, shape = overlap_case("ov_fast_24x40")
    whole = vw.overlap_counts_torch(E, K, pairs, shape)
    keep = vw._CHUNK_RAYS
    try:
        for chunk in (1 << 8, 24 * 40 * 3 + 1):
            vw._CHUNK_RAYS = chunk
            assert torch.equal(vw.overlap_counts_torch(E, K, pairs, shape), whole), chunk
    finally:
        vw._CHUNK_RAYS = keep


def test_index_generator_reproduces_the_recorded_entries_and_json(tmp_path):
    gen = check_index()
    assert list(gen.index) == INDEX_SCENES
    want = json.loads(str(G["index_json"]))
    path = gen.save_index(tmp_path / "out" / "evaluation_index.json")
    assert json.loads(path.read_text()) == want
    gen.cfg.output_path = tmp_path / "by_cfg"
    assert gen.save_index() == tmp_path / "by_cfg" / "evaluation_index.json" and json.loads((tmp_path / "by_cfg" / "evaluation_index.json").read_text()) == want
    back = vw.load_index(path)
    assert back == gen.index and isinstance(back["steady"].context, tuple) and back["spin"] is None
    assert gen.load_index(path) == back


def test_index_walk_candidates_include_the_frame_past_max_distance():
    gen = index_generator()
    fwd, bwd = gen.candidates(30, 60)
    assert fwd == list(range(35, 52)) and bwd == list(range(25, 8, -1))              # distance 5 .. 21 = max_distance + 1
    assert gen.candidates(3, 40) == [list(range(8, 25)), []] and gen.candidates(2, 6) == [[], []]
    with pytest.raises(NotImplementedError):
        vw.EvaluationIndexGenerator(vw.EvaluationIndexGeneratorCfg(3, 5, 20, 0.6, 1.0, Path("x"), True, 0))


def test_add_scene_refuses_more_distinct_targets_than_frames_between_the_pair():
    """where the reference would draw targets forever: at most 22 frames lie between a pair 21 apart"""
    cfg = {k: v for k, v in INDEX_CFG.items() if k != "image_shape"}
    gen = vw.EvaluationIndexGenerator(vw.EvaluationIndexGeneratorCfg(output_path=Path("unused"), **{**cfg, "num_target_views": 23}))
    with pytest.raises(ValueError, match="distinct targets do not fit"):
        gen.add_scene("steady", T("index_steady_E"), T("index_steady_K"), INDEX_CFG["image_shape"])


def build_sampler(case, index_path):
    cfg_cls = {"bounded": vw.ViewSamplerBoundedCfg, "arbitrary": vw.ViewSamplerArbitraryCfg, "evaluation": vw.ViewSamplerEvaluationCfg}[case["kind"]]
    kw = dict(case["cfg"], index_path=index_path) if case["kind"] == "evaluation" else case["cfg"]
    tracker = None if case["step"] is None else vw.StepTracker(case["step"])
    sampler = vw.get_view_sampler(cfg_cls(**kw), case["stage"], case["overfit"], case["circular"], tracker)
    assert type(sampler).__name__ == "ViewSampler" + case["kind"].capitalize()
    return sampler


@pytest.fixture(scope="module")
def index_path(tmp_path_factory):
    path = tmp_path_factory.mktemp("index") / "evaluation_index.json"
    path.write_text(str(G["index_json"]))
    return path


@pytest.mark.parametrize("n", range(len(SAMPLER_CASES)))
def test_samplers_reproduce_every_recorded_draw_and_error(n, index_path):
    case = SAMPLER_CASES[n]
    sampler = build_sampler(case, index_path)
    E, K = torch.eye(4).repeat(case["views"], 1, 1), torch.eye(3).repeat(case["views"], 1, 1)
    state = torch.get_rng_state()
    try:
        for draw in case["draws"]:
            torch.manual_seed(draw["seed"])
            for want in draw["samples"]:
                if "next" in want:
                    assert int(torch.randint(0, 1 << 30, tuple())) == want["next"], (case, draw["seed"])       # the generator stands where the reference's does
                elif "error" in want:
                    with pytest.raises(ValueError, match=re.escape(want["error"])):
                        sampler.sample(case.get("scene", "scene"), E, K)
                else:
                    c, t, o = sampler.sample(case.get("scene", "scene"), E, K)
                    assert c.dtype == torch.int64 and t.dtype == torch.int64 and o.dtype == torch.float32
                    assert (c.tolist(), t.tolist(), o.tolist()) == (want["context"], want["target"], want["overlap"]), (case, draw["seed"])
    finally:
        torch.set_rng_state(state)


def test_sampler_fixture_covers_what_it_should():
    errors = {s["error"] for c in SAMPLER_CASES for d in c["draws"] for s in d["samples"] if "error" in s}
    assert "Example does not have enough frames!" in errors and any(e.startswith("No indices available") for e in errors)
    kinds = {(c["kind"], c["stage"], c["circular"], c["overfit"], c["cfg"]["num_context_views"]) for c in SAMPLER_CASES}
    assert {k[0] for k in kinds} == {"bounded", "arbitrary", "evaluation"} and {k[1] for k in kinds} >= {"train", "test"}
    assert any(k[2] for k in kinds) and any(k[3] for k in kinds) and any(k[4] >= 3 for k in kinds)


def test_all_sampler_and_additional_context_views():
    E, K = torch.eye(4).repeat(7, 1, 1), torch.eye(3).repeat(7, 1, 1)
    sampler = vw.get_view_sampler(vw.ViewSamplerAllCfg("all"), "test", False, False, None)
    c, t, o = sampler.sample("s", E, K)
    assert c.tolist() == t.tolist() == list(range(7)) and o.tolist() == [0.5] and sampler.num_context_views == sampler.num_target_views == 0
    assert vw.add_additional_context_index(torch.tensor([4, 31]), 4).tolist() == [4, 13, 22, 31]
    assert vw.add_additional_context_index(torch.tensor([10, 13]), 3).tolist() == [10, 11, 13]


def _scene(n=12, hw=(20, 24)):
    g = torch.Generator().manual_seed(5)
    frames = torch.randint(0, 256, (n, *hw, 3), generator=g, dtype=torch.uint8)
    E = torch.eye(4).repeat(n, 1, 1)
    E[:, 0, 3] = torch.arange(n) * 0.1
    K = torch.eye(3).repeat(n, 1, 1)
    K[:, 0, 0], K[:, 1, 1], K[:, 0, 2], K[:, 1, 2] = 0.9, 1.1, 0.5, 0.5
    return frames, K, E


def test_example_from_scene_samples_then_prepares_and_skips_short_scenes():
    frames, K, E = _scene()
    cfg = si.InputCfg(input_image_shape=(16, 16), augment=False)
    bounded = vw.ViewSamplerBoundedCfg("bounded", 2, 3, 4, 8, 1, 0, 4, 8)
    sampler = vw.get_view_sampler(bounded, "train", False, False, None)
    state = torch.get_rng_state()
    try:
        torch.manual_seed(3)
        ci, ti, _ = sampler.sample("room", E, K)
        want = si.prepare_example(frames, K, E, ci, ti, None, cfg, stage="train", scene="room")
        torch.manual_seed(3)
        got = si.example_from_scene(frames, K, E, sampler, "room", None, cfg, stage="train")
    finally:
        torch.set_rng_state(state)
    assert got["scene"] == "room" and got["context"]["index"].tolist() == ci.tolist() and got["target"]["index"].tolist() == ti.tolist()
    for part in ("context", "target"):
        for k, v in want[part].items():
            assert torch.equal(got[part][k], v), (part, k)
    with pytest.raises(si.SkipExample, match="does not have enough frames"):
        si.example_from_scene(frames[:4], K[:4], E[:4], sampler, "room", None, cfg, stage="train")


def test_example_from_scene_skips_scenes_the_evaluation_index_lacks(index_path):
    frames, K, E = _scene(48)
    sampler = vw.get_view_sampler(vw.ViewSamplerEvaluationCfg("evaluation", index_path, 2), "test", False, False, None)
    cfg = si.InputCfg(input_image_shape=(16, 16), augment=False)
    ex = si.example_from_scene(frames, K, E, sampler, "steady", None, cfg, stage="test")
    assert ex["context"]["index"].tolist() == INDEX_ENTRIES["steady"]["context"] and ex["target"]["index"].tolist() == INDEX_ENTRIES["steady"]["target"]
    for scene in ("spin", "absent"):
        with pytest.raises(si.SkipExample, match="No indices available"):
            si.example_from_scene(frames, K, E, sampler, scene, None, cfg, stage="test")


def test_view_symbols_and_argument_checks_without_a_device():
    _lib.build_library()
    lib = _lib.load()
    header = (ROOT / "include/gsr.h").read_text()
    for name in ("gsr_view_overlap_scratch_bytes", "gsr_view_overlap"):
        assert name in _lib.EXPORTS and re.search(rf"\b{name}\s*\(", header) and hasattr(lib, name), name
    assert "gsr_views.hip" in _lib._SOURCES
    assert lib.gsr_view_overlap_scratch_bytes(3, 5) >= 3 * 50 * 8
    assert lib.gsr_view_overlap_scratch_bytes(0, 5) == 0 and lib.gsr_view_overlap_scratch_bytes(3, 0) == 0
    one = C.c_void_p(64)                                           # (any aligned non-null value: validation only, nothing is dereferenced)
    ok = dict(E=one, K=one, V=2, pairs=one, P=3, H=4, W=5, scratch=one, nbytes=1 << 20, counts=one)
    call = lambda **kw: (lambda a: lib.gsr_view_overlap(a["E"], a["K"], a["V"], a["pairs"], a["P"], a["H"], a["W"], a["scratch"], a["nbytes"],
                                                        a["counts"], None))({**ok, **kw})
    for bad in (dict(E=None), dict(K=None), dict(pairs=None), dict(scratch=None), dict(counts=None), dict(V=0), dict(V=-1), dict(P=0), dict(P=-5),
                dict(H=0), dict(W=0), dict(H=-3), dict(H=4097, W=4096), dict(H=1 << 20, W=1 << 20)):
        assert call(**bad) == -1, bad                              # GSR_EINVAL before any launch
    assert call(nbytes=2 * 50 * 8 - 1) == -2                       # GSR_ENOSPACE
    # the bound on P that keeps the launch inside the grid limits: 2^22 pairs pass the checks, one more does not
    assert call(P=(1 << 22) + 1) == -1 and lib.gsr_view_overlap_scratch_bytes(3, (1 << 22) + 1) == 0
    assert lib.gsr_view_overlap_scratch_bytes(3, 1 << 22) == lib.gsr_view_overlap_scratch_bytes(3, 5) > 0
    assert call(P=1 << 22, nbytes=8) == -2                         # (past the argument checks, stopped by the scratch size: nothing launched)
