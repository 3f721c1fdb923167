"""Generate tests/golden/view_selection.npz: seeded cameras and what the REFERENCE's own functions return for them --
src/geometry/epipolar_lines.py::project_rays on get_world_rays of sample_image_grid (the view overlap),
src/evaluation/evaluation_index_generator.py::EvaluationIndexGenerator (test_step, save_index) and the samplers of
src/dataset/view_sampler/.  Inputs and recorded results only: cameras, integers and two JSON texts.  The tests read the .npz and
nothing else.

    STYL3R_REFERENCE=<reference checkout> python tests/golden/make_view_fixtures.py        (needs einops and tqdm)

Own stubs: jaxtyping, lightning (a LightningModule that is a plain object on the CPU), dacite (from_dict with cast=[tuple] on the one
flat dataclass it is used for), src.global_cfg, src.misc.image_io, src.visualization.* (imported by the generator for its previews,
which are off), and empty `src.*` packages so that no heavy __init__ runs.

The file REFUSES to be written unless
  * every recorded overlap pair has the same count in the reference's fp32 run and in a run of the same functions fed float64 tensors
    (pixel coordinates formed in fp32 first) -- the condition under which the tests may demand integer equality with no tolerance;
  * no overlap the index walk evaluates lies within 1e-3 of min_overlap or max_overlap;
  * the index scenes show what they are there to show (a scene that ends None, one whose first context frame fails, one where the
    frame at max_distance + 1 is among the valid ones).
"""
import importlib
import json
import os
import sys
import tempfile
import types
from pathlib import Path

import numpy as np
import torch

REF = os.environ.get("STYL3R_REFERENCE", "reference")
OUT = Path(__file__).resolve().parent / "view_selection.npz"

SHAPES = [(5, 7), (16, 16), (24, 40), (33, 65), (64, 64)]
INDEX_CFG = dict(num_target_views=3, min_distance=5, max_distance=20, min_overlap=0.6, max_overlap=1.0, save_previews=False, seed=123)
INDEX_SHAPE = (32, 32)


def install():
    sys.path.insert(0, REF)
    jt = types.ModuleType("jaxtyping")

    class _Sub:
        def __class_getitem__(cls, item):
            return cls
    for n in ("Float", "Int64", "Bool", "UInt8", "Shaped", "Int"):
        setattr(jt, n, type(n, (_Sub,), {}))
    sys.modules["jaxtyping"] = jt

    lt = types.ModuleType("lightning")
    lp = types.ModuleType("lightning.pytorch")

    class LightningModule:
        device = torch.device("cpu")

        def __init__(self):
            pass
    lp.LightningModule = LightningModule
    lt.pytorch = lp
    sys.modules["lightning"], sys.modules["lightning.pytorch"] = lt, lp

    dc = types.ModuleType("dacite")
    dc.Config = lambda cast=None: None
    dc.from_dict = lambda data_class, data, config=None: data_class(**{k: tuple(v) if isinstance(v, list) else v for k, v in data.items()})
    sys.modules["dacite"] = dc

    for name in ("src", "src.misc", "src.dataset", "src.dataset.view_sampler", "src.geometry", "src.evaluation", "src.visualization"):
        m = types.ModuleType(name)
        m.__path__ = [REF + "/" + name.replace(".", "/")]
        sys.modules[name] = m
    for name, attrs in (("src.global_cfg", ("get_cfg",)), ("src.misc.image_io", ("save_image",)), ("src.visualization.annotation", ("add_label",)),
                        ("src.visualization.layout", ("add_border", "hcat")), ("src.misc.step_tracker", ("StepTracker",))):
        m = types.ModuleType(name)
        for a in attrs:
            setattr(m, a, type(a, (), {}))
        sys.modules[name] = m
    imp = importlib.import_module
    vs = "src.dataset.view_sampler."
    return (imp("src.geometry.projection"), imp("src.geometry.epipolar_lines"), imp("src.evaluation.evaluation_index_generator"),
            {"bounded": imp(vs + "view_sampler_bounded"), "arbitrary": imp(vs + "view_sampler_arbitrary"),
             "evaluation": imp(vs + "view_sampler_evaluation")})


def rot(axis, angle):
    axis = np.asarray(axis, np.float64)
    x, y, z = axis / np.linalg.norm(axis)
    c, s = np.cos(angle), np.sin(angle)
    return np.array([[c + x * x * (1 - c), x * y * (1 - c) - z * s, x * z * (1 - c) + y * s],
                     [y * x * (1 - c) + z * s, c + y * y * (1 - c), y * z * (1 - c) - x * s],
                     [z * x * (1 - c) - y * s, z * y * (1 - c) + x * s, c + z * z * (1 - c)]])


def track(n, yaw, pitch, roll, step, wobble=0.0, seed=0):
    """n camera-to-world poses, fp32: per-frame yaw / pitch / roll drift (radians) and a translation step, with a seeded wobble"""
    rng = np.random.default_rng(seed)
    E = np.tile(np.eye(4), (n, 1, 1))
    for v in range(n):
        j = rng.normal(size=6) * wobble
        E[v, :3, :3] = rot((0, 1, 0), yaw * v + j[0]) @ rot((1, 0, 0), pitch * v + j[1]) @ rot((0, 0, 1), roll * v + j[2])
        E[v, :3, 3] = np.asarray(step) * v + j[3:] * 0.5
    return torch.from_numpy(E.astype(np.float32))


def carousel(n, turn, radius, wobble=0.0, seed=0):
    """n poses on a circle, looking OUTWARD, `turn` radians apart: two frames half a circle apart stand back to back"""
    E = track(n, turn, 0.0, 0.0, (0.0, 0.0, 0.0), wobble, seed).double().numpy()
    E[:, :3, 3] += radius * E[:, :3, 2]
    return torch.from_numpy(E.astype(np.float32))


def intrinsics(n, fx=0.86, fy=1.27, cx=0.47, cy=0.54):
    K = torch.eye(3).repeat(n, 1, 1)
    K[:, 0, 0], K[:, 1, 1], K[:, 0, 2], K[:, 1, 2] = fx, fy, cx, cy
    return K


def ref_overlap(proj, epi, E, K, pairs, shape, dtype):
    """the reference's two projections per pair, as its index generator calls them -> (counts (P,2) int, means (P,2) fp32)"""
    xy, _ = proj.sample_image_grid(shape)
    xy = xy.reshape(-1, 2).to(dtype)                                   # formed in fp32 first
    E, K = E.to(dtype), K.to(dtype)
    counts, means = [], []
    for a, b in pairs:
        row_c, row_m = [], []
        for s, d in ((a, b), (b, a)):
            o, r = proj.get_world_rays(xy, E[s], K[s])
            hit = epi.project_rays(o, r, E[d], K[d])["overlaps_image"]
            row_c.append(int(hit.sum()))
            row_m.append(hit.float().mean().item())
        counts.append(row_c)
        means.append(row_m)
    return np.array(counts, np.int32), np.array(means, np.float32)


def main():
    proj, epi, evalgen, samplers = install()
    out = {}

    # ---- overlap: tracks whose overlaps span 0 .. 1 ----
    tracks = {"slow": (track(40, 0.012, 0.004, 0.006, (0.03, 0.004, 0.008), 0.004, 1), intrinsics(40)),
              "fast": (track(40, 0.055, -0.02, 0.03, (0.09, -0.02, 0.05), 0.01, 2), intrinsics(40, 1.31, 0.92, 0.55, 0.44))}
    rng = np.random.default_rng(7)
    names, rays, n_pairs, spread = [], 0, 0, []
    for tname, (E, K) in tracks.items():
        out[f"track_{tname}_E"], out[f"track_{tname}_K"] = E.numpy(), K.numpy()
        for H, W in SHAPES:
            pairs = [(0, 1), (3, 8), (20, 39), (39, 0), (10, 30), (17, 5)] + [tuple(int(i) for i in rng.integers(0, 40, 2)) for _ in range(14)]
            pairs = [p for p in pairs if p[0] != p[1]]
            c32, m32 = ref_overlap(proj, epi, E, K, pairs, (H, W), torch.float32)
            c64, _ = ref_overlap(proj, epi, E, K, pairs, (H, W), torch.float64)
            assert np.array_equal(c32, c64), f"{tname} {H}x{W}: a ray flips between fp32 and float64: {c32[c32 != c64]} / {c64[c32 != c64]}"
            key = f"ov_{tname}_{H}x{W}"
            out[key + "_pairs"], out[key + "_counts"], out[key + "_means"] = np.array(pairs, np.int32), c32, m32
            out[key + "_counts_f64"] = c64
            names.append(key)
            rays += 2 * len(pairs) * H * W
            n_pairs += len(pairs)
            spread += [c32.min() / (H * W), c32.max() / (H * W)]
    assert min(spread) < 0.05 and max(spread) > 0.95, spread
    out["overlap_cases"] = np.array(names)
    print(f"overlap: {n_pairs} pairs, {rays} rays, fp32 == float64 on all; overlaps {min(spread):.3f} .. {max(spread):.3f}")

    # ---- degenerate pairs, float64 run only ----
    E = torch.eye(4).repeat(4, 1, 1)
    E[0, :3, 3] = torch.tensor([0.25, -0.5, 1.0])
    E[1, :3, :3] = torch.tensor(np.diag([-1.0, 1.0, -1.0]), dtype=torch.float32)          # half a turn about y ...
    E[1, :3, 3] = torch.tensor([0.25, -0.5, 0.25])                                          # ... 0.75 behind view 0: facing away
    E[2, :3, 3] = torch.tensor([0.25, -0.5, 1.75])                                          # 0.75 along view 0's optical axis
    E[3, :3, :3] = torch.tensor(rot((0.2, 1, 0.1), 0.4), dtype=torch.float32)             # a generic view, for (i, i)
    E[3, :3, 3] = torch.tensor([-0.3, 0.2, 0.6])
    K = intrinsics(4, 0.86, 1.27, 0.5, 0.5)                                                 # centred: the middle ray of an odd image is the axis
    out["deg_E"], out["deg_K"] = E.numpy(), K.numpy()
    pairs = [(0, 0), (3, 3), (0, 1), (0, 2), (3, 0)]
    names = []
    for H, W in ((5, 7), (33, 65), (16, 16)):
        c64, m64 = ref_overlap(proj, epi, E, K, pairs, (H, W), torch.float64)
        key = f"deg_{H}x{W}"
        out[key + "_pairs"], out[key + "_counts"], out[key + "_means"] = np.array(pairs, np.int32), c64, m64
        names.append(key)
        assert c64[0].tolist() == [H * W, H * W] and c64[1].tolist() == [H * W, H * W] and c64[2].tolist() == [0, 0], c64
        if H % 2 and W % 2:
            assert c64[3].tolist() == [H * W - 1, H * W], c64            # the ray through the epipole never enters the frame from behind
    out["degenerate_cases"] = np.array(names)

    # ---- the evaluation index ----
    h, w = INDEX_SHAPE
    lateral = (0.035, 0.0, 0.004)
    scenes = {
        "steady": track(48, 0.01, 0.002, 0.0, lateral, 0.002, 11),                           # overlap holds past max_distance + 1
        "spin": carousel(40, np.pi / 5, 0.3, 0.004, 12),                                    # five frames on it faces the other way: None
        "turning": track(60, 0.034, -0.006, 0.01, (0.05, 0.01, 0.0), 0.004, 13),
        "mixed": torch.cat([carousel(30, np.pi / 5, 0.3, 0.004, 14),           # a wild first half, a calm second one
                            track(30, 0.012, 0.0, 0.004, lateral, 0.002, 15)]),
        "short": track(41, 0.02, 0.004, -0.008, (0.04, -0.005, 0.01), 0.003, 16),
        "drift": track(55, 0.016, 0.01, 0.02, (0.02, 0.02, 0.03), 0.005, 17),
    }
    log = []
    real = evalgen.project_rays

    def spy(*args, **kwargs):
        res = real(*args, **kwargs)
        log[-1][1].append(res["overlaps_image"].float().mean().item())
        return res
    evalgen.project_rays = spy
    with tempfile.TemporaryDirectory() as tmp:
        cfg = evalgen.EvaluationIndexGeneratorCfg(output_path=Path(tmp), **INDEX_CFG)
        gen = evalgen.EvaluationIndexGenerator(cfg)
        for name, E in scenes.items():
            v = E.shape[0]
            K = intrinsics(v)
            out[f"index_{name}_E"], out[f"index_{name}_K"] = E.numpy(), K.numpy()
            log.append((name, []))
            gen.test_step({"target": {"image": torch.zeros(1, v, 3, h, w), "extrinsics": E[None], "intrinsics": K[None]}, "scene": [name]}, 0)
        gen.save_index()
        out["index_json"] = np.array((Path(tmp) / "evaluation_index.json").read_text())
    evalgen.project_rays = real
    entries = {k: None if e is None else {"context": list(e.context), "target": list(e.target), "overlap": e.overlap} for k, e in gen.index.items()}
    out["index_entries"] = np.array(json.dumps(entries))
    out["index_cfg"] = np.array(json.dumps({**INDEX_CFG, "image_shape": list(INDEX_SHAPE)}))
    out["index_scenes"] = np.array(list(scenes))
    evaluated = 0
    for name, means in log:
        both = np.minimum(np.array(means[0::2], np.float32), np.array(means[1::2], np.float32))
        evaluated += len(both)
        for thr in (INDEX_CFG["min_overlap"], INDEX_CFG["max_overlap"]):
            assert not len(both) or np.abs(both.astype(np.float64) - thr).min() > 1e-3, f"{name}: an overlap within 1e-3 of {thr}: {both}"
    assert entries["spin"] is None and sum(e is None for e in entries.values()) == 1, entries
    # the walk of a scene: its evaluated pairs, replayed here from the log, tell which context frames failed
    replay = torch.Generator().manual_seed(INDEX_CFG["seed"])
    first_failed, far_frame = [], []
    for name, means in log:
        v = scenes[name].shape[0]
        order = torch.randperm(v, generator=replay).tolist()
        both = np.minimum(np.array(means[0::2], np.float32), np.array(means[1::2], np.float32)).tolist()
        k, found = 0, False
        for n_ctx, ctx in enumerate(order):
            valid = []
            for step in (1, -1):
                cur = ctx + step * INDEX_CFG["min_distance"]
                while 0 <= cur < v:
                    ov = both[k]
                    k += 1
                    if INDEX_CFG["min_overlap"] <= ov <= INDEX_CFG["max_overlap"]:
                        valid.append(cur)
                    if ov < INDEX_CFG["min_overlap"] or abs(cur - ctx) > INDEX_CFG["max_distance"]:
                        break
                    cur += step
            if valid:
                found = True
                if n_ctx > 0:
                    first_failed.append(name)
                if any(abs(f - ctx) == INDEX_CFG["max_distance"] + 1 for f in valid):
                    far_frame.append(name)
                torch.randint(0, len(valid), size=tuple(), generator=replay)
                while True:
                    e = entries[name]
                    t = torch.randint(e["context"][0], e["context"][1] + 1, (INDEX_CFG["num_target_views"],), generator=replay)
                    if len(set(t.tolist())) == len(t):
                        break
                assert sorted(t.tolist()) == e["target"], (name, t, e)
                break
        assert k == len(both) and found == (entries[name] is not None), (name, k, len(both))
    assert first_failed and far_frame, (first_failed, far_frame)
    print(f"index: {evaluated} evaluated pairs; entries {entries}; first context failed in {first_failed}; frame at max_distance + 1 valid in {far_frame}")

    # ---- the samplers ----
    class Steps:
        def __init__(self, step):
            self.step = step

        def get_step(self):
            return self.step
    re10k = dict(name="bounded", num_context_views=2, num_target_views=4, min_distance_between_context_views=45,
                 max_distance_between_context_views=192, min_distance_to_context_views=0, warm_up_steps=150000,
                 initial_min_distance_between_context_views=25, initial_max_distance_between_context_views=45)
    dl3dv = dict(re10k, min_distance_between_context_views=8, max_distance_between_context_views=22, warm_up_steps=0,
                 initial_min_distance_between_context_views=5, initial_max_distance_between_context_views=7, num_target_views=3)
    cases = []
    for step in (0, 60000, 200000):
        cases.append(dict(kind="bounded", cfg=re10k, stage="train", circular=False, overfit=False, step=step, views=280))
    cases += [dict(kind="bounded", cfg=dl3dv, stage="train", circular=False, overfit=False, step=0, views=60),
              dict(kind="bounded", cfg=re10k, stage="test", circular=False, overfit=False, step=0, views=280),
              dict(kind="bounded", cfg=dl3dv, stage="test", circular=False, overfit=False, step=None, views=60),
              dict(kind="bounded", cfg=dict(dl3dv, min_distance_to_context_views=2), stage="val", circular=False, overfit=False, step=None, views=33),
              dict(kind="bounded", cfg=dl3dv, stage="train", circular=True, overfit=False, step=0, views=30),
              dict(kind="bounded", cfg=dl3dv, stage="train", circular=False, overfit=True, step=0, views=60),
              dict(kind="bounded", cfg=dict(dl3dv, num_context_views=3), stage="train", circular=False, overfit=False, step=0, views=60),
              dict(kind="bounded", cfg=dict(dl3dv, num_context_views=5), stage="train", circular=False, overfit=False, step=0, views=40),
              dict(kind="bounded", cfg=re10k, stage="train", circular=False, overfit=False, step=200000, views=40),        # too few frames
              dict(kind="bounded", cfg=dict(dl3dv, min_distance_to_context_views=12), stage="train", circular=False, overfit=False, step=0, views=60),
              dict(kind="bounded", cfg=dl3dv, stage="train", circular=False, overfit=False, step=0, views=8),             # too few frames
              dict(kind="arbitrary", cfg=dict(name="arbitrary", num_context_views=2, num_target_views=3, context_views=None, target_views=None),
                   stage="train", circular=False, overfit=False, step=None, views=50),
              dict(kind="arbitrary", cfg=dict(name="arbitrary", num_context_views=2, num_target_views=3, context_views=[4, 31], target_views=[9, 10, 22]),
                   stage="test", circular=False, overfit=False, step=None, views=50),
              dict(kind="arbitrary", cfg=dict(name="arbitrary", num_context_views=4, num_target_views=2, context_views=[4, 31], target_views=None),
                   stage="test", circular=False, overfit=False, step=None, views=50)]
    for n_ctx in (2, 3, 4):
        for scene in ("steady", "turning", "spin", "absent"):
            cases.append(dict(kind="evaluation", cfg=dict(name="evaluation", num_context_views=n_ctx), stage="test", circular=False, overfit=False,
                              step=None, views=48, scene=scene))
    with tempfile.TemporaryDirectory() as tmp:
        index_path = Path(tmp) / "evaluation_index.json"
        index_path.write_text(str(out["index_json"]))
        for case in cases:
            mod = samplers[case["kind"]]
            cls = getattr(mod, "ViewSampler" + case["kind"].capitalize())
            cfg_cls = getattr(mod, "ViewSampler" + case["kind"].capitalize() + "Cfg")
            kw = dict(case["cfg"], index_path=index_path) if case["kind"] == "evaluation" else case["cfg"]
            sampler = cls(cfg_cls(**kw), case["stage"], case["overfit"], case["circular"], None if case["step"] is None else Steps(case["step"]))
            E, K = torch.eye(4).repeat(case["views"], 1, 1), torch.eye(3).repeat(case["views"], 1, 1)
            case["draws"] = []
            for seed in (0, 1, 2024):
                torch.manual_seed(seed)
                rec = []
                for _ in range(3):                                        # three samples in a row: the generator moves as recorded
                    try:
                        c, t, o = sampler.sample(case.get("scene", "scene"), E, K)
                        assert c.dtype == torch.int64 and t.dtype == torch.int64 and o.dtype == torch.float32
                        rec.append({"context": c.tolist(), "target": t.tolist(), "overlap": o.tolist()})
                    except ValueError as e:
                        rec.append({"error": str(e)})
                rec.append({"next": int(torch.randint(0, 1 << 30, tuple()))})   # where the global generator stands afterwards
                case["draws"].append({"seed": seed, "samples": rec})
    assert any("error" in s for c in cases for d in c["draws"] for s in d["samples"])
    out["sampler_cases"] = np.array(json.dumps(cases))
    print(f"samplers: {len(cases)} cases")

    np.savez_compressed(OUT, **out)
    print("wrote", OUT, OUT.stat().st_size, "bytes,", len(out), "arrays")


if __name__ == "__main__":
    main()
