"""Generate tests/golden/scene_outputs.npz: seeded inputs and what the REFERENCE's own functions return for them --
camera_trajectory/interpolation.py and wobble.py, layout.py's vcat / hcat with utils.vis_depth_map and the clip / cast / loop of
render_video_generic, and the structured array ply_export.export_ply hands to plyfile.  Inputs and recorded results only; the tests read
the .npz and nothing else (no reference tree, scipy or matplotlib at test time).

    python tests/golden/make_scene_output_fixtures.py        (needs the reference checkout, scipy and matplotlib)

Own stubs (tests/golden/ref_stubs.py is for the model code and stays as it is): jaxtyping, colorspacious (imported by color_map.py,
not called here), plyfile (records the array given to PlyElement.describe), matplotlib.cm.get_cmap where the installed matplotlib
has dropped it, and empty `src.*` packages so that no heavy __init__ runs.
"""
import importlib
import math
import sys
import types
from pathlib import Path

import numpy as np
import torch

REF = "/root/reference"
OUT = Path(__file__).resolve().parent / "scene_outputs.npz"
RECORDED = []


def install():
    sys.path.insert(0, REF)
    jt = types.ModuleType("jaxtyping")

    class _Sub:
        def __class_getitem__(cls, item):
            return cls
    for n in ("Float", "Int64", "Bool", "UInt8", "Shaped", "Int"):
        setattr(jt, n, type(n, (_Sub,), {}))
    sys.modules["jaxtyping"] = jt
    sys.modules["colorspacious"] = types.ModuleType("colorspacious")
    sys.modules["colorspacious"].cspace_convert = None
    pf = types.ModuleType("plyfile")

    class PlyElement:
        @staticmethod
        def describe(elements, name):
            RECORDED.append(np.array(elements))
            return name

    class PlyData:
        def __init__(self, elements):
            pass

        def write(self, path):
            pass
    pf.PlyElement, pf.PlyData = PlyElement, PlyData
    sys.modules["plyfile"] = pf
    import matplotlib
    from matplotlib import cm
    if not hasattr(cm, "get_cmap"):
        cm.get_cmap = lambda name: matplotlib.colormaps[name]
    for name in ("src", "src.misc", "src.model", "src.visualization", "src.visualization.camera_trajectory"):
        m = types.ModuleType(name)
        m.__path__ = [REF + "/" + name.replace(".", "/")]
        sys.modules[name] = m
    imp = importlib.import_module
    return (imp("src.visualization.camera_trajectory.interpolation"), imp("src.visualization.camera_trajectory.wobble"),
            imp("src.visualization.layout"), imp("src.misc.utils"), imp("src.model.ply_export"))


def rot(axis, angle):
    axis = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + math.sin(angle) * K + (1 - math.cos(angle)) * K @ K


def pose(R, o):
    m = np.eye(4)
    m[:3, :3], m[:3, 3] = R, o
    return torch.tensor(m, dtype=torch.float32)


def main():
    interp, wobble, layout, utils, ply = install()
    out = {}
    gen = torch.Generator().manual_seed(20)

    # ---- trajectories ----
    pairs = {
        "generic": (pose(rot((0.2, 1, 0.1), 0.3) @ rot((1, 0, 0), 0.1), (0.1, -0.2, 0.3)),
                    pose(rot((-0.1, 1, 0.3), -0.5) @ rot((0, 0, 1), 0.2), (1.2, 0.1, -0.4))),
        "re10k": (pose(np.eye(3), (0, 0, 0)), pose(np.eye(3), (1, 0, 0))),
        "identical": (pose(rot((0.3, 0.5, 1), 0.7), (0.5, 0.25, -1)), pose(rot((0.3, 0.5, 1), 0.7), (0.5, 0.25, -1))),
        # looks in the XZ plane with a x b = +Y, rolled by +0.1 and -0.1 about their own look axes: twist angles 0.1 and 2 pi - 0.1
        "straddle": (pose(rot((0, 1, 0), -0.25) @ rot((0, 0, 1), 0.1), (-0.6, 0.05, 0.1)),
                     pose(rot((0, 1, 0), 0.2) @ rot((0, 0, 1), -0.1), (0.7, -0.05, 0.0))),
    }
    tau = 2 * math.pi
    a, b = (p.double() for p in pairs["straddle"])
    la, lb = a[:3, 2], b[:3, 2]
    frame = interp.generate_rotation_coordinate_frame(la, lb)
    pivot = interp.intersect_rays(a[:3, 3], la, b[:3, 3], lb)
    pa = interp.extrinsics_to_pivot_parameters(a, frame, pivot)
    pb = interp.extrinsics_to_pivot_parameters(b, frame, pivot)
    assert max(abs(float(pa[i] % tau) - float(pb[i] % tau)) for i in (3, 4)) > math.pi, "the straddle pair must cross 0 / 2 pi"
    times = {"f60": torch.linspace(0, 1, 60), "f2": torch.linspace(0, 1, 2), "f1": torch.linspace(0, 1, 1)}
    times["f60s"] = (torch.cos(torch.pi * (times["f60"] + 1)) + 1) / 2
    times["exag"] = torch.linspace(0, 1, 30) * 5 - 2
    for name, (pa_, pb_) in pairs.items():
        out[f"traj_{name}_a"], out[f"traj_{name}_b"] = pa_.numpy(), pb_.numpy()
        for tn, t in times.items():
            if name != "generic" and tn in ("f2", "f1"):
                continue
            out[f"traj_{name}_{tn}_ref"] = interp.interpolate_extrinsics(pa_, pb_, t).numpy()
    for tn, t in times.items():
        out[f"traj_t_{tn}"] = t.numpy()
    Ka = torch.tensor([[0.9, 0, 0.5], [0, 1.1, 0.5], [0, 0, 1]])
    Kb = torch.tensor([[0.7, 0, 0.45], [0, 0.8, 0.55], [0, 0, 1]])
    out["traj_Ka"], out["traj_Kb"] = Ka.numpy(), Kb.numpy()
    out["traj_K_f60s_ref"] = interp.interpolate_intrinsics(Ka, Kb, times["f60s"]).numpy()
    out["traj_K_exag_ref"] = interp.interpolate_intrinsics(Ka, Kb, times["exag"]).numpy()
    radius = torch.tensor(0.3)
    out["wobble_radius"] = radius.numpy()
    out["wobble_scaled_ref"] = wobble.generate_wobble(pairs["generic"][0], radius, times["f60s"]).numpy()
    out["wobble_tf_unscaled_ref"] = wobble.generate_wobble_transformation(radius, times["f60s"], 1, False).numpy()
    out["wobble_tf_scaled_ref"] = wobble.generate_wobble_transformation(radius, times["f60s"], 1, True).numpy()

    # ---- frames ----
    F, H, W = 4, 5, 6
    rgb = [torch.rand(F, 3, H, W, generator=gen) * 1.4 - 0.2 for _ in range(2)]
    rgb[0][0, 0, 0, 0], rgb[0][1, 1, 2, 3], rgb[1][2, 2, 4, 5] = 1.0, 1.0, 1.0
    depth = torch.rand(F, H, W, generator=gen) * 4 + 0.5
    depth[1, 2, 3] = 0.0
    out["frames_rgb0"], out["frames_rgb1"], out["frames_depth"] = rgb[0].numpy(), rgb[1].numpy(), depth.numpy()
    zero = torch.zeros(F, H, W)
    # the reference evaluates the colour index in float32; in float64 it must land on the same node for (nearly) every pixel, or the
    # comparison of a second float32 evaluation with it would be a comparison of rounding
    far, near = depth.view(-1).quantile(0.99).log(), depth[depth > 0].quantile(0.01).log()
    i32 = ((1 - (depth.log() - near) / (far - near)).clip(0, 1) * 256).long().clamp(max=255)
    d64 = depth.double()
    i64 = ((1 - (d64.log() - near.double()) / (far.double() - near.double())).clip(0, 1) * 256).long().clamp(max=255)
    assert (i32 != i64).float().mean() <= 0.01 and (i32 - i64).abs().max() <= 1, "depth fixture sits on colour-node boundaries"

    def video(kinds, axis, gap, frames, dsrc):
        dcol = utils.vis_depth_map(dsrc[:frames]) if "d" in kinds else None
        cat = layout.vcat if axis == 0 else layout.hcat
        images = []
        for f in range(frames):
            parts = [dcol[f] if k == "d" else rgb[int(k)][f] for k in kinds]
            images.append(cat(*parts, gap=gap))
        v = (torch.stack(images).clip(min=0, max=1) * 255).type(torch.uint8).numpy()
        return np.concatenate([v, v[::-1][1:-1]], axis=0)

    cases = []
    for kinds in ("0", "0d", "d01"):
        for axis in (0, 1):
            for gap in (0, 8):
                cases.append((kinds, axis, gap, 3, "depth"))
    cases += [("0d", 0, 8, f, "depth") for f in (1, 2, 4)] + [("d0", 1, 8, 3, "zero")]
    for kinds, axis, gap, frames, dname in cases:
        out[f"frames_{kinds}_a{axis}_g{gap}_f{frames}_{dname}_ref"] = video(kinds, axis, gap, frames, depth if dname == "depth" else zero)
    out["frames_cases"] = np.array(["|".join(map(str, c)) for c in cases])

    # ---- PLY ----
    G = 64
    for d_sh in (1, 4, 25):
        means = torch.randn(G, 3, generator=gen) * torch.tensor([2.0, 0.5, 1.0]) + torch.tensor([0.3, -1.0, 4.0])
        scales = torch.rand(G, 3, generator=gen) * 0.2 + 1e-3
        rots = torch.randn(G, 4, generator=gen)
        rots[:4] = torch.tensor([[0.0, 0, 0, 1], [1, 0, 0, 0], [0, -1, 0, 0.2], [0.1, 0.2, -0.9, -0.3]])
        sh = torch.randn(G, 3, d_sh, generator=gen)
        opac = torch.rand(G, generator=gen)
        for k, v in (("means", means), ("scales", scales), ("rotations", rots), ("harmonics", sh), ("opacities", opac)):
            out[f"ply_d{d_sh}_{k}"] = v.numpy()
        for dc in (0, 1):
            for shift in (0, 1):
                RECORDED.clear()
                _export(ply, means, scales, rots, sh, opac, shift, dc)
                arr = RECORDED[-1]
                out[f"ply_d{d_sh}_dc{dc}_shift{shift}_ref"] = np.stack([arr[n] for n in arr.dtype.names], axis=1).astype(np.float32)
                out[f"ply_d{d_sh}_dc{dc}_names"] = np.array(arr.dtype.names)
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, OUT.stat().st_size, "bytes,", len(out), "arrays")


def _export(ply, means, scales, rots, sh, opac, shift, dc):
    import tempfile
    with tempfile.TemporaryDirectory() as d:     # (export_ply creates the parent directory; the stubbed writer writes nothing)
        ply.export_ply(means, scales, rots, sh, opac, Path(d) / "x" / "g.ply", shift_and_scale=bool(shift), save_sh_dc_only=bool(dc))


if __name__ == "__main__":
    main()
