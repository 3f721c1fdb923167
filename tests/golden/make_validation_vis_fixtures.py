"""Generate tests/golden/validation_vis.npz: seeded drawing, camera, projection and layout cases and what the REFERENCE's own functions
return for them -- src/visualization/drawing/{lines,points,cameras}.py, validation_in_3d.py and layout.py.  Inputs and recorded results
only; the tests read the .npz and nothing else.

    python tests/golden/make_validation_vis_fixtures.py        (from the repository root; needs einops and, for the label case, PIL)

THE GOLDEN DATA IS THE REFERENCE RUN IN FLOAT64.  In fp32 a sub-sample on a primitive's edge can fall on either side, so the fp32 run is not
reproducible sample for sample by another summation order; the float64 run is.  Starts from `ref_stubs.install()`, registers the
`src.visualization` / `src.visualization.drawing` package shims here, widens the reference's `sanitize_*` by assignment (they would round every
argument to fp32), stubs `add_label` (the labels are tested on their own) and replaces `render_cuda_orthographic` with a recorder of its
arguments (no CUDA rasterizer is needed), compares `pil_labeler` with the reference's draw_label where PIL is present (nothing of it is stored); the float64 camera runs also set torch's default dtype to float64, for the corner grid that
unproject_frustum_corners makes itself.  Inputs are stored as the fp32 values that were widened.

Per drawing case the file holds the float64 picture, the float64 alpha of every layer (`render`'s fourth channel) and how far the fp32
reference is from the float64 one: the number of pixels that differ by more than 1e-6 (flips) and the maximum difference.

The file REFUSES to be written unless
  * the package's host restatement (styl3r_amd.visualization.draw_layers_reference, float64 unrounded) equals the reference's float64 run in
    every pixel of every case, and so does the alpha of every layer;
  * every drawing case has partial-alpha pixels;
  * the file is under 1 MB and no image is larger than 64 x 64.
"""
import importlib
import json
import sys
import types
from pathlib import Path

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
sys.path.insert(0, str(HERE.parent.parent))
OUT = HERE / "validation_vis.npz"

import ref_stubs  # noqa: E402


def install():
    ref_stubs.install()
    REF = ref_stubs.REF
    for name in ("src.visualization", "src.visualization.drawing"):
        m = types.ModuleType(name)
        m.__path__ = [REF + "/" + name.replace(".", "/")]
        sys.modules[name] = m
    ann = types.ModuleType("src.visualization.annotation")
    ann.add_label = lambda image, label, *a, **k: image
    sys.modules["src.visualization.annotation"] = ann
    calls = []
    cs = types.ModuleType("src.model.decoder.cuda_splatting")

    def render_cuda_orthographic(extrinsics, width, height, near, far, image_shape, background_color, means, covariances, harmonics, opacities,
                                 fov_degrees=0.1):
        calls.append(dict(extrinsics=extrinsics.clone(), width=width.clone(), height=height.clone(), near=near.clone(), far=far.clone(),
                          image_shape=tuple(image_shape), background_color=background_color.clone(), fov_degrees=fov_degrees))
        b = extrinsics.shape[0]
        return torch.full((b, 3, *image_shape), 0.5) * (len(calls) % 3 + 1) / 4
    cs.render_cuda_orthographic = render_cuda_orthographic
    sys.modules["src.model.decoder.cuda_splatting"] = cs
    ty = types.ModuleType("src.model.types")
    ty.Gaussians = types.SimpleNamespace
    sys.modules["src.model.types"] = ty
    imp = importlib.import_module
    mods = types.SimpleNamespace(types=imp("src.visualization.drawing.types"), conv=imp("src.visualization.drawing.coordinate_conversion"),
                                 rendering=imp("src.visualization.drawing.rendering"), lines=imp("src.visualization.drawing.lines"),
                                 points=imp("src.visualization.drawing.points"), cameras=imp("src.visualization.drawing.cameras"),
                                 layout=imp("src.visualization.layout"), v3d=imp("src.visualization.validation_in_3d"), ortho_calls=calls)
    mods.narrow = {n: getattr(mods.types, n) for n in ("sanitize_vector", "sanitize_scalar", "sanitize_pair")}
    return mods


def widened(narrow):
    """float64 stand-ins for the reference's sanitize_* (same shape rules, no rounding to fp32)"""
    def tensor(value):
        return value.double() if isinstance(value, torch.Tensor) else torch.tensor(value, dtype=torch.float64)

    def sanitize_vector(vector, dim, device):
        vector = tensor(vector)
        while vector.ndim < 2:
            vector = vector[None]
        if vector.shape[-1] == 1:
            vector = vector.expand(*vector.shape[:-1], dim)
        assert vector.ndim == 2 and vector.shape[-1] == dim
        return vector

    def sanitize_scalar(scalar, device):
        scalar = tensor(scalar)
        while scalar.ndim < 1:
            scalar = scalar[None]
        assert scalar.ndim == 1
        return scalar

    def sanitize_pair(pair, device):
        pair = tensor(pair)
        assert pair.shape == (2,)
        return pair
    return dict(sanitize_vector=sanitize_vector, sanitize_scalar=sanitize_scalar, sanitize_pair=sanitize_pair)


def set_sanitize(mods, fns):
    for mod in (mods.types, mods.conv, mods.lines, mods.points, mods.cameras):
        for n, fn in fns.items():
            if hasattr(mod, n):
                setattr(mod, n, fn)


class AlphaSpy:
    """records the alpha channel of every `render` (one per draw call) while it is installed"""

    def __init__(self, mods):
        self.mods, self.alphas = mods, []

    def __enter__(self):
        real = self.real = self.mods.rendering.render_over_image
        render = self.mods.rendering.render

        def spy(image, color_function, device, subdivision=8, num_passes=1):
            self.alphas.append(render(image.shape[1:], color_function, device, subdivision=subdivision, num_passes=num_passes)[3].clone())
            return real(image, color_function, device, subdivision=subdivision, num_passes=num_passes)
        self.mods.lines.render_over_image = self.mods.points.render_over_image = spy
        return self

    def __exit__(self, *exc):
        self.mods.lines.render_over_image = self.mods.points.render_over_image = self.real


def f32(x):
    return torch.as_tensor(np.asarray(x, dtype=np.float32))


def drawing_cases():
    """name -> (kind, image shape, [draw calls]); a draw call = dict of fp32 arrays / scalars, the reference's keyword names"""
    rng = np.random.default_rng(20)
    cases = {}
    xr, yr = (-1.5, 2.25), (0.5, 3.0)

    def world(n):
        return np.stack([rng.uniform(xr[0] - 0.3, xr[1] + 0.3, n), rng.uniform(yr[0] - 0.2, yr[1] + 0.2, n)], 1).astype(np.float32)
    s9, e9, c9, w9 = world(9), world(9), rng.uniform(0, 1, (9, 3)).astype(np.float32), rng.uniform(0.6, 5.0, 9).astype(np.float32)
    for cap in ("butt", "round", "square"):
        for passes in (0, 1):
            cases[f"lines_{cap}_p{passes}"] = ("lines", (37, 53), [dict(start=s9, end=e9, color=c9, width=w9, cap=cap, num_msaa_passes=passes,
                                                                     x_range=list(xr), y_range=list(yr))])
    cases["line_single_p2"] = ("lines", (16, 16), [dict(start=[2.25, 3.5], end=[13.0, 11.75], color=[1.0, 0.5, 0.25], width=3, num_msaa_passes=2)])
    cases["line_single"] = ("lines", (16, 16), [dict(start=[2.25, 3.5], end=[13.0, 11.75], color=[1.0, 0.5, 0.25], width=3)])
    # 40 x 24: a degenerate line (round caps only), a sub-pixel line that covers no centre (vanishes), two adjacent lines of one colour
    # (no edge between them), crossing colours (the highest index wins), ends outside the image
    s = np.array([[5.0, 5.0], [10.25, 2.0], [3.0, 12.0], [3.0, 14.0], [20.0, 3.0], [20.0, 20.0], [-6.0, 10.0], [30.0, -4.0]], np.float32)
    e = np.array([[5.0, 5.0], [30.25, 2.3], [16.0, 12.0], [16.0, 14.0], [36.0, 21.0], [37.0, 4.0], [8.0, 30.0], [47.0, 19.0]], np.float32)
    c = np.array([[1, 0, 0], [0, 1, 0], [0.5, 0.5, 1], [0.5, 0.5, 1], [1, 1, 0], [0, 1, 1], [1, 0, 1], [0.25, 0.25, 0.25]], np.float32)
    w = np.array([6.0, 0.3, 2.0, 2.0, 3.0, 3.0, 2.5, 4.0], np.float32)
    for cap in ("round", "butt"):
        cases[f"lines_special_{cap}"] = ("lines", (24, 40), [dict(start=s, end=e, color=c, width=w, cap=cap)])
    s70, e70 = rng.uniform(-4, 44, (70, 2)).astype(np.float32), rng.uniform(-4, 28, (70, 2)).astype(np.float32)
    cases["lines_70"] = ("lines", (24, 40), [dict(start=s70, end=e70[:, ::-1].copy() * np.float32(1.5), color=rng.uniform(0, 1, (70, 3)).astype(np.float32),
                                                  width=1.5, cap="square")])
    cases["lines_broadcast"] = ("lines", (20, 28), [dict(start=[4.0, 4.0], end=rng.uniform(0, 28, (5, 2)).astype(np.float32), color=0.75, width=[1.0, 2.0, 3.0, 2.0, 1.0])])
    p = rng.uniform(-2, 34, (12, 2)).astype(np.float32)
    cases["points_annuli"] = ("points", (30, 33), [dict(points=p, color=rng.uniform(0, 1, (12, 3)).astype(np.float32),
                                                         radius=rng.uniform(1.5, 6, 12).astype(np.float32), inner_radius=rng.uniform(0, 1.5, 12).astype(np.float32))])
    cases["points_defaults"] = ("points", (17, 19), [dict(points=[[3.0, 3.0], [9.5, 8.25], [18.5, 16.0]])])
    cases["points_ranges_p0"] = ("points", (21, 35), [dict(points=world(6), color=[0.25, 1.0, 0.5], radius=2.5, inner_radius=[1.0], num_msaa_passes=0,
                                                           x_range=list(xr), y_range=list(yr))])
    # layers on one image: points over lines over a non-black image
    cases["stacked"] = ("mixed", (32, 32), [dict(fn="lines", start=world(4), end=world(4), color=[0.0, 0.5, 1.0], width=2, x_range=list(xr), y_range=list(yr)),
                                            dict(fn="points", points=rng.uniform(0, 32, (5, 2)).astype(np.float32), color=[1.0, 1.0, 0.0], radius=3, inner_radius=1.5)])
    return cases


def background(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand((3, *shape), generator=g)


def to_args(call):
    return {k: (f32(v) if isinstance(v, np.ndarray) else v) for k, v in call.items() if k != "fn"}


def run_reference(mods, kind, image, calls, dtype):
    with AlphaSpy(mods) as spy:
        for call in calls:
            fn = {"lines": mods.lines.draw_lines, "points": mods.points.draw_points}[call.get("fn", kind)]
            args = {k: (v.to(dtype) if isinstance(v, torch.Tensor) else v) for k, v in to_args(call).items()}
            image = fn(image, **args)
    return image, spy.alphas


def run_package(vis, kind, image, calls):
    layers = []
    for call in calls:
        make = {"lines": vis.line_layer, "points": vis.point_layer}[call.get("fn", kind)]
        layers.append(make(image.shape[1:], **to_args(call)))
    final = vis.draw_layers_reference(image[None], [layers], dtype=torch.float64)[0]
    return final, [vis.render_overlay(image.shape[1:], layer, image.device)[3] for layer in layers]


def cameras(n, seed):
    rng = np.random.default_rng(seed)
    E = np.tile(np.eye(4), (n, 1, 1))
    for v in range(n):
        a, b = rng.normal(size=2) * 0.4
        ry = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
        rx = np.array([[1, 0, 0], [0, np.cos(b), -np.sin(b)], [0, np.sin(b), np.cos(b)]])
        E[v, :3, :3] = ry @ rx
        E[v, :3, 3] = rng.normal(size=3) * 0.5 + [0.4 * v, 0, 0]
    K = np.tile(np.eye(3), (n, 1, 1))
    K[:, 0, 0], K[:, 1, 1] = rng.uniform(0.8, 1.3, n), rng.uniform(0.8, 1.3, n)
    K[:, 0, 2], K[:, 1, 2] = rng.uniform(0.45, 0.55, n), rng.uniform(0.45, 0.55, n)
    return f32(E), f32(K)


def main():
    mods = install()
    import styl3r_amd.visualization as vis
    out, summary = {}, {}
    wide = widened(mods.narrow)

    # ---- draw_lines / draw_points ----
    names, recursive = [], []                                             # (recursive: two MSAA passes, the restatement's own path)
    for seed, (name, (kind, shape, calls)) in enumerate(drawing_cases().items()):
        assert max(shape) <= 64
        image = background(shape, seed) if name in ("stacked", "lines_round_p1", "points_annuli") else torch.zeros((3, *shape))
        set_sanitize(mods, wide)
        gold, alphas = run_reference(mods, kind, image.double(), calls, torch.float64)
        set_sanitize(mods, mods.narrow)
        ref32, _ = run_reference(mods, kind, image, calls, torch.float32)
        mine, mine_alphas = run_package(vis, kind, image, calls)
        passes = [c.get("num_msaa_passes", 1) for c in calls]
        assert gold.dtype == torch.float64 and mine.dtype == torch.float64
        assert torch.equal(mine, gold), f"{name}: the host restatement differs from the reference's float64 run by {(mine - gold).abs().max().item()}"
        for a, b in zip(alphas, mine_alphas):
            assert torch.equal(a, b), f"{name}: alpha differs"
            assert torch.equal(a * 64 ** max(passes), (a * 64 ** max(passes)).round())
        partial = sum(int(((a > 0) & (a < 1)).sum()) for a in alphas)
        assert partial > 0 or max(passes) == 0, f"{name}: no partial-alpha pixel"
        diff = (ref32.double() - gold).abs()
        out[f"draw_{name}_image"] = image.numpy()
        out[f"draw_{name}_gold"] = gold.numpy()
        out[f"draw_{name}_alpha"] = torch.stack(alphas).numpy()
        out[f"draw_{name}_fp32_distance"] = np.array([float((diff > 1e-6).any(dim=0).sum()), diff.max().item()])
        out[f"draw_{name}_calls"] = np.array(json.dumps([{k: (v.tolist() if isinstance(v, np.ndarray) else v) for k, v in c.items()} for c in calls]))
        out[f"draw_{name}_kind"] = np.array(kind)
        (names if max(passes) <= 1 else recursive).append(name)
        summary[name] = dict(partial=partial, fp32_flips=int((diff > 1e-6).any(dim=0).sum()), fp32_max=diff.max().item())
    out["draw_cases"] = np.array(names)
    out["draw_cases_recursive"] = np.array(recursive)

    # ---- draw_cameras / render_cameras: 2 + 1 cameras at 48^2 ----
    E, K = cameras(3, 5)
    near, far = f32([0.6, 0.7, 0.65]), f32([2.0, 2.4, 2.2])
    color = f32([[1, 1, 1], [1, 1, 1], [1, 0, 0]])
    out.update(cam_E=E.numpy(), cam_K=K.numpy(), cam_near=near.numpy(), cam_far=far.numpy(), cam_color=color.numpy())
    cam_cases = {"nearfar": dict(near=near, far=far), "plain": dict(), "near_only": dict(near=near), "margin": dict(near=f32([0.5]), far=far, margin=0.25, frustum_scale=0.1)}
    for name, kw in cam_cases.items():
        kw64 = {k: (v.double() if isinstance(v, torch.Tensor) else v) for k, v in kw.items()}
        set_sanitize(mods, wide)
        torch.set_default_dtype(torch.float64)                             # (unproject_frustum_corners' own linspace: float64 too)
        with AlphaSpy(mods) as spy:
            gold = mods.cameras.draw_cameras(48, E.double(), K.double(), color.double(), **kw64)
        torch.set_default_dtype(torch.float32)
        set_sanitize(mods, mods.narrow)
        ref32 = mods.cameras.draw_cameras(48, E, K, color, **kw)
        stacks = vis.camera_layers(48, E, K, color, **kw)
        mine = vis.draw_layers_reference(torch.zeros(3, 3, 48, 48), stacks, dtype=torch.float64)
        assert gold.dtype == torch.float64 and torch.equal(mine, gold), f"cameras {name}: {(mine - gold).abs().max().item()}"
        mine_alpha = [vis.render_overlay((48, 48), layer, "cpu")[3] for stack in stacks for layer in stack]
        assert len(mine_alpha) == len(spy.alphas) and all(torch.equal(a, b) for a, b in zip(mine_alpha, spy.alphas))
        assert any(((a > 0) & (a < 1)).any() for a in spy.alphas)
        diff = (ref32.double() - gold).abs()
        out[f"cam_{name}_gold"] = gold.numpy()
        out[f"cam_{name}_alpha"] = torch.stack(spy.alphas).numpy()
        out[f"cam_{name}_fp32_distance"] = np.array([float((diff > 1e-6).any(dim=1).sum()), diff.max().item()])
        out[f"cam_{name}_kwargs"] = np.array(json.dumps({k: (v.tolist() if isinstance(v, torch.Tensor) else v) for k, v in kw.items()}))
        summary["cam_" + name] = dict(fp32_flips=int((diff > 1e-6).any(dim=1).sum()), fp32_max=diff.max().item())
    out["cam_cases"] = np.array(list(cam_cases))
    batch = {"context": dict(extrinsics=E[None, :2], intrinsics=K[None, :2], near=near[None, :2], far=far[None, :2]),
             "target": dict(extrinsics=E[None, 2:], intrinsics=K[None, 2:], near=near[None, 2:], far=far[None, 2:])}
    set_sanitize(mods, wide)
    wide_batch = {k: {n: t.double() for n, t in v.items()} for k, v in batch.items()}
    torch.set_default_dtype(torch.float64)
    gold = mods.v3d.render_cameras(wide_batch, 48)
    torch.set_default_dtype(torch.float32)
    set_sanitize(mods, mods.narrow)
    assert torch.equal(gold, torch.from_numpy(out["cam_nearfar_gold"])), "render_cameras is draw_cameras of the concatenated views, white / red"

    # ---- render_projections: the arguments render_cuda_orthographic receives, and the padded stack ----
    g = torch.Generator().manual_seed(9)
    means = torch.randn((2, 64, 3), generator=g) * torch.tensor([1.0, 0.4, 2.0]) + torch.tensor([0.3, -0.2, 1.5])
    gaussians = types.SimpleNamespace(means=means, covariances=torch.zeros(2, 64, 3, 3), harmonics=torch.zeros(2, 64, 3, 1), opacities=torch.ones(2, 64))
    del mods.ortho_calls[:]
    stack = mods.v3d.render_projections(gaussians, 32, margin=0.1, draw_label=False)
    assert len(mods.ortho_calls) == 3 and stack.shape == (2, 3, 3, 32, 32)
    out["proj_means"] = means.numpy()
    for i, call in enumerate(mods.ortho_calls):
        assert call["fov_degrees"] == 10.0 and call["image_shape"] == (32, 32) and not call["background_color"].any()
        for k in ("extrinsics", "width", "height", "near", "far"):
            out[f"proj_{i}_{k}"] = call[k].numpy()
    out["proj_stack_shape"] = np.array(stack.shape)
    ragged = [torch.rand((2, 3, 5, 7), generator=g), torch.rand((2, 3, 9, 4), generator=g), torch.rand((1, 3, 6, 6), generator=g)]
    for i, (x, y) in enumerate(zip(ragged, mods.v3d.pad(ragged))):
        out[f"pad_in_{i}"], out[f"pad_out_{i}"] = x.numpy(), y.numpy()

    # ---- labels: nothing recorded (PIL's default font differs between PIL versions); compared here, where both run ----
    try:
        import importlib.util
        import PIL  # noqa: F401
        spec = importlib.util.spec_from_file_location("src.visualization.annotation_real", ref_stubs.REF + "/src/visualization/annotation.py")
        real = importlib.util.module_from_spec(spec)
        real.__package__ = "src.visualization"
        spec.loader.exec_module(real)
        for text in ("XY Projection", "Target (Ground Truth)", "2D Baseline"):
            want = real.draw_label(text, Path("assets/Inter-Regular.otf"), 24)
            assert torch.equal(vis.pil_labeler(Path("assets/Inter-Regular.otf"), 24)(text), want), f"pil_labeler differs from draw_label on {text!r}"
        print("labels: pil_labeler equals the reference's draw_label on 3 texts")
    except ImportError:
        print("labels: PIL is missing, not compared")

    # ---- layout ----
    L = mods.layout
    imgs = [torch.rand((3, 5, 9), generator=g), torch.rand((3, 8, 4), generator=g), torch.rand((3, 6, 6), generator=g)]
    for i, x in enumerate(imgs):
        out[f"layout_in_{i}"] = x.numpy()
    layout_cases = []
    for axis, fn, aligns in (("h", L.hcat, ("start", "center", "end", "top", "bottom")), ("v", L.vcat, ("start", "center", "end", "left", "right"))):
        for align in aligns:
            for gap, gap_color in ((0, 1), (8, 1), (3, [0.25, 0.5, 0.75])):
                key = f"layout_{axis}cat_{align}_{gap}_{'grey' if gap_color == 1 else 'rgb'}"
                out[key] = fn(*imgs, align=align, gap=gap, gap_color=gap_color).numpy()
                layout_cases.append(dict(key=key, fn=axis + "cat", align=align, gap=gap, gap_color=gap_color))
    for main in ("horizontal", "vertical"):
        for align in ("start", "center", "end"):
            key = f"layout_cat_{main}_{align}"
            out[key] = L.cat(main, *imgs, align=align).numpy()
            layout_cases.append(dict(key=key, fn="cat", main_axis=main, align=align))
            for cross in ("start", "center", "end"):
                key = f"layout_overlay_{main}_{align}_{cross}"
                out[key] = L.overlay(torch.zeros(3, 11, 13), imgs[0], main, align, cross).numpy()
                layout_cases.append(dict(key=key, fn="overlay", main_axis=main, main_align=align, cross_align=cross))
    for border, color in ((8, 1), (2, [0.1, 0.2, 0.3]), (0, 0.5)):
        key = f"layout_border_{border}"
        out[key] = L.add_border(imgs[1], border, color).numpy()
        layout_cases.append(dict(key=key, fn="add_border", border=border, color=color))
    out["layout_cases"] = np.array(json.dumps(layout_cases))

    np.savez_compressed(OUT, **out)
    size = OUT.stat().st_size
    assert size < 1_000_000, size
    print(json.dumps(summary, indent=1))
    print("wrote", OUT, size, "bytes,", len(out), "arrays")


if __name__ == "__main__":
    main()
