"""Validation visuals on the host (styl3r_amd/visualization.py): the float64 restatement of the reference's drawing -- the yardstick of
tests/test_gpu_vis.py -- the camera and projection geometry, the layout functions and the panel geometry of `validation_images`, against
tests/golden/validation_vis.npz (the reference run in float64; tolerances: tests/vis_common.py)."""
import json
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from styl3r_amd import visualization as vis
from tests.vis_common import CAM_CASES, DRAW_CASES, T, TOL, camera_inputs, check_camera_case, check_draw_case, draw_case, golden32, max_diff

CPU = torch.device("cpu")


@pytest.mark.parametrize("name", DRAW_CASES)
def test_draw_layers_on_the_host_matches_the_reference_in_float64(name):
    check_draw_case(name, CPU)


@pytest.mark.parametrize("name", [n for n in DRAW_CASES if n != "stacked"])
def test_draw_lines_and_draw_points_take_the_references_arguments(name):
    """the public one-call functions, with the scalar / list / (n,) / (n,d) arguments as the fixture recorded them"""
    kind, image, calls = draw_case(name)
    fn = {"lines": vis.draw_lines, "points": vis.draw_points}[kind]
    got = fn(image, **calls[0])
    assert got.shape == image.shape and got.dtype == torch.float32
    assert max_diff(got, golden32(f"draw_{name}_gold")) <= TOL


def test_the_fixture_holds_what_the_tests_rely_on():
    caps = {json.loads(str(T[f"draw_{n}_calls"]))[0].get("cap", "round") for n in DRAW_CASES}
    assert caps == {"butt", "round", "square"}
    for name in DRAW_CASES:
        alpha = T[f"draw_{name}_alpha"]
        passes = [c.get("num_msaa_passes", 1) for c in json.loads(str(T[f"draw_{name}_calls"]))]
        assert np.array_equal(alpha * 64, np.round(alpha * 64))
        assert (((alpha > 0) & (alpha < 1)).any()) == (max(passes) > 0), name          # partial alpha wherever MSAA ran, none without
        assert max(T[f"draw_{name}_gold"].shape[1:]) <= 64 and T[f"draw_{name}_gold"].dtype == np.float64
        flips, worst = T[f"draw_{name}_fp32_distance"]                                # how far the fp32 reference is from the golden run:
        assert flips == 0 and 0 <= worst < 1e-6, name                                 # no sub-sample flipped in these cases, rounding only
    for name in CAM_CASES:
        flips, worst = T[f"cam_{name}_fp32_distance"]
        assert flips == 0 and 0 <= worst < 1e-6, name
        alpha = T[f"cam_{name}_alpha"]
        assert ((alpha > 0) & (alpha < 1)).any()
    assert any(h != w for h, w in (T[f"draw_{n}_gold"].shape[1:] for n in DRAW_CASES))


def test_special_lines_behave_as_the_reference_says():
    """lines_special: [0] degenerate (round caps only), [1] thinner than a pixel and covering no centre (never drawn), [2] and [3] adjacent
    and of one colour (no edge between them), [4] and [5] crossing (the higher index on top)"""
    _, image, calls = draw_case("lines_special_round")
    call = calls[0]
    layer = vis.line_layer(image.shape[1:], **call)
    assert np.isnan(layer.records[0, 6:8]).all() and layer.records[2, 1] == layer.records[3, 1] == 2        # NaN direction; one colour class
    rgba = vis.render_overlay(image.shape[1:], layer, CPU)
    assert torch.equal(rgba[:3, 5, 5].float(), call["color"][0]) and rgba[3, 5, 5] == 1                    # the degenerate line's disc
    butt = vis.render_overlay(image.shape[1:], vis.line_layer(image.shape[1:], **{**call, "cap": "butt"}), CPU)
    assert butt[3, 5, 5] == 0                                                                               # ... and nothing without caps
    green = (rgba[0] == 0) & (rgba[1] == 1) & (rgba[2] == 0) & (rgba[3] > 0)
    assert not green.any()                                                                                  # the sub-pixel line vanished
    assert (rgba[3, 12:15, 5:15] == 1).all()                                                                # the seam of [2] | [3]: no edge
    only = lambda i: vis.render_overlay(image.shape[1:], vis.line_layer(image.shape[1:], call["start"][i], call["end"][i], call["color"][i],
                                                                          call["width"][i], num_msaa_passes=0), CPU)[3] > 0
    both = only(4) & only(5)
    assert both.any() and all(torch.equal(rgba[:3, y, x].float(), call["color"][5]) for y, x in both.nonzero().tolist()
                              if rgba[3, y, x] == 1 and not vis.detect_msaa_pixels(rgba[None])[0, y, x])


def test_two_msaa_passes_take_the_recursive_restatement():
    """no caller uses a second pass; it is the reference's recursion (edge SAMPLES subdivided again), restated and held to the same fixture"""
    (name,) = [str(x) for x in T["draw_cases_recursive"]]
    _, image, calls = draw_case(name)
    assert calls[0]["num_msaa_passes"] == 2
    two = vis.draw_lines(image, **calls[0])
    assert max_diff(two, golden32(f"draw_{name}_gold")) <= TOL
    alpha = T[f"draw_{name}_alpha"][0]
    assert np.array_equal(alpha * 4096, np.round(alpha * 4096)) and not np.array_equal(alpha * 64, np.round(alpha * 64))
    assert max_diff(two, vis.draw_lines(image, **{**calls[0], "num_msaa_passes": 1})) > 1e-3


@pytest.mark.parametrize("name", CAM_CASES)
def test_draw_cameras_on_the_host_matches_the_reference_in_float64(name):
    check_camera_case(name, CPU)


def test_render_cameras_draws_context_white_and_target_red():
    E, K, _, near, far = camera_inputs()
    batch = {"context": dict(extrinsics=E[None, :2], intrinsics=K[None, :2], near=near[None, :2], far=far[None, :2]),
             "target": dict(extrinsics=E[None, 2:], intrinsics=K[None, 2:], near=near[None, 2:], far=far[None, 2:])}
    got = vis.render_cameras(batch, 48)
    assert max_diff(got, golden32("cam_nearfar_gold")) <= TOL
    assert ((got[:, 0] == 1) & (got[:, 1] == 0) & (got[:, 2] == 0)).any() and (got == 1).all(dim=1).any()


def test_frustum_corners_and_boxes():
    E, K, _, near, far = camera_inputs()
    corners = vis.unproject_frustum_corners(E, K, near)
    assert corners.shape == (3, 4, 3) and corners.dtype == torch.float64
    cam = torch.einsum("bij,bpj->bpi", E.double()[:, :3, :3].transpose(1, 2), corners - E.double()[:, None, :3, 3])
    assert torch.allclose(cam[..., 2], near.double()[:, None].expand(3, 4), rtol=0, atol=1e-6)             # z-depth, not distance (fp32 rotations: orthonormal to ~2^-23)
    uv = torch.einsum("bij,bpj->bpi", K.double(), cam / cam[..., 2:])[..., :2]
    assert torch.allclose(uv, torch.tensor([[0.0, 0], [1, 0], [1, 1], [0, 1]], dtype=torch.float64).expand(3, 4, 2), atol=1e-6)
    lo, hi = vis.compute_aabb(E, K, near, far)
    assert (lo <= corners.reshape(-1, 3).min(0).values).all() and (hi >= corners.reshape(-1, 3).max(0).values).all()
    lo2, hi2 = vis.compute_equal_aabb_with_margin(lo, hi, margin=0.1)
    assert torch.allclose(hi2 - lo2, ((hi - lo).max() * 1.1).expand(3)) and torch.allclose((lo2 + hi2) / 2, (lo + hi) / 2)


def test_projection_cameras_match_the_arguments_the_reference_hands_its_rasterizer():
    """Every recorded value is at most three fp32 operations (a difference, a product with 1 + margin or 0.5, a sum) away from the minima /
    maxima of the means, each rounding by at most half an ulp of a magnitude no larger than M = max(|coordinate|) + the scene extent.
    The bar is 4 * 2^-24 * M: only rounding differences pass, a wrong margin (10 % of the extent) or axis does not."""
    means = torch.from_numpy(T["proj_means"])
    M = float(means.abs().max() + (means.amax(dim=(0, 1)) - means.amin(dim=(0, 1))).max() * 1.1)
    cams = vis.projection_cameras(means, margin=0.1)
    assert len(cams) == 3
    for i, cam in enumerate(cams):
        for k, got in zip(("extrinsics", "width", "height", "near", "far"), cam):
            want = torch.from_numpy(T[f"proj_{i}_{k}"])
            assert got.shape == want.shape and got.dtype == torch.float32
            assert max_diff(got, want) <= 4 * 2.0 ** -24 * M, (i, k)
    assert tuple(T["proj_stack_shape"]) == (2, 3, 3, 32, 32)


def test_pad_fills_with_ones_to_the_largest_shape():
    ragged = [torch.from_numpy(T[f"pad_in_{i}"]) for i in range(3)]
    for got, i in zip(vis.pad(ragged), range(3)):
        assert torch.equal(got, torch.from_numpy(T[f"pad_out_{i}"]))


def test_layout_functions_match_the_reference_bit_for_bit():
    imgs = [torch.from_numpy(T[f"layout_in_{i}"]) for i in range(3)]
    cases = json.loads(str(T["layout_cases"]))
    assert {c["fn"] for c in cases} == {"hcat", "vcat", "cat", "overlay", "add_border"}
    for c in cases:
        if c["fn"] in ("hcat", "vcat"):
            got = getattr(vis, c["fn"])(*imgs, align=c["align"], gap=c["gap"], gap_color=c["gap_color"])
        elif c["fn"] == "cat":
            got = vis.cat(c["main_axis"], *imgs, align=c["align"])
        elif c["fn"] == "overlay":
            got = vis.overlay(torch.zeros(3, 11, 13), imgs[0], c["main_axis"], c["main_align"], c["cross_align"])
        else:
            got = vis.add_border(imgs[1], c["border"], c["color"])
        assert torch.equal(got, torch.from_numpy(T[c["key"]])), c["key"]


def _stub_labeler(text):
    return torch.full((3, 5, 2 * len(text)), 0.5)


def test_add_label_puts_the_label_above_the_image():
    image = torch.rand(3, 10, 12)
    got = vis.add_label(image, "abcd", _stub_labeler)                       # label 5 x 8, gap 4, image 10 x 12
    assert got.shape == (3, 19, 12)
    assert (got[:, :5, :8] == 0.5).all() and (got[:, :5, 8:] == 1).all() and (got[:, 5:9] == 1).all() and torch.equal(got[:, 9:], image)
    assert vis.add_label(image, "abcd", None) is image
    wide = vis.add_label(image, "abcdefgh", _stub_labeler)                  # label wider than the image: the image is padded on the right
    assert wide.shape == (3, 19, 16) and torch.equal(wide[:, 9:, :12], image) and (wide[:, 9:, 12:] == 1).all()


def test_pil_labeler_draws_black_text_on_white_sized_by_the_font():
    """No bitmap is recorded from the reference: what PIL's default font draws depends on the PIL version.  The fixture generator compares
    `pil_labeler` with the reference's draw_label bit for bit where it runs; here the label's geometry and colours are checked against the
    font's own boxes, with the fallback to the default font that the reference takes (its font file is not in its tree)."""
    pytest.importorskip("PIL")
    import string

    from PIL import ImageFont
    font = ImageFont.load_default()
    labeler = vis.pil_labeler(font="no-such-font.otf")
    box = font.getbbox(string.digits + string.punctuation + string.ascii_letters)
    short, long = labeler("XY"), labeler("XY Projection")
    for text, label in (("XY", short), ("XY Projection", long)):
        left, _, right, _ = font.getbbox(text)
        assert label.shape == (3, box[3] - box[1], right - left) and label.dtype == torch.float32
        assert torch.equal(label[0], label[1]) and torch.equal(label[0], label[2]) and 0 <= float(label.min()) < 0.5 and float(label.max()) == 1
        assert torch.equal(label * 255, (label * 255).round())                # bytes / 255
    assert torch.equal(long[:, :, :short.shape[2] - 2], short[:, :, :-2])    # the same glyphs at the same place
    assert (labeler(" ") == 1).all()
    labelled = vis.draw_cameras(64, *camera_inputs()[:3], labeler=vis.pil_labeler())     # (64: wider than every label, as the reference needs)
    assert labelled.shape == (3, 3, 64 + 4 + long.shape[1], 64)


def test_validation_images_panel_geometry():
    """comparison = border 8 | style | gap 8 | [extra] | Context (image, depth per view) | Target GT | Prediction | Depth; columns 8 apart, panels
    of a column 8 apart; every gap and the border are 1.0; RGB panels are copied bit for bit; depth panels are bytes / 255"""
    from styl3r_amd.export import pack_frames
    g = torch.Generator().manual_seed(3)
    h, w, v, t = 12, 20, 2, 3
    ctx, gt, pred, extra = (torch.rand((n, 3, h, w), generator=g) for n in (v, t, t, t))
    ctx_depth, depth = torch.rand((v, h, w), generator=g) + 0.5, torch.rand((t, h, w), generator=g) + 0.5
    style = torch.rand((3, 9, 7), generator=g)
    E, K, _, near, far = camera_inputs()
    batch = {"context": dict(extrinsics=E[None, :2], intrinsics=K[None, :2], near=near[None, :2], far=far[None, :2]),
             "target": dict(extrinsics=E[None, 2:], intrinsics=K[None, 2:], near=near[None, 2:], far=far[None, 2:])}
    out = vis.validation_images(ctx, ctx_depth, gt, pred, depth, None, batch, extra_columns=[("2D Baseline", extra)], style_image=style, resolution=48)
    assert set(out) == {"comparison", "cameras"}                            # (no Gaussians: no projection)
    comp = out["comparison"]
    tall = 2 * v * h + (2 * v - 1) * 8                                     # the Context column: 4 panels
    assert comp.shape == (3, tall + 16, 8 + 7 + 8 + 5 * w + 4 * 8 + 8) and comp.dtype == torch.float32
    seen = torch.zeros(comp.shape[1:], dtype=torch.bool)

    def panel(x0, y0, want):
        ph, pw = want.shape[1:]
        assert torch.equal(comp[:, 8 + y0:8 + y0 + ph, x0:x0 + pw], want), (x0, y0)
        seen[8 + y0:8 + y0 + ph, x0:x0 + pw] = True
    panel(8, 0, style)
    x = 8 + 7 + 8
    ctx_bytes = pack_frames([ctx_depth], loop_reverse=False).permute(0, 3, 1, 2).float() / 255
    depth_bytes = pack_frames([depth], loop_reverse=False).permute(0, 3, 1, 2).float() / 255
    columns = [list(extra), [p for i in range(v) for p in (ctx[i], ctx_bytes[i])], list(gt), list(pred), list(depth_bytes)]
    for col, panels in enumerate(columns):
        for row, p in enumerate(panels):
            panel(x + col * (w + 8), row * (h + 8), p)
    assert (comp[:, ~seen] == 1).all() and int((~seen).sum()) > 0              # gaps, padding and border
    cams = out["cameras"]
    assert cams.shape == (3, 48 + 16, 3 * 48 + 2 * 8 + 16)
    inner = vis.render_cameras(batch, 48)
    for i in range(3):
        assert torch.equal(cams[:, 8:56, 8 + i * 56:8 + i * 56 + 48], inner[i])
    assert (cams[:, :8] == 1).all() and (cams[:, :, 56:64] == 1).all()
    labelled = vis.validation_images(ctx, ctx_depth, gt, pred, depth, None, batch, labeler=_stub_labeler, resolution=48)["comparison"]
    assert labelled.shape[1] == tall + 9 + 16                               # stub label 5 rows + gap 4


def test_argument_errors_are_raised_on_the_host():
    image = torch.zeros(3, 8, 8)
    with pytest.raises(ValueError):
        vis.draw_lines(image, [0, 0], [4, 4], 1, 2, cap="flat")
    with pytest.raises(ValueError):
        vis.draw_lines(image, [0, 0], [4, 4], 1, 2, num_msaa_passes=-1)
    with pytest.raises(ValueError):
        vis.draw_lines(image, [0, 0, 0], [4, 4], 1, 2)
    with pytest.raises(ValueError):
        vis.draw_lines(image, torch.zeros(3, 2), torch.zeros(2, 2), 1, 2)
    with pytest.raises(ValueError):
        vis.draw_lines(image, [0, 0], [4, 4], float("nan"), 2)
    with pytest.raises(ValueError):
        vis.draw_lines(image, [0, 0], [4, 4], 1, 2, x_range=[0, 1, 2])
    with pytest.raises(ValueError):
        vis.draw_points(image, [[1, 1]], radius=torch.ones(2, 2))
    with pytest.raises(ValueError):
        vis.draw_points(torch.zeros(8, 8), [[1, 1]])
    with pytest.raises(ValueError):
        vis.draw_layers(torch.zeros(2, 3, 8, 8), [[]])
    with pytest.raises(ValueError):
        vis.draw_layers(torch.zeros(1, 3, 8, 8), [[vis.Layer(np.zeros((2, 5)))]])
    with pytest.raises(ValueError):
        vis.draw_layers(torch.zeros(1, 4, 8, 8), [[]])
    with pytest.raises(ValueError):
        vis.draw_cameras(0, torch.eye(4)[None], torch.eye(3)[None], 1)
    with pytest.raises(ValueError):
        vis.draw_cameras(8, torch.eye(4)[None], torch.eye(3)[None].repeat(2, 1, 1), 1)
    with pytest.raises(ValueError):
        vis.hcat(image, image, align="left")
    with pytest.raises(ValueError):
        vis.overlay(image, torch.zeros(3, 9, 9), "horizontal", "start", "start")
    with pytest.raises(ValueError):
        vis.projection_cameras(torch.zeros(4, 3))


def test_the_library_exports_gsr_draw_layers_and_refuses_bad_arguments_before_any_launch():
    from styl3r_amd import _lib
    lib = _lib.load()
    header = (Path(__file__).resolve().parents[1] / "include" / "gsr.h").read_text()
    assert "gsr_draw_layers" in _lib.EXPORTS and re.search(r"\bgsr_draw_layers\s*\(", header) and hasattr(lib, "gsr_draw_layers")
    assert "gsr_draw.hip" in _lib._SOURCES
    for name, value in (("GSR_DRAW_RECORD_DOUBLES", _lib.GSR_DRAW_RECORD_DOUBLES), ("GSR_DRAW_CHUNK", _lib.GSR_DRAW_CHUNK),
                        ("GSR_DRAW_POINT", _lib.GSR_DRAW_POINT)):
        assert re.search(rf"#define {name} {value}\b", header), name
    ok = dict(images=64, out=64, B=1, H=8, W=8, il=64, lp=64, lm=64, NL=1, prims=64, NP=1)
    call = lambda **kw: (lambda a: lib.gsr_draw_layers(a["images"], a["out"], a["B"], a["H"], a["W"], a["il"], a["lp"], a["lm"], a["NL"], a["prims"],
                                                       a["NP"], None))({**ok, **kw})
    for bad in (dict(images=None), dict(out=None), dict(il=None), dict(lp=None), dict(lm=None), dict(B=0), dict(B=65536), dict(H=0), dict(W=0),
                dict(NL=-1), dict(NP=-1), dict(prims=None), dict(prims=72), dict(H=1 << 15, W=1 << 14), dict(NP=(1 << 30) + 1)):
        assert call(**bad) == -1, bad                                     # GSR_EINVAL; no pointer is followed, nothing is launched
