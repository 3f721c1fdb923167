"""-m gpu: k_draw_layers (csrc/gsr_draw.hip behind gsr_draw_layers) through styl3r_amd/visualization.py -- against the reference's float64
run (tests/golden/validation_vis.npz) and against the float64 host restatement of the same module, which tests/test_vis_host.py holds to the
same fixture.  Coverage (alpha * 64) is compared as integers; pictures within 2^-22 (tests/vis_common.py says why).  Then the pictures
built on the kernel: draw_cameras, render_projections, validation_images, validation_step."""
import ctypes as C

import numpy as np
import pytest
import torch

from styl3r_amd import _lib
from styl3r_amd import visualization as vis
from tests.vis_common import CAM_CASES, DRAW_CASES, TOL, camera_inputs, check_camera_case, check_draw_case, coverage64, max_diff

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
CPU = torch.device("cpu")


@pytest.mark.parametrize("name", DRAW_CASES)
def test_every_drawing_case_of_the_fixture_on_the_device(name):
    check_draw_case(name, DEV)


@pytest.mark.parametrize("name", CAM_CASES)
def test_every_camera_case_of_the_fixture_on_the_device(name):
    check_camera_case(name, DEV)


def random_layers(shape, seed, n_lines=12, n_points=4, cap="round", passes=1):
    """a line layer and a point layer over an image of `shape`, ends and centres up to 4 pixels outside it"""
    h, w = shape
    rng = np.random.default_rng(seed)
    xy = lambda n: np.stack([rng.uniform(-4, w + 4, n), rng.uniform(-4, h + 4, n)], 1).astype(np.float32)
    layers = []
    if n_lines:
        layers.append(vis.line_layer(shape, xy(n_lines), xy(n_lines), rng.uniform(0, 1, (n_lines, 3)).astype(np.float32).tolist(),
                                     rng.uniform(0.5, 4, n_lines).astype(np.float32).tolist(), cap, passes))
    if n_points:
        layers.append(vis.point_layer(shape, xy(n_points), rng.uniform(0, 1, (n_points, 3)).astype(np.float32).tolist(),
                                      rng.uniform(1.5, 5, n_points).astype(np.float32).tolist(), rng.uniform(0, 1.5, n_points).astype(np.float32).tolist(), passes))
    return layers


def device_equals_host(images, stacks, what):
    got = vis.draw_layers(images.to(DEV), stacks).cpu()
    want = vis.draw_layers_reference(images, stacks)
    d = max_diff(got, want)
    print(f"{what}: max |device - host| = {d:.3g}")
    shape = images.shape[2:]
    for stack in stacks:
        for layer in stack:
            if len(layer.records):
                assert torch.equal(coverage64(layer, shape, DEV), vis.render_overlay(shape, layer, CPU)[3] * 64), f"{what}: coverage differs"
    assert d <= TOL, (what, d)
    return got


# one pixel; one tile; one pixel past a tile in each direction (four workgroups, three of them nearly empty); an odd shape of 3 x 4 tiles
@pytest.mark.parametrize("shape", [(1, 1), (16, 16), (17, 33), (37, 53)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("cap", ["butt", "round", "square"])
def test_device_equals_host_on_small_and_odd_shapes(shape, cap):
    g = torch.Generator().manual_seed(shape[1])
    device_equals_host(torch.rand((1, 3, *shape), generator=g), [random_layers(shape, 7 + shape[0], cap=cap)], f"{shape} {cap}")


@pytest.mark.parametrize("n", [1, _lib.GSR_DRAW_CHUNK, _lib.GSR_DRAW_CHUNK + 1, 2 * _lib.GSR_DRAW_CHUNK + 5])
def test_primitive_counts_around_the_lds_chunk(n):
    """one primitive; a full chunk; one more than the chunk holds (the last primitive, alone in its chunk, is on top); three chunks"""
    shape = (20, 36)
    (layer,) = random_layers(shape, 100 + n, n_lines=n, n_points=0)
    layer.records[-1] = vis.line_layer(shape, [2.0, 3.0], [33.0, 17.0], [0.125, 0.25, 0.5], 3).records[0]     # the last line crosses the image ...
    layer.records[-1, 1] = n - 1                                          # ... in a colour of its own
    got = device_equals_host(torch.zeros((1, 3, *shape)), [[layer]], f"{n} primitives")
    assert torch.equal(got[0, :, 10, 17], torch.tensor([0.125, 0.25, 0.5]))      # (17.5, 10.5) is on it: the highest index wins


def test_three_images_of_four_layers_in_one_call():
    """different primitive counts per layer, an empty layer, a layer without MSAA, and an image without layers -- one launch"""
    shape = (21, 40)
    g = torch.Generator().manual_seed(5)
    images = torch.rand((3, 3, *shape), generator=g)
    empty = vis.Layer(np.zeros((0, vis.REC)), 1)
    a, b = random_layers(shape, 1, 5, 3), random_layers(shape, 2, 40, 1, cap="square")
    c = random_layers(shape, 3, 2, 7, passes=0)
    stacks = [[a[0], empty, a[1], b[0]], [b[1], c[0], c[1], a[0]], [empty, b[0], empty, c[1]]]
    got = device_equals_host(images, stacks, "3 x 4 layers")
    alone = vis.draw_layers(images[1:2].to(DEV), [stacks[1]]).cpu()
    assert torch.equal(alone[0], got[1])                                  # an image's picture does not depend on its neighbours in the call
    none = vis.draw_layers(images.to(DEV), [[], [empty], []]).cpu()
    assert torch.equal(none, images)


def test_lines_on_tile_borders_and_across_the_image_border():
    shape = (40, 40)
    start = [[0.0, 16.0], [16.0, -5.0], [-8.0, -8.0], [31.5, 0.0], [-3.0, 32.0], [39.5, 39.5]]
    end = [[40.0, 16.0], [16.0, 45.0], [48.0, 48.0], [32.5, 40.0], [43.0, 32.0], [60.0, 39.5]]
    for cap in ("butt", "square"):
        layer = vis.line_layer(shape, start, end, [[1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 1, 0], [0, 1, 1], [1, 0, 1]], [2, 1, 3, 0.75, 2.5, 4], cap)
        device_equals_host(torch.zeros((1, 3, *shape)), [[layer]], f"tile borders {cap}")


def test_degenerate_and_sub_pixel_lines():
    shape = (18, 34)
    start = [[8.0, 8.0], [2.2, 11.9], [20.0, 4.0], [16.0, 16.0]]         # [1]: 0.3 wide, between the centre rows 11.5 and 12.5 all the way
    end = [[8.0, 8.0], [30.2, 12.1], [20.0, 4.0], [16.0, 16.0]]
    for cap in ("round", "butt"):
        layer = vis.line_layer(shape, start, end, [[1, 0.5, 0], [0, 1, 0], [0, 0.5, 1], [1, 1, 1]], [5, 0.3, 0.6, 3], cap)
        assert np.isnan(layer.records[[0, 2, 3], 6:8]).all()
        got = device_equals_host(torch.zeros((1, 3, *shape)), [[layer]], f"degenerate {cap}")
        assert (got[0, :, 8, 8] != 0).any() == (cap == "round")          # a degenerate line is its round caps and nothing else
        assert not ((got[0, 0] == 0) & (got[0, 1] > 0) & (got[0, 2] == 0)).any()     # the 0.3-pixel green line covers no centre: never drawn


def test_no_msaa_passes_and_points_with_an_inner_radius():
    shape = (33, 31)
    hard = random_layers(shape, 11, 6, 5, passes=0)
    got = device_equals_host(torch.zeros((1, 3, *shape)), [hard], "no MSAA")
    colours = {tuple(c) for layer in hard for c in layer.records[:, 11:14].astype(np.float32).tolist()} | {(0.0, 0.0, 0.0)}
    assert {tuple(p) for p in got[0].reshape(3, -1).T.tolist()} <= colours                       # no blended pixel anywhere
    ring = vis.point_layer(shape, [[15.5, 16.5]], [1.0, 1.0, 1.0], 9, 5)
    got = device_equals_host(torch.zeros((1, 3, *shape)), [[ring]], "annulus")
    assert got[0, 0, 16, 15] == 0 and got[0, 0, 16, 22] == 1 and got[0, 0, 16, 27] == 0


def test_two_runs_give_equal_bits():
    shape = (37, 53)
    g = torch.Generator().manual_seed(8)
    images = torch.rand((2, 3, *shape), generator=g).to(DEV)
    stacks = [random_layers(shape, 21, 30, 6), random_layers(shape, 22, 9, 9, cap="square")]
    first = vis.draw_layers(images, stacks)
    again = vis.draw_layers(images, stacks)
    assert torch.equal(first, again) and not torch.equal(first, images)


def test_the_c_entry_point_refuses_bad_arguments_and_draws_in_place():
    lib = _lib.load()
    shape = (9, 20)
    (layer,) = random_layers(shape, 4, 3, 0)
    image = torch.zeros((1, 3, *shape), device=DEV)
    want = vis.draw_layers(image, [[layer]])
    table = torch.tensor([0, 1, 0, 3, 1], dtype=torch.int32, device=DEV)
    rec = torch.from_numpy(layer.records).to(DEV)
    stream = C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
    call = lambda B, H, W, prims: lib.gsr_draw_layers(image.data_ptr(), image.data_ptr(), B, H, W, table.data_ptr(), table[2:].data_ptr(),
                                                      table[4:].data_ptr(), 1, prims, 3, stream)
    assert call(0, 9, 20, rec.data_ptr()) == -1 and call(1, 0, 20, rec.data_ptr()) == -1 and call(1, 9, 20, rec.data_ptr() + 8) == -1
    assert call(1, 9, 20, None) == -1
    assert call(1, 9, 20, rec.data_ptr()) == 0
    torch.cuda.synchronize()
    assert torch.equal(image, want)                                       # out == images: in place


def test_draw_cameras_on_the_device_equals_the_host_restatement():
    E, K, color, near, far = camera_inputs()
    E5, K5 = torch.cat([E, E[:2]]), torch.cat([K, K[:2]])
    E5[3:, :3, 3] += torch.tensor([0.3, -0.2, 0.5])
    colors = torch.tensor([[1.0, 1, 1], [1, 1, 1], [1, 0, 0], [1, 0, 0], [1, 0, 0]])
    near5, far5 = torch.cat([near, near[:2]]), torch.cat([far, far[:2]])
    got = vis.draw_cameras(64, E5.to(DEV), K5.to(DEV), colors, near5.to(DEV), far5.to(DEV))
    want = vis.draw_cameras(64, E5, K5, colors, near5, far5)
    assert got.is_cuda and got.shape == (3, 3, 64, 64)
    d = max_diff(got.cpu(), want)
    print(f"draw_cameras 5 cameras at 64^2: max |device - host| = {d:.3g}")
    assert d <= TOL and (want > 0).any()


def _gaussians(b, n, seed):
    from styl3r_amd.decoder import Gaussians
    g = torch.Generator().manual_seed(seed)
    means = torch.randn((b, n, 3), generator=g) * torch.tensor([1.0, 0.5, 1.5]) + torch.tensor([0.2, -0.1, 2.0])
    L = torch.randn((b, n, 3, 3), generator=g) * 0.15
    cov = L @ L.transpose(-1, -2) + 0.01 * torch.eye(3)
    return Gaussians(means.to(DEV), cov.to(DEV), torch.rand((b, n, 3, 1), generator=g).to(DEV), (torch.rand((b, n), generator=g) * 0.8 + 0.1).to(DEV))


def test_render_projections_is_the_orthographic_renderer_with_projection_cameras():
    from styl3r_amd.decoder import render_hip_orthographic
    gs = _gaussians(2, 64, 6)
    got = vis.render_projections(gs, 32)
    assert got.shape == (2, 3, 3, 32, 32) and got.dtype == torch.float32          # the reference's padded stack: (b, axis, 3, h, w)
    for look, (E, width, height, near, far) in enumerate(vis.projection_cameras(gs.means)):
        want = render_hip_orthographic(E, width, height, near, far, (32, 32), torch.zeros((2, 3), device=DEV), gs, 1, fov_degrees=10.0)
        assert torch.equal(got[:, look], want)
    assert (got > 0).any() and torch.isfinite(got).all()
    labelled = vis.render_projections(gs, 32, labeler=lambda text: torch.full((3, 5, 40 if text.startswith("XY") else 20), 0.5), extra_label="x")
    assert labelled.shape == (2, 3, 3, 32 + 9, 40)                               # labels of unequal width: padded with ones to the widest
    assert (labelled[:, 1, :, :, 32:] == 1).all() and torch.equal(labelled[:, 1, :, 9:, :32], got[:, 1])


class _Encoder(torch.nn.Module):
    """stands in for the encoder: the scene's Gaussians, and the context depth in the dump"""

    stylized = True

    def __init__(self, g, depth):
        super().__init__()
        self.g, self.depth, self.style = g, depth, None

    def forward(self, context, style, global_step, visualization_dump=None):
        visualization_dump["depth"] = self.depth
        self.style = style
        return self.g


def test_validation_step_returns_the_scores_and_the_three_pictures():
    from styl3r_amd import evaluation, metrics
    from styl3r_amd.decoder import DecoderSplattingCUDACfg, Gaussians, get_decoder
    from styl3r_amd.scenes import make_scene
    from tests.test_gpu_metrics import _fixed_lpips
    hw = 64
    sc = make_scene(n_ctx=1, grid_hw=(hw, hw), n_views=3, image_hw=(hw, hw), sh_degree=0, seed=5).to(DEV)
    g = Gaussians(sc.means[None], sc.covariances[None], sc.harmonics[None], sc.opacities[None])
    dec = get_decoder(DecoderSplattingCUDACfg("splatting_cuda", [0.0, 0.0, 0.0], True)).to(DEV)
    E, K, n, f = sc.extrinsics[None], sc.intrinsics[None], sc.near[None], sc.far[None]
    with torch.no_grad():
        target = dec.forward(g, E, K, n, f, (hw, hw)).color
    gt = (target + 0.05 * torch.rand(target.shape, device=DEV)).clamp(0, 1)
    batch = {"context": {"image": gt[:, :2], "extrinsics": E[:, :2], "intrinsics": K[:, :2], "near": n[:, :2], "far": f[:, :2]},
             "target": {"image": gt, "extrinsics": E, "intrinsics": K, "near": n, "far": f},
             "style": {"image": torch.rand((1, 3, 40, 40), device=DEV)}}
    depth = torch.rand((1, 2, hw, hw, 1, 1), device=DEV) + 0.5
    lp = _fixed_lpips(11)
    encoder = _Encoder(g, depth)
    out, scores, images = evaluation.validation_step(encoder, dec, batch, 7, lpips=lp, resolution=48)
    assert torch.equal(encoder.style["image"], (batch["style"]["image"] - 0.5) / 0.5)       # a stylized encoder takes the style in [-1, 1] ...
    assert torch.equal(out.color, target)
    assert torch.equal(scores["val/psnr"], metrics.compute_psnr(gt[0], target[0]).mean()) and 0 < float(scores["val/ssim"]) <= 1
    assert float(scores["val/lpips"]) >= 0
    assert set(images) == {"comparison", "projection", "cameras"}
    for name, image in images.items():
        assert image.is_cuda and image.dtype == torch.float32 and image.dim() == 3 and image.shape[0] == 3, name
        assert (image[:, :8] == 1).all() and (image[:, :, -8:] == 1).all() and torch.isfinite(image).all(), name
    assert images["projection"].shape == images["cameras"].shape == (3, 48 + 16, 3 * 48 + 16 + 16)
    comp = images["comparison"]                                            # style | Context (2 x (image, depth)) | GT | prediction | depth
    assert comp.shape == (3, 4 * hw + 3 * 8 + 16, 40 + 4 * hw + 4 * 8 + 16)
    assert torch.equal(comp[:, 8:48, 8:48], batch["style"]["image"][0])                      # ... and the Style panel shows it as it came
    x = 8 + (40 + 8) + (hw + 8)
    for i in range(3):
        y = 8 + i * (hw + 8)
        assert torch.equal(comp[:, y:y + hw, x:x + hw], gt[0, i]) and torch.equal(comp[:, y:y + hw, x + hw + 8:x + 2 * hw + 8], target[0, i])
    assert torch.equal(images["cameras"][:, 8:56, 8:56], vis.render_cameras(batch, 48)[0])
    assert torch.equal(images["projection"][:, 8:56, 8:56], vis.render_projections(g, 48)[0, 0])


def test_the_new_symbols_are_exported_by_the_built_library():
    lib = _lib.load()
    assert "gsr_draw_layers" in _lib.EXPORTS and hasattr(lib, "gsr_draw_layers") and "gsr_draw.hip" in _lib._SOURCES
    assert _lib.built_digest() == _lib.build_digest()                     # the loaded library was built from this tree's sources
