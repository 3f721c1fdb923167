"""-m gpu: the composite backward cut into depth segments (include/gsr.h GSR_FLAG_SEG_SHIFT).

K6 walks one (view, tile, segment) unit per wavefront; every segment in front of a tile's deepest one starts from the checkpoint
the composite forward stored at its end.  Gradients against the f32 / f64 oracles at the rasterizer's bars (tests/test_gpu_rasterizer.py),
with the segment length forced through rasterizer.EXTRA_FLAGS, and the segmented backward against the one-segment one.

Segmented vs one segment: a segment starts from the forward's own T_b where the one-segment walk reconstructs it by dividing out the
alphas behind it, and from S = g.(C_final - C_b) where that walk sums the same terms back to front; both are fp32 rounding of the same
quantities (~1e-6 relative on 600-entry lists), and the gradient atomics arrive in another order.  Bar: 5e-5 of the largest gradient."""
import numpy as np
import pytest
import torch

from styl3r_amd import _lib
from styl3r_amd import rasterizer as rz
from tests.gpu_utils import assert_close_rel, hip_single_view, oracle_single_view, ws_view
from tests.helpers import simple_camera
from tests.test_gpu_rasterizer import _check_backward, _scene_view_cam

pytestmark = pytest.mark.gpu

SEG = {64: 1, 128: 2, 192: 3, 256: 4, 384: 5, "one": 7}
SEG_VS_ONE = 5e-5


def _flags(L):
    return SEG[L] << _lib.GSR_FLAG_SEG_SHIFT


@pytest.fixture(autouse=True)
def _debug_on():
    rz.KEEP_DEBUG = True
    yield
    rz.KEEP_DEBUG = False
    rz.LAST_DEBUG.clear()


def _one_tile_scene(G, seed, op=(0.02, 0.08), scale=0.02):
    """G splats inside a 16 x 16 image: one tile whose list holds every one of them"""
    rng = np.random.default_rng(seed)
    z = rng.uniform(2.0, 6.0, G)
    t = 0.5 / 0.86 * 0.8
    means = np.stack([rng.uniform(-t, t, G) * z, rng.uniform(-t, t, G) * z, z], 1)
    cov6 = np.tile(np.array([1.0, 0, 0, 1.0, 0, 1.0]) * scale ** 2, (G, 1)) * (z[:, None] ** 2)
    return means, cov6, rng.uniform(*op, G), rng.uniform(0, 1, (G, 3))


def _grads_single_view(means, cov6, opac, cam, colors, seed=0):
    dev = torch.device("cuda:0")
    out = hip_single_view(means, cov6, opac, cam, colors=colors, bg=(0.2, 0.3, 0.1), requires_grad=True)
    rng = np.random.default_rng(seed)
    wI = torch.tensor(rng.normal(size=(3, cam["H"], cam["W"])), dtype=torch.float32, device=dev)
    wD = torch.tensor(rng.normal(size=(cam["H"], cam["W"])) * 0.3, dtype=torch.float32, device=dev)
    ((out["image"] * wI).sum() + (out["depth"][0] * wD).sum()).backward()
    t = out["inputs"]
    return [x.grad.detach().cpu().numpy() for x in (t["means"], t["cov6"], t["opac"], t["colors"])] + \
        [out["means2D"].grad.detach().cpu().numpy()]


def _seg_vs_one(monkeypatch, run, L, what):
    monkeypatch.setattr(rz, "EXTRA_FLAGS", _flags(L))
    a = run()
    monkeypatch.setattr(rz, "EXTRA_FLAGS", _flags("one"))
    b = run()
    for x, y, name in zip(a, b, ("means", "cov", "opac", "colors", "means2D")):
        assert np.isfinite(x).all(), name
        assert_close_rel(x, y, SEG_VS_ONE, f"{what}: L={L} vs one segment d{name}")


@pytest.mark.parametrize("L", [64, 128])
@pytest.mark.parametrize("dn", [-1, 0, 1, "2L"])
def test_list_lengths_around_a_boundary(monkeypatch, L, dn):
    """one tile of L-1, L, L+1 and 2L entries (no pixel saturates): depth gradient instantiation, both oracles"""
    n = 2 * L if dn == "2L" else L + dn
    cam = simple_camera(16, 16)
    means, cov6, opac, colors = _one_tile_scene(n, seed=n)
    _, st, _ = oracle_single_view("f32", means, cov6, opac, cam, colors=colors)
    assert st.R == n, (st.R, n)        # every splat lands in the one tile
    monkeypatch.setattr(rz, "EXTRA_FLAGS", _flags(L))
    _check_backward(means, cov6, opac, cam, colors=colors, bg=(0.2, 0.3, 0.1), seed=n)
    _seg_vs_one(monkeypatch, lambda: _grads_single_view(means, cov6, opac, cam, colors, seed=n), L, f"n={n}")


def test_tile_saturates_before_a_boundary(monkeypatch):
    """dense opaque splats: every pixel's T falls below 1e-4 long before the end of its 600-entry list -- the segments behind the deepest
    contributor have no work, the one holding it starts as the whole-list walk, the ones in front from checkpoints of frozen pixels"""
    cam = simple_camera(16, 16)
    means, cov6, opac, colors = _one_tile_scene(600, seed=3, op=(0.6, 0.99), scale=0.2)
    monkeypatch.setattr(rz, "EXTRA_FLAGS", _flags(64))
    _check_backward(means, cov6, opac, cam, colors=colors, bg=(0.2, 0.3, 0.1), seed=3, f64_rel=1e-2)
    last = ws_view("n_contrib", np.uint32, 256)      # the deepest contribution stops well in front of the list's end
    assert 64 < last.max() < 600 - 128, last.max()
    _seg_vs_one(monkeypatch, lambda: _grads_single_view(means, cov6, opac, cam, colors, seed=3), 64, "saturated tile")


def test_single_segment_tile(monkeypatch):
    """a list shorter than L: one unit, the deepest, no checkpoint"""
    cam = simple_camera(16, 16)
    means, cov6, opac, colors = _one_tile_scene(100, seed=11)
    monkeypatch.setattr(rz, "EXTRA_FLAGS", _flags(256))
    _check_backward(means, cov6, opac, cam, colors=colors, bg=(0.2, 0.3, 0.1), seed=11)


def _full_size_view(n_ctx, seed, view):
    from styl3r_amd.decoder import prepare_views
    from styl3r_amd.scenes import make_scene
    sc = make_scene(n_ctx=n_ctx, grid_hw=(256, 256), n_views=2, image_hw=(256, 256), sh_degree=0, seed=seed)
    views = prepare_views(sc.extrinsics, sc.intrinsics, sc.near, sc.far, torch.zeros(2, 3), True).numpy()
    s, cov6, cam = _scene_view_cam(sc, views, view)
    return sc.means.numpy() * s, cov6, sc.opacities.numpy(), sc.harmonics.numpy().transpose(0, 2, 1), cam


def test_headline_view_with_headline_segments(monkeypatch):
    """one view of the headline scene (lists of ~630 entries) cut at the headline's L = 256, every gradient, depth gradient included"""
    means, cov6, opac, shs, cam = _full_size_view(1, 1234, 1)
    monkeypatch.setattr(rz, "EXTRA_FLAGS", _flags(256))
    _check_backward(means, cov6, opac, cam, shs=shs, seed=5, f64_rel=1e-3)


def test_one_view_launch_default_segments():
    """a one-view launch (256 tiles) takes the short segments of the size rule (gsr_common.h seg_len): against both oracles"""
    means, cov6, opac, shs, cam = _full_size_view(1, 99, 0)
    assert rz.EXTRA_FLAGS == 0
    # parity bar: 1e-4 against the f32 oracle; fp64 bounds the fp32 arithmetic itself (single alpha >= 1/255 flips on ~630-entry lists
    # reach 1.3e-3 in this scene, one-segment and segmented alike)
    _check_backward(means, cov6, opac, cam, shs=shs, seed=8, f64_rel=5e-3)


def test_c4_size_lists_many_segments(monkeypatch):
    """C4-size lists (~2 250 entries, up to ~4 700): 18 - 37 segments of 128 per tile"""
    means, cov6, opac, shs, cam = _full_size_view(4, 4321, 0)
    monkeypatch.setattr(rz, "EXTRA_FLAGS", _flags(128))
    _check_backward(means, cov6, opac, cam, shs=shs, seed=6, f64_rel=1e-2)


def _decoder_grads(B, Vt, mse, seed=0, hw=(256, 256)):
    from styl3r_amd.decoder import DecoderSplattingCUDACfg, Gaussians, get_decoder
    from styl3r_amd.scenes import make_scene
    dev = torch.device("cuda:0")
    scs = [make_scene(n_ctx=1, grid_hw=(256, 256), n_views=Vt, image_hw=hw, sh_degree=0, seed=1234 + i) for i in range(B)]
    st = lambda n: torch.stack([getattr(sc, n) for sc in scs]).to(dev)
    g = Gaussians(*(st(n).requires_grad_(True) for n in ("means", "covariances", "harmonics", "opacities")))
    dec = get_decoder(DecoderSplattingCUDACfg("splatting_cuda", [0.0, 0.0, 0.0], True)).to(dev)
    gen = torch.Generator(dev).manual_seed(seed)
    w = torch.rand(B, Vt, 3, *hw, device=dev, generator=gen)
    args = (g, st("extrinsics"), st("intrinsics"), st("near"), st("far"), hw)
    if mse:
        target = torch.rand(B, Vt, 3, *hw, device=dev, generator=gen)
        out = dec.forward(*args, mse_target=target, mse_weight=0.7)
        loss = out.loss_mse + (out.color * w).sum() * 1e-4
    else:
        loss = (dec.forward(*args).color * w).sum()
    return [x.detach().cpu().numpy() for x in torch.autograd.grad(loss, (g.means, g.covariances, g.opacities, g.harmonics))] + \
        [np.zeros(1)]


def test_headline_workload_segmented_equals_one_segment(monkeypatch):
    """the bench's workload (10 scenes x 4 views, G = 65 536, 256 x 256) through the decoder: the size rule's segments (L = 256 at
    10 240 tiles) against one segment per tile"""
    monkeypatch.setattr(rz, "EXTRA_FLAGS", 0)
    a = _decoder_grads(10, 4, mse=True)
    monkeypatch.setattr(rz, "EXTRA_FLAGS", _flags("one"))
    b = _decoder_grads(10, 4, mse=True)
    for x, y, name in zip(a, b, ("means", "cov", "opac", "sh")):
        assert np.isfinite(x).all(), name
        assert_close_rel(x, y, SEG_VS_ONE, f"headline: segmented vs one segment d{name}")


@pytest.mark.parametrize("L", [64, 256])
def test_fused_mse_plus_external_image_gradient(monkeypatch, L):
    """fused LossMse plus another consumer of the colour (the prologue adds both image gradients) on a segmented backward"""
    _seg_vs_one(monkeypatch, lambda: _decoder_grads(2, 2, mse=True, seed=L), L, "fused MSE + dL/dimage")
