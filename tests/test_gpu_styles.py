"""-m gpu: the multi-style forward (csrc/gsr_styles.hip through `rasterize_views_styles` / `DecoderSplattingHIP.forward_styles`),
the encoder's scene cache on the device and `inference.stylize_scene`.

Bars (all the project's existing ones): the integers of the shared pass -- radii, n_contrib, the sorted list words with their
quadrant-mask bits, tile ranges, the pair count -- are exactly those of `rasterize_views` on style 0 and do not depend on S; every
style's image, the depth, the opacity and final_T are within 1e-4 relative of the fp32 CPU oracle on the oracle's non-fragile pixels;
against per-style `rasterize_views` calls images are within 1e-4 (expected: bit-identical; the observed distance is printed)."""
import numpy as np
import pytest
import torch

from styl3r_amd import rasterizer as rz
from tests.gpu_utils import assert_close_rel, ws_view
from tests.helpers import deterministic_init_

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
S_ALL = (2, 3, 4, 5, 8)
MODES = ("sh0", "sh2", "sh4", "rgb")
POOL = 8        # colour sets per scene: a call with S styles takes the first S


@pytest.fixture(autouse=True)
def _debug_on():
    rz.KEEP_DEBUG = True
    yield
    rz.KEEP_DEBUG = False
    rz.LAST_DEBUG.clear()


def _problem(mode, V, hw=(256, 256), grid=(64, 64), seed=77):
    """2 x grid Gaussians seen from V cameras; POOL colour sets in the layout `mode` asks for.  Host tensors + packed views."""
    from styl3r_amd.decoder import prepare_views
    from styl3r_amd.scenes import make_scene, sh_mask
    deg = 0 if mode == "rgb" else int(mode[2:])
    sc = make_scene(n_ctx=2, grid_hw=grid, n_views=V, image_hw=hw, sh_degree=deg, seed=seed)
    gen = torch.Generator().manual_seed(seed + 1)
    G, M = sc.means.shape[0], (deg + 1) ** 2
    cols = []
    for s in range(POOL):
        if mode == "rgb":
            cols.append(torch.rand(G, 3, generator=gen))
        else:
            hm = sc.harmonics if s == 0 else torch.randn(G, 3, M, generator=gen) * sh_mask(M) * (0.5 + 0.25 * s)
            cols.append(hm.permute(0, 2, 1).contiguous())                    # (G, M, 3)
    views = prepare_views(sc.extrinsics, sc.intrinsics, sc.near, sc.far, torch.tensor([[0.1, 0.3, 0.2]]).expand(V, 3), True)
    return sc, cols, views, deg, mode != "rgb"


def _snap(V, G, H, W):
    """integers and per-pixel state the last forward left in its workspace"""
    T = ((H + 15) // 16) * ((W + 15) // 16)
    R = rz.LAST_DEBUG["num_pairs"]
    return dict(R=R, off=ws_view("tile_offset", np.uint32, V * T + 1).copy(), pl=ws_view("point_list", np.uint32, max(R, 1))[:R].copy(),
                nc=ws_view("n_contrib", np.uint32, V * H * W).copy(), fT=ws_view("final_T", np.float32, V * H * W).copy())


def _single(sc, col, views, V, deg, use_sh):
    H, W = sc.image_shape
    d = lambda t: t.to(DEV)
    out = rz.rasterize_views(d(sc.means)[None], d(sc.covariances)[None], d(sc.opacities)[None], d(col)[None], d(views), (H, W), V,
                             sh_degree=deg, use_sh=use_sh)
    torch.cuda.synchronize()
    return out, _snap(V, sc.means.shape[0], H, W)


def _styles(sc, cols, views, V, deg, use_sh):
    H, W = sc.image_shape
    d = lambda t: t.to(DEV)
    with torch.no_grad():
        out = rz.rasterize_views_styles(d(sc.means)[None], d(sc.covariances)[None], d(sc.opacities)[None], [d(c)[None] for c in cols],
                                        d(views), (H, W), V, sh_degree=deg, use_sh=use_sh)
    torch.cuda.synchronize()
    return out, _snap(V, sc.means.shape[0], H, W)


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-12))


@pytest.mark.parametrize("mode,V,hw", [(m, V, (256, 256)) for m in MODES for V in (3, 40)] + [("sh2", 3, (100, 84)), ("rgb", 5, (50, 70))])
def test_shared_pass_equals_the_single_style_call_for_every_S(mode, V, hw):
    """V * T = 768 and 10 240 tiles (below / above 1 024), and ragged images: integers exact and independent of S; every style's image
    against a single-style call with that style's colours"""
    sc, cols, views, deg, use_sh = _problem(mode, V, hw, grid=(64, 64) if hw == (256, 256) else (32, 32))
    singles = [_single(sc, c, views, V, deg, use_sh) for c in cols]
    ref, ref_ws = singles[0]
    assert ref_ws["R"] > 20 * V and (ref_ws["pl"] >> 28).any(), "the scene must fill the lists and set quadrant bits"
    worst = dict(image=0.0, depth=0.0, opacity=0.0, final_T=0.0)
    for S in S_ALL:
        out, ws = _styles(sc, cols[:S], views, V, deg, use_sh)
        assert out.image.shape == (S, V, 3, *hw)
        assert torch.equal(out.radii, ref.radii), f"S={S}: radii"
        assert ws["R"] == ref_ws["R"], f"S={S}: pair count"
        assert np.array_equal(ws["off"], ref_ws["off"]), f"S={S}: tile ranges"
        assert np.array_equal(ws["pl"], ref_ws["pl"]), f"S={S}: sorted list words incl. the quadrant-mask bits"
        assert np.array_equal(ws["nc"], ref_ws["nc"]), f"S={S}: n_contrib"
        worst["depth"] = max(worst["depth"], _rel(out.depth.cpu().numpy(), ref.depth.cpu().numpy()))
        worst["opacity"] = max(worst["opacity"], _rel(out.opacity.cpu().numpy(), ref.opacity.cpu().numpy()))
        worst["final_T"] = max(worst["final_T"], _rel(ws["fT"], ref_ws["fT"]))
        for s in range(S):
            a, b = out.image[s].cpu().numpy(), singles[s][0].image.cpu().numpy()
            worst["image"] = max(worst["image"], _rel(a, b))
            assert_close_rel(a, b, 1e-4, f"S={S}: image of style {s} vs rasterize_views")
    print(f"[styles vs single-style calls] {mode} V={V} {hw}: worst rel " + ", ".join(f"{k} {v:.3e}" for k, v in worst.items()))
    for k in ("depth", "opacity", "final_T"):
        assert worst[k] <= 1e-4, (k, worst[k])


@pytest.mark.parametrize("mode", MODES)
def test_every_style_meets_the_oracle_bar(mode):
    """fp32 CPU oracle once per (view, style) with that style's colours; the fragile-pixel mask comes from geometry only, so it is the
    same for every style and hides no more than in the single-style case"""
    from oracle.gsr_oracle import Oracle
    V, hw = 3, (256, 256)
    sc, cols, views, deg, use_sh = _problem(mode, V, hw)
    H, W = hw
    orc = Oracle("f32")
    vw = views.numpy()
    cov = sc.covariances.numpy()
    cov6 = np.stack([cov[:, 0, 0], cov[:, 0, 1], cov[:, 0, 2], cov[:, 1, 1], cov[:, 1, 2], cov[:, 2, 2]], 1)
    check_views = (0, 2)
    want = {}
    for v in check_views:
        row = vw[v]; s = np.float32(row[56])
        for i, c in enumerate(cols):
            kw = dict(shs=c.numpy()) if use_sh else dict(colors=c.numpy())
            st, _ = orc.forward(sc.means.numpy() * s, cov6 * (s * s), sc.opacities.numpy(), H=H, W=W, tanfovx=row[51], tanfovy=row[52],
                                bg=tuple(row[53:56]), view=row[0:16], proj=row[16:32], proj_raw=row[32:48], campos=row[48:51],
                                sh_degree=deg, nthreads=8, **kw)
            want[v, i] = st
        ok0 = want[v, 0].fragile == 0
        assert ok0.mean() > 0.97
        for i in range(1, POOL):
            ok = want[v, i].fragile == 0
            assert ok.sum() >= ok0.sum() and np.array_equal(ok, ok0), f"view {v}: the mask of style {i} hides other pixels than style 0's"
    single, single_ws = _single(sc, cols[0], views, V, deg, use_sh)
    for S in S_ALL:
        out, ws = _styles(sc, cols[:S], views, V, deg, use_sh)
        for v in check_views:
            st0 = want[v, 0]
            ok = st0.fragile == 0
            assert np.array_equal(out.radii[v].cpu().numpy(), st0.radii), "radii"
            nc = ws["nc"].reshape(V, H, W)[v]
            assert np.array_equal(nc[ok], st0.n_contrib[ok].astype(np.uint32)), "n_contrib"
            assert_close_rel(out.depth[v].cpu().numpy()[ok], st0.out_depth[ok], 1e-4, f"S={S} view {v}: depth")
            assert_close_rel(out.opacity[v].cpu().numpy()[ok], st0.out_opacity[ok], 1e-4, f"S={S} view {v}: opacity")
            assert_close_rel(ws["fT"].reshape(V, H, W)[v][ok], st0.final_T[ok], 1e-4, f"S={S} view {v}: final_T")
            for i in range(S):
                assert_close_rel(out.image[i, v].cpu().numpy()[:, ok], want[v, i].image[:, ok], 1e-4, f"S={S} view {v}: image of style {i}")
    # the single-style call on the same scene sits at the same bar with the same mask
    for v in check_views:
        ok = want[v, 0].fragile == 0
        assert_close_rel(single.image[v].cpu().numpy()[:, ok], want[v, 0].image[:, ok], 1e-4, "single-style image")


@pytest.mark.parametrize("mode", ("sh0", "sh2", "rgb"))
def test_a_style_with_style_0s_colours_renders_image_0_bit_for_bit(mode):
    """catches a mis-indexed colour side array: slots of the first launch (record colour + side array) and of a later one (side array only)"""
    sc, cols, views, deg, use_sh = _problem(mode, 3)
    c0 = cols[0]
    out, _ = _styles(sc, [c0, cols[1], c0.clone(), cols[2], c0.clone(), cols[3], c0.clone()], views, 3, deg, use_sh)     # 7 styles: 4 + 3
    for s in (2, 4, 6):
        assert torch.equal(out.image[s], out.image[0]), f"style {s}"
    assert not torch.equal(out.image[1], out.image[0]) and not torch.equal(out.image[3], out.image[5])
    ref, _ = _single(sc, cols[3], views, 3, deg, use_sh)
    assert_close_rel(out.image[5].cpu().numpy(), ref.image.cpu().numpy(), 1e-4, "style 5")


def test_overflow_grows_the_capacity_and_returns_the_same_images():
    sc, cols, views, deg, use_sh = _problem("sh2", 3, (128, 128), grid=(48, 48))
    key = (1, 3, sc.means.shape[0], 128, 128)
    want, want_ws = _styles(sc, cols[:5], views, 3, deg, use_sh)
    old = rz._CAP_HINT.copy()
    try:
        rz._CAP_HINT[key] = 64                      # far below R: the first attempt overflows
        got, got_ws = _styles(sc, cols[:5], views, 3, deg, use_sh)
        assert got_ws["R"] == want_ws["R"] > 64 and rz._CAP_HINT[key] >= got_ws["R"]
    finally:
        rz._CAP_HINT.clear(); rz._CAP_HINT.update(old)
    assert torch.equal(got.image, want.image) and torch.equal(got.depth, want.depth) and torch.equal(got.opacity, want.opacity)
    assert np.array_equal(got_ws["pl"], want_ws["pl"])


def test_styles_per_launch_flag_changes_the_dispatch_not_the_images(monkeypatch):
    """GSR_FLAG_STYLES_CHUNK_SHIFT: 5 styles as 3 + 2 (default), 2 + 2 + 1, 3 + 2 -- same images"""
    from styl3r_amd import _lib
    sc, cols, views, deg, use_sh = _problem("sh0", 3)
    want, _ = _styles(sc, cols[:5], views, 3, deg, use_sh)
    for per in (2, 3):
        monkeypatch.setattr(rz, "STYLES_EXTRA_FLAGS", per << _lib.GSR_FLAG_STYLES_CHUNK_SHIFT)
        got, _ = _styles(sc, cols[:5], views, 3, deg, use_sh)
        assert torch.equal(got.image, want.image), per


def test_one_style_forwards_to_the_existing_call_and_two_scenes_index_their_own_colours():
    sc, cols, views, deg, use_sh = _problem("sh0", 3)
    one, _ = _styles(sc, cols[:1], views, 3, deg, use_sh)
    ref, _ = _single(sc, cols[0], views, 3, deg, use_sh)
    assert torch.equal(one.image[0], ref.image) and torch.equal(one.depth, ref.depth)
    # b = 2 scenes x 2 views (degree 0: the side array is per scene; degree 2: per view)
    for mode in ("sh0", "sh2"):
        a = _problem(mode, 2, (128, 128), grid=(32, 32), seed=5)
        b = _problem(mode, 2, (128, 128), grid=(32, 32), seed=6)
        d = lambda x, y: torch.stack((x, y)).to(DEV)
        with torch.no_grad():
            out = rz.rasterize_views_styles(d(a[0].means, b[0].means), d(a[0].covariances, b[0].covariances), d(a[0].opacities, b[0].opacities),
                                            [d(x, y) for x, y in zip(a[1][:3], b[1][:3])], torch.cat((a[2], b[2])).to(DEV), (128, 128), 2,
                                            sh_degree=a[3], use_sh=True)
        for k, p in enumerate((a, b)):
            for s in range(3):
                ref, _ = _single(p[0], p[1][s], p[2], 2, p[3], True)
                assert_close_rel(out.image[s, 2 * k:2 * k + 2].cpu().numpy(), ref.image.cpu().numpy(), 1e-4, f"{mode} scene {k} style {s}")


# --------------------------------------------------------------------------- encoder + the serving call
def _tiny_encoder(sh_degree=0):
    from tests.test_encoder import _build
    return deterministic_init_(_build(sh_degree)).to(DEV)


def _tiny_inputs(tag="sh0"):
    from tests.test_encoder import G
    T = lambda k: torch.tensor(G[f"{tag}_{k}"], device=DEV)
    return dict(image=T("image"), intrinsics=T("intrinsics")), dict(image=T("style"))


@pytest.mark.parametrize("linear_mode", ["bf16x6", "f16x3"])
def test_restyle_of_encode_scene_matches_forward_on_the_device(monkeypatch, linear_mode):
    """harmonics at the bar of the tiny-encoder tests in that mode (1e-4 relative: the heads' split-contraction kernels add in atomic order,
    so two runs are not bit-equal); two restyles of one state return the same geometry tensors"""
    from styl3r_amd import vit_ops
    monkeypatch.setattr(vit_ops, "LINEAR_MODE", linear_mode)
    m = _tiny_encoder(1)
    ctx, style = _tiny_inputs("sh1")
    other = dict(image=(style["image"].flip(-1) * 0.5).contiguous())
    with torch.no_grad():
        want, want2 = m(ctx, style, 0), m(ctx, other, 0)
        state = m.encode_scene(ctx, 0)
        got, got2 = m.restyle(state, style), m.restyle(state, other)
        both = m.restyle(m.encode_scene(ctx, 0), dict(image=torch.cat((style["image"], other["image"]))))
    for name in ("means", "covariances", "harmonics", "opacities"):
        assert_close_rel(getattr(got, name).cpu().numpy(), getattr(want, name).cpu().numpy(), 1e-4, f"{linear_mode}: {name}")
    assert_close_rel(got2.harmonics.cpu().numpy(), want2.harmonics.cpu().numpy(), 1e-4, f"{linear_mode}: harmonics, second style")
    for name in ("means", "covariances", "opacities"):
        assert getattr(got2, name) is getattr(got, name) and getattr(both[0], name) is getattr(both[1], name), name
    for i, w in enumerate((want, want2)):
        assert_close_rel(both[i].harmonics.cpu().numpy(), w.harmonics.cpu().numpy(), 1e-4, f"{linear_mode}: batched restyle, style {i}")
    assert (got.harmonics - got2.harmonics).abs().max() > 1e-2 * want.harmonics.abs().max()


def test_stylize_scene_renders_what_per_style_decoder_forwards_render():
    from styl3r_amd.decoder import DecoderSplattingCUDACfg, get_decoder
    from styl3r_amd.inference import stylize_scene
    from styl3r_amd.scenes import recentre_output_heads_
    from tests.helpers import e2e_cameras
    m = _tiny_encoder(1)
    ctx, style = _tiny_inputs("sh1")
    recentre_output_heads_(m, ctx, style)
    dec = get_decoder(DecoderSplattingCUDACfg("splatting_cuda", [0.1, 0.2, 0.3], True)).to(DEV)
    h, w = ctx["image"].shape[-2:]
    s0 = style["image"][0]
    gen = torch.Generator().manual_seed(3)
    # two styles of the fixture's style size, one of the context's size (it shares the identity style's batch), one of a third size
    styles = [s0, (s0.flip(-1) * 0.5).contiguous(), torch.rand(3, h, w, generator=gen).to(DEV), torch.rand(3, 48, 64, generator=gen).to(DEV)]
    target = {k: t.to(DEV) for k, t in e2e_cameras(1).items()}
    target["image_shape"] = (64, 96)
    res = stylize_scene(m, dec, ctx, styles, target, align=None)
    assert res.extrinsics is target["extrinsics"]                                   # align=None: cameras come back unchanged
    assert len(res.gaussians) == 5 and res.color.shape == (5, 1, 2, 3, 64, 96) and res.depth.shape == (1, 2, 64, 96)
    assert all(g.means is res.gaussians[0].means and g.opacities is res.gaussians[0].opacities for g in res.gaussians)
    assert "scales" in res.visualization_dump and "rotations" in res.visualization_dump
    R = rz.LAST_STATS["pairs"]
    assert R > 1000, "the recentred tiny encoder must put Gaussians in front of the cameras"
    with torch.no_grad():
        for i, g in enumerate(res.gaussians):
            ref = dec.forward(g, res.extrinsics, target["intrinsics"], target["near"], target["far"], (64, 96))
            d = _rel(res.color[i].cpu().numpy(), ref.color.cpu().numpy())
            print(f"[stylize_scene] set {i}: colour vs decoder.forward rel {d:.3e}")
            assert_close_rel(res.color[i].cpu().numpy(), ref.color.cpu().numpy(), 1e-4, f"set {i}: colour vs decoder.forward")
            assert_close_rel(res.depth.cpu().numpy(), ref.depth.cpu().numpy(), 1e-4, f"set {i}: depth")
        # the plain set is the encoder's forward with the first context image as style; the stylized ones its forward with that style
        plain = m(ctx, dict(image=ctx["image"][:, 0]), 0)
        assert_close_rel(res.gaussians[0].harmonics.cpu().numpy(), plain.harmonics.cpu().numpy(), 1e-4, "identity-style harmonics")
        for i in (1, 2, 3):
            want = m(ctx, dict(image=styles[i][None]), 0)
            assert_close_rel(res.gaussians[1 + i].harmonics.cpu().numpy(), want.harmonics.cpu().numpy(), 1e-4, f"harmonics of style {i}")
    assert (res.color[1] - res.color[0]).abs().max() > 1e-3 and (res.color[2] - res.color[1]).abs().max() > 1e-3


def test_stylize_scene_aligns_on_the_plain_set_when_asked():
    from styl3r_amd.decoder import DecoderSplattingCUDACfg, get_decoder
    from styl3r_amd.evaluation import TestCfg
    from styl3r_amd.inference import stylize_scene
    from styl3r_amd.losses import LossMse
    from styl3r_amd.scenes import recentre_output_heads_
    from tests.helpers import e2e_cameras
    m = _tiny_encoder(0)
    ctx, style = _tiny_inputs("sh0")
    recentre_output_heads_(m, ctx, style)
    dec = get_decoder(DecoderSplattingCUDACfg("splatting_cuda", [0.0, 0.0, 0.0], True)).to(DEV)
    cams = {k: t.to(DEV) for k, t in e2e_cameras(1).items()}
    first = stylize_scene(m, dec, ctx, style, dict(cams, image_shape=(64, 96)), align=None)
    moved = cams["extrinsics"].clone()
    moved[..., 0, 3] += 0.01
    target = dict(cams, extrinsics=moved, image=first.color[0].contiguous())          # ground truth: the plain render from the true cameras
    res = stylize_scene(m, dec, ctx, style, target, align=TestCfg(pose_align_steps=20, rot_opt_lr=5e-4, trans_opt_lr=5e-4), losses=[LossMse()])
    assert res.extrinsics is not moved and not torch.equal(res.extrinsics, moved)
    # the alignment ran on the plain set: its render from the returned cameras is closer to the ground truth than from the moved ones
    with torch.no_grad():
        before = dec.forward(res.gaussians[0], moved, cams["intrinsics"], cams["near"], cams["far"], (64, 96)).color
    mse = lambda x: float(((x - target["image"]) ** 2).mean())
    print(f"[stylize_scene align] plain-render mse {mse(before):.4g} -> {mse(res.color[0]):.4g}")
    assert mse(res.color[0]) < mse(before)
    assert res.color.shape == (2, 1, 2, 3, 64, 96)
