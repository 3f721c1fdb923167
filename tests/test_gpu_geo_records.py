"""-m gpu: the dense geometry array beside the splat records (include/gsr.h GsrLayout.geo, round 15).

K1 writes `geo[vg]` = the first 16 bytes of `records[vg]` (x, y, depth, radius + clamp flags); the scatter kernels (K3, LDS and
ballot form) and the preprocess backward (K7) stream it instead of striding through the 48-byte records, and K7 forms the conic
from its own geom_eval and takes the opacity from the forward's per-Gaussian copy (GsrLayout.opac).  Checked here on 2 scenes x 3
views of a ragged 50 x 70 image (4 x 5 tiles): the copy bit for bit, the tile ranges and sorted lists against the oracle under both
binning forms, every gradient at the project's bar (<= 1e-4 of the fp32 oracle, max-norm); and on a one-tile scene
in which every gradient address has one adder: two backward calls bit-identical."""
import numpy as np
import pytest
import torch

from styl3r_amd import _lib
from styl3r_amd import rasterizer as rz
from tests.gpu_utils import assert_close_rel, ws_view

pytestmark = pytest.mark.gpu

B, VT, G, H, W = 2, 3, 1500, 50, 70
T = ((W + 15) // 16) * ((H + 15) // 16)


@pytest.fixture(autouse=True)
def _debug_on():
    rz.KEEP_DEBUG = True
    yield
    rz.KEEP_DEBUG = False
    rz.LAST_DEBUG.clear()


def _scenes():
    """2 scenes of 30 x 50 Gaussians, SH degree 1: harmonics scaled so that channels clamp at 0, every fifth Gaussian moved behind
    the cameras and every seventh far off screen (radius 0)"""
    from styl3r_amd.scenes import make_scene
    scs = [make_scene(n_ctx=1, grid_hw=(30, 50), n_views=VT, image_hw=(H, W), sh_degree=1, seed=1500 + i) for i in range(B)]
    for sc in scs:
        sc.harmonics.mul_(3.0)
        sc.means[::5, 2] = -sc.means[::5, 2]
        sc.means[::7, 0] += 40.0
    return scs


def _view_cam(sc, views, i):
    row = views[i]; s = np.float32(row[56])
    cov = sc.covariances.numpy()
    cov6 = np.stack([cov[:, 0, 0], cov[:, 0, 1], cov[:, 0, 2], cov[:, 1, 1], cov[:, 1, 2], cov[:, 2, 2]], 1) * (s * s)
    cam = dict(tanfovx=row[51], tanfovy=row[52], view=row[0:16].reshape(4, 4), proj=row[16:32].reshape(4, 4),
               proj_raw=row[32:48].reshape(4, 4), campos=row[48:51])
    return s, np.float32(cov6), cam


@pytest.fixture(scope="module")
def reference():
    """the fp32 oracle's forward state per (scene, view) and its gradients summed over a scene's views: computed once, read only"""
    from oracle.gsr_oracle import Oracle
    from styl3r_amd.decoder import prepare_views
    dev = torch.device("cuda:0")
    scs = _scenes()
    rng = np.random.default_rng(15)
    wI = rng.normal(size=(B, VT, 3, H, W)).astype(np.float32)
    wD = (0.3 * rng.normal(size=(B, VT, H, W))).astype(np.float32)
    orc = Oracle("f32")
    states, grads = [], []
    for b, sc in enumerate(scs):
        # the cameras as the decoder builds them with torch_view_setup: the same op sequence on the same device
        views = prepare_views(sc.extrinsics.to(dev), sc.intrinsics.to(dev), sc.near.to(dev), sc.far.to(dev),
                              torch.tensor([[0.2, 0.1, 0.3]], device=dev).expand(VT, 3), True).cpu().numpy()
        acc = dict(means=np.zeros((G, 3)), cov=np.zeros((G, 3, 3)), sh=np.zeros((G, 3, 4)), opac=np.zeros(G))
        for v in range(VT):
            s, cov6, cam = _view_cam(sc, views, v)
            st, ctx = orc.forward(np.float32(sc.means.numpy() * s), cov6, sc.opacities.numpy(), shs=sc.harmonics.numpy().transpose(0, 2, 1),
                                  H=H, W=W, bg=(0.2, 0.1, 0.3), sh_degree=1, nthreads=8, **cam)
            gr = orc.backward(st, ctx, wI[b, v], wD[b, v], nthreads=8)
            acc["means"] += gr["means3D"] * s
            r, c = np.triu_indices(3)
            acc["cov"][:, r, c] += gr["cov6"] * (s * s)
            acc["sh"] += gr["shs"].transpose(0, 2, 1)
            acc["opac"] += gr["opacities"]
            states.append(st)
        grads.append(acc)
    for a in grads:
        for x in a.values():
            x.setflags(write=False)
    return dict(scenes=scs, wI=wI, wD=wD, states=states, grads=grads)


def _run(ref):
    from styl3r_amd.decoder import DecoderSplattingCUDACfg, Gaussians, get_decoder
    dev = torch.device("cuda:0")
    st = lambda n: torch.stack([getattr(sc, n) for sc in ref["scenes"]]).to(dev)
    g = Gaussians(*(st(n).requires_grad_(True) for n in ("means", "covariances", "harmonics", "opacities")))
    dec = get_decoder(DecoderSplattingCUDACfg("splatting_cuda", [0.2, 0.1, 0.3], True)).to(dev)
    dec.torch_view_setup = True
    out = dec.forward(g, st("extrinsics"), st("intrinsics"), st("near"), st("far"), (H, W))
    return g, out


def _check_workspace(ref):
    V = B * VT
    recs = ws_view("records", np.uint32, V * G * 12).reshape(V * G, 12)
    geo = ws_view("geo", np.uint32, V * G * 4).reshape(V * G, 4)
    assert np.array_equal(geo, recs[:, 0:4]), "geo != first 16 bytes of the records"
    rad = geo[:, 3] & 0xFFFFFF
    assert (rad == 0).any() and (rad > 0).any() and ((geo[:, 3] >> 24) != 0).any(), "the scene must hold culled, visible and colour-clamped entries"
    assert not geo[rad == 0].any(), "culled entries are all-zero"
    sg = np.concatenate([sc.opacities.numpy() for sc in ref["scenes"]])
    assert np.array_equal(ws_view("opac", np.float32, B * G), sg), "the backward's opacity copy"
    off = ws_view("tile_offset", np.uint32, V * T + 1).astype(np.int64)
    pl = ws_view("point_list", np.uint32, int(off[-1])) & np.uint32(_lib.GSR_ID_MASK)
    assert off[0] == 0 and off[-1] == rz.LAST_DEBUG["num_pairs"] == sum(s.R for s in ref["states"])
    for v, st in enumerate(ref["states"]):
        o = off[v * T:(v + 1) * T + 1]
        assert np.array_equal(np.diff(o), st.ranges[:, 1] - st.ranges[:, 0]), f"view {v}: tile ranges"
        assert np.array_equal(pl[o[0]:o[-1]], st.point_list.astype(np.uint32)), f"view {v}: sorted (tile, id) lists"


@pytest.mark.parametrize("ballot", [False, True], ids=["lds", "ballot"])
def test_geo_is_the_record_head_and_lists_and_gradients_match_the_oracle(reference, ballot, monkeypatch):
    if ballot:
        monkeypatch.setattr(rz, "EXTRA_FLAGS", _lib.GSR_FLAG_BIN_BALLOT)
    dev = torch.device("cuda:0")
    g, out = _run(reference)
    _check_workspace(reference)
    loss = (out.color * torch.tensor(reference["wI"], device=dev)).sum() + (out.depth * torch.tensor(reference["wD"], device=dev)).sum()
    loss.backward()
    for b in range(B):
        acc = reference["grads"][b]
        for name, t in (("means", g.means), ("cov", g.covariances), ("sh", g.harmonics), ("opac", g.opacities)):
            got = t.grad[b].cpu().numpy()
            assert np.isfinite(got).all(), name
            assert_close_rel(got, acc[name], 1e-4, f"scene {b} d{name} vs f32 oracle ({VT} views summed)")


def test_one_tile_scene_backward_is_bit_reproducible():
    """16 x 16 image, 48 Gaussians: one tile and one depth segment per view, so every gradient address has a single adder and nothing
    depends on the order in which atomics arrive.  Two backward calls through the same graph must agree bit for bit."""
    from styl3r_amd.decoder import DecoderSplattingCUDACfg, Gaussians, get_decoder
    from styl3r_amd.scenes import make_scene
    dev = torch.device("cuda:0")
    sc = make_scene(n_ctx=1, grid_hw=(6, 8), n_views=2, image_hw=(16, 16), sh_degree=1, seed=16)
    ex = lambda n: getattr(sc, n)[None].to(dev)
    g = Gaussians(*(ex(n).requires_grad_(True) for n in ("means", "covariances", "harmonics", "opacities")))
    dec = get_decoder(DecoderSplattingCUDACfg("splatting_cuda", [0.2, 0.1, 0.3], True)).to(dev)
    out = dec.forward(g, ex("extrinsics"), ex("intrinsics"), ex("near"), ex("far"), (16, 16))
    assert rz.LAST_DEBUG["num_pairs"] > 0 and int(rz.LAST_DEBUG["status"][2]) <= 48
    gen = torch.Generator(dev).manual_seed(3)
    loss = (out.color * torch.randn(out.color.shape, device=dev, generator=gen)).sum() + \
           (out.depth * torch.randn(out.depth.shape, device=dev, generator=gen)).sum()
    leaves = (g.means, g.covariances, g.harmonics, g.opacities)
    first = torch.autograd.grad(loss, leaves, retain_graph=True)
    second = torch.autograd.grad(loss, leaves)
    for x, y, name in zip(first, second, ("means", "cov", "sh", "opac")):
        assert x.abs().sum() > 0, name
        assert torch.equal(x, y), f"d{name}: two backward calls differ"
