"""-m gpu: the composite backward's nine-value reduction through the LDS (gsr_common.h wave_reduce9_lds, DESIGN R17) and the swap form
kept behind GSR_FLAG_K6_SWAP_SUM.

1. gsr_test_reduce9 on small integers (every sum exact in fp32): the totals of both forms equal numpy's bit for bit, for one and for
   five reductions back to back (the second reduction's stores follow the first one's loads in the same 2 KiB) and for 1 and 96 workgroups.
2. Every gradient of the depth-free kernel against the fp32 oracle at the project's bar (<= 1e-4 of the largest gradient, max-norm,
   tests/gpu_utils.assert_close_rel) under both forms: 2 scenes x 3 views of the ragged 50 x 70 image of tests/test_gpu_geo_records.py
   (culled and colour-clamped Gaussians), with a plain colour gradient, with the fused MSE, and with 64-entry depth segments on lists of
   more than three segments (checkpoint-started segments).
3. A one-tile scene (one adder per gradient address): two backward calls bit-identical under each form.
4. The occupancy the runtime computes for both instantiations: 32 single-wave workgroups per CU (8 waves per SIMD)."""
import ctypes as C

import numpy as np
import pytest
import torch

from styl3r_amd import _lib
from styl3r_amd import rasterizer as rz
from tests.gpu_utils import assert_close_rel, ws_view
from tests.test_gpu_geo_records import B, G, H, VT, W, _scenes, _view_cam

pytestmark = pytest.mark.gpu

VARIANTS = {"lds": 0, "swap": _lib.GSR_FLAG_K6_SWAP_SUM}
BG = (0.2, 0.1, 0.3)
MSE_WEIGHT = 0.7


@pytest.fixture(autouse=True)
def _debug_on():
    rz.KEEP_DEBUG = True
    yield
    rz.KEEP_DEBUG = False
    rz.LAST_DEBUG.clear()


# ---------------------------------------------------------------- 1. the reduction alone
@pytest.mark.parametrize("variant", [0, 1], ids=["lds", "swap"])
@pytest.mark.parametrize("blocks", [1, 96])
@pytest.mark.parametrize("rounds", [1, 5])
def test_reduce9_totals_are_exact(rounds, blocks, variant):
    lib = _lib.load()
    rng = np.random.default_rng(100 * rounds + blocks)
    # distinct integers per (round, value, lane), another set per workgroup; |x| < 2^18, so every partial sum of 64 of them is exact
    x = np.stack([rng.permutation(rounds * 9 * 64) + 1 + 1000 * b for b in range(blocks)]).reshape(blocks, rounds, 9, 64)
    x = (x * np.where(rng.random(x.shape) < 0.5, -1, 1)).astype(np.float32)
    want = x.astype(np.float64).sum(-1).astype(np.float32)
    dev = torch.device("cuda:0")
    xin = torch.tensor(x, device=dev)
    out = torch.full((blocks, rounds, 9), float("nan"), device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    _lib.check(lib.gsr_test_reduce9(xin.data_ptr(), out.data_ptr(), rounds, blocks, variant, C.c_void_p(stream)), "gsr_test_reduce9")
    got = out.cpu().numpy()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), np.argwhere(got != want)[:8]


def test_reduce9_rejects_bad_arguments():
    lib = _lib.load()
    buf = torch.zeros(9 * 64, device="cuda:0")
    for rounds, blocks, variant in ((0, 1, 0), (1, 0, 0), (1, 1, 2)):
        assert lib.gsr_test_reduce9(buf.data_ptr(), buf.data_ptr(), rounds, blocks, variant, None) == -1
    assert lib.gsr_test_reduce9(None, buf.data_ptr(), 1, 1, 0, None) == -1


# ---------------------------------------------------------------- 4. occupancy
@pytest.mark.parametrize("variant", [0, 1], ids=["lds", "swap"])
def test_k6_blocks_per_cu(variant):
    """8 waves per SIMD: <= 64 VGPRs, and 32 x 5 120 B of LDS is exactly the CU's 160 KiB"""
    assert _lib.load().gsr_k6_blocks_per_cu(variant) == 32


# ---------------------------------------------------------------- 2. gradients against the oracle
@pytest.fixture(scope="module")
def reference():
    """the fp32 oracle's gradients, summed over a scene's views, for (a) a plain colour gradient and (b) the MSE against a target --
    dL/dimage = 2 weight / n (image - target), n over the whole batch, from the oracle's own image.  Computed once, read only."""
    from oracle.gsr_oracle import Oracle
    from styl3r_amd.decoder import prepare_views
    dev = torch.device("cuda:0")
    scs = _scenes()
    rng = np.random.default_rng(17)
    wI = rng.normal(size=(B, VT, 3, H, W)).astype(np.float32)
    target = rng.uniform(size=(B, VT, 3, H, W)).astype(np.float32)
    n = B * VT * 3 * H * W
    orc = Oracle("f32")
    grads = {"colour": [], "mse": []}
    longest = 0
    for b, sc in enumerate(scs):
        views = prepare_views(sc.extrinsics.to(dev), sc.intrinsics.to(dev), sc.near.to(dev), sc.far.to(dev),
                              torch.tensor([list(BG)], device=dev).expand(VT, 3), True).cpu().numpy()
        acc = {k: dict(means=np.zeros((G, 3)), cov=np.zeros((G, 3, 3)), sh=np.zeros((G, 3, 4)), opac=np.zeros(G)) for k in grads}
        for v in range(VT):
            s, cov6, cam = _view_cam(sc, views, v)
            st, ctx = orc.forward(np.float32(sc.means.numpy() * s), cov6, sc.opacities.numpy(), shs=sc.harmonics.numpy().transpose(0, 2, 1),
                                  H=H, W=W, bg=BG, sh_degree=1, nthreads=8, **cam)
            longest = max(longest, int((st.ranges[:, 1] - st.ranges[:, 0]).max()))
            gI = {"colour": wI[b, v], "mse": np.float32(2.0 * MSE_WEIGHT / n) * (st.image.astype(np.float32) - target[b, v])}
            for k in grads:
                gr = orc.backward(st, ctx, gI[k], None, nthreads=8)
                a = acc[k]
                a["means"] += gr["means3D"] * s
                r, c = np.triu_indices(3)
                a["cov"][:, r, c] += gr["cov6"] * (s * s)
                a["sh"] += gr["shs"].transpose(0, 2, 1)
                a["opac"] += gr["opacities"]
        for k in grads:
            for x in acc[k].values():
                x.setflags(write=False)
            grads[k].append(acc[k])
    return dict(scenes=scs, wI=wI, target=target, grads=grads, longest=longest)


def _gpu_grads(ref, loss_kind):
    from styl3r_amd.decoder import DecoderSplattingCUDACfg, Gaussians, get_decoder
    dev = torch.device("cuda:0")
    st = lambda n: torch.stack([getattr(sc, n) for sc in ref["scenes"]]).to(dev)
    g = Gaussians(*(st(n).requires_grad_(True) for n in ("means", "covariances", "harmonics", "opacities")))
    dec = get_decoder(DecoderSplattingCUDACfg("splatting_cuda", list(BG), True)).to(dev)
    dec.torch_view_setup = True
    args = (g, st("extrinsics"), st("intrinsics"), st("near"), st("far"), (H, W))
    if loss_kind == "mse":
        loss = dec.forward(*args, mse_target=torch.tensor(ref["target"], device=dev), mse_weight=MSE_WEIGHT).loss_mse
    else:
        loss = (dec.forward(*args).color * torch.tensor(ref["wI"], device=dev)).sum()
    loss.backward()       # no depth gradient: the nine-value kernel
    return g


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("case", ["colour", "mse", "colour-seg64", "mse-seg64"])
def test_every_gradient_matches_the_oracle_under_both_reductions(reference, variant, case, monkeypatch):
    loss_kind, _, seg = case.partition("-")
    flags = VARIANTS[variant] | ((1 << _lib.GSR_FLAG_SEG_SHIFT) if seg else 0)
    monkeypatch.setattr(rz, "EXTRA_FLAGS", flags)
    g = _gpu_grads(reference, loss_kind)
    if seg:      # lists of more than three 64-entry segments whose contributors reach into the fourth: segments started from checkpoints
        assert reference["longest"] > 192 and int(rz.LAST_DEBUG["status"][2]) == reference["longest"]
        assert int(ws_view("n_contrib", np.uint32, B * VT * H * W).max()) > 192
    for b in range(B):
        acc = reference["grads"][loss_kind][b]
        for name, t in (("means", g.means), ("cov", g.covariances), ("sh", g.harmonics), ("opac", g.opacities)):
            got = t.grad[b].cpu().numpy()
            assert np.isfinite(got).all() and np.abs(got).max() > 0, name
            assert_close_rel(got, acc[name], 1e-4, f"{variant} {case}: scene {b} d{name} vs f32 oracle ({VT} views summed)")


# ---------------------------------------------------------------- 3. determinism
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_one_tile_scene_backward_is_bit_reproducible(variant, monkeypatch):
    """16 x 16 image, 48 Gaussians, colour gradient only: one tile and one depth segment per view, a single adder per gradient address"""
    from styl3r_amd.decoder import DecoderSplattingCUDACfg, Gaussians, get_decoder
    from styl3r_amd.scenes import make_scene
    monkeypatch.setattr(rz, "EXTRA_FLAGS", VARIANTS[variant])
    dev = torch.device("cuda:0")
    sc = make_scene(n_ctx=1, grid_hw=(6, 8), n_views=2, image_hw=(16, 16), sh_degree=1, seed=16)
    ex = lambda n: getattr(sc, n)[None].to(dev)
    g = Gaussians(*(ex(n).requires_grad_(True) for n in ("means", "covariances", "harmonics", "opacities")))
    dec = get_decoder(DecoderSplattingCUDACfg("splatting_cuda", list(BG), True)).to(dev)
    out = dec.forward(g, ex("extrinsics"), ex("intrinsics"), ex("near"), ex("far"), (16, 16))
    assert rz.LAST_DEBUG["num_pairs"] > 0 and int(rz.LAST_DEBUG["status"][2]) <= 48
    gen = torch.Generator(dev).manual_seed(3)
    loss = (out.color * torch.randn(out.color.shape, device=dev, generator=gen)).sum()
    leaves = (g.means, g.covariances, g.harmonics, g.opacities)
    first = torch.autograd.grad(loss, leaves, retain_graph=True)
    second = torch.autograd.grad(loss, leaves)
    for x, y, name in zip(first, second, ("means", "cov", "sh", "opac")):
        assert x.abs().sum() > 0, name
        assert torch.equal(x, y), f"d{name}: two backward calls differ"
