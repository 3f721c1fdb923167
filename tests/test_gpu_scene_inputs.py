"""-m gpu: the kernels of csrc/gsr_inputs.hip (k_resample_h, k_resample_v behind gsr_resample_crop) through styl3r_amd/inputs.py, bit
for bit against the reference's PIL results (tests/golden/scene_inputs.npz) and against the host path of the same module (which
tests/test_scene_inputs_host.py holds to the same fixtures), and `prepare_example` / `prepare_scene` end to end on a tiny encoder.
Every comparison is of int32 views: there is no tolerance anywhere in this file."""
import numpy as np
import pytest
import torch

from styl3r_amd import _lib
from styl3r_amd import inputs as si
from tests.test_scene_inputs_host import G, IMAGE_CASES, T, camera_example, case_input, run_case, same_bits

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


@pytest.mark.parametrize("flags", [0, _lib.GSR_RESAMPLE_DIRECT], ids=["staged", "direct"])
@pytest.mark.parametrize("key", IMAGE_CASES)
def test_every_fixture_case_on_the_device(key, flags):
    """float and byte input, the LDS-staged horizontal pass and the direct one (the path of supports too large for the LDS budget):
    all of them the fixture's bits, intrinsics included"""
    x = case_input(key)
    img, K = run_case(key, x.to(DEV), flags)
    assert img.is_cuda and img.dtype == torch.float32 and same_bits(img, G[key + "_ref"]), key
    assert same_bits(img, run_case(key, x)[0])                                      # the host path
    if K is not None:
        assert same_bits(K, G[key + "_K_ref"])
    raw = T(key + "_in")
    if raw.dtype == torch.uint8:
        assert same_bits(run_case(key, raw.to(DEV), flags)[0], G[key + "_ref"]), key


def test_batch_with_flips_equals_the_single_image_calls_and_repeats_itself():
    frames, K = T("flip_frames").to(DEV), T("flip_K").to(DEV)
    flips = [False, True, False]
    for src in (frames, frames.permute(0, 3, 1, 2).float() / 255):
        batch, Kb = si.rescale_and_crop(src, K, (16, 16), flip=flips)
        again, _ = si.rescale_and_crop(src, K, (16, 16), flip=flips)
        assert same_bits(batch, again)                                             # two identical calls
        for n in range(3):
            one, _ = si.rescale_and_crop(src[n:n + 1], K[n:n + 1], (16, 16), flip=flips[n:n + 1])
            assert same_bits(one[0], batch[n]), n                                  # image n does not depend on N
        assert same_bits(batch[0], G["flip_plain_ref"][0]) and same_bits(batch[2], G["flip_plain_ref"][2])
        assert same_bits(batch[1], G["flip_mirrored_ref"][1]) and same_bits(Kb, G["flip_K_ref"])
        assert same_bits(si.rescale_and_crop(src, K, (16, 16), flip=True)[0], G["flip_mirrored_ref"])


# shapes the fixtures do not reach: several column blocks, a row count that is no multiple of the block's four rows, a window away from
# the border, and a segment that outgrows the LDS budget by itself (256 columns at 6:1 span 1572 source pixels x 4 rows x 3 bytes)
@pytest.mark.parametrize("hw,scaled,window", [((9, 700), (9, 520), None), ((23, 300), (11, 300), (3, 17, 5, 270)), ((7, 1800), (5, 300), None),
                                              ((50, 70), (31, 333), (2, 30, 27, 290))])
def test_block_edges_and_the_lds_budget_against_the_host_path(hw, scaled, window):
    g = torch.Generator().manual_seed(hw[0] * 1000 + hw[1])
    frames = torch.randint(0, 256, (2, *hw, 3), generator=g, dtype=torch.uint8)
    frames[1, :, ::2] = 255
    frames[1, ::3] = 255 - frames[1, ::3]
    want = si.resample_crop(frames, scaled, window, flip=[True, False])
    assert same_bits(si.resample_crop(frames.to(DEV), scaled, window, flip=[True, False]), want)
    assert same_bits(si.resample_crop(frames.to(DEV), scaled, window, flip=[True, False], flags=_lib.GSR_RESAMPLE_DIRECT), want)
    planes = frames.permute(0, 3, 1, 2).float() / 255
    assert same_bits(si.resample_crop(planes.to(DEV), scaled, window, flip=[True, False]), want)


def test_float_quantisation_on_the_device():
    x = torch.tensor([-0.5, 0.0, 0.999 / 255, 1.0 / 255, 0.5, 1.0, 1.7, float("nan"), float("inf"), -float("inf")])
    x = torch.cat([x, torch.arange(256).float() / 255, torch.zeros(22)]).reshape(1, 1, 12, 24).expand(1, 3, 12, 24)
    want = si.rescale(x, (12, 24))
    assert same_bits(si.rescale(x.to(DEV), (12, 24)), want)
    assert same_bits(want[0, 0].reshape(-1)[10:266], (torch.arange(256).double() / 255).float())


def test_rejected_arguments_launch_nothing():
    frames = T("flip_frames").to(DEV)
    with pytest.raises(ValueError):
        si.resample_crop(frames, (16, 23), (0, 8, 16, 16))
    with pytest.raises(ValueError):
        si.resample_crop(frames, (16, 23), flip=[True])


@pytest.mark.parametrize("tag", ["norm", "pixel_flip"])
def test_prepare_example_on_the_device_equals_the_host_path(tag):
    host, _, _ = camera_example(tag)
    for ex in (camera_example(tag, device=DEV)[0], camera_example(tag, frames_on=DEV)[0]):       # bytes uploaded by the call / already there
        for name in ("context", "target"):
            for field, want in host[name].items():
                got = ex[name][field]
                assert got.is_cuda and got.dtype == want.dtype, (name, field)
                assert torch.equal(got.cpu(), want) if field == "index" else same_bits(got, want), (name, field)
        assert same_bits(ex["style"]["image"], host["style"]["image"]) and ex["scene"] == tag


def test_prepare_scene_feeds_stylize_scene_the_host_prepared_batch():
    """Every tensor `prepare_scene` hands to `stylize_scene` -- context and target images, cameras, near / far, the style images -- is
    bit-equal between the device path and the host path, and `stylize_scene` runs on the device-prepared batch.

    The OUTPUTS of the two `stylize_scene` calls cannot be compared bit for bit: the encoder does not repeat itself on one and the same
    batch.  Measured on an MI355X with this test's inputs, three calls on the identical device-prepared batch: means, covariances,
    harmonics and opacities of every Gaussian set differ in their last bits, colours by 7.1e-6 and 6.5e-6 (default linear mode, whose
    split-K tiles are summed with fp32 atomics, csrc/vit_gemm_x6.hip) and by 1.2e-5 and 9.6e-6 in the "f32" linear mode.  Bit equality
    of the inputs is therefore the whole statement about this module; the outputs are held to the bar this suite uses for renders whose
    sums may be reordered (1e-4 of a colour range of 1: tests/test_gpu_styles.py, smoke()), and their distance is printed."""
    from styl3r_amd.decoder import DecoderSplattingCUDACfg, get_decoder
    from styl3r_amd.inference import prepare_scene, stylize_scene
    from styl3r_amd.scenes import recentre_output_heads_
    from tests.helpers import deterministic_init_, e2e_cameras
    from tests.test_encoder import _build
    m = deterministic_init_(_build(1)).to(DEV)
    g = torch.Generator().manual_seed(11)
    frames = torch.randint(0, 256, (4, 37, 53, 3), generator=g, dtype=torch.uint8)
    styles = [torch.randint(0, 256, (40, 61, 3), generator=g, dtype=torch.uint8), torch.rand(3, 50, 33, generator=g)]
    cams = e2e_cameras(1)
    c2w = torch.stack([cams["extrinsics"][0, 0], cams["extrinsics"][0, 1], cams["extrinsics"][0, 1] @ cams["extrinsics"][0, 1],
                       cams["extrinsics"][0, 1].inverse()])
    K = cams["intrinsics"][0, [0, 1, 0, 1]]
    cfg = si.InputCfg(input_image_shape=(32, 32), style_size=32, near=0.5)
    args = (K, c2w, [0, 1], [2, 3, 0])
    hctx, hstyles, htgt = prepare_scene(frames, *args, styles, cfg)
    ctx, sty, tgt = prepare_scene(frames, *args, styles, cfg, device=DEV)
    assert ctx["image"].shape == (1, 2, 3, 32, 32) and tgt["image"].shape == (1, 3, 3, 32, 32) and ctx["image"].is_cuda
    assert [tuple(s.shape) for s in sty] == [(3, 32, 32)] * 2
    for a, b in ((ctx, hctx), (tgt, htgt)):
        assert a.keys() == b.keys()
        for k in ("image", "extrinsics", "intrinsics", "near", "far"):
            assert a[k].is_cuda and same_bits(a[k], b[k]), k
        assert torch.equal(a["index"].cpu(), b["index"])
    assert all(same_bits(a, b) for a, b in zip(sty, hstyles))
    moved = lambda d: {k: v.to(DEV) for k, v in d.items()}
    recentre_output_heads_(m, ctx, dict(image=sty[0][None]))
    dec = get_decoder(DecoderSplattingCUDACfg("splatting_cuda", [0.1, 0.2, 0.3], True)).to(DEV)
    scene = stylize_scene(m, dec, ctx, sty, tgt)
    want = stylize_scene(m, dec, moved(hctx), [s.to(DEV) for s in hstyles], moved(htgt))
    assert scene.color.shape == (3, 1, 3, 3, 32, 32) and same_bits(scene.extrinsics, want.extrinsics)
    assert float((scene.color[0, 0] - torch.tensor([0.1, 0.2, 0.3], device=DEV)[:, None, None]).abs().max()) > 1e-2, "nothing was rendered"
    dist = float((scene.color - want.color).abs().max())
    print(f"[prepare_scene -> stylize_scene] colours of the device-prepared and the host-prepared batch differ by {dist:.3e}")
    assert dist <= 1e-4
