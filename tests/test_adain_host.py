"""The 2D-AdaIN baseline without a GPU (styl3r_amd/baseline.py, the baseline column of styl3r_amd/visualization.py): the key layout, the
float64 expression against tests/golden/adain_ref.npz (the reference's AdaIN2D.generate + vgg_denorm in float64,
tests/golden/make_adain_fixtures.py), the C ABI's exports and argument errors, and the pictures' layout.  GPU side: tests/test_gpu_adain.py."""
import ctypes as C
import functools
from pathlib import Path

import numpy as np
import pytest
import torch

from styl3r_amd import baseline, losses
from styl3r_amd import visualization as vis
from tests import adain_inputs as ai
from tests.vis_common import camera_inputs

ROOT = Path(__file__).resolve().parents[1]
EINVAL = -1
RELU_IN, GATE, REFLECT, UP2 = 1, 2, 4, 8


@functools.lru_cache(maxsize=None)
def fixture():
    return dict(np.load(ROOT / "tests/golden/adain_ref.npz"))


@functools.lru_cache(maxsize=None)
def model64():
    m = baseline.AdaIN2D()
    m.load_state_dict(ai.reference_state_dict(), strict=True)
    return m.double()


def rel(a, b):
    return float((a - b).abs().max() / b.abs().max())


def test_state_dict_has_the_references_keys_and_shapes():
    f = fixture()
    sd = baseline.AdaIN2D().state_dict()
    assert list(sd) == [str(k) for k in f["keys"]]
    assert [";".join(map(str, v.shape)) for v in sd.values()] == [str(s) for s in f["shapes"]]
    assert set(sd) == set(ai.reference_state_dict())
    m = baseline.AdaIN2D()
    assert list(m.parameters()) == [] and len(list(m.buffers())) == 36 + 2           # buffers only (+ the two de-normalisation constants)


def test_the_references_layout_loads_strictly_and_wrong_keys_are_refused():
    sd = ai.reference_state_dict()
    m = baseline.AdaIN2D()
    m.load_state_dict(sd, strict=True)
    assert torch.equal(m.vgg_encoder.features[19].weight, sd["vgg_encoder.slice4.19.weight"])
    assert torch.equal(m.decoder.rc9.conv.bias, sd["decoder.rc9.conv.bias"])
    assert all(torch.equal(v, sd[k]) for k, v in m.state_dict().items())                 # round trip under the reference's names
    wrong = {("vgg_encoder.slice3.19.weight" if k == "vgg_encoder.slice4.19.weight" else k): v for k, v in sd.items()}
    with pytest.raises(RuntimeError, match="slice3.19.weight"):
        baseline.AdaIN2D().load_state_dict(wrong, strict=True)
    with pytest.raises(RuntimeError, match="Missing"):
        baseline.AdaIN2D().load_state_dict({k: v for k, v in sd.items() if k != "decoder.rc4.conv.bias"}, strict=True)


@pytest.mark.parametrize("scene", sorted(ai.SCENES))
def test_expression_in_float64_matches_the_reference(scene):
    """the same arithmetic restated: 1e-12 relative (max abs error over max abs of the reference) at every stage"""
    f, m = fixture(), model64()
    target, style = (torch.from_numpy(f[f"{scene}_{k}"]).double() for k in ("images", "style"))
    assert torch.equal(target.float(), ai.images(scene)[0]) and torch.equal(style.float(), ai.images(scene)[1])
    x, s = losses._imagenet_normalize(target), losses._imagenet_normalize(style[None])
    index = torch.zeros(target.shape[0], dtype=torch.int32)
    calls = dict(baseline.CALLS)
    with torch.no_grad():
        fc, fs = m.vgg_encoder(x, output_last_feature=True), m.vgg_encoder(s, output_last_feature=True)
        assert rel(fc, torch.from_numpy(f[f"{scene}_relu41_content"])) <= 1e-12 and rel(fs, torch.from_numpy(f[f"{scene}_relu41_style"])) <= 1e-12
        t = baseline.adain(fc, fs, 1.0, index)
        assert rel(t, torch.from_numpy(f[f"{scene}_adain"])) <= 1e-12
        assert rel(m.generate(x, s, 1.0, style_index=index), torch.from_numpy(f[f"{scene}_raw"])) <= 1e-12
        assert rel(m.generate(x, s.repeat(x.shape[0], 1, 1, 1), 1), torch.from_numpy(f[f"{scene}_raw"])) <= 1e-12       # the reference's signature
        assert rel(m.generate(x, s, 0.3, style_index=index), torch.from_numpy(f[f"{scene}_raw_alpha03"])) <= 1e-12
        final = m.stylize(target, style)
        assert rel(final, torch.from_numpy(f[f"{scene}_final"])) <= 1e-12
        assert float(final.min()) >= 0 and float(final.max()) <= 1
    assert baseline.CALLS["adain2d_expression"] == calls["adain2d_expression"] + 4          # CPU tensors take the expression
    assert all(baseline.CALLS[k] == calls[k] for k in ("adain_hip", "conv_rc_x6", "conv_rgb_hip"))


def test_fixture_conditions_hold():
    """what the generator asserted: no near-dead content channel at relu4_1, and the clamp cannot hide an error"""
    f = fixture()
    for scene in ai.SCENES:
        fc = torch.from_numpy(f[f"{scene}_relu41_content"])
        assert float(fc.flatten(2).std(-1).min()) >= 1e-3 * float(fc.abs().max())
        pre = f[f"{scene}_preclamp"]
        assert ((pre > 0) & (pre < 1)).mean() >= 0.25
        assert fc.shape[-2:] == {"A": (2, 2), "B": (3, 5)}[scene]


def test_adain_expression_is_the_references_formula_and_refuses_single_positions():
    c, s = ai.adain_case(1, 3, 2, 8, 6, 5)
    c, s = c.double(), s.double()
    index = torch.tensor([0, 1, 1])
    got = baseline.adain(c, s, 0.3, index)
    cm, cs = c.mean(-1, keepdim=True), c.std(-1, keepdim=True) + 1e-8
    sm, ss = s[index].mean(-1, keepdim=True), s[index].std(-1, keepdim=True) + 1e-8
    want = 0.3 * (ss * (c - cm) / cs + sm) + (1 - 0.3) * c
    assert torch.equal(got, want)
    with pytest.raises(ValueError, match="two positions"):
        baseline.adain(c[..., :1], s, 1.0, index)
    with pytest.raises(ValueError, match="style_index"):
        baseline.adain(c, s)                                                          # 3 images, 2 styles, no index


def test_forward_is_not_implemented_and_says_why():
    with pytest.raises(NotImplementedError, match="trains the AdaIN network"):
        baseline.AdaIN2D()(torch.zeros(1, 3, 16, 16), torch.zeros(1, 3, 16, 16))


def test_inputs_that_require_a_gradient_take_the_expression():
    m = model64()
    x = losses._imagenet_normalize(ai.images("A")[0][:1].double()).requires_grad_(True)
    s = losses._imagenet_normalize(ai.images("A")[1][None].double())
    before = baseline.CALLS["adain2d_expression"]
    out = m.generate(x, s)
    assert out.requires_grad and baseline.CALLS["adain2d_expression"] == before + 1


# ---- the C ABI ------------------------------------------------------------------------------------------------------
def test_the_library_exports_the_new_entries_and_refuses_bad_arguments_before_any_launch():
    from styl3r_amd import vit_ops
    vit_ops.build_library()
    lib = vit_ops.load()
    for name in ("vit_adain_fwd", "vit_adain_scratch_bytes", "vit_conv3_rgb_fwd"):
        assert name in vit_ops.EXPORTS and hasattr(lib, name)
    header = (ROOT / "include/vit_ops.h").read_text()
    assert "#define VIT_CONV_REFLECT 4" in header and "#define VIT_CONV_UP2 8" in header
    assert (baseline.VIT_CONV_RELU_IN, baseline.VIT_CONV_REFLECT, baseline.VIT_CONV_UP2) == (RELU_IN, REFLECT, UP2)
    one = C.c_void_p(16)                                           # (any non-null value: validation only, nothing is dereferenced)
    conv = lambda H, W, k, flags, bias=None, res=None: lib.vit_conv_x6_fwd(one, one, bias, res, one, 1, 16, 16, H, W, k, flags, None)
    assert conv(8, 8, 1, REFLECT) == EINVAL                                      # ksize != 3
    assert conv(8, 8, 3, REFLECT | GATE, None, one) == EINVAL and conv(8, 8, 3, REFLECT | UP2 | GATE, None, one) == EINVAL
    assert conv(8, 8, 3, UP2) == EINVAL and conv(8, 8, 3, UP2 | RELU_IN) == EINVAL   # UP2 without REFLECT
    assert conv(7, 8, 3, REFLECT | UP2) == EINVAL and conv(8, 7, 3, REFLECT | UP2) == EINVAL
    assert conv(1, 8, 3, REFLECT) == EINVAL and conv(8, 1, 3, REFLECT) == EINVAL and conv(1, 1, 3, REFLECT | RELU_IN) == EINVAL
    # vit_adain_fwd
    assert lib.vit_adain_scratch_bytes(4, 2, 512) == 2 * 512 * 2 * 4 and lib.vit_adain_scratch_bytes(0, 2, 512) == 0
    idx = (C.c_int32 * 3)(0, 1, 1)
    ada = lambda B=3, Bs=2, Cc=8, N=4, M=4, index=idx, content=one, scratch=one: lib.vit_adain_fwd(
        content, one, index, one, B, Bs, Cc, N, M, 1.0, 1e-8, one, scratch, None)
    assert ada(N=1) == EINVAL and ada(M=1) == EINVAL and ada(N=0) == EINVAL
    assert ada(content=None) == EINVAL and ada(scratch=None) == EINVAL and ada(index=None) == EINVAL
    assert ada(B=0) == EINVAL and ada(Bs=0) == EINVAL and ada(Cc=0) == EINVAL
    assert ada(index=(C.c_int32 * 3)(0, 2, 1)) == EINVAL and ada(index=(C.c_int32 * 3)(0, -1, 1)) == EINVAL      # outside [0, Bs)
    assert ada(scratch=C.c_void_p(18)) == EINVAL                                  # misaligned scratch
    # vit_conv3_rgb_fwd
    rgb = lambda Ci=64, Co=3, H=8, W=8, flags=REFLECT, inp=one, scale=None, shift=None, lo=0.0, hi=1.0: lib.vit_conv3_rgb_fwd(
        inp, one, one, scale, shift, lo, hi, one, 1, Ci, Co, H, W, flags, None)
    assert rgb(Ci=12) == EINVAL and rgb(Ci=72) == EINVAL and rgb(Ci=0) == EINVAL
    assert rgb(Co=5) == EINVAL and rgb(Co=0) == EINVAL
    assert rgb(flags=GATE) == EINVAL and rgb(flags=REFLECT | UP2) == EINVAL and rgb(flags=16) == EINVAL
    assert rgb(H=1) == EINVAL and rgb(W=1) == EINVAL and rgb(inp=None) == EINVAL
    assert rgb(scale=one) == EINVAL and rgb(scale=one, shift=one, lo=1.0, hi=0.0) == EINVAL


# ---- the pictures ---------------------------------------------------------------------------------------------------
class _StubBaseline:
    """what the pictures need of an AdaIN2D: stylize(images, style) -> images of the same shape"""

    def __init__(self):
        self.seen = []

    def stylize(self, images01, style01, alpha=1.0, style_index=None):
        self.seen.append((images01, style01))
        return (1 - images01) * style01.mean()


def _stub_labeler(text):
    return torch.full((3, 5, 4 * len(text)), 0.5)


def _vis_inputs():
    g = torch.Generator().manual_seed(3)
    h, w, v, t = 12, 20, 2, 3
    ctx, gt, pred = (torch.rand((n, 3, h, w), generator=g) for n in (v, t, t))
    ctx_depth, depth = torch.rand((v, h, w), generator=g) + 0.5, torch.rand((t, h, w), generator=g) + 0.5
    style = torch.rand((3, 9, 7), generator=g)
    E, K, _, near, far = camera_inputs()
    batch = {"context": dict(extrinsics=E[None, :2], intrinsics=K[None, :2], near=near[None, :2], far=far[None, :2]),
             "target": dict(extrinsics=E[None, 2:], intrinsics=K[None, 2:], near=near[None, 2:], far=far[None, 2:])}
    return ctx, ctx_depth, gt, pred, depth, style, batch


def test_validation_images_without_a_baseline_are_unchanged_and_with_one_it_is_the_first_column():
    ctx, ctx_depth, gt, pred, depth, style, batch = _vis_inputs()
    h, w = gt.shape[-2:]
    plain = vis.validation_images(ctx, ctx_depth, gt, pred, depth, None, batch, style_image=style, resolution=48)
    none = vis.validation_images(ctx, ctx_depth, gt, pred, depth, None, batch, style_image=style, resolution=48, baseline=None)
    assert set(plain) == set(none) and all(torch.equal(plain[k], none[k]) for k in plain)
    # today's picture: border 8 | style | gap 8 | Context | Target GT | Prediction | Depth
    assert plain["comparison"].shape[2] == 8 + 7 + 8 + 4 * w + 3 * 8 + 8
    stub = _StubBaseline()
    out = vis.validation_images(ctx, ctx_depth, gt, pred, depth, None, batch, style_image=style, resolution=48, baseline=stub)
    comp = out["comparison"]
    assert comp.shape[2] == plain["comparison"].shape[2] + w + 8 and torch.equal(out["cameras"], plain["cameras"])
    assert len(stub.seen) == 1 and stub.seen[0][0] is gt and torch.equal(stub.seen[0][1], style)
    want = stub.stylize(gt, style)
    x0 = 8 + 7 + 8
    for row in range(gt.shape[0]):
        assert torch.equal(comp[:, 8 + row * (h + 8):8 + row * (h + 8) + h, x0:x0 + w], want[row])
    assert torch.equal(comp[:, :, x0 + w + 8:], plain["comparison"][:, :, x0:])       # everything behind the new column is today's picture
    assert torch.equal(comp[:, :, :x0], plain["comparison"][:, :, :x0])
    # the same column as an extra column with the reference's label
    extra = vis.validation_images(ctx, ctx_depth, gt, pred, depth, None, batch, extra_columns=[("2D Baseline", want)], style_image=style,
                                  resolution=48, labeler=_stub_labeler)
    labelled = vis.validation_images(ctx, ctx_depth, gt, pred, depth, None, batch, style_image=style, resolution=48, labeler=_stub_labeler,
                                     baseline=stub)
    assert torch.equal(extra["comparison"], labelled["comparison"])
    with pytest.raises(ValueError, match="style"):
        vis.validation_images(ctx, ctx_depth, gt, pred, depth, None, batch, resolution=48, baseline=stub)
    other = torch.rand(3, 5, 5)
    vis.comparison_image(ctx, ctx_depth, gt, pred, depth, baseline=stub, baseline_style=other)
    assert torch.equal(stub.seen[-1][1], other)


def test_train_comparison_image_layout():
    """first and last sample side by side; per sample: baseline | context interleaved with the style | ground truth | prediction | depth"""
    from styl3r_amd.export import pack_frames
    g = torch.Generator().manual_seed(5)
    b, v, t, h, w = 3, 2, 2, 12, 20
    ctx, gt, pred = torch.rand((b, v, 3, h, w), generator=g), torch.rand((b, t, 3, h, w), generator=g), torch.rand((b, t, 3, h, w), generator=g)
    depth = torch.rand((b, t, h, w), generator=g) + 0.5
    styles = torch.rand((b, 3, h, w), generator=g)
    stub = _StubBaseline()
    image, caption = vis.train_comparison_image(ctx, styles, gt, pred, depth, baseline=stub, scenes=["s0", "s1", "s2"], style_names=["a", "b", "c"])
    assert caption == "s0 | a | s2 | c"
    assert [torch.equal(seen[0], gt[i]) and torch.equal(seen[1], styles[i]) for seen, i in zip(stub.seen, (0, 2))] == [True, True]
    tall = 2 * v * h + (2 * v - 1) * 8
    wide = 5 * w + 4 * 8
    assert image.shape == (3, tall + 16, 2 * wide + 8 + 16) and image.dtype == torch.float32
    seen = torch.zeros(image.shape[1:], dtype=torch.bool)
    for k, i in enumerate((0, 2)):
        dbytes = pack_frames([depth[i]], loop_reverse=False).permute(0, 3, 1, 2).float() / 255
        columns = [list(stub.stylize(gt[i], styles[i])), [p for j in range(v) for p in (ctx[i, j], styles[i])], list(gt[i]), list(pred[i]), list(dbytes)]
        for col, panels in enumerate(columns):
            for row, p in enumerate(panels):
                x0, y0 = 8 + k * (wide + 8) + col * (w + 8), 8 + row * (h + 8)
                assert torch.equal(image[:, y0:y0 + h, x0:x0 + w], p), (k, col, row)
                seen[y0:y0 + h, x0:x0 + w] = True
    assert (image[:, ~seen] == 1).all()
    labelled, _ = vis.train_comparison_image(ctx, styles, gt, pred, depth, baseline=stub, labeler=_stub_labeler)
    assert labelled.shape[1] == tall + 2 * 9 + 16                              # the column labels and "Sample Index" above them
    no_base, cap = vis.train_comparison_image(ctx, styles, gt, pred, depth)
    assert no_base.shape[2] == 2 * (wide - w - 8) + 8 + 16 and cap == "sample 0 | style 0 | sample 2 | style 2"
