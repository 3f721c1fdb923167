"""GPU tests (-m gpu) of the 2D-AdaIN baseline: the source modes of vit_conv_x6_fwd (VIT_CONV_REFLECT, VIT_CONV_UP2), vit_adain_fwd,
vit_conv3_rgb_fwd (csrc/vit_adain.hip), `baseline.AdaIN2D` end to end against tests/golden/adain_ref.npz, the poisoned runs and the
validation picture.  Errors are max |a - e64| / max |e64| against a float64 CPU result on the same fp32 inputs.  The bars:
  source modes   error <= 2 x the error of today's conv_x6_forward on the materialised map (pad(interpolate(x)), cropped): kernel, arithmetic
                 and K order are the same, only the split-K summation order may differ; bit-equal where neither launch splits K
  adain, rgb     error <= 4 x the error of the framework's fp32 expression on the same device (both accumulate in at least fp32; 4 covers
                 the order of the sums); two runs bit-identical
  end to end     bf16x6: <= 4 x the fp32 framework expression of the same network on the device; bf16x3 / f16x3: <= 4 x the same network on
                 the materialised route in that mode
Every figure is printed before it is asserted (pytest -s)."""
import ctypes as C
import functools
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from styl3r_amd import baseline, losses, vit_ops
from tests import adain_inputs as ai
from tests import poison

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = Path(__file__).resolve().parents[1]
MODES = ("bf16x6", "bf16x3", "f16x3")
RELU_IN, REFLECT, UP2 = 1, 4, 8


def rel(a, e64):
    return float((a.detach().cpu().double() - e64).abs().max() / e64.abs().max())


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


@pytest.fixture(autouse=True)
def _fp32_framework():
    keep = torch.backends.cudnn.allow_tf32, torch.backends.cuda.matmul.allow_tf32
    torch.backends.cudnn.allow_tf32 = torch.backends.cuda.matmul.allow_tf32 = False
    yield
    torch.backends.cudnn.allow_tf32, torch.backends.cuda.matmul.allow_tf32 = keep


@functools.lru_cache(maxsize=None)
def fixture():
    return {k: (torch.from_numpy(v) if v.dtype.kind == "f" else v) for k, v in np.load(ROOT / "tests/golden/adain_ref.npz").items()}


@functools.lru_cache(maxsize=None)
def model():
    f = fixture()
    sd = ai.reference_state_dict()
    m = baseline.AdaIN2D()
    m.load_state_dict({str(k): sd[str(k)] for k in f["keys"]}, strict=True)      # the reference's key layout, from the fixture's key list
    return m.to(DEV)


# ---- 1. source modes against the materialised route ------------------------------------------------------------------------------------
CONV_SHAPES = ((2, 16, 8, 2, 2), (1, 64, 24, 5, 35), (2, 32, 130, 6, 34), (1, 512, 16, 4, 4), (4, 16, 128, 128, 64))
# (relu_in, bias, residual): each of the three with and without
CONV_VARIANTS = ((False, False, False), (True, True, False), (False, True, True), (True, False, True))


def halo_splits(B, Co, H, W, Ci, source_mode=False):
    """K splits of a halo-kernel launch (conv_x6_fwd in csrc/vit_gemm_x6.hip)"""
    ht, nslab, S = -(-Co // 128) * B * -(-W // 32) * -(-H // 4), Ci // 16, 1
    if ht < 256:
        S = 512 // ht
        while S > 1 and nslab // S < 2:
            S -= 1
        S = min(max(S, 1), 16 if source_mode and W < 32 else 8)
    return S


@functools.lru_cache(maxsize=None)
def conv_case(i, up2):
    B, Ci, Co, H, W = CONV_SHAPES[i]
    h, w = (H // 2, W // 2) if up2 else (H, W)
    return ai.conv_case(10 * i + up2, B, Ci, Co, h, w, H, W)


def materialise(x, up2):
    return F.pad(F.interpolate(x, scale_factor=2) if up2 else x, (1, 1, 1, 1), mode="reflect")


@functools.lru_cache(maxsize=None)
def conv_reference(i, up2, relu_in):
    """float64 CPU convolution of the materialised map, without bias and residual (added in float64 by the caller)"""
    x, w, _, _ = conv_case(i, up2)
    x = x.double()
    return F.conv2d(materialise(torch.relu(x) if relu_in else x, up2), w.double())


def flagged_conv(x, w, bias, residual, flags, H, W):
    B, Ci = x.shape[:2]
    Co = w.shape[0]
    assert vit_ops._x6()
    wp = vit_ops.split_conv_weight(w)
    out = torch.full((B, Co, H, W), float("nan"), device=DEV)
    if vit_ops._f16():
        vit_ops._announce(vit_ops._amax_word(x))                         # the SOURCE tensor's |max|
    rc = vit_ops.load().vit_conv_x6_fwd(x.data_ptr(), wp.data_ptr(), bias.data_ptr() if bias is not None else None,
                                        residual.data_ptr() if residual is not None else None, out.data_ptr(), B, Ci, Co, H, W, 3, flags, stream())
    assert rc == 0, vit_ops.load().vit_last_error()
    return out


@pytest.mark.parametrize("i", range(len(CONV_SHAPES)), ids=["x".join(map(str, s)) for s in CONV_SHAPES])
@pytest.mark.parametrize("mode", MODES)
def test_source_modes_against_the_materialised_route(mode, i, monkeypatch):
    monkeypatch.setattr(vit_ops, "LINEAR_MODE", mode)
    B, Ci, Co, H, W = CONV_SHAPES[i]
    if i == 3:
        assert halo_splits(B, Co, H, W, Ci, True) == 16                       # forces split-K
    if i == 4:                                                                # neither launch splits K
        assert halo_splits(B, Co, H, W, Ci, True) == 1 and halo_splits(B, Co, H + 2, W + 2, Ci) == 1
    for up2 in (False, True):
        if up2 and (H % 2 or W % 2):
            continue
        x, w, bias, res = (t.to(DEV) for t in conv_case(i, up2))
        for relu_in, with_bias, with_res in CONV_VARIANTS:
            ref = conv_reference(i, up2, relu_in)
            if with_bias:
                ref = ref + bias.cpu().double().view(1, -1, 1, 1)
            if with_res:
                ref = ref + res.cpu().double()
            flags = REFLECT | (UP2 if up2 else 0) | (RELU_IN if relu_in else 0)
            got = flagged_conv(x, w, bias if with_bias else None, res if with_res else None, flags, H, W)
            mat = vit_ops.conv_x6_forward(materialise(x, up2), w, bias if with_bias else None, F.pad(res, (1, 1, 1, 1)) if with_res else None,
                                          relu_in=relu_in)[..., 1:-1, 1:-1]
            assert bool(torch.isfinite(got).all())
            e_got, e_mat = rel(got, ref), rel(mat, ref)
            same = torch.equal(got, mat)
            print(f"{mode} {CONV_SHAPES[i]} up2={int(up2)} relu={int(relu_in)} bias={int(with_bias)} res={int(with_res)}: flagged {e_got:.3e}, "
                  f"materialised {e_mat:.3e}, bit-equal {same}")
            assert e_got <= 2 * e_mat, (up2, relu_in, with_bias, with_res, e_got, e_mat)
            if i == 4:
                assert same, "unsplit launches of the same kernel in the same K order differ"


def test_source_mode_argument_errors_on_the_device():
    x, w, _, _ = (t.to(DEV) for t in conv_case(0, False))
    lib = vit_ops.load()
    wp = vit_ops.split_conv_weight(w) if vit_ops._x6() else None
    out = torch.full((2, 8, 2, 2), 3.0, device=DEV)
    for k, flags, H, W in ((1, REFLECT, 2, 2), (3, UP2, 2, 2), (3, REFLECT | UP2, 3, 2), (3, REFLECT, 1, 2), (3, REFLECT | 2, 2, 2)):
        assert lib.vit_conv_x6_fwd(x.data_ptr(), wp.data_ptr(), None, x.data_ptr() if flags & 2 else None, out.data_ptr(), 2, 16, 8, H, W, k, flags,
                                   stream()) == -1
    torch.cuda.synchronize()
    assert bool((out == 3.0).all())                                           # nothing ran


# ---- 2. vit_adain_fwd ----------------------------------------------------------------------------------------------------------------------
ADAIN_SHAPES = ((3, 2, 8, 2, 2), (2, 1, 64, 15, 1027), (4, 2, 512, 1024, 1024))
ADAIN_INDEX = {3: (0, 1, 1), 2: (0, 0), 4: (0, 0, 1, 1)}


def raw_adain(c, s, index, alpha, pattern=None):
    """vit_adain_fwd through the C ABI; with `pattern`, output and scratch are `poison.guarded` buffers of exactly their sizes"""
    lib = vit_ops.load()
    (B, Cc, N), (Bs, _, M) = c.shape, s.shape
    nbytes = lib.vit_adain_scratch_bytes(B, Bs, Cc)
    assert nbytes == Bs * Cc * 8
    if pattern is None:
        out, scratch, checks = torch.full((B * Cc * N,), float("nan"), device=DEV), torch.empty(nbytes, dtype=torch.uint8, device=DEV), ()
    else:
        (out8, chk_o), (scratch, chk_s) = poison.guarded(B * Cc * N * 4, pattern=pattern), poison.guarded(nbytes, pattern=pattern)
        out, checks = out8.view(torch.float32), (chk_o, chk_s)
    idev = index.to(DEV)
    rc = lib.vit_adain_fwd(c.data_ptr(), s.data_ptr(), index.data_ptr(), idev.data_ptr(), B, Bs, Cc, N, M, alpha, 1e-8, out.data_ptr(),
                           scratch.data_ptr(), stream())
    assert rc == 0, lib.vit_last_error()
    torch.cuda.synchronize()
    for chk in checks:
        chk()
    return out.view(B, Cc, N).clone()


@pytest.mark.parametrize("alpha", (1.0, 0.3))
@pytest.mark.parametrize("shape", ADAIN_SHAPES, ids=["x".join(map(str, s)) for s in ADAIN_SHAPES])
def test_adain_kernel_against_the_float64_expression(shape, alpha):
    B, Bs, Cc, N, M = shape
    c, s = ai.adain_case(ADAIN_SHAPES.index(shape), B, Bs, Cc, N, M)
    index = torch.tensor(ADAIN_INDEX[B], dtype=torch.int32)
    ref = baseline.adain_expression(c.double(), s.double(), alpha, index)
    cd, sd = c.to(DEV), s.to(DEV)
    e32 = rel(baseline.adain_expression(cd, sd, alpha, index), ref)
    got = raw_adain(cd, sd, index, alpha)
    assert bool(torch.isfinite(got).all())
    err = rel(got, ref)
    print(f"adain {shape} alpha {alpha}: kernel {err:.3e}, fp32 expression on the device {e32:.3e}")
    assert err <= 4 * e32
    assert torch.equal(raw_adain(cd, sd, index, alpha), got), "two runs differ"
    n0 = dict(baseline.CALLS)
    routed = baseline.adain(cd.view(B, Cc, N, 1), sd.view(Bs, Cc, M, 1), alpha, index)
    assert baseline.CALLS["adain_hip"] == n0["adain_hip"] + 1 and torch.equal(routed.view(B, Cc, N), got)
    for pattern in poison.PATTERNS:
        assert torch.equal(raw_adain(cd, sd, index, alpha, pattern), got), pattern


# ---- 3. vit_conv3_rgb_fwd ------------------------------------------------------------------------------------------------------------------
RGB_SHAPES = ((2, 8, 3, 2, 2), (1, 64, 3, 5, 35), (1, 64, 4, 24, 40))


def raw_rgb(x, w, bias, scale, shift, flags, pattern=None):
    lib = vit_ops.load()
    B, Ci, H, W = x.shape
    Co = w.shape[0]
    if pattern is None:
        out, checks = torch.full((B * Co * H * W,), float("nan"), device=DEV), ()
    else:
        out8, chk = poison.guarded(B * Co * H * W * 4, pattern=pattern)
        out, checks = out8.view(torch.float32), (chk,)
    rc = lib.vit_conv3_rgb_fwd(x.data_ptr(), w.data_ptr(), bias.data_ptr(), scale.data_ptr() if scale is not None else None,
                               shift.data_ptr() if shift is not None else None, 0.0, 1.0, out.data_ptr(), B, Ci, Co, H, W, flags, stream())
    assert rc == 0, lib.vit_last_error()
    torch.cuda.synchronize()
    for chk in checks:
        chk()
    return out.view(B, Co, H, W).clone()


@pytest.mark.parametrize("epilogue", (False, True))
@pytest.mark.parametrize("flags", (REFLECT | RELU_IN, REFLECT, 0))
@pytest.mark.parametrize("shape", RGB_SHAPES, ids=["x".join(map(str, s)) for s in RGB_SHAPES])
def test_rgb_convolution_against_the_float64_convolution(shape, flags, epilogue):
    B, Ci, Co, H, W = shape
    x, w, bias, _ = ai.conv_case(100 + RGB_SHAPES.index(shape), B, Ci, Co, H, W, H, W)
    scale, shift = torch.tensor([0.229, 0.224, 0.225, 0.3][:Co]) * 2, torch.tensor([0.485, 0.456, 0.406, 0.5][:Co])

    def expression(x, w, bias, scale, shift):
        h = torch.relu(x) if flags & RELU_IN else x
        y = F.conv2d(F.pad(h, (1, 1, 1, 1), mode="reflect"), w, bias) if flags & REFLECT else F.conv2d(h, w, bias, padding=1)
        return torch.clamp(y * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1), 0, 1) if epilogue else y
    ref = expression(x.double(), w.double(), bias.double(), scale.double(), shift.double())
    if epilogue:
        inside = float(((ref > 0) & (ref < 1)).double().mean())
        assert 0.25 <= inside < 1.0, inside                                   # the clamp acts, and cannot hide an error
    xd, wd, bd, scd, shd = (t.to(DEV) for t in (x, w, bias, scale, shift))
    e32 = rel(expression(xd, wd, bd, scd, shd), ref)
    got = raw_rgb(xd, wd, bd, scd if epilogue else None, shd if epilogue else None, flags)
    assert bool(torch.isfinite(got).all())
    err = rel(got, ref)
    print(f"rgb {shape} flags {flags} epilogue {int(epilogue)}: kernel {err:.3e}, framework fp32 conv2d {e32:.3e}")
    assert err <= 4 * e32
    assert torch.equal(raw_rgb(xd, wd, bd, scd if epilogue else None, shd if epilogue else None, flags), got), "two runs differ"
    for pattern in poison.PATTERNS:
        assert torch.equal(raw_rgb(xd, wd, bd, scd if epilogue else None, shd if epilogue else None, flags, pattern), got), pattern
    if flags & REFLECT:
        n0 = baseline.CALLS["conv_rgb_hip"]
        routed = baseline.conv_rgb(xd, wd, bd, relu_in=bool(flags & RELU_IN), scale=scd if epilogue else None, shift=shd if epilogue else None)
        assert torch.equal(routed, got) and baseline.CALLS["conv_rgb_hip"] == n0 + 1


# ---- 4. end to end ---------------------------------------------------------------------------------------------------------------------------
def scene_inputs(scene):
    f = fixture()
    target, style = f[f"{scene}_images"].to(DEV), f[f"{scene}_style"].to(DEV)
    return target, style, torch.zeros(target.shape[0], dtype=torch.int32)


def end_to_end_errors(scene):
    """(generate error, stylize error) of the device route in the current mode, with the route counters checked"""
    f, m = fixture(), model()
    target, style, index = scene_inputs(scene)
    n0 = dict(baseline.CALLS)
    raw = m.generate(losses._imagenet_normalize(target), losses._imagenet_normalize(style[None]), 1.0, style_index=index)
    final = m.stylize(target, style)
    assert baseline.CALLS["adain2d_expression"] == n0["adain2d_expression"]
    assert [baseline.CALLS[k] - n0[k] for k in ("adain_hip", "conv_rc_x6", "conv_rgb_hip")] == [2, 16, 2]
    assert raw.shape == f[f"{scene}_raw"].shape and bool(torch.isfinite(raw).all()) and float(final.min()) >= 0 and float(final.max()) <= 1
    return rel(raw, f[f"{scene}_raw"].double()), rel(final, f[f"{scene}_final"].double())


@functools.lru_cache(maxsize=None)
def end_to_end_bars(mode, scene):
    """4 x the error of the yardstick route on this device: bf16x6 -- the fp32 framework expression of the same network; bf16x3 / f16x3 -- the
    same network through the materialised route in that mode.  Computed once per (mode, scene)."""
    assert vit_ops.LINEAR_MODE == mode
    f, m = fixture(), model()
    target, style, index = scene_inputs(scene)
    x, s = losses._imagenet_normalize(target), losses._imagenet_normalize(style[None])
    with torch.no_grad():
        if mode == "bf16x6":
            raw, final = m.generate_expression(x, s, 1.0, index), m.generate_expression(x, s, 1.0, index, denorm=True)
        else:
            raw = m._generate(x, s, 1.0, index, denorm=False, materialised=True)
            final = m._generate(x, s, 1.0, index, denorm=True, materialised=True)
    b_raw, b_final = rel(raw, f[f"{scene}_raw"].double()), rel(final, f[f"{scene}_final"].double())
    print(f"{mode} scene {scene}: {'fp32 framework expression' if mode == 'bf16x6' else 'materialised route'}: generate {b_raw:.3e}, stylize {b_final:.3e}")
    return 4 * b_raw, 4 * b_final


@pytest.mark.parametrize("scene", sorted(ai.SCENES))
@pytest.mark.parametrize("mode", MODES)
def test_generate_and_stylize_against_the_fixture(mode, scene, monkeypatch):
    monkeypatch.setattr(vit_ops, "LINEAR_MODE", mode)
    bar_raw, bar_final = end_to_end_bars(mode, scene)
    e_raw, e_final = end_to_end_errors(scene)
    print(f"{mode} scene {scene}: generate {e_raw:.3e} (bar {bar_raw:.3e}), stylize {e_final:.3e} (bar {bar_final:.3e})")
    assert e_raw <= bar_raw
    assert e_final <= bar_final


def test_batched_scenes_share_one_call_where_the_sizes_agree():
    """two scenes of one size in one call (style_index = [0, 0, 1, 1]) equal the two calls up to the split-K summation order"""
    m = model()
    target, style, _ = scene_inputs("A")
    styles = torch.stack([style, style.flip(-1)])
    both = m.stylize(target, styles, style_index=torch.tensor([0, 0, 1, 1], dtype=torch.int32))
    one = m.stylize(target[:2], styles[0])
    two = m.stylize(target[2:], styles[1])
    # (the launches split K with atomics at these sizes: a few fp32 ulps per layer, 1e-5 of a [0, 1] picture leaves two orders of margin)
    assert float((both - torch.cat([one, two])).abs().max()) <= 1e-5
    assert float((one - m.stylize(target[:2], styles[1])).abs().max()) > 1e-3    # the style matters


# ---- 5. poison --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ("bf16x6", "f16x3"))
def test_the_chain_on_poisoned_allocations(mode, monkeypatch):
    """every uninitialised allocation of generate / stylize filled with zeros, ones and 1e30: the results meet the bars of test_generate_and_stylize_against_the_fixture.
    (Not bit-equal: the small frames split K, whose zero fill is the entry's own and whose atomics arrive in any order --
    docs/SCRATCH_CONTRACTS.md, vit_conv_x6_fwd.)"""
    monkeypatch.setattr(vit_ops, "LINEAR_MODE", mode)
    for pattern in poison.PATTERNS:
        for scene in sorted(ai.SCENES):
            bar_raw, bar_final = end_to_end_bars(mode, scene)
            with poison.poisoned_allocations(pattern) as record:
                e_raw, e_final = end_to_end_errors(scene)
            assert len(record) >= 2 * 11, "the chain's outputs and scratch were not allocated under the patch"
            print(f"{mode} {pattern} scene {scene}: generate {e_raw:.3e} (bar {bar_raw:.3e}), stylize {e_final:.3e} (bar {bar_final:.3e})")
            assert e_raw <= bar_raw and e_final <= bar_final, (pattern, scene)


# ---- 6. the validation picture ----------------------------------------------------------------------------------------------------------------
def test_validation_step_puts_the_baseline_first():
    from styl3r_amd import evaluation
    from styl3r_amd.decoder import DecoderSplattingCUDACfg, Gaussians, get_decoder
    from styl3r_amd.scenes import make_scene
    from tests.test_gpu_metrics import _fixed_lpips
    from tests.test_gpu_vis import _Encoder
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
    m = model()
    n0 = dict(baseline.CALLS)
    _, _, plain = evaluation.validation_step(_Encoder(g, depth), dec, batch, 7, lpips=lp, resolution=48)
    assert all(baseline.CALLS[k] == n0[k] for k in ("adain_hip", "conv_rc_x6", "conv_rgb_hip", "adain2d_expression"))
    _, _, images = evaluation.validation_step(_Encoder(g, depth), dec, batch, 7, lpips=lp, resolution=48, baseline=m)
    assert [baseline.CALLS[k] - n0[k] for k in ("adain_hip", "conv_rc_x6", "conv_rgb_hip", "adain2d_expression")] == [1, 8, 1, 0]
    comp = images["comparison"]                                            # style | 2D Baseline | Context | GT | prediction | depth
    assert comp.shape == (3, plain["comparison"].shape[1], plain["comparison"].shape[2] + hw + 8)
    want = m.stylize(gt[0], batch["style"]["image"][0])
    assert want.shape == (3, 3, hw, hw) and float(want.std()) > 1e-3
    x = 8 + (40 + 8)
    for i in range(3):
        y = 8 + i * (hw + 8)
        # (two runs of the route differ by the split-K summation order of the small frames: see test_batched_scenes_...)
        assert float((comp[:, y:y + hw, x:x + hw] - want[i]).abs().max()) <= 1e-5
    assert torch.equal(comp[:, :, x + hw + 8:], plain["comparison"][:, :, x:]) and torch.equal(comp[:, :, :x], plain["comparison"][:, :, :x])
    assert torch.equal(images["cameras"], plain["cameras"]) and torch.equal(images["projection"], plain["projection"])
