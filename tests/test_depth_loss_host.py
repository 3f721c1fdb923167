"""CPU tests (-m "not gpu") of the depth-smoothness loss: the torch restatement (losses.depth_smoothness_expression) against the golden
vectors of the reference's own LossDepth (tests/golden/make_depth_loss_fixtures.py), LossDepth / get_losses, and the C boundary of
gsr_depth_smooth_* (the header, _lib.EXPORTS and the library agree; bad arguments are refused before any launch, so no device is needed)."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from styl3r_amd import _lib, losses
from styl3r_amd.decoder import DecoderOutput
from tests.depth_loss_inputs import CONFIGS, GRAD_RTOL, assert_sign_condition, value_tolerance

ROOT = Path(__file__).resolve().parents[1]
GOLD = np.load(ROOT / "tests/golden/depth_loss_ref.npz")


def gold_inputs(dtype=torch.float32):
    return tuple(torch.from_numpy(GOLD[k]).to(dtype) for k in ("depth", "near", "far", "image"))


def test_fixture_inputs_keep_every_sign_unambiguous():
    depth, near, far, image = gold_inputs()
    assert depth.shape == (2, 3, 19, 37) and depth.dtype == torch.float32
    assert_sign_condition(depth, near, far, image)
    n1 = int((near.flatten() == 1).nonzero()[0])
    flat = depth.flatten(0, 1)
    assert (flat[n1] == 0).any() and (flat[-1] > far.flatten()[-1].log()).all()                     # ties at log(1) = 0; a view beyond far
    assert (flat[1] < near.flatten()[1].log()).any() and (flat[1] > far.flatten()[1].log()).any()   # beyond both bounds
    assert len(set(near.flatten().tolist())) == near.numel() and len(set(far.flatten().tolist())) == far.numel()


@pytest.mark.parametrize("tag", list(CONFIGS))
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_expression_matches_the_reference(tag, dtype):
    sigma, second = CONFIGS[tag]
    weight = float(GOLD["weight"])
    depth, near, far, image = gold_inputs(dtype)
    depth.requires_grad_(True)
    value = losses.depth_smoothness(depth, near, far, image, weight, sigma, second)               # CPU tensors: the plain expression
    value.backward()
    ref_v, ref_g = float(GOLD[f"{tag}_value"]), GOLD[f"{tag}_grad"]
    verr, gerr = abs(float(value.detach()) - ref_v), float(np.abs(depth.grad.double().numpy() - ref_g).max())
    print(f"{tag} {dtype}: value error {verr:.3e}, gradient error {gerr:.3e} of max |g| {np.abs(ref_g).max():.3e}")
    assert value.dtype == dtype
    if dtype == torch.float64:
        assert verr <= 1e-14 and gerr <= 1e-14 * np.abs(ref_g).max()
    else:
        assert verr <= value_tolerance(weight, sigma) and gerr <= GRAD_RTOL * np.abs(ref_g).max()
        assert abs(float(GOLD[f"{tag}_value_fp32"]) - ref_v) <= value_tolerance(weight, sigma)     # and so is the reference's own fp32 value


def test_loss_depth_module_reads_the_decoder_output_and_the_batch():
    depth, near, far, image = gold_inputs(torch.float64)
    batch = {"target": {"near": near, "far": far, "image": image}}
    cfg = losses.LossDepthCfg()
    assert (cfg.weight, cfg.sigma_image, cfg.use_second_derivative) == (0.25, None, False)        # config/loss/depth.yaml
    got = losses.LossDepth()(DecoderOutput(None, depth), batch, None, 0)
    assert abs(float(got) - float(GOLD["plain_value"])) <= 1e-14
    got = losses.LossDepth(losses.LossDepthCfg(0.25, 10.0, True))(DecoderOutput(None, depth), batch)
    assert abs(float(got) - float(GOLD["bilateral_second_value"])) <= 1e-14
    del batch["target"]["image"]                                                                  # not read without sigma_image
    assert abs(float(losses.LossDepth()(DecoderOutput(None, depth), batch)) - float(GOLD["plain_value"])) <= 1e-14


def test_tiny_shapes_and_mismatched_arguments_raise():
    one = torch.ones(1, 1)
    with pytest.raises(ValueError, match="no difference"):
        losses.depth_smoothness(torch.zeros(1, 1, 1, 5), one, 2 * one)
    with pytest.raises(ValueError, match="no difference"):
        losses.depth_smoothness(torch.zeros(1, 1, 2, 5), one, 2 * one, use_second_derivative=True)
    with pytest.raises(ValueError, match="needs the target image"):
        losses.depth_smoothness(torch.zeros(1, 1, 4, 5), one, 2 * one, sigma_image=10.0)
    with pytest.raises(ValueError, match="near / far"):
        losses.depth_smoothness(torch.zeros(1, 2, 4, 5), one, 2 * one)
    assert torch.isfinite(losses.depth_smoothness(torch.zeros(1, 1, 2, 2), one, 2 * one))


def test_get_losses_is_the_registry():
    cfgs = [losses.LossMseCfg(), losses.LossLpipsCfg(), losses.LossDepthCfg(sigma_image=10.0), losses.LossStyleCfg()]
    built = losses.get_losses(cfgs)
    assert [type(m) for m in built] == [losses.LossMse, losses.LossLpips, losses.LossDepth, losses.LossStyle]
    assert all(m.cfg is c for m, c in zip(built, cfgs))
    assert losses.get_losses([]) == []
    with pytest.raises(NotImplementedError, match="adaattn"):
        losses.get_losses([losses.LossMseCfg(), {"adaattn": {"weight": 1.0}}])


@pytest.fixture(scope="module")
def lib():
    _lib.build_library()
    return _lib.load()


def test_the_library_exports_the_three_symbols(lib):
    header = (ROOT / "include/gsr.h").read_text()
    for name in ("gsr_depth_smooth_scratch_bytes", "gsr_depth_smooth_fwd", "gsr_depth_smooth_bwd"):
        assert name in _lib.EXPORTS and re.search(rf"\b{name}\s*\(", header) and hasattr(lib, name), name
    assert "gsr_depth.hip" in _lib._SOURCES and (ROOT / "styl3r_amd/csrc/gsr_depth.hip").is_file()
    assert lib.gsr_depth_smooth_scratch_bytes(40, 256, 256) == 40 * 2 * 32 * 16                    # two float64 per tile of 128 x 8 pixels
    assert lib.gsr_depth_smooth_scratch_bytes(1, 2, 2) == 16
    for bad in ((0, 8, 8), (1, 1, 8), (1, 8, 1), (-3, 8, 8), (1 << 40, 8, 8)):
        assert lib.gsr_depth_smooth_scratch_bytes(*bad) == 0


def test_bad_arguments_are_refused_before_any_launch(lib):
    one = C.c_void_p(256)                                           # (any non-null value: validation only, nothing is dereferenced)
    good = dict(depth=one, image=None, near=one, far=one, N=2, H=4, W=4, second=0, scratch=one, out=one)
    fwd = lambda **kw: (lambda a: lib.gsr_depth_smooth_fwd(a["depth"], a["image"], a["near"], a["far"], a["N"], a["H"], a["W"], 1.0, 10.0,
                                                           a["second"], a["scratch"], a["out"], None))({**good, **kw})
    bwd = lambda **kw: (lambda a: lib.gsr_depth_smooth_bwd(a["depth"], a["image"], a["near"], a["far"], None, a["N"], a["H"], a["W"], 1.0, 10.0,
                                                           a["second"], a["out"], None))({**good, **kw})
    for call in (fwd, bwd):
        for kw in (dict(N=0), dict(N=-1), dict(H=1), dict(W=1), dict(H=0), dict(H=2, second=1), dict(W=2, second=1),
                   dict(depth=None), dict(near=None), dict(far=None), dict(out=None), dict(N=1 << 40)):
            assert call(**kw) == -1, kw
    assert fwd(scratch=None) == -1
