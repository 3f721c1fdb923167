"""Multi-style serving, the parts a machine without a GPU can check: the encoder's scene cache (`encode_scene` + `restyle`) on host
tensors against `forward`, the C ABI of the multi-style rasterizer pass (declared, exported, argument checks), and the refusals of the
forward-only decoder call."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from styl3r_amd import _lib
from tests.gpu_utils import assert_close_rel
from tests.helpers import deterministic_init_
from tests.test_encoder import TINY

ROOT = Path(__file__).resolve().parent.parent
G = np.load(ROOT / "tests" / "golden" / "encoder_tiny.npz")
FIELDS = ("means", "covariances", "harmonics", "opacities")


def _tiny(sh_degree=1):
    from styl3r_amd.encoder import EncoderNoPoSplatMultiTokenStyle, EncoderNoPoSplatTokenStyleCfg, GaussianAdapterCfg
    cfg = EncoderNoPoSplatTokenStyleCfg(gaussian_adapter=GaussianAdapterCfg(0.5, 15.0, sh_degree))
    return deterministic_init_(EncoderNoPoSplatMultiTokenStyle(cfg, trunk_params=TINY).eval())


def _inputs(tag="sh1"):
    T = lambda k: torch.tensor(G[f"{tag}_{k}"])
    return dict(image=T("image"), intrinsics=T("intrinsics")), dict(image=T("style"))


@pytest.fixture(scope="module")
def tiny_run():
    """forward, and the split run on the same inputs: (encoder, ctx, style, forward's Gaussians + dump, state, restyle's Gaussians + dump)"""
    from oracle.encoder_cpu import cpu_attention
    m = _tiny(1)
    ctx, style = _inputs()
    with torch.no_grad(), cpu_attention():
        d_ref, d_got = {}, {}
        ref = m(ctx, style, 0, visualization_dump=d_ref)
        state = m.encode_scene(ctx, 0)
        got = m.restyle(state, style, visualization_dump=d_got)
    return m, ctx, style, ref, d_ref, state, got, d_got


def test_restyle_of_encode_scene_is_forward_bit_for_bit(tiny_run):
    """the same framework ops on the same shapes: no tolerance"""
    _, _, _, ref, d_ref, _, got, d_got = tiny_run
    for name in FIELDS:
        a, b = getattr(got, name), getattr(ref, name)
        assert a.shape == b.shape and torch.equal(a, b), name
    assert sorted(d_got) == sorted(d_ref) and len(d_ref) >= 5
    for k in d_ref:
        assert torch.equal(d_got[k], d_ref[k]), f"visualization_dump[{k!r}]"


def test_second_style_changes_the_harmonics_and_returns_the_same_geometry_tensors(tiny_run):
    from oracle.encoder_cpu import cpu_attention
    m, ctx, style, ref, _, state, got, _ = tiny_run
    other = dict(image=style["image"].flip(-1).contiguous() * 0.5)
    with torch.no_grad(), cpu_attention():
        g2 = m.restyle(state, other)
        want = m(ctx, other, 0)
    for name in ("means", "covariances", "opacities"):
        assert getattr(g2, name) is getattr(got, name), f"{name}: a restyle of the same state returns the same tensor"
        assert torch.equal(getattr(g2, name), getattr(want, name)), name
    assert torch.equal(g2.harmonics, want.harmonics)
    scale = want.harmonics.abs().max()
    assert (g2.harmonics - got.harmonics).abs().max() > 1e-2 * scale      # the style image really entered


def test_two_styles_in_one_restyle_call_match_the_single_style_calls(tiny_run):
    """batched GEMMs may block differently: the project's bar for b = 2 against b = 1 through the encoder, 1e-4 relative"""
    from oracle.encoder_cpu import cpu_attention
    m, ctx, style, ref, _, _, _, _ = tiny_run
    s0 = style["image"]
    s1 = s0.flip(-1).contiguous() * 0.5
    with torch.no_grad(), cpu_attention():
        state = m.encode_scene(ctx, 0)
        both = m.restyle(state, dict(image=torch.cat((s0, s1), dim=0)))
        one = [m.restyle(state, dict(image=s)) for s in (s0, s1)]
    assert isinstance(both, list) and len(both) == 2
    for name in ("means", "covariances", "opacities"):
        assert getattr(both[0], name) is getattr(both[1], name), name          # ONE geometry under both styles
        assert torch.equal(getattr(both[0], name), getattr(ref, name)), name
    for i in range(2):
        assert both[i].harmonics.shape == ref.harmonics.shape
        assert_close_rel(both[i].harmonics.numpy(), one[i].harmonics.numpy(), 1e-4, f"harmonics of style {i}")
    scale = one[0].harmonics.abs().max()
    assert (both[0].harmonics - both[1].harmonics).abs().max() > 1e-2 * scale   # a call that ignored the second style cannot pass
    with pytest.raises(ValueError, match="b == 1"):
        ctx2 = {k: torch.cat((t, t), dim=0) for k, t in ctx.items()}
        with torch.no_grad(), cpu_attention():
            m.restyle(m.encode_scene(ctx2, 0), dict(image=torch.cat((s0, s1, s0), dim=0)))


def test_encoders_without_the_split_say_so():
    from styl3r_amd.encoder import EncoderNoPoSplatMulti, EncoderNoPoSplatTokenStyle
    for cls in (EncoderNoPoSplatMulti, EncoderNoPoSplatTokenStyle):
        with pytest.raises(NotImplementedError, match="noposplat_multi_token_style"):
            cls.encode_scene(None, {})


# --------------------------------------------------------------------------- C ABI
@pytest.fixture(scope="module")
def lib():
    _lib.build_library()
    return _lib.load()


def test_styles_entry_points_are_declared_and_exported(lib):
    header = (ROOT / "include/gsr.h").read_text()
    declared = set(re.findall(r"\b(gsr_[a-z_0-9]+)\s*\(", header))
    for name in ("gsr_forward_styles", "gsr_styles_extra_bytes"):
        assert name in declared and name in _lib.EXPORTS and hasattr(lib, name), name
    assert f"#define GSR_FLAG_STYLES_CHUNK_SHIFT {_lib.GSR_FLAG_STYLES_CHUNK_SHIFT} " in header
    assert "gsr_styles.hip" in _lib._SOURCES


def test_every_library_source_exists():
    assert "gsr_ssim.hip" in _lib._SOURCES
    for name in _lib._SOURCES:
        assert (ROOT / "styl3r_amd/csrc" / name).is_file(), name


def test_styles_extra_bytes(lib):
    d0 = _lib.GsrDims(2, 5, 1000, 64, 64, 1, 0, 0, None)        # degree 0: per (style, scene, Gaussian)
    d2 = _lib.GsrDims(2, 5, 1000, 64, 64, 9, 2, 0, None)        # degree 2: per (style, view, Gaussian)
    rgb = _lib.GsrDims(2, 5, 1000, 64, 64, 0, 0, 0, None)
    assert lib.gsr_styles_extra_bytes(C.byref(d0), 1) == 0
    assert lib.gsr_styles_extra_bytes(C.byref(d0), 4) == 3 * 2 * 1000 * 16
    assert lib.gsr_styles_extra_bytes(C.byref(rgb), 4) == 3 * 2 * 1000 * 16
    assert lib.gsr_styles_extra_bytes(C.byref(d2), 4) == 3 * 10 * 1000 * 16
    assert lib.gsr_styles_extra_bytes(C.byref(d0), 0) == 0 and lib.gsr_styles_extra_bytes(None, 2) == 0
    assert lib.gsr_styles_extra_bytes(C.byref(_lib.GsrDims(1, 1, 10, 16, 16, 25, 5, 0, None)), 2) == 0


def test_forward_styles_rejects_bad_arguments_before_any_launch(lib):
    """NULL pointers, S < 1, a degree the layout rejects: GSR_EINVAL, no GPU needed"""
    d = _lib.GsrDims(1, 3, 4096, 64, 64, 1, 0, 0, None)
    fake = C.c_void_p(4096)                                       # never dereferenced: every call below fails its checks first
    shs = (C.c_void_p * 2)(None, None)

    def call(dims, S, ptr, shs_arg, ws=None, extra=None):
        return lib.gsr_forward_styles(C.byref(dims) if dims is not None else None, S, ptr, ptr, ptr, ptr, shs_arg, 1 << 16, ws, 1 << 40,
                                      extra, 1 << 40, None, ptr, ptr, ptr, ptr, ptr, None)

    assert call(None, 2, None, shs) == -1
    assert call(d, 2, None, shs) == -1                                               # all NULL
    assert call(d, 2, fake, None, fake, fake) == -1                                  # no style table
    assert call(d, 2, fake, shs, fake, fake) == -1                                   # NULL entries in the style table
    ok_shs = (C.c_void_p * 2)(4096, 4096)
    assert call(d, 0, fake, ok_shs, fake, fake) == -1 and call(d, -3, fake, ok_shs, fake, fake) == -1      # S < 1
    assert call(d, 2, fake, ok_shs, None, fake) == -1                                # no workspace
    assert call(d, 2, fake, ok_shs, fake, None) == -1                                # S > 1 without the colour buffer
    for bad in (_lib.GsrDims(1, 1, 10, 16, 16, 25, 5, 0, None), _lib.GsrDims(1, 1, 10, 16, 16, 1, 1, 0, None),
                _lib.GsrDims(1, 1, 10, 16, 16, 0, 2, 0, None), _lib.GsrDims(0, 4, 10, 16, 16, 1, 0, 0, None)):
        assert call(bad, 2, fake, ok_shs, fake, fake) == -1                          # a degree / size the layout rejects
    for flag in (_lib.GSR_FLAG_NTOUCHED, _lib.GSR_FLAG_PREZERO_GRADS):               # forward-only: what only a backward needs is refused
        assert call(_lib.GsrDims(1, 3, 4096, 64, 64, 1, 0, flag, None), 2, fake, ok_shs, fake, fake) == -1
    # too small a workspace / colour buffer: GSR_ENOSPACE
    assert lib.gsr_forward_styles(C.byref(d), 2, fake, fake, fake, fake, ok_shs, 1 << 16, fake, 16, fake, 1 << 40, None, fake, fake, fake,
                                  fake, fake, None) == -2
    assert lib.gsr_forward_styles(C.byref(d), 2, fake, fake, fake, fake, ok_shs, 1 << 16, fake, 1 << 40, fake, 16, None, fake, fake, fake,
                                  fake, fake, None) == -2


# --------------------------------------------------------------------------- decoder
def _decoder_and_set(requires_grad=False):
    from styl3r_amd.decoder import DecoderSplattingCUDACfg, Gaussians, get_decoder
    dec = get_decoder(DecoderSplattingCUDACfg("splatting_cuda", [0.0, 0.0, 0.0], True))
    g = Gaussians(torch.zeros(1, 8, 3), torch.eye(3).expand(1, 8, 3, 3).contiguous(), torch.zeros(1, 8, 3, 1), torch.full((1, 8), 0.5))
    cams = (torch.eye(4)[None, None], torch.eye(3)[None, None], torch.ones(1, 1), torch.full((1, 1), 100.0))
    return dec, g, cams


def test_forward_styles_refuses_host_tensors():
    dec, g, cams = _decoder_and_set()
    with torch.no_grad(), pytest.raises(RuntimeError, match="no CPU path"):
        dec.forward_styles(g, [g.harmonics, g.harmonics], *cams, (16, 16))


def test_forward_styles_refuses_inputs_that_require_grad_and_names_forward():
    """the refusal comes before anything touches a device, so host tensors that claim `is_cuda` reach it on a machine without a GPU"""
    from styl3r_amd import rasterizer as rz

    class _Dev(torch.Tensor):
        is_cuda = True

    mk = lambda t: t.as_subclass(_Dev)
    means, cov, opac = mk(torch.zeros(1, 8, 3)), mk(torch.zeros(1, 8, 6)), mk(torch.zeros(1, 8))
    cols = [mk(torch.zeros(1, 8, 1, 3)), mk(torch.zeros(1, 8, 1, 3).requires_grad_(True))]
    views = mk(torch.zeros(1, 64))
    with pytest.raises(RuntimeError, match=r"forward-only.*rasterize_views"):
        rz.rasterize_views_styles(means, cov, opac, cols, views, (16, 16), 1)
    dec, g, cams = _decoder_and_set()
    from styl3r_amd.decoder import Gaussians
    gd = Gaussians(mk(g.means), mk(g.covariances), mk(g.harmonics), mk(g.opacities))
    hm = mk(g.harmonics.clone().requires_grad_(True))
    with pytest.raises(RuntimeError, match=r"`forward` is the differentiable path"):
        dec.forward_styles(gd, [gd.harmonics, hm], *[mk(c) for c in cams], (16, 16))
