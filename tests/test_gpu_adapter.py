"""-m gpu: the fused head-tail + Gaussian-adapter kernels (include/vit_ops.h vit_adapter_fwd / vit_adapter_bwd) against the
element-wise expression of the same reference math -- reg_dense_depth(mode='exp') (postprocess.py:22-60), sigmoid +
map_pdf_to_opacity (encoder_noposplat_multi_token_style.py:115-128), UnifiedGaussianAdapter.forward
(gaussian_adapter.py:122-153), build_covariance (gaussians.py:8-44) -- evaluated by the framework in float64.  (That
expression itself is pinned to the reference by the encoder golden vectors, tests/test_encoder.py.)

Regimes, reference, yardstick and bars: tests/adapter_cases.py (checked without a GPU by test_adapter_host.py).  Every regime case compares
each forward output and each gradient group (pts, density, scale, quaternion, SH) at that group's own maximum."""
import ctypes as ct
from types import SimpleNamespace

import pytest
import torch

from tests import adapter_cases as ac
from tests.adapter_cases import reference_expression as _reference

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("b,v,H,W,sh_degree,exponent,separate_app", [(2, 3, 16, 24, 0, 1.0, True), (1, 1, 8, 8, 1, 1.0, True),
                                                                    (2, 2, 12, 20, 2, 1.7, True), (1, 2, 16, 16, 1, 1.0, False),
                                                                    (1, 4, 32, 32, 4, 0.6, True)])
def test_adapter_kernels_match_float64_expression(b, v, H, W, sh_degree, exponent, separate_app):
    from styl3r_amd.vit_ops import gaussian_adapter_hip
    dev = torch.device("cuda:0")
    g = torch.Generator(dev).manual_seed(17 + v)
    d_sh = (sh_degree + 1) ** 2
    C = 8 if separate_app else 8 + 3 * d_sh
    R = lambda *s: torch.randn(*s, device=dev, generator=g)
    pts0, par0 = R(b, 3, H, W) * 0.8, R(b, C, H, W) * 2
    ptsr, parr = (R(b * (v - 1), 3, H, W) * 0.8, R(b * (v - 1), C, H, W) * 2) if v > 1 else (None, None)
    app = R(b * v, 3 * d_sh, H, W) if separate_app else None
    # four Gaussians with the scale raws (25, 310, -30): softplus's x > 20 branch, the 0.3 clamp (0.001 softplus(x) passes 0.3 at x = 300), a tiny scale
    par0[0, 1:4, 0, :4] = torch.tensor([25.0, 310.0, -30.0], device=dev)[:, None]
    mask = torch.ones(d_sh, device=dev)
    for deg in range(1, sh_degree + 1):
        mask[deg ** 2:(deg + 1) ** 2] = 0.1 * 0.25 ** deg
    ins = [t.requires_grad_(True) if t is not None else None for t in (pts0, ptsr, par0, parr, app)]
    out = gaussian_adapter_hip(*ins, mask, exponent, v, True)
    ins64 = [t.detach().double().requires_grad_(True) if t is not None else None for t in ins]
    ref = _reference(*ins64, mask.double(), exponent, v)
    names = ("means", "cov", "sh", "opac", "scales", "rot")
    for n, a, e in zip(names, out, ref):
        err = float((a.double() - e).abs().max() / e.abs().max().clamp_min(1e-30))
        assert err < 2e-6, (n, err)
    ws = [torch.randn(t.shape, device=dev, generator=g) for t in out[:4]]
    sum((a * w).sum() for a, w in zip(out[:4], ws)).backward()
    sum((e * w.double()).sum() for e, w in zip(ref[:4], ws)).backward()
    for n, a, e in zip(("pts0", "ptsr", "par0", "parr", "app"), ins, ins64):
        if a is None:
            continue
        err = float((a.grad.double() - e.grad).abs().max() / e.grad.abs().max().clamp_min(1e-30))
        assert err < 2e-5, (n, err)
    # the same comparison per gradient group: the density channel's gradient is 1e4 times the scale and quaternion channels', which the
    # per-tensor maximum above judges at a third of their size.  (The four planted Gaussians, whose clamped axis carries Sigma ~ 0.09, set
    # the quaternion group's maximum here; the regime cases below judge the rotation chain at homogeneous scales.)
    case = SimpleNamespace(regime="mixed", b=b, v=v)
    cpu = lambda t: None if t is None else t.detach().cpu()
    want = dict(zip(ac.FORWARD, map(cpu, ref)), **ac.gradient_groups(*(cpu(e.grad) if e is not None else None for e in ins64), case))
    got = dict(zip(ac.FORWARD, map(cpu, out)), **ac.gradient_groups(*(cpu(a.grad) if a is not None else None for a in ins), case))
    ins32 = [cpu(t).requires_grad_(True) if t is not None else None for t in ins]
    ref32 = _reference(*ins32, mask.cpu(), exponent, v)
    sum((e * w.cpu()).sum() for e, w in zip(ref32[:4], ws)).backward()
    f32 = dict(zip(ac.FORWARD, map(cpu, ref32)), **ac.gradient_groups(*(t.grad if t is not None else None for t in ins32), case))
    yard, errs = ac.group_errors(f32, want, case), ac.group_errors(got, want, case)
    print()
    for n, e in errs.items():
        limit = max(ac.FLOOR[n], ac.YARDSTICK_FACTOR * yard[n])
        print(f"    [adapter] mixed {n:13s} yardstick {yard[n]:.2e} kernel {e:.2e} bar {limit:.2e}")
        assert e <= limit, (n, e, limit)
    assert bool((got["d_scale"][0, :4, 1] == 0).all()) and bool((want["d_scale"][0, :4, 1] == 0).all())     # the clamped axis passes nothing


def test_encoder_takes_the_fused_adapter_and_matches_the_elementwise_path():
    """the style encoder on a GPU routes E10-E12 through vit_adapter_*; Gaussians, visualization_dump and input gradients equal
    the element-wise path's (fused_adapter = False)"""
    from styl3r_amd import vit_ops
    from styl3r_amd.encoder import EncoderNoPoSplatMultiTokenStyle, EncoderNoPoSplatTokenStyleCfg, GaussianAdapterCfg
    from tests.helpers import deterministic_init_
    from tests.gpu_utils import assert_close_rel
    tiny = dict(enc_depth=1, dec_depth=12, enc_embed_dim=1024, dec_embed_dim=128, enc_num_heads=16, dec_num_heads=2,
                pos_embed="RoPE100", img_size=(512, 512))
    dev = "cuda:0"
    m = deterministic_init_(EncoderNoPoSplatMultiTokenStyle(EncoderNoPoSplatTokenStyleCfg(gaussian_adapter=GaussianAdapterCfg(0.5, 15.0, 1)),
                                                            trunk_params=tiny).eval()).to(dev)
    g = torch.Generator(dev).manual_seed(2)
    img = torch.rand(2, 3, 3, 32, 48, device=dev, generator=g) * 2 - 1
    K = torch.tensor([[0.86, 0, 0.5], [0, 0.86, 0.5], [0, 0, 1.0]], device=dev).expand(2, 3, 3, 3).contiguous()
    style = torch.rand(2, 3, 32, 32, device=dev, generator=g) * 2 - 1
    res = {}
    for fused in (True, False):
        m.fused_adapter = fused
        before = vit_ops.CALLS["adapter_hip"]
        x = img.clone().requires_grad_(True)
        dump = {}
        gs = m(dict(image=x, intrinsics=K), dict(image=style), 0, dump)
        assert (vit_ops.CALLS["adapter_hip"] - before == 1) == fused
        (gs.means.sum() * 0.01 + gs.covariances.sum() * 1e3 + gs.harmonics.sum() + gs.opacities.sum()).backward()
        res[fused] = (gs, dump, x.grad)
    m.fused_adapter = True
    for name in ("means", "covariances", "harmonics", "opacities"):
        a, e = getattr(res[True][0], name), getattr(res[False][0], name)
        assert a.shape == e.shape
        assert_close_rel(a.detach().cpu().numpy(), e.detach().cpu().numpy(), 1e-5, name)
    for k in ("depth", "scales", "rotations", "means", "opacities"):
        a, e = res[True][1][k], res[False][1][k]
        assert a.shape == e.shape, k
        assert_close_rel(a.detach().cpu().numpy(), e.detach().cpu().numpy(), 1e-5, "dump " + k)
    assert_close_rel(res[True][2].cpu().numpy(), res[False][2].cpu().numpy(), 1e-3, "d image")   # deep fp32 gradient, two summation orders


# --------------------------------------------------------------------------- per regime, per gradient group (tests/adapter_cases.py)
DEV = "cuda:0"
REGIME_CASES = [(r, e, l) for r in ac.REGIMES for e in ac.EXPONENTS for l in ac.LAYOUTS]
ABI_LAYOUTS = ("app_b2_v3_5x7_sh2", "packed_b2_v1_5x7_sh0")          # 5 x 7: the last workgroup is partly empty; v = 1: no ptsr / parr


def _fused(pts0, ptsr, par0, parr, app, sh_mask, exponent, v):
    from styl3r_amd.vit_ops import gaussian_adapter_hip
    return gaussian_adapter_hip(pts0, ptsr, par0, parr, app, sh_mask, exponent, v, True)


def _report(tag, regime, layout, exponent, errs, other=None):
    """one line per group: yardstick (float32 expression on the CPU), measured error(s), bar -- `pytest -s` shows the table of DESIGN.md"""
    print()
    for n, e in errs.items():
        more = "" if other is None else f" elementwise {other[n]:.2e}"
        print(f"    [adapter] {tag} {regime:16s} {layout:22s} e={exponent} {n:13s} yardstick {ac.YARDSTICK[regime][n]:.2e} kernel {e:.2e}{more} bar {ac.bar(regime, n):.2e}")


@pytest.mark.parametrize("regime,exponent,layout", REGIME_CASES)
def test_adapter_kernels_per_regime_and_gradient_group(regime, exponent, layout):
    """every forward output and every gradient group of a case whose Gaussians all lie in one regime, against the float64 expression, each at
    max(floor, 4 x the float32 expression's own error); the gradients that are 0 by construction are 0 bit for bit"""
    case, want = ac.case_of(regime, layout), ac.reference(regime, layout, exponent)
    got = ac.evaluate(_fused, case, exponent, torch.float32, DEV)
    errs = ac.group_errors(got, want, case)
    _report("regime", regime, layout, exponent, errs)
    ac.assert_within_bars(errs, regime, f"{regime} {layout} exponent {exponent}")
    ac.assert_exact_zeros(got, regime, f"{regime} {layout} exponent {exponent}")


@pytest.mark.parametrize("regime,exponent", [(r, e) for r in ac.REGIMES for e in ac.EXPONENTS])
def test_fused_and_elementwise_paths_are_both_within_the_bar(regime, exponent):
    """the fused kernels and the element-wise float32 expression (what `fused_adapter = False` runs), both on the device, both against float64:
    neither path leans on the other"""
    layout = "app_b2_v3_5x7_sh2"
    case, want = ac.case_of(regime, layout), ac.reference(regime, layout, exponent)
    fused = ac.group_errors(ac.evaluate(_fused, case, exponent, torch.float32, DEV), want, case)
    elementwise = ac.group_errors(ac.evaluate(_reference, case, exponent, torch.float32, DEV), want, case)
    _report("paths ", regime, layout, exponent, fused, elementwise)
    ac.assert_within_bars(fused, regime, f"fused {regime} exponent {exponent}")
    ac.assert_within_bars(elementwise, regime, f"element-wise {regime} exponent {exponent}")


@pytest.mark.parametrize("regime", ac.REGIMES)
def test_two_runs_are_bit_identical(regime):
    layout = "packed_b1_v3_8x16_sh2"
    runs = [ac.evaluate(_fused, ac.case_of(regime, layout), 0.6, torch.float32, DEV) for _ in range(2)]
    for n in ac.FORWARD + ac.GRADIENT:
        a, e = runs[0][n].contiguous(), runs[1][n].contiguous()
        assert torch.equal(a.view(torch.int32), e.view(torch.int32)), n


# ---- the C ABI: guarded buffers
_PAD = 64                       # floats of canary on either side of every buffer
_CANARY = -7.0e11


def _guarded(n):
    """n floats, NaN-filled, inside a larger allocation of canaries"""
    buf = torch.full((n + 2 * _PAD,), _CANARY, dtype=torch.float32, device=DEV)
    buf[_PAD:_PAD + n] = float("nan")
    return buf


def _inner(buf):
    return buf[_PAD:buf.numel() - _PAD]


def _ptr(buf):
    return None if buf is None else _inner(buf).data_ptr()


def _canaries_intact(buf):
    bits = torch.tensor([_CANARY], dtype=torch.float32).view(torch.int32).item()
    raw = buf.view(torch.int32)
    return bool((raw[:_PAD] == bits).all()) and bool((raw[-_PAD:] == bits).all())


def _abi_forward(case, args, with_dump):
    from styl3r_amd import vit_ops
    n = case.b * case.v * case.H * case.W
    out = [_guarded(n * k) for k in (3, 9, 3 * case.d_sh, 1)] + ([_guarded(n * 3), _guarded(n * 4)] if with_dump else [None, None])
    vit_ops._check(vit_ops.load().vit_adapter_fwd(ct.byref(args), *map(_ptr, out), vit_ops._stream(torch.device(DEV))), "vit_adapter_fwd")
    return out


def _abi_backward(case, args, ins, ups):
    from styl3r_amd import vit_ops
    grads = [None if t is None else _guarded(t.numel()) for t in ins]
    vit_ops._check(vit_ops.load().vit_adapter_bwd(ct.byref(args), *(u.data_ptr() for u in ups), *map(_ptr, grads),
                                                  vit_ops._stream(torch.device(DEV))), "vit_adapter_bwd")
    return grads


@pytest.mark.parametrize("regime,layout", [(r, l) for r in ac.REGIMES for l in ABI_LAYOUTS])
def test_c_abi_writes_every_element_and_nothing_else(regime, layout):
    """vit_adapter_fwd / vit_adapter_bwd on buffers that sit inside larger allocations: every output and gradient element is written (the
    buffers start as NaN, the reference is finite in every regime), no byte around them changes, leaving out scales / rot changes no
    other output, a second run gives the same bytes, and v = 1 runs without ptsr / parr.  The values are the float64 expression's."""
    from styl3r_amd import vit_ops
    case, exponent = ac.case_of(regime, layout), 1.7
    ins = [None if t is None else t.to(DEV, torch.float32) for t in case.ins]
    mask = case.sh_mask.to(DEV, torch.float32)
    ups = [w.to(DEV, torch.float32).contiguous() for w in case.weights]
    p = lambda t: None if t is None else t.data_ptr()
    assert (case.v == 1) == (ins[1] is None and ins[3] is None)
    args = vit_ops.VitAdapterArgs(case.b, case.v, case.H, case.W, case.d_sh, ins[2].shape[1], exponent, *map(p, ins), p(mask))
    full, lean = _abi_forward(case, args, True), _abi_forward(case, args, False)
    again = _abi_forward(case, args, True)
    grads, grads_again = _abi_backward(case, args, ins, ups), _abi_backward(case, args, ins, ups)
    torch.cuda.synchronize()
    for name, a, l_, a2 in zip(ac.FORWARD, full, lean, again):
        assert _canaries_intact(a) and _canaries_intact(a2), name
        assert not bool(torch.isnan(_inner(a)).any()), f"{name}: elements left unwritten"
        assert torch.equal(a.view(torch.int32), a2.view(torch.int32)), f"{name}: two runs differ"
        if l_ is not None:
            assert _canaries_intact(l_) and torch.equal(a.view(torch.int32), l_.view(torch.int32)), f"{name} changes when scales / rot are left out"
    for name, t, a, a2 in zip(("d_pts0", "d_ptsr", "d_par0", "d_parr", "d_app"), ins, grads, grads_again):
        if t is None:
            continue
        assert _canaries_intact(a) and _canaries_intact(a2), name
        assert not bool(torch.isnan(_inner(a)).any()), f"{name}: elements left unwritten"
        assert torch.equal(a.view(torch.int32), a2.view(torch.int32)), f"{name}: two runs differ"
    G = case.v * case.H * case.W
    got = {n: _inner(a).reshape(case.b, G, *s) for n, a, s in zip(ac.FORWARD, full, ((3,), (3, 3), (3, case.d_sh), (), (3,), (4,)))}
    got.update(ac.gradient_groups(*(None if t is None else _inner(a).reshape(t.shape) for t, a in zip(ins, grads)), case))
    errs = ac.group_errors(got, ac.reference(regime, layout, exponent), case)
    ac.assert_within_bars(errs, regime, f"C ABI {regime} {layout}")
    ac.assert_exact_zeros(got, regime, f"C ABI {regime} {layout}")
