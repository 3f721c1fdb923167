"""-m gpu: the bandwidth-bound pass kernels on the dispatch paths the train step takes at 20 views x 256^2 -- past the grid cap with a ragged
last grid-stride round, every branch of the up-sampling dispatch (fast / LDS / shift-mask / generic / 16-byte-alignment fallback), and the
pure copies bit for bit.  Yardsticks: tests/pass_reference.py (host Philox, the float32-index bilinear operator, the unfold orders), float64
of the same expression, or the framework where it defines the result (max-pool, RoPE).

The launch caps of the sources are mirrored below; every test asserts that its shape is beyond (or on the intended side of) the mirrored
constant, so a later change of a cap makes the test fail instead of silently testing nothing.  The comment beside each bar gives the
distance measured on an MI355X; `PARITY_VERBOSE=1 pytest -s` prints them."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests import pass_reference as R
from tests.gpu_utils import assert_close_rel

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24

# ---- the launch caps, as the sources state them (workgroups of 256 threads) ----
RELU_DROPOUT_CAP_WG = 256 * 64    # vit_resample.hip, relu_dropout_fwd / _bwd: `(n4 + 255) / 256 < 256 * 64 ? (n4 + 255) / 256 : 256 * 64`; a lane = one float4
HEAD_TAIL_FWD_CAP_WG = 2048       # vit_head_tail.hip, ht_grid: `blocks < 2048 ? blocks : 2048`; a lane = one float4 of pixels
HEAD_TAIL_BWD_CAP_WG = 1024       # vit_head_tail.hip, head_tail_bwd: `(total + 255) / 256 < 1024 ? (total + 255) / 256 : 1024`
MAXPOOL_CAP_WG = 65536            # vit_lpips.hip, mp_grid: `b > 65536 ? 65536 : b`; a lane = one output
LN_FWD_CAP_WG = 2048              # vit_layernorm.hip, layernorm_fwd: `(M + 3) / 4 < 2048 ? (M + 3) / 4 : 2048`; a WAVE = one row, 4 rows per workgroup
LN_BWD_CAP_WG = 512               # vit_layernorm.hip, LN_BWD_BLOCKS (ln_blocks)
LN_MAX_C = 8 * 256                # vit_layernorm.hip, LN_MAX_N4 = 8 float4 per lane
ROPE_CAP_WG = 256 * 8             # vit_rope.hip, rope2d: `(total + 255) / 256 < 256 * 8 ? (total + 255) / 256 : 256 * 8`; a lane = one (token, head, d < D/4)
POINTMAP_CAP_WG = 4096            # gsr_points.hip, gsr_pointmap_post: `if (groups > 4096) groups = 4096`; a lane = one point
IM2COL3_MAX_GRID_Z = 65535        # vit_resample.hip, im2col3_rows: `gz > 65535`


def _lib():
    from styl3r_amd import vit_ops
    return vit_ops.load()


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _past_cap(count, per_round):
    """at least one full grid-stride round plus a remainder"""
    assert count > per_round and count % per_round != 0, (count, per_round)
    return count / per_round


def _say(what, value, bar, unit=""):
    if os.environ.get("PARITY_VERBOSE"):
        print(f"    [parity] {what}: {value:.3e}{unit} (bar {bar:.1e}{unit})")


def _randn(*shape, seed=0, dtype=torch.float32):
    return torch.randn(*shape, device=DEV, dtype=dtype, generator=torch.Generator(DEV).manual_seed(seed))


def _windows(n4, starts, count=4096):
    """element indices of `count` float4 from each start (clipped to the tensor)"""
    out = []
    for s in starts:
        s = max(0, min(int(s), n4 - count))
        out.append(np.arange(4 * s, 4 * (s + count), dtype=np.int64))
    return np.concatenate(out)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# =========================================================================================================================================
# a. past the grid cap, with a ragged last round
# =========================================================================================================================================
def test_relu_dropout_past_the_grid_cap_is_the_host_philox_mask_bit_for_bit():
    """vit_relu_dropout_fwd / _bwd over 2.5 grid-stride rounds: output bits = where(keep & x > 0, x * float32(1 / keep), 0) with keep from the
    host Philox at the first / last float4, across both round boundaries and at 100 000 random elements; over the whole tensor every
    output is 0 or x * scale, the kept fraction of the positives is 1 - p within 4 sigma, and the backward is g * scale exactly where y > 0."""
    from styl3r_amd import vit_ops
    shape, p, seed = (5, 8, 1024, 1025), 0.1, 0x1D2C_3B4A_5968_7071
    n = int(np.prod(shape)); n4 = n // 4
    per_round = RELU_DROPOUT_CAP_WG * 256
    assert n % 4 == 0 and _past_cap(n4, per_round) > 2 and n4 - 2 * per_round > 4096       # two round boundaries inside, a ragged third round
    x0 = _randn(*shape, seed=1)
    leaf = x0.clone().requires_grad_(True)
    y = vit_ops._ReluDropout.apply(leaf * 1.0, p, seed)
    scale = float(R.keep_scale(p))
    # ---- sampled, against the host generator ----
    idx = np.concatenate((_windows(n4, (0, n4 - 4096, per_round - 2048, 2 * per_round - 2048)),
                          np.random.default_rng(3).integers(0, n, 100_000)))
    ti = torch.from_numpy(idx).to(DEV)
    xs, ys = x0.reshape(-1)[ti].cpu().numpy(), y.detach().reshape(-1)[ti].cpu().numpy()
    keep = R.keep(seed, idx, p, "relu_dropout")
    want = np.where(keep & (xs > 0), xs * np.float32(scale), np.float32(0)).astype(np.float32)
    bad = np.nonzero(_bits(ys) != _bits(want))[0]
    assert bad.size == 0, (bad.size, idx[bad[:8]], ys[bad[:8]], want[bad[:8]])
    assert 0.85 < keep.mean() < 0.95
    # ---- the whole tensor ----
    yd = y.detach()
    kept, pos = yd > 0, x0 > 0
    assert torch.equal(yd, torch.where(kept, x0 * scale, torch.zeros_like(x0))) and not bool((kept & ~pos).any())
    npos = int(pos.sum()); frac = int(kept.sum()) / npos
    sigma = (p * (1 - p) / npos) ** 0.5
    _say("relu_dropout kept fraction - (1 - p)", abs(frac - (1 - p)) / sigma, 4.0, " sigma")        # measured 0.18 sigma
    assert abs(frac - (1 - p)) <= 4 * sigma, (frac, sigma)
    g = _randn(*shape, seed=2)
    y.backward(g)
    assert torch.equal(leaf.grad, torch.where(kept, g * scale, torch.zeros_like(g)))


@pytest.mark.parametrize("CO,p,bias", [(3, 0.0, True), (3, 0.1, True), (8, 0.0, True), (8, 0.1, True), (8, 0.1, False)])
def test_head_tail_past_both_grid_caps_matches_fp64(CO, p, bias):
    """vit_head_tail_fwd / _bwd at 1 310 760 float4 of pixels: 2.5 forward rounds; 5 backward rounds and a sixth with 40 live float4 in
    which every wave must still join the butterflies.  y, dh, dW, db against float64 of the same expression at the bars of the small-shape
    test; the mask is the host Philox's on sampled windows (read off dh, which is non-zero exactly where the element is kept and
    positive) and vit_relu_dropout_fwd's over the whole tensor."""
    from styl3r_amd import vit_ops
    B, Cc, H, W, seed = 3, 8, 1320, 1324, 987654321012345
    HW4 = H * W // 4; total = B * HW4
    assert (H * W) % 4 == 0 and total == 1_310_760
    assert _past_cap(total, HEAD_TAIL_FWD_CAP_WG * 256) > 2
    assert _past_cap(total, HEAD_TAIL_BWD_CAP_WG * 256) > 5 and total % (HEAD_TAIL_BWD_CAP_WG * 256) == 40       # a mostly dead last round
    h = _randn(B, Cc, H, W, seed=CO).requires_grad_(True)
    w = (_randn(CO, Cc, 1, 1, seed=11) / Cc ** 0.5).requires_grad_(True)
    b = _randn(CO, seed=12).requires_grad_(True) if bias else None
    y = vit_ops._HeadTail.apply(h, w, b, p, seed)
    g = _randn(B, CO, H, W, seed=13)
    y.backward(g)
    hd = h.detach()
    # ---- the mask ----
    if p > 0:
        a_mask = vit_ops._ReluDropout.apply(hd.clone() * 1.0, p, seed)
        kept = a_mask > 0
        del a_mask
        scale = float(R.keep_scale(p))
    else:
        kept, scale = hd > 0, 1.0
    n = hd.numel()
    idx = np.concatenate((_windows(n // 4, (0, n // 4 - 4096, HW4 - 2048, (B * Cc - 1) * HW4 - 2048)), np.random.default_rng(5).integers(0, n, 100_000)))
    ti = torch.from_numpy(idx).to(DEV)
    hs = hd.reshape(-1)[ti].cpu().numpy()
    host = (hs > 0) & (R.keep(seed, idx, p, "head_tail") if p > 0 else True)
    assert np.array_equal(h.grad.reshape(-1)[ti].cpu().numpy() != 0, host), "dh is not gated by the host Philox mask"
    assert np.array_equal(kept.reshape(-1)[ti].cpu().numpy(), host)
    # ---- float64 of the same expression ----
    fac = kept.double() * scale
    a = hd.double() * fac
    wd, gd = w.detach().double().reshape(CO, Cc), g.double()
    ref = torch.einsum("oc,bchw->bohw", wd, a) + (b.detach().double().reshape(1, CO, 1, 1) if bias else 0.0)
    assert_close_rel(y.detach().cpu().numpy(), ref.cpu().numpy(), 2e-6, f"head tail fwd CO={CO} p={p}")          # measured <= 1.8e-7
    del ref
    dh = torch.einsum("oc,bohw->bchw", wd, gd) * fac
    assert_close_rel(h.grad.cpu().numpy(), dh.cpu().numpy(), 2e-6, f"head tail dh CO={CO} p={p}")                # measured <= 1.3e-7
    del dh
    dw = torch.einsum("bohw,bchw->oc", gd, a)
    assert_close_rel(w.grad.reshape(CO, Cc).cpu().numpy(), dw.cpu().numpy(), 1e-5, f"head tail dW CO={CO} p={p}")    # measured <= 8.9e-7
    if bias:
        assert_close_rel(b.grad.cpu().numpy(), gd.sum((0, 2, 3)).cpu().numpy(), 1e-5, f"head tail db CO={CO} p={p}")     # measured <= 1.4e-6


def test_maxpool_past_the_grid_cap_equals_the_framework():
    from styl3r_amd import vit_ops
    shape = (5, 8, 2048, 1026)
    outputs = shape[0] * shape[1] * (shape[2] // 2) * (shape[3] // 2)
    assert outputs == 21_012_480 and _past_cap(outputs, MAXPOOL_CAP_WG * 256) > 1
    x = _randn(*shape, seed=4).requires_grad_(True)
    before = vit_ops.CALLS["maxpool_hip_fwd"], vit_ops.CALLS["maxpool_hip_bwd"], vit_ops.CALLS["framework_maxpool"]
    y = vit_ops.maxpool2x2(x)
    g = _randn(*y.shape, seed=5)
    y.backward(g)
    assert (vit_ops.CALLS["maxpool_hip_fwd"], vit_ops.CALLS["maxpool_hip_bwd"], vit_ops.CALLS["framework_maxpool"]) == (before[0] + 1, before[1] + 1, before[2])
    x2 = x.detach().clone().requires_grad_(True)
    ref = torch.nn.functional.max_pool2d(x2, 2, 2)
    ref.backward(g)
    assert torch.equal(y.detach(), ref.detach()) and torch.equal(x.grad, x2.grad)


@pytest.mark.parametrize("slot", [0, 1, 2, 3])
def test_maxpool_scan_order_with_nan_and_ties_equals_the_framework(slot):
    """the kernel's comment claims aten's scan (row-major over the window, `val > max || isnan(val)` replaces): a NaN in window position
    `slot`, and windows of equal values, must give the framework's output and route the gradient to the framework's element"""
    from styl3r_amd import vit_ops
    x = torch.randint(-1, 2, (2, 2, 4, 4), generator=torch.Generator().manual_seed(slot)).float()      # values -1, 0, 1: ties in every window
    x[0, 0] = 1.0                                                                                         # four equal values per window
    x[0, 1, slot // 2::2, slot % 2::2] = float("nan")                                                     # NaN at `slot` of every window of a plane
    x[1, 0, slot // 2, slot % 2] = float("nan")                                                           # ... and of one window among ties
    x[1, 1, 2, 2:4] = float("nan")                                                                        # two NaNs in one window
    x = x.to(DEV).requires_grad_(True)
    y = vit_ops.maxpool2x2(x)
    g = _randn(*y.shape, seed=6) + 3.0
    y.backward(g)
    x2 = x.detach().clone().requires_grad_(True)
    ref = torch.nn.functional.max_pool2d(x2, 2, 2)
    ref.backward(g)
    assert torch.equal(torch.isnan(y), torch.isnan(ref)) and torch.equal(y.detach().nan_to_num(9.0), ref.detach().nan_to_num(9.0))
    assert bool(torch.isnan(ref[0, 1]).all()) and torch.equal(x.grad, x2.grad)


def _ln_hip(x, gamma, beta, gy, eps=1e-6):
    """LayerNorm module -> (y, mean, rstd, dx, dgamma, dbeta), asserting that the HIP kernels ran and the framework path did not"""
    from styl3r_amd import vit_ops
    Cn = x.shape[-1]
    m = vit_ops.LayerNorm(Cn, eps=eps, bias=beta is not None).to(DEV)
    with torch.no_grad():
        m.weight.copy_(gamma)
        if beta is not None:
            m.bias.copy_(beta)
    before = dict(vit_ops.CALLS)
    xg = x.clone().requires_grad_(True)
    y = m(xg)
    stats = y.grad_fn.saved_tensors[2]
    y.backward(gy)
    ran = {k: vit_ops.CALLS[k] - before[k] for k in ("layernorm_hip_fwd", "layernorm_hip_bwd", "layernorm_framework")}
    assert ran == {"layernorm_hip_fwd": 1, "layernorm_hip_bwd": 1, "layernorm_framework": 0}, ran
    return y.detach(), stats[0], stats[1], xg.grad, m.weight.grad, (m.bias.grad if beta is not None else None)


def _ln_reference(x, gamma, beta, gy, eps=1e-6, dtype=torch.float64):
    xd = x.to(dtype).requires_grad_(True)
    wd = gamma.to(dtype).requires_grad_(True)
    bd = beta.to(dtype).requires_grad_(True) if beta is not None else None
    y = torch.nn.functional.layer_norm(xd, (x.shape[-1],), wd, bd, eps)
    y.backward(gy.to(dtype))
    mean = xd.detach().mean(-1)
    rstd = 1.0 / torch.sqrt(xd.detach().var(-1, unbiased=False) + eps)
    return y.detach(), mean, rstd, xd.grad, wd.grad, (bd.grad if beta is not None else None)


LN_NAMES = ("y", "mean", "rstd", "dx", "dgamma", "dbeta")
LN_BARS = dict(y=2e-6, mean=2e-6, rstd=2e-6, dx=5e-6, dgamma=1e-5, dbeta=1e-5)       # the bars of test_layernorm_kernels_match_fp64_with_and_without_skip


def _ln_inputs(M, Cn, seed, mean=0.7, std=3.0):
    x = std * _randn(M, Cn, seed=seed) + mean
    return x, 1 + 0.3 * _randn(Cn, seed=seed + 1), 0.2 * _randn(Cn, seed=seed + 2), _randn(M, Cn, seed=seed + 3)


@pytest.mark.parametrize("M,Cn", [(16387, 256), (1, 1024), (2, 1024), (3, 1024), (5, 1024), (37, 1280), (37, 1536), (37, 1792), (37, 2048)])
def test_layernorm_rounds_tiny_m_and_the_wide_instantiations_match_fp64(M, Cn):
    """two full forward rounds + 3 rows at C = 256 (8 backward rounds + 3 rows); fewer rows than the waves of one workgroup; and the
    C / 256 = 5 .. 8 instantiations, which the module takes itself (C <= 2048)"""
    if Cn == 256:
        assert _past_cap(M, LN_FWD_CAP_WG * 4) > 2 and M % (LN_FWD_CAP_WG * 4) == 3 and _past_cap(M, LN_BWD_CAP_WG * 4) > 8
    elif Cn == 1024:
        assert M <= 5                                        # one workgroup, idle waves (M < 4) or one wave with a second row (M = 5)
    else:
        assert Cn // 256 in (5, 6, 7, 8) and Cn <= LN_MAX_C and M % 4 != 0
    x, gamma, beta, gy = _ln_inputs(M, Cn, seed=M + Cn)
    got = _ln_hip(x, gamma, beta, gy)
    want = _ln_reference(x, gamma, beta, gy)
    for name, a, e in zip(LN_NAMES, got, want):                      # measured over the nine cases: y 1.3e-7, mean 1.3e-7, rstd 1.2e-7, dx 1.5e-7, dgamma 1.8e-7, dbeta 1.6e-7
        assert_close_rel(a.cpu().numpy(), e.cpu().numpy(), LN_BARS[name], f"ln {name} M={M} C={Cn}")


def test_layernorm_bwd_accumulate_adds_to_the_prefilled_parameter_gradients():
    """vit_layernorm_bwd(..., accumulate = 1) through the C ABI (the module never passes it): pre-fill + the accumulate = 0 result, the
    same bits as the addition on the host; dx is the same either way.  M spans more than one backward round."""
    lib = _lib()
    M, Cn = 2051, 512
    assert _past_cap(M, LN_BWD_CAP_WG * 4) > 1
    x, gamma, beta, gy = _ln_inputs(M, Cn, seed=9)
    y, mean, rstd = torch.empty_like(x), torch.empty(M, device=DEV), torch.empty(M, device=DEV)
    assert lib.vit_layernorm_fwd(x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), y.data_ptr(), mean.data_ptr(), rstd.data_ptr(), M, Cn, 1e-6, _stream()) == 0
    scratch = torch.empty(lib.vit_layernorm_scratch_bytes(M, Cn), dtype=torch.uint8, device=DEV)

    def bwd(dg, db, accumulate):
        dx = torch.empty_like(x)
        assert lib.vit_layernorm_bwd(gy.data_ptr(), x.data_ptr(), mean.data_ptr(), rstd.data_ptr(), gamma.data_ptr(), None, dx.data_ptr(),
                                     dg.data_ptr(), db.data_ptr(), scratch.data_ptr(), M, Cn, accumulate, _stream()) == 0
        return dx
    dg0, db0 = torch.full((Cn,), 7.0, device=DEV), torch.full((Cn,), 7.0, device=DEV)
    dx0 = bwd(dg0, db0, 0)
    pre_g, pre_b = 50 * _randn(Cn, seed=20), 50 * _randn(Cn, seed=21)
    dg1, db1 = pre_g.clone(), pre_b.clone()
    dx1 = bwd(dg1, db1, 1)
    assert torch.equal(dg1, pre_g + dg0) and torch.equal(db1, pre_b + db0) and torch.equal(dx1, dx0)
    want = _ln_reference(x, gamma, beta, gy)
    assert_close_rel(dg0.cpu().numpy(), want[4].cpu().numpy(), 1e-5, "ln dgamma (C ABI)")        # measured 1.6e-7
    assert_close_rel(db0.cpu().numpy(), want[5].cpu().numpy(), 1e-5, "ln dbeta (C ABI)")          # measured 1.0e-7


def test_layernorm_constant_row_is_finite_and_equals_beta():
    x, gamma, beta, gy = _ln_inputs(3, 1024, seed=31)
    x[1] = 1.25                                              # variance exactly 0: rstd = 1 / sqrt(eps)
    y, mean, rstd, dx, dg, db = _ln_hip(x, gamma, beta, gy)
    for t in (y, mean, rstd, dx, dg, db):
        assert bool(torch.isfinite(t).all())
    assert torch.equal(y[1], beta) and float(mean[1]) == 1.25 and abs(float(rstd[1]) - 1000.0) <= 1e-3


def test_layernorm_large_mean_small_spread_within_twice_the_frameworks_own_fp32_distance():
    """mean 30, std 0.3: x - mean cancels two decimal digits whoever computes it in fp32.  The bar of each output is twice the distance of
    the framework's fp32 F.layer_norm (same device, same input) from float64, with the usual bars as a floor."""
    M, Cn = 64, 1024
    x, gamma, beta, gy = _ln_inputs(M, Cn, seed=41, mean=30.0, std=0.3)
    got = _ln_hip(x, gamma, beta, gy)
    want = _ln_reference(x, gamma, beta, gy)
    fw = _ln_reference(x, gamma, beta, gy, dtype=torch.float32)
    for name, a, e, f in zip(LN_NAMES, got, want, fw):
        scale = float(e.abs().max())
        fw_rel = float((f.double() - e).abs().max()) / scale
        bar = max(LN_BARS[name], 2 * fw_rel)
        rel = float((a.double() - e).abs().max()) / scale
        # measured (kernel / framework): y 2.0e-6 / 1.9e-6, mean 6.5e-8 / 8.3e-8, rstd 9.9e-8 / 5.0e-7, dx 2.6e-7 / 3.8e-7, dgamma 2.8e-6 / 2.6e-6, dbeta 9.5e-8 / 1.7e-7
        print(f"    ln mean-30 {name}: kernel {rel:.3e}, framework fp32 {fw_rel:.3e}, bar {bar:.3e}")
        assert rel <= bar, (name, rel, fw_rel, bar)


def _rope_reference(t, pos, cos, sin):
    """the `half` expression of test_rope_kernel_matches_reference_golden_and_is_inplace_on_views, on t (B, H, N, 64)"""
    def half(x, p):
        c = torch.cat((cos, cos), -1)[p][:, None]; s = torch.cat((sin, sin), -1)[p][:, None]
        x1, x2 = x[..., :16], x[..., 16:]
        return x * c + torch.cat((-x2, x1), -1) * s
    return torch.cat((half(t[..., :32], pos[:, :, 0]), half(t[..., 32:], pos[:, :, 1])), -1)


def test_rope_past_the_grid_cap_contiguous_and_on_a_packed_qkv_view():
    from styl3r_amd.vit_ops import RoPE2D, rope_tables
    B, N, H, D = 10, 256, 16, 64
    assert _past_cap(B * N * H * (D // 4), ROPE_CAP_WG * 256) > 1
    cos, sin = rope_tables(D, 17, 100.0, torch.device(DEV))
    rope = RoPE2D(100.0, max_pos=16)
    grid = torch.stack(torch.meshgrid(torch.arange(16), torch.arange(16), indexing="ij"), -1).reshape(256, 2)
    gen = torch.Generator().manual_seed(8)
    pos = torch.stack([grid[torch.randperm(256, generator=gen)] for _ in range(B)]).to(DEV)          # (B, N, 2): the 16 x 16 positions, another order per image
    t = _randn(B, H, N, D, seed=7)
    ref = _rope_reference(t, pos, cos, sin)
    work = t.clone()
    out = rope(work, pos)
    assert out.data_ptr() == work.data_ptr() and torch.equal(out, ref)
    qkv = _randn(B, N, 3, H, D, seed=9)
    before = qkv.clone()
    rope(qkv[:, :, 0].transpose(1, 2), pos)
    assert torch.equal(qkv[:, :, 0].transpose(1, 2), _rope_reference(before[:, :, 0].transpose(1, 2), pos, cos, sin))
    assert torch.equal(qkv[:, :, 1:], before[:, :, 1:])              # k, v untouched


def test_pointmap_post_past_the_grid_cap_against_the_float64_expression():
    from styl3r_amd.points import pointmap_post, pointmap_post_expression
    P, H, W = 5, 512, 512
    per_round = POINTMAP_CAP_WG * 256
    assert _past_cap(P * H * W, per_round) > 1
    raw = torch.randn(P, 4, H, W, generator=torch.Generator().manual_seed(2)) * 1.5
    v = torch.tensor([0.3, -0.5, 0.81])
    special = []
    for p, (a, b, c) in ((0, ((0, 0), (0, 1), (2, 3))), (4, ((511, 509), (511, 511), (300, 7)))):       # before the cap and in the second round
        raw[p, :3, a[0], a[1]] = 0.0                                      # |xyz| = 0
        raw[p, :3, b[0], b[1]] = torch.tensor([1e-9, 0.0, 0.0])           # |xyz| = 1e-9: below the 1e-8 clip
        raw[p, :3, c[0], c[1]] = v / v.norm() * 20.0                      # |xyz| = 20: expm1 amplifies the error of the norm twenty-fold
        raw[p, 3, 1, 1] = 12.0
        special.append([p * H * W + y * W + x for y, x in (a, b, c)])
    assert max(special[0]) < per_round < min(special[1])
    want = pointmap_post_expression(raw.double())
    got = pointmap_post(raw.to(DEV))
    assert got["pts3d"].shape == (P, H, W, 3) and got["conf"].shape == (P, H, W) and got["pts3d"].dtype == torch.float32
    for k in ("pts3d", "conf"):
        err = (got[k].cpu().double() - want[k]).abs()
        worst = float((err / want[k].abs().clamp_min(1e-300)).max())
        _say(f"pointmap_post {k} (element-wise relative)", worst, 1e-6)                          # measured: pts3d 6.0e-8, conf 1.1e-7
        assert (err <= 1e-6 * want[k].abs()).all(), (k, worst)
    assert float(got["pts3d"][0, 0, 0].abs().max()) == 0.0 and float(got["pts3d"][4, 511, 509].abs().max()) == 0.0
    assert float(want["pts3d"][4, 300, 7].norm()) > 4e8


# =========================================================================================================================================
# b. up-sampling: every dispatch branch
# =========================================================================================================================================
def _pow2(v):
    return v > 0 and v & (v - 1) == 0


def _fwd_branch(planes, H, W, ptr):
    """upsample_p2_ok of vit_resample.hip, restated"""
    ow4 = 2 * W // 4
    return "fast" if W % 4 == 0 and ow4 <= 256 and _pow2(ow4) and planes * 2 * H < 0x7fffffff and ptr % 16 == 0 else "generic"


def _bwd_branch(planes, H, W, ptr):
    """the dispatch of upsample2x_bwd of vit_resample.hip, restated"""
    Rr = 256 // W if _pow2(W) and 2 <= W <= 256 else 0
    if Rr and _pow2(H) and H >= Rr and planes * (H // Rr) < 0x7fffffff and ptr % 16 == 0:
        return "lds"
    if _pow2(W) and planes * H * W < 0x7fffffff:
        return "shift"
    return "generic"


def _misaligned(t):
    """the same values as a contiguous view that starts 4 bytes into a larger buffer"""
    buf = torch.zeros(t.numel() + 8, device=t.device, dtype=t.dtype)
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and buf.data_ptr() % 16 == 0 and v.data_ptr() % 16 == 4
    return v


FWD_BAR, BWD_BAR = 8.0, 24.0          # units of 2^-24 max|input|: four taps with at most six roundings on a path plus the rounding of 1 - lambda;
#                                       at most nine non-zero taps per axis pair with total weight <= 4


@pytest.mark.parametrize("shape,branch", [
    ((3, 5, 128), "fast"),        # the production width; 30 rows, not a multiple of the 4 rows of a workgroup
    ((2, 3, 4), "fast"),          # 128 rows per workgroup
    ((1, 2, 512), "fast"),        # one row per workgroup, the whole LDS tile in use
    ((3, 1, 8), "fast"),          # H = 1
    ((2, 7, 6), "generic"), ((1, 16, 24), "generic"), ((1, 2, 1024), "generic")])
def test_upsample_forward_every_branch_against_the_float32_index_operator(shape, branch):
    from styl3r_amd import vit_ops
    P, H, W = shape
    x = _randn(1, P, H, W, seed=H * 100 + W)
    c = _randn(1, P, 2 * H, 2 * W, seed=H * 100 + W + 1)                 # both signs: the fused ReLU matters
    assert x.data_ptr() % 16 == 0 and _fwd_branch(P, H, W, x.data_ptr()) == branch
    before = vit_ops.CALLS["framework_upsample"]
    y = vit_ops.upsample2x(x)
    z = vit_ops._UpsampleAddRelu.apply(x, c)
    assert vit_ops.CALLS["framework_upsample"] == before and y.shape == (1, P, 2 * H, 2 * W)
    up = R.upsample_forward(x.cpu().numpy()[0])
    xmax = float(x.abs().max())
    e_y = np.abs(y.cpu().numpy()[0] - up).max() / (U * xmax)
    e_z = np.abs(z.cpu().numpy()[0] - (up + np.maximum(c.cpu().numpy()[0].astype(np.float64), 0))).max() / (U * xmax)
    _say(f"upsample fwd {shape} {branch}", e_y, FWD_BAR, " units")                              # measured <= 1.2 units (fast), <= 1.1 (generic)
    _say(f"upsample+relu+add fwd {shape} {branch}", e_z, FWD_BAR, " units")                     # measured <= 2.2 units (fast), <= 1.7 (generic)
    assert e_y <= FWD_BAR and e_z <= FWD_BAR, (shape, e_y, e_z)
    assert bool((c < 0).any()) and bool((c > 0).any())


def test_upsample_forward_alignment_fallback_gives_the_fast_kernels_bits():
    """an input 4 bytes off a 16-byte boundary cannot be read by the fast kernel's float4 loads: the dispatch must take the generic
    kernel, whose arithmetic is the same in the same order"""
    from styl3r_amd import vit_ops
    P, H, W = 3, 5, 128
    x = _randn(1, P, H, W, seed=77)
    c = _randn(1, P, 2 * H, 2 * W, seed=78)
    xm = _misaligned(x)
    assert _fwd_branch(P, H, W, x.data_ptr()) == "fast" and _fwd_branch(P, H, W, xm.data_ptr()) == "generic"
    assert torch.equal(vit_ops.upsample2x(xm), vit_ops.upsample2x(x))
    assert torch.equal(vit_ops._UpsampleAddRelu.apply(xm, c), vit_ops._UpsampleAddRelu.apply(x, c))
    assert torch.equal(xm, x)


def _upsample_bwd(dout, H, W):
    P = dout.shape[0]
    din = torch.full((P, H, W), 7.0, device=DEV)
    assert _lib().vit_upsample2x_bwd(dout.data_ptr(), din.data_ptr(), P, H, W, _stream()) == 0
    return din


@pytest.mark.parametrize("shape,branch", [
    ((2, 128, 2), "lds"),         # R = 128: a single band, both clamps of the band in one workgroup
    ((2, 16, 16), "lds"),         # a single band
    ((2, 64, 16), "lds"),         # first, interior and last bands
    ((2, 128, 128), "lds"),       # production, R = 2
    ((2, 4, 256), "lds"),         # R = 1
    ((10, 8, 8), "shift"),        # H < R
    ((2, 48, 64), "shift"),       # H not a power of two
    ((1, 2, 512), "shift"),       # W > 256
    ((2, 7, 6), "generic"), ((1, 16, 24), "generic")])
def test_upsample_backward_every_branch_against_the_float32_index_operator(shape, branch):
    P, H, W = shape
    g = _randn(P, 2 * H, 2 * W, seed=H * 100 + W + 2)
    assert _bwd_branch(P, H, W, g.data_ptr()) == branch
    din = _upsample_bwd(g, H, W)
    err = np.abs(din.cpu().numpy() - R.upsample_backward(g.cpu().numpy())).max() / (U * float(g.abs().max()))
    _say(f"upsample bwd {shape} {branch}", err, BWD_BAR, " units")                               # measured <= 3.2 units (LDS), <= 2.6 (shift / mask), <= 2.4 (generic)
    assert err <= BWD_BAR, (shape, err)


def test_upsample_backward_alignment_fallback_gives_the_lds_kernels_bits():
    P, H, W = 2, 64, 16
    g = _randn(P, 2 * H, 2 * W, seed=88)
    gm = _misaligned(g)
    assert _bwd_branch(P, H, W, g.data_ptr()) == "lds" and _bwd_branch(P, H, W, gm.data_ptr()) == "shift"
    assert torch.equal(_upsample_bwd(gm, H, W), _upsample_bwd(g, H, W))


@pytest.mark.parametrize("shape,branch", [((2, 64, 16), "lds"), ((2, 7, 6), "generic")])
def test_upsample_backward_of_an_overflowed_gradient_is_inf_only_under_nonzero_weights(shape, branch):
    """the kernel selects zero-weight taps away instead of multiplying by 0 (0 * inf = NaN): din is +inf exactly at the input pixels with
    a non-zero weight on an infinite output gradient, finite and right elsewhere.  The framework's scatter does not promise this; the
    operator with zero-weight taps skipped is the reference."""
    P, H, W = shape
    g = _randn(P, 2 * H, 2 * W, seed=99)
    gmax = float(g.abs().max())
    g[0, 0, 0] = g[P - 1, 2 * H - 1, 2 * W - 1] = g[0, H + 1, W - 1] = float("inf")
    assert _bwd_branch(P, H, W, g.data_ptr()) == branch
    got = _upsample_bwd(g, H, W).cpu().numpy()
    want = R.upsample_backward(g.cpu().numpy())
    inf = np.isposinf(want)
    assert not np.isnan(got).any() and np.array_equal(np.isposinf(got), inf) and not np.isneginf(got).any()
    assert inf[0, 0, 0] and inf[P - 1, H - 1, W - 1] and 3 <= inf.sum() <= 1 + 4 + 4
    err = np.abs(got[~inf] - want[~inf]).max() / (U * gmax)
    _say(f"upsample bwd with inf {shape} {branch}", err, BWD_BAR, " units")                    # measured 1.8 units (LDS), 2.6 (generic)
    assert err <= BWD_BAR


# =========================================================================================================================================
# c. the copies, exactly; argument checks launch nothing
# =========================================================================================================================================
@pytest.mark.parametrize("B,H,W", [(2, 1, 4), (1, 2, 8), (3, 9, 12), (1, 5, 64)])
def test_im2col7_is_the_unfold_order_exactly(B, H, W):
    img = _randn(B, 3, H, W, seed=B + H + W)
    cols = torch.full((B, 160, H, W), 7.0, device=DEV)
    assert _lib().vit_im2col7(img.data_ptr(), cols.data_ptr(), B, H, W, _stream()) == 0
    assert torch.equal(cols, R.im2col7_reference(img)) and float(cols[:, 147:].abs().max()) == 0.0


@pytest.mark.parametrize("Ci", [1, 31, 32, 33, 48])
def test_im2col3_rows_is_the_unfold_order_exactly(Ci):
    B = 2                                                    # blockIdx.z = (b, channel tile)
    for H, W in ((1, 1), (2, 31), (5, 33), (3, 70)):
        x = _randn(B, Ci, H, W, seed=Ci + H + W)
        assert bool((x < 0).any()) or x.numel() < 4
        for relu in (0, 1):
            cols = torch.full((B * H * W, 9 * Ci), 7.0, device=DEV)
            assert _lib().vit_im2col3_rows(x.data_ptr(), cols.data_ptr(), B, Ci, H, W, relu, _stream()) == 0
            assert torch.equal(cols, R.im2col3_rows_reference(x, bool(relu))), (Ci, H, W, relu)


def test_argument_checks_return_einval_and_launch_nothing():
    lib, s = _lib(), _stream()
    src = torch.ones(1 << 16, device=DEV)
    out = torch.full((1 << 16,), 7.0, device=DEV)
    a, o = src.data_ptr(), out.data_ptr()
    assert lib.vit_upsample2x_fwd(a, o, 2, 4, 5, s) == -1                                    # odd W
    assert lib.vit_upsample2x_add_relu_fwd(a, a, o, 2, 4, 5, s) == -1
    assert lib.vit_im2col7(a, o, 1, 4, 6, s) == -1                                           # W % 4 != 0
    for Cc, CO, HW in ((12, 3, 16), (264, 8, 16), (8, 5, 16), (8, 3, 6)):                    # C % 8, C > 256, CO = 5, HW % 4
        assert lib.vit_head_tail_fwd(a, a, a, o, 1, Cc, CO, HW, 0.1, 1, s) == -1, (Cc, CO, HW)
        assert lib.vit_head_tail_bwd(a, a, a, o, o, o, 1, Cc, CO, HW, 0.1, 1, s) == -1, (Cc, CO, HW)
    assert (IM2COL3_MAX_GRID_Z + 1) * ((1 + 31) // 32) > IM2COL3_MAX_GRID_Z
    assert lib.vit_im2col3_rows(a, o, IM2COL3_MAX_GRID_Z + 1, 1, 1, 1, 0, s) == -1           # B * ceil(Ci / 32) > 65 535
    assert lib.vit_im2col3_rows(a, o, 32768, 33, 1, 1, 0, s) == -1                           # 32 768 images x 2 channel tiles
    torch.cuda.synchronize()
    assert float(out.min()) == 7.0 and float(out.max()) == 7.0 and float(src.min()) == 1.0
