"""-m gpu: point-map distillation on the device -- the exact radix selection, the Regr3D kernels against the float64 expression, the
teacher's post-processing and forward against the reference, and the distillation modes of the train step."""
import ctypes as C

import pytest
import torch

from tests.test_distill_host import F, MODES, distill_batch, tiny_student, tiny_teacher

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
Q = torch.tensor([0.002, 0.998])


def _hip(gt1, gt2, pr1, pr2, c1, c2, norm_mode=None, **kw):
    from styl3r_amd.losses import Regr3D
    d = {}
    loss = Regr3D(norm_mode=norm_mode)(gt1, gt2, pr1, pr2, c1, c2, details=d, **kw)
    assert set(d) == {"status", "quantiles", "valid"}, "the kernels did not run"
    return loss, d


def _same_bits(a, b):
    a, b = a.cpu(), b.cpu()
    return bool(((a == b) | (torch.isnan(a) & torch.isnan(b))).all())


def _z_rows(B, N, seed):
    """|gt| exact in fp32 whatever the operation order: points on the z axis.  Rows: random, quantised to 1/8 (heavy ties), all equal,
    one NaN, random with three points of |gt| = 0 and (N >= 1536) one of |gt| = +inf -- key 0 and key 0x7f800000, the two ends of the radix
    range; the inf has no NaN component and lies above the 99.8 % rank (B = 1: the random row only)."""
    g = torch.Generator().manual_seed(seed)
    z = (torch.randn(B, N, generator=g) * 2).abs() + 0.01
    if B >= 4:
        z[1] = (z[1] * 8).round() / 8
        z[2] = 1.25
        z[3, N // 3] = float("nan")
        z[4, [1, N // 2, N - 1]] = 0.0
        if N >= 1536:
            z[4, N // 5] = float("inf")
    sign = torch.where(torch.rand(B, N, generator=g) < 0.5, -1.0, 1.0)
    return z, torch.stack((torch.zeros_like(z), torch.zeros_like(z), z * sign), dim=-1)


@pytest.mark.parametrize("B", [1, 5])
# r < 1 (lo = 0); both ranks integral (w == 0); one workgroup per map; 8 192: the last size on one workgroup, every register slot full; 8 193: the
# first on several (9 chunks of 911: the last 256-lane step of a chunk has dead lanes); 40 001 (B = 5: 40 chunks of 1 001); 65 536: whole chunks
@pytest.mark.parametrize("N", [256, 501, 1536, 8192, 8193, 40001, 65536])
def test_selection_is_exact(N, B):
    from styl3r_amd._lib import GSR_PT_NAN
    d1, gt1 = _z_rows(B, N, 10 + N)
    d2, gt2 = _z_rows(B, N, 20 + N)
    if B >= 4:
        for d, gt in ((d1, gt1), (d2, gt2)):
            assert int((d[4] == 0).sum()) == 3 and int(torch.isinf(d[4]).sum()) == (1 if N >= 1536 else 0) and not torch.isnan(gt[4]).any()
            assert torch.isfinite(torch.quantile(d[4], Q)).all()          # the yardstick's own row is finite: the inf lies above the 99.8 % rank
    conf = torch.full((B, N), 5.0)
    loss, det = _hip(gt1.to(DEV), gt2.to(DEV), (gt1 + 0.1).nan_to_num(0.0).to(DEV), (gt2 - 0.1).nan_to_num(0.0).to(DEV), conf.to(DEV), conf.to(DEV))
    want = torch.stack((torch.quantile(d1, Q, dim=1).t(), torch.quantile(d2, Q, dim=1).t()))        # (2, B, 2)
    got = det["quantiles"].cpu()
    assert _same_bits(got, want), (N, B, got, want)
    dis = torch.stack((d1, d2))
    mask = (dis >= want[..., 0:1]) & (dis <= want[..., 1:2])
    assert torch.equal(det["valid"].cpu().bool(), mask)
    status = det["status"].cpu()
    assert torch.equal(status[..., 0], mask.sum(-1).int())
    nan_rows = torch.isnan(dis).any(-1)
    assert torch.equal((status[..., 1] & GSR_PT_NAN) != 0, nan_rows) and (B < 4 or bool(nan_rows.any()))
    assert not mask[nan_rows].any() and torch.isfinite(loss)


def test_both_selection_paths_are_exact_on_a_shared_prefix():
    """8 192 points of one row on the one-workgroup path, the same points and one more on the chunked path"""
    d, gt = _z_rows(1, 8193, 77)
    for n in (8192, 8193):
        g = gt[:, :n].contiguous().to(DEV)
        conf = torch.full((1, n), 5.0, device=DEV)
        _, det = _hip(g, g, g + 0.1, g - 0.1, conf, conf)
        want = torch.quantile(d[:, :n], Q, dim=1).t()
        assert _same_bits(det["quantiles"].cpu(), torch.stack((want, want))), (n, det["quantiles"], want)


def _clouds(seed=5, B=3, N=1536):
    g = torch.Generator().manual_seed(seed)
    gt1 = torch.randn(B, N, 3, generator=g) * 2
    gt2 = torch.randn(B, N, 3, generator=g) * 2 + 0.5
    pr1 = gt1 + 0.1 * torch.randn(B, N, 3, generator=g)
    pr2 = gt2 + 0.1 * torch.randn(B, N, 3, generator=g)
    c1 = 1 + torch.exp(torch.randn(B, N, generator=g) + 1)
    c2 = 1 + torch.exp(torch.randn(B, N, generator=g) + 1)
    return gt1, gt2, pr1, pr2, c1, c2


@pytest.mark.parametrize("mode", list(MODES))
def test_mask_loss_and_gradients_on_random_clouds(mode):
    from styl3r_amd.losses import regr3d_expression, regr3d_valid_masks
    kw = dict(MODES[mode])
    ins = _clouds()
    # ---- a property of the INPUTS: no decision of the mask sits within 1e-6 of its threshold ----
    gt1d, gt2d, pr1d, pr2d, c1d, c2d = (t.double() for t in ins)
    v1, v2, quant = regr3d_valid_masks(gt1d, gt2d, c1d, c2d, kw.get("dist_clip"))
    for dis, k in ((gt1d.norm(dim=-1), 0), (gt2d.norm(dim=-1), 1)):
        if quant is None:
            assert ((dis - kw["dist_clip"]).abs() > 1e-6 * kw["dist_clip"]).all()
        else:
            for j in range(2):
                assert ((dis - quant[k, :, j:j + 1]).abs() > 1e-6 * quant[k, :, j:j + 1]).all()
    assert ((c1d - 3).abs() > 1e-6).all() and ((c2d - 3).abs() > 1e-6).all()
    # ---- the float64 yardstick ----
    pr1d.requires_grad_(True); pr2d.requires_grad_(True)
    want = regr3d_expression(gt1d, gt2d, pr1d, pr2d, c1d, c2d, **kw)
    want.backward()
    g1w = pr1d.grad if pr1d.grad is not None else torch.zeros_like(pr1d)
    g2w = pr2d.grad
    # ---- the kernels ----
    gt1, gt2, pr1, pr2, c1, c2 = (t.to(DEV) for t in ins)
    pr1.requires_grad_(True); pr2.requires_grad_(True)
    loss, det = _hip(gt1, gt2, pr1, pr2, c1, c2, **kw)
    loss.backward()
    valid = det["valid"].cpu().bool()
    assert torch.equal(valid[0], v1) and torch.equal(valid[1], v2)
    loss, want = float(loss.detach()), float(want.detach())
    print(f"  {mode}: loss {loss:.9f} vs {want:.9f} (rel {abs(loss - want) / want:.2e}), valid {int(v1.sum())} + {int(v2.sum())}")
    assert abs(loss - want) <= 1e-6 * want
    for got, ref, v, name in ((pr1.grad.cpu(), g1w, v1, "d pr1"), (pr2.grad.cpu(), g2w, v2, "d pr2")):
        scale = float(ref.abs().max())
        err = float((got.double() - ref).abs().max())
        print(f"  {mode}: {name} max err {err:.3e} of scale {scale:.3e}")
        assert err <= 2e-6 * max(scale, 1e-30), (mode, name, err, scale)
        assert float(got[~v].abs().max()) == 0.0, (mode, name)


def test_strided_means_are_read_in_place_and_runs_are_bit_identical():
    b, h, w = 2, 24, 32
    g = torch.Generator().manual_seed(3)
    means = (torch.randn(b, 3, h, w, 1, 3, generator=g) * 2).to(DEV).requires_grad_(True)
    gt1 = (means.detach()[:, 0].squeeze(-2) + 0.1 * torch.randn(b, h, w, 3, generator=g).to(DEV)).contiguous()
    gt2 = (means.detach()[:, 1].squeeze(-2) + 0.1 * torch.randn(b, h, w, 3, generator=g).to(DEV)).contiguous()
    conf = (1 + torch.exp(torch.randn(b, h, w, generator=g) + 1)).to(DEV)
    for norm_mode in (None, "avg_dis"):
        out = []
        for strided in (True, False, True):
            means.grad = None
            if strided:
                p1, p2 = means[:, 0].squeeze(-2), means[:, 1].squeeze(-2)
                assert not p1.is_contiguous()
            else:
                p1 = means.detach()[:, 0].squeeze(-2).contiguous().requires_grad_(True)
                p2 = means.detach()[:, 1].squeeze(-2).contiguous().requires_grad_(True)
            loss, _ = _hip(gt1, gt2, p1, p2, conf, conf, norm_mode=norm_mode)
            loss.backward()
            grads = (means.grad[:, 0, :, :, 0], means.grad[:, 1, :, :, 0]) if strided else (p1.grad, p2.grad)
            if strided:
                assert float(means.grad[:, 2].abs().max()) == 0.0          # the third view is not part of the loss
            out.append((loss.detach().clone(), grads[0].clone(), grads[1].clone()))
        for other in out[1:]:
            assert all(torch.equal(x, y) for x, y in zip(out[0], other)), norm_mode
        assert float(out[0][1].abs().max()) > 0


@pytest.mark.parametrize("norm_mode", [None, "avg_dis"])
def test_no_confident_point_gives_zero_loss_zero_gradients_and_the_status_code(norm_mode):
    from styl3r_amd._lib import GSR_PT_EMPTY_MAP, GSR_PT_EMPTY_VIEW
    gt1, gt2, pr1, pr2, c1, c2 = (t.to(DEV) for t in _clouds(B=2, N=600))
    pr1.requires_grad_(True); pr2.requires_grad_(True)
    low = torch.full_like(c1, 2.5)
    loss, det = _hip(gt1, gt2, pr1, pr2, low, low, norm_mode=norm_mode)
    loss.backward()
    assert float(loss.detach()) == 0.0 and float(pr1.grad.abs().max()) == 0.0 and float(pr2.grad.abs().max()) == 0.0
    st = det["status"].cpu()
    assert (st[..., 0] == 0).all() and ((st[..., 1] & (GSR_PT_EMPTY_MAP | GSR_PT_EMPTY_VIEW)) == (GSR_PT_EMPTY_MAP | GSR_PT_EMPTY_VIEW)).all()
    # one view empty: the other still counts, and nothing is NaN
    pr1.grad = None; pr2.grad = None
    loss, det = _hip(gt1, gt2, pr1, pr2, low, c2, norm_mode=norm_mode)
    loss.backward()
    assert float(loss.detach()) > 0 and torch.isfinite(pr2.grad).all() and float(pr2.grad.abs().max()) > 0
    st = det["status"].cpu()
    assert (st[0, :, 1] & GSR_PT_EMPTY_VIEW).all() and not (st[1, :, 1] & GSR_PT_EMPTY_VIEW).any()


def test_c_abi_rejects_bad_arguments_before_any_launch():
    from styl3r_amd import _lib
    lib = _lib.load()
    B, N = 2, 64
    t = lambda *s: torch.ones(*s, device=DEV)
    gt, conf, pr = t(B, N, 3), t(B, N), t(B, N, 3)
    scratch = torch.empty(lib.gsr_regr3d_scratch_bytes(B, N), dtype=torch.uint8, device=DEV)
    loss, status = torch.full((1,), 7.0, device=DEV), torch.zeros(2, B, 2, dtype=torch.int32, device=DEV)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def fwd(gt1=gt.data_ptr(), B_=B, N_=N, s1=3 * N, norm=0, scratch_=scratch.data_ptr()):
        return lib.gsr_regr3d_fwd(gt1, gt.data_ptr(), conf.data_ptr(), conf.data_ptr(), pr.data_ptr(), pr.data_ptr(), s1, 3 * N, B_, N_, norm, 0, 0.0,
                                  scratch_, loss.data_ptr(), status.data_ptr(), None, None, stream)
    assert fwd() == 0
    torch.cuda.synchronize()
    loss.fill_(7.0)
    for bad in (dict(gt1=None), dict(B_=0), dict(N_=1), dict(s1=3 * N - 1), dict(norm=2), dict(scratch_=None)):
        assert fwd(**bad) == -1, bad
    grad = t(B, N, 3)
    g = t(1)
    bwd = lambda g_=g.data_ptr(), B_=B, N_=N: lib.gsr_regr3d_bwd(gt.data_ptr(), gt.data_ptr(), pr.data_ptr(), pr.data_ptr(), 3 * N, 3 * N, B_, N_, 0, 0, g_,
                                                                scratch.data_ptr(), grad.data_ptr(), grad.data_ptr(), stream)
    assert bwd(g_=None) == -1 and bwd(B_=0) == -1 and bwd(N_=1) == -1
    assert lib.gsr_pointmap_post(None, 1, 4, 4, grad.data_ptr(), grad.data_ptr(), stream) == -1
    assert lib.gsr_pointmap_post(grad.data_ptr(), 0, 4, 4, grad.data_ptr(), grad.data_ptr(), stream) == -1
    assert lib.gsr_regr3d_scratch_bytes(0, N) == 0 and lib.gsr_regr3d_scratch_bytes(B, 1) == 0
    torch.cuda.synchronize()
    assert float(loss) == 7.0 and float(grad.min()) == 1.0          # nothing was launched


def test_pointmap_post_against_the_float64_expression():
    from styl3r_amd.points import pointmap_post, pointmap_post_expression
    g = torch.Generator().manual_seed(2)
    raw = torch.randn(3, 4, 9, 13, generator=g) * 1.5
    raw[0, :3, 0, 0] = 0.0                                            # |xyz| = 0
    raw[0, :3, 0, 1] = torch.tensor([1e-9, 0.0, 0.0])                 # |xyz| = 1e-9: below the 1e-8 clip
    v = torch.tensor([0.3, -0.5, 0.81])
    raw[1, :3, 2, 3] = v / v.norm() * 20.0                            # |xyz| = 20: expm1 amplifies the error of the norm twenty-fold
    raw[2, 3, 1, 1] = 12.0
    want = pointmap_post_expression(raw.double())
    got = pointmap_post(raw.to(DEV))
    assert got["pts3d"].shape == (3, 9, 13, 3) and got["conf"].shape == (3, 9, 13) and got["pts3d"].dtype == torch.float32
    for k in ("pts3d", "conf"):
        err = (got[k].cpu().double() - want[k]).abs()
        assert (err <= 1e-6 * want[k].abs()).all(), (k, float((err / want[k].abs().clamp_min(1e-300)).max()))
    assert float(got["pts3d"][0, 0, 0].abs().max()) == 0.0 and float(want["pts3d"][1, 2, 3].norm()) > 4e8


def test_tiny_teacher_matches_the_reference_on_the_device():
    from tests.gpu_utils import assert_close_rel
    m = tiny_teacher().to(DEV)
    r1, r2 = m({"image": torch.tensor(F["t_image"], device=DEV)}, False)
    for r, k in ((r1, "1"), (r2, "2")):
        assert r["pts3d"].is_cuda and not r["pts3d"].requires_grad
        assert_close_rel(r["pts3d"].cpu().numpy(), F["t_pts" + k], 2e-5, "pts3d " + k)
        assert_close_rel(r["conf"].cpu().numpy(), F["t_conf" + k], 2e-5, "conf " + k)


def _teacher_targets(teacher, enc, batch, **kw):
    from styl3r_amd.losses import Regr3D
    with torch.no_grad():
        dump = {}
        out = enc(batch["context"], {"image": batch["context"]["image"][:, 0]}, 0, visualization_dump=dump, **kw)
        gt1, gt2 = teacher(batch["context"], False)
        m = dump["means"]
        return out, Regr3D(norm_mode=None)(gt1["pts3d"], gt2["pts3d"], m[:, 0].squeeze(-2), m[:, 1].squeeze(-2), gt1["conf"], gt2["conf"])


def test_train_step_distill_only_on_the_device():
    from styl3r_amd.train import TrainStep
    enc, teacher, batch = tiny_student(DEV), tiny_teacher().to(DEV), distill_batch(DEV)
    none, want = _teacher_targets(teacher, enc, batch, distill_only=True)
    assert none is None and float(want) > 0
    step = TrainStep(enc, None, distiller=teacher, distill_only=True)
    loss = step(batch)
    assert abs(float(loss) - float(want)) <= 1e-5 * float(want), (float(loss), float(want))
    with_grad = {n for n, p in enc.named_parameters() if p.grad is not None and float(p.grad.abs().max()) > 0}
    assert with_grad and all(n.startswith(("structure_builder.", "downstream_head1.", "backbone.")) for n in with_grad), sorted(with_grad)[:5]
    for part in ("structure_builder.", "downstream_head1.", "backbone."):
        assert any(n.startswith(part) for n in with_grad), part
    assert all(p.grad is None for n, p in enc.named_parameters() if n.startswith(("token_stylizer.", "gaussian_")))
    assert all(p.grad is None for p in teacher.parameters())


def test_train_step_adds_the_distillation_loss_to_the_render_loss():
    from styl3r_amd.decoder import DecoderSplattingCUDACfg, get_decoder
    from styl3r_amd.losses import mse_loss
    from styl3r_amd.scenes import make_scene
    from styl3r_amd.train import TrainStep
    enc, teacher, batch = tiny_student(DEV), tiny_teacher().to(DEV), distill_batch(DEV)
    dec = get_decoder(DecoderSplattingCUDACfg("splatting_cuda", [0.0, 0.0, 0.0], True)).to(DEV)
    b, H, W = 2, 32, 48
    sc = make_scene(n_ctx=2, grid_hw=(8, 8), n_views=2, image_hw=(H, W), seed=3)
    ex = lambda t: t.to(DEV)[None].expand(b, *t.shape).contiguous()
    batch["target"] = dict(image=torch.rand(b, 2, 3, H, W, device=DEV, generator=torch.Generator(DEV).manual_seed(1)), extrinsics=ex(sc.extrinsics),
                           intrinsics=ex(sc.intrinsics), near=ex(sc.near), far=ex(sc.far))
    tgt = batch["target"]
    gaussians, distill = _teacher_targets(teacher, enc, batch)
    with torch.no_grad():
        render = mse_loss(dec.forward(gaussians, tgt["extrinsics"], tgt["intrinsics"], tgt["near"], tgt["far"], (H, W)).color, tgt["image"])
    assert float(distill) > 0 and float(render) > 0
    step = TrainStep(enc, dec, distiller=teacher)
    assert step.distill_weight == 0.1 and step.distill_max_steps == 1_000_000
    total = step(batch)
    want = float(render) + 0.1 * float(distill)                          # the wrappers' weight of the additive term
    assert abs(float(total) - want) <= 1e-4 * want, (float(total), float(render), float(distill))
    assert abs(float(total) - float(render)) > 1e-3 * want               # ... and it really is in the total
    # past distill_max_steps the step is the plain render step again
    enc2 = tiny_student(DEV)
    late = TrainStep(enc2, dec, distiller=teacher, distill_max_steps=-1)
    assert abs(float(late(batch)) - float(render)) <= 1e-4 * float(render)
