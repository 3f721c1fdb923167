"""CPU tests (-m "not gpu") of the relative-pose evaluation: the structure term of the reference's SSIM, `compute_pose_error` / `pose_auc`
against values recorded from the reference (tests/golden/make_pose_eval_fixtures.py), the float64 restatement of the PnP-RANSAC stages,
and `estimate_relative_pose` end to end on host tensors."""
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]
GOLD = np.load(ROOT / "tests/golden/pose_eval_ref.npz")


@pytest.mark.parametrize("tag", ["smooth", "flat"])
def test_structure_expression_matches_the_reference_value_and_gradient(tag):
    from styl3r_amd.losses import LossSsimStructure, ssim_structure, ssim_structure_map
    x = torch.from_numpy(GOLD[f"{tag}_x"]).double()
    y = torch.from_numpy(GOLD[f"{tag}_y"]).double().requires_grad_(True)
    s = ssim_structure(x, y)
    (1 - s).backward()
    want, want_grad = float(GOLD[f"{tag}_scalars"][3]), torch.from_numpy(GOLD[f"{tag}_grad"])
    rel_v = abs(float(s.detach()) - want) / abs(want)
    rel_g = float((y.grad - want_grad).abs().max() / want_grad.abs().max())
    print(f"structure {tag}: value rel {rel_v:.3g}, gradient rel {rel_g:.3g}")
    assert rel_v <= 1e-10 and rel_g <= 1e-10, (rel_v, rel_g)
    if tag == "flat":                                            # the fixture exercises both clamps
        _, raw, _, _, _, raw2 = ssim_structure_map(x, y.detach(), details=True)
        assert bool((raw > 0.98).any()) and bool((raw2 < torch.finfo(torch.float32).eps ** 2).any())
    # the loss module: weight * (1 - structure) of (b, v, c, h, w) tensors
    from types import SimpleNamespace
    loss = LossSsimStructure(weight=0.5).forward(SimpleNamespace(color=y.detach()[None]), {"target": {"image": x[None]}}, None, 0)
    assert abs(float(loss) - 0.5 * (1 - want)) <= 1e-12
    with pytest.raises(ValueError):
        ssim_structure(x[..., :10], y[..., :10])


def test_pose_error_and_auc_match_the_reference():
    from styl3r_amd.metrics import compute_pose_error, pose_auc
    gt, pred = torch.from_numpy(GOLD["pose_gt"]), torch.from_numpy(GOLD["pose_pred"])
    want = torch.from_numpy(GOLD["pose_errors"])
    e_t, e_s, e_R = compute_pose_error(gt, pred)                  # a leading batch dimension
    got = torch.stack([e_t, e_s, e_R], 1)
    assert got.shape == want.shape and float((got - want).abs().max()) <= 1e-9, (got, want)
    for i in range(gt.shape[0]):                                   # batched equals looped
        one = compute_pose_error(gt[i], pred[i])
        assert all(o.shape == () for o in one)
        assert float((torch.stack(one) - got[i]).abs().max()) <= 1e-12
    assert bool((e_t <= 90).all()) and float(want[3, 0]) < 90     # pair 3 has a flipped translation: folded to min(e, 180 - e)
    two = compute_pose_error(gt.reshape(2, 3, 4, 4), pred.reshape(2, 3, 4, 4))
    assert two[0].shape == (2, 3) and torch.equal(two[2].reshape(-1), e_R)
    auc = pose_auc(GOLD["auc_errors"], [5, 10, 20])
    assert np.abs(np.array(auc) - GOLD["auc"]).max() <= 1e-12, (auc, GOLD["auc"])
    assert pose_auc(np.array([1.0, 2.0]), [4])[0] == pytest.approx((0.5 * 1 * 0.5 + 0.75 * 1 + 1.0 * 2) / 4)


def _pnp_problem(hw, seed, noise_px=0.0, pixel_offset=0.0, outliers=0.3, masked=0.2):
    """random depths in [1, 5] through a known K and a known pose (rotation ~ 20 degrees, translation of order 1), fp32 storage; `outliers`
    of the points moved so that they reproject >= 20 px away, `masked` of them under the opacity threshold and filled with garbage"""
    from styl3r_amd.pose_align import SE3_exp
    g = torch.Generator().manual_seed(seed)
    H = W = hw
    K = torch.tensor([[0.86, 0, 0.5], [0, 0.9, 0.48], [0, 0, 1.0]], dtype=torch.float64)
    Kp = K.clone(); Kp[0] *= W; Kp[1] *= H
    axis = torch.randn(3, generator=g, dtype=torch.float64); axis /= axis.norm()
    w2c = SE3_exp(torch.cat([torch.tensor([0.7, -0.4, 0.5], dtype=torch.float64), axis * 0.35]))
    c2w = w2c.inverse()
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float64) + pixel_offset, torch.arange(W, dtype=torch.float64) + pixel_offset, indexing="ij")
    d = 1 + 4 * torch.rand(H, W, generator=g, dtype=torch.float64)
    pix = torch.stack([xs, ys], -1)

    def lift(p, depth):
        v = (p[..., 1] - Kp[1, 2]) / Kp[1, 1]
        u = (p[..., 0] - Kp[0, 2] - Kp[0, 1] * v) / Kp[0, 0]
        cam = torch.stack([u * depth, v * depth, depth], -1)
        return cam @ c2w[:3, :3].T + c2w[:3, 3]
    world = lift(pix, d)
    if noise_px:                                                  # Gaussian noise on the 3-D points equivalent to ~ noise_px pixels
        world = world + noise_px * (d / Kp[0, 0])[..., None] * torch.randn(H, W, 3, generator=g, dtype=torch.float64)
    is_out = torch.rand(H, W, generator=g) < outliers
    ang = 6.2832 * torch.rand(H, W, generator=g, dtype=torch.float64)
    shift = (20 + 60 * torch.rand(H, W, generator=g, dtype=torch.float64))[..., None] * torch.stack([ang.cos(), ang.sin()], -1)
    world = torch.where(is_out[..., None], lift(pix + shift, d), world)
    opacity = 0.31 + 0.69 * torch.rand(H, W, generator=g)
    is_masked = torch.rand(H, W, generator=g) < masked
    opacity[is_masked] = 0.3 * torch.rand(int(is_masked.sum()), generator=g)
    world[is_masked] = 1e4 * torch.randn(int(is_masked.sum()), 3, generator=g, dtype=torch.float64)
    return dict(means=world.float(), opacity=opacity.float(), K=K.float(), Kp=Kp, c2w=c2w, inliers=~is_out & ~is_masked, hw=(H, W))


def _pose_distance(a, b):
    """(rotation angle in rad, translation distance) between two camera-to-world matrices"""
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    chord = (a[:3, :3] - b[:3, :3]).norm() / 8 ** 0.5           # |Ra - Rb|_F = 2 sqrt(2) sin(angle / 2): well conditioned near 0, unlike acos
    return float(2 * torch.asin(chord.clamp(max=1.0))), float((a[:3, 3] - b[:3, 3]).norm())


def test_host_pnp_recovers_a_known_pose_among_outliers_and_masked_garbage():
    from styl3r_amd.pose_align import pnp_pose
    pr = _pnp_problem(64, seed=3)
    pose, st = pnp_pose(pr["means"], pr["opacity"], pr["K"], pr["hw"], seed=1, strict=True)
    assert pose.shape == (4, 4) and pose.dtype == torch.float32 and int(st["code"]) == 0
    assert torch.equal(st["inlier_mask"], pr["inliers"]) and int(st["inliers"]) == int(pr["inliers"].sum())
    assert int(st["masked"]) == int((pr["opacity"] > 0.3).sum()) and 0 <= int(st["winner"]) < 100
    rot, trans = _pose_distance(pose, pr["c2w"])
    print(f"host pnp 64x64: rotation {rot:.3g} rad, translation {trans:.3g}")
    assert rot <= 1e-5 and trans <= 1e-5, (rot, trans)           # fp32 storage of the points and of the result
    again, st2 = pnp_pose(pr["means"], pr["opacity"], pr["K"], pr["hw"], seed=1)
    assert torch.equal(again, pose) and all(torch.equal(st[k], st2[k]) for k in st)
    # a batch of two problems: each equals its own call
    both, stb = pnp_pose(torch.stack([pr["means"]] * 2), torch.stack([pr["opacity"]] * 2), torch.stack([pr["K"]] * 2), pr["hw"], seed=1)
    assert both.shape == (2, 4, 4) and torch.equal(both[0], pose) and stb["inlier_mask"].shape == (2, 64, 64)
    assert torch.equal(both[1], pose)
    with pytest.raises(ValueError):
        pnp_pose(pr["means"], pr["opacity"], pr["K"], (64, 32))


def test_host_pnp_honours_the_pixel_offset():
    from styl3r_amd.pose_align import pnp_pose
    pr = _pnp_problem(48, seed=4, pixel_offset=0.5)
    pose, st = pnp_pose(pr["means"], pr["opacity"], pr["K"], pr["hw"], pixel_offset=0.5)
    rot, trans = _pose_distance(pose, pr["c2w"])
    assert rot <= 1e-5 and trans <= 1e-5, (rot, trans)
    wrong, _ = pnp_pose(pr["means"], pr["opacity"], pr["K"], pr["hw"], pixel_offset=0.0)
    assert _pose_distance(wrong, pr["c2w"])[1] > 1e-3              # half a pixel of disagreement is visible in the pose


def test_host_pnp_reports_too_few_points_as_a_status():
    from styl3r_amd.pose_align import pnp_pose
    pr = _pnp_problem(32, seed=5)
    op = torch.zeros_like(pr["opacity"]); op.view(-1)[[5, 200, 901]] = 0.9
    pose, st = pnp_pose(pr["means"], op, pr["K"], pr["hw"])
    assert int(st["code"]) == 1 and int(st["masked"]) == 3 and int(st["inliers"]) == 0 and int(st["winner"]) == -1
    assert torch.equal(pose, torch.eye(4)) and not bool(st["inlier_mask"].any())
    with pytest.raises(RuntimeError, match="fewer than 6"):
        pnp_pose(pr["means"], op, pr["K"], pr["hw"], strict=True)


class _StubEncoder(torch.nn.Module):
    """returns fixed 'Gaussians' (here: the point cloud itself) and fills the visualization dump the way the encoder does"""

    def __init__(self, means, opacities):
        super().__init__()
        self.means, self.opacities = means, opacities          # (b, v, h, w, 3), (b, v, h, w)
        self.calls = 0

    def forward(self, context, style, global_step=0, visualization_dump=None):
        self.calls += 1
        b, v, h, w, _ = self.means.shape
        if visualization_dump is not None:
            visualization_dump["means"] = self.means.reshape(b, v, h, w, 1, 3)
            visualization_dump["opacities"] = self.opacities.reshape(b, v, h, w, 1, 1)
        return self.means


class _StubDecoder:
    """a differentiable stand-in for the rasterizer on the host: 'renders' the translation of the camera into a smooth image"""

    def forward(self, gaussians, extrinsics, intrinsics, near, far, image_shape, cam_rot_delta=None, cam_trans_delta=None, **kw):
        from types import SimpleNamespace
        h, w = image_shape
        b, v = extrinsics.shape[:2]
        ys, xs = torch.meshgrid(torch.arange(h) / h, torch.arange(w) / w, indexing="ij")
        t = extrinsics[..., :3, 3] + (cam_trans_delta if cam_trans_delta is not None else 0) + 0.3 * (cam_rot_delta if cam_rot_delta is not None else 0)
        img = torch.stack([0.5 + 0.4 * torch.sin(6 * xs + 3 * t[..., k, None, None]) * torch.cos(5 * ys + k) for k in range(3)], 2)
        return SimpleNamespace(color=img.float(), depth=None)


def test_estimate_relative_pose_runs_end_to_end_on_host_tensors():
    from styl3r_amd import evaluation
    from styl3r_amd.losses import LossMse
    prs = [_pnp_problem(32, seed=s) for s in (7, 8)]
    b, v, h, w = 2, 3, 32, 32
    means = torch.stack([torch.stack([p["means"]] * v) for p in prs])
    opac = torch.stack([torch.stack([p["opacity"]] * v) for p in prs])
    E = torch.eye(4).repeat(b, v, 1, 1)
    for i, p in enumerate(prs):
        E[i, 1:] = p["c2w"].float()
    ctx = {"image": torch.rand(b, v, 3, h, w) * 2 - 1, "intrinsics": prs[0]["K"].repeat(b, v, 1, 1), "near": torch.full((b, v), 0.1),
           "far": torch.full((b, v), 100.0), "extrinsics": E}
    enc = _StubEncoder(means, opac)
    cfg = evaluation.PoseEvalCfg(steps=2)
    assert (cfg.rot_lr, cfg.trans_lr, cfg.opacity_threshold, cfg.pnp_iterations, cfg.reprojection_error, cfg.ssim_structure_weight, cfg.seed,
            cfg.pixel_offset, cfg.context_normalized) == (0.005, 0.005, 0.3, 100, 5.0, 1.0, 0, 0.0, True) and evaluation.PoseEvalCfg().steps == 200
    out = evaluation.estimate_relative_pose(enc, _StubDecoder(), {"context": ctx}, [LossMse()], cfg)
    assert enc.calls == 1
    assert set(out) == {"pose_init", "pose", "losses", "pnp_status", "e_t_ours", "e_R_ours", "e_pose_ours"}
    assert out["pose_init"].shape == out["pose"].shape == (b, v - 1, 4, 4) and len(out["losses"]) == 2
    assert out["e_pose_ours"].shape == (b, v - 1) and torch.equal(out["e_pose_ours"], torch.maximum(out["e_t_ours"], out["e_R_ours"]))
    assert bool((out["pnp_status"]["code"] == 0).all()) and out["pnp_status"]["inlier_mask"].shape == (b, v - 1, h, w)
    for i, p in enumerate(prs):                                   # PnP found every view's pose; two steps of 0.005 move it a little
        assert _pose_distance(out["pose_init"][i, 0], p["c2w"])[1] <= 1e-4
        assert 0 < float((out["pose"][i, 0] - out["pose_init"][i, 0]).abs().max()) < 0.05
    init = E[:, 1:].clone(); init[..., 0, 3] += 0.25
    out2 = evaluation.estimate_relative_pose(enc, _StubDecoder(), {"context": ctx}, [LossMse()], cfg, init_pose=init)
    assert torch.equal(out2["pose_init"], init) and out2["pnp_status"] is None
    assert float(out2["e_t_ours"].min()) > float(out["e_t_ours"].max())          # the worse start shows in the error
