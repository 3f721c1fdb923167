"""evaluation.test_step / align_target_poses on the MI355X: the reference's test step (model_wrapper_style.py:317-461) with the
[mse, lpips] objective of every NVS experiment, against the existing pose_align.align_poses and the metrics module."""
import pytest
import torch

from tests.test_gpu_metrics import _fixed_lpips

DEV = torch.device("cuda:0")
HW = 96
TAUS = [[0.02, -0.015, 0.01, 0.01, -0.008, 0.012], [-0.015, 0.01, 0.02, -0.01, 0.01, 0.005], [0.01, 0.02, -0.01, 0.006, 0.012, -0.01]]


class _FixedGaussians(torch.nn.Module):
    """stands in for the encoder: returns the scene's Gaussians whatever the context"""

    def __init__(self, g):
        super().__init__()
        self.g = g

    def forward(self, context, style, global_step):
        return self.g


def _scene(seeds, taus):
    """b = len(seeds) scenes of 3 target views; returns (Gaussians, decoder, batch with perturbed target poses, true c2w)"""
    from styl3r_amd.decoder import DecoderSplattingCUDACfg, Gaussians, get_decoder
    from styl3r_amd.pose_align import SE3_exp
    from styl3r_amd.scenes import make_scene
    scs = [make_scene(n_ctx=1, grid_hw=(HW, HW), n_views=3, image_hw=(HW, HW), sh_degree=0, seed=s).to(DEV) for s in seeds]
    st = lambda f: torch.stack([f(sc) for sc in scs])
    g = Gaussians(st(lambda s: s.means), st(lambda s: s.covariances), st(lambda s: s.harmonics), st(lambda s: s.opacities))
    dec = get_decoder(DecoderSplattingCUDACfg("splatting_cuda", [0.0, 0.0, 0.0], True)).to(DEV)
    E, K, n, f = st(lambda s: s.extrinsics), st(lambda s: s.intrinsics), st(lambda s: s.near), st(lambda s: s.far)
    with torch.no_grad():
        target = dec.forward(g, E, K, n, f, (HW, HW)).color
    t = torch.tensor(taus, device=DEV)
    E0 = torch.stack([torch.stack([(SE3_exp(t[(i + b) % 3]) @ E[b, i].inverse()).inverse() for i in range(3)]) for b in range(len(seeds))])
    batch = {"context": {"image": target[:, :1]},
             "target": {"image": target, "extrinsics": E0, "intrinsics": K, "near": n, "far": f}}
    return g, dec, batch, E


def _losses(lpips):
    from styl3r_amd.losses import LossLpips, LossMse
    return [LossMse(), LossLpips(lpips=lpips)]


@pytest.mark.gpu
def test_test_step_without_alignment_scores_the_decoder_output():
    from styl3r_amd import evaluation, metrics
    g, dec, batch, _ = _scene([5], TAUS)
    lp = _fixed_lpips(11)
    out, scores = evaluation.test_step(_FixedGaussians(g), dec, batch, _losses(lp), evaluation.TestCfg(align_pose=False), lpips=lp)
    assert set(scores) == {"psnr_ours", "ssim_ours", "lpips_ours", "lpips_weights_loaded"} and scores["lpips_weights_loaded"] is False
    tgt = batch["target"]
    with torch.no_grad():
        color = dec.forward(g, tgt["extrinsics"], tgt["intrinsics"], tgt["near"], tgt["far"], (HW, HW)).color
    assert torch.equal(out.color, color)
    gt, pred = tgt["image"][0], color[0]
    per_scene = lambda t: t.reshape(1, 3).mean(dim=1)
    assert torch.equal(scores["psnr_ours"], per_scene(metrics.compute_psnr(gt, pred)))
    assert torch.equal(scores["ssim_ours"], per_scene(metrics.compute_ssim(gt, pred)))
    # LPIPS is not bit-reproducible from call to call after other GPU work in the process (its 64-channel conv1_x layers run on the
    # framework's convolution library): equal to the last few bits, not bitwise
    lp_again = per_scene(metrics.compute_lpips(gt, pred, lp))
    rel = float((scores["lpips_ours"] - lp_again).abs().max() / lp_again.abs().max())
    print(f"test_step lpips vs compute_lpips: rel {rel:.3g}")
    assert rel <= 1e-5, (scores["lpips_ours"], lp_again)
    _, none = evaluation.test_step(_FixedGaussians(g), dec, batch, _losses(lp), evaluation.TestCfg(align_pose=False, compute_scores=False))
    assert none == {}


@pytest.mark.gpu
def test_alignment_with_mse_and_lpips_recovers_perturbed_cameras_and_follows_align_poses():
    from styl3r_amd import evaluation
    from styl3r_amd.losses import mse_loss
    from styl3r_amd.pose_align import align_poses
    g, dec, batch, E = _scene([5], TAUS)
    lp = _fixed_lpips(11)
    losses = _losses(lp)
    tgt = batch["target"]
    cfg = evaluation.TestCfg(pose_align_steps=120, rot_opt_lr=0.003, trans_opt_lr=0.003)
    E1, hist = evaluation.align_target_poses(dec, g, batch, losses, cfg)
    err0, err1 = float((tgt["extrinsics"] - E).abs().max()), float((E1 - E).abs().max())
    assert len(hist) == 120 and hist[-1] < 0.1 * hist[0], (hist[0], hist[-1])
    assert err1 < 0.35 * err0, (err0, err1)
    # the existing host loop with the same objective as its loss_fn
    w = losses[1].cfg.weight
    obj = lambda pred, t: mse_loss(pred, t) + w * lp(pred.reshape(-1, 3, HW, HW), t.reshape(-1, 3, HW, HW), normalize=True).mean()
    _, hist_ref = align_poses(dec, g, tgt["image"], tgt["extrinsics"], tgt["intrinsics"], tgt["near"], tgt["far"], steps=10,
                              rot_lr=0.003, trans_lr=0.003, loss_fn=obj)
    rel = [abs(a - b) / abs(b) for a, b in zip(hist[:10], hist_ref)]
    # Adam's first steps are sign-like: a gradient component within rounding of zero may legitimately take another sign on the two paths
    assert max(rel) <= 1e-3, ("per-step losses, new vs align_poses", list(zip(hist[:10], hist_ref)))
    print(f"alignment [mse, lpips]: loss {hist[0]:.4g} -> {hist[-1]:.4g}, pose err {err0:.3g} -> {err1:.3g}, "
          f"first 10 losses within {max(rel):.3g} rel of align_poses")


@pytest.mark.gpu
def test_two_scenes_align_and_score_as_two_single_scene_calls():
    from styl3r_amd import evaluation
    lp = _fixed_lpips(11)
    cfg = evaluation.TestCfg(pose_align_steps=40)
    g2, dec, batch2, _ = _scene([5, 6], TAUS)
    out2, sc2 = evaluation.test_step(_FixedGaussians(g2), dec, batch2, _losses(lp), cfg, lpips=lp)
    E2, _ = evaluation.align_target_poses(dec, g2, batch2, _losses(lp), cfg)
    worst = {}
    for b, seed in enumerate([5, 6]):
        g1, _, batch1, _ = _scene([seed], TAUS[b:] + TAUS[:b])
        assert torch.equal(batch1["target"]["extrinsics"][0], batch2["target"]["extrinsics"][b])
        _, sc1 = evaluation.test_step(_FixedGaussians(g1), dec, batch1, _losses(lp), cfg, lpips=lp)
        E1, _ = evaluation.align_target_poses(dec, g1, batch1, _losses(lp), cfg)
        worst["pose"] = max(worst.get("pose", 0.0), float((E1[0] - E2[b]).abs().max()))
        for k in ("psnr_ours", "ssim_ours", "lpips_ours"):
            worst[k] = max(worst.get(k, 0.0), abs(float(sc1[k][0]) - float(sc2[k][b])))
    print("b = 2 vs two b = 1 calls:", {k: f"{v:.3g}" for k, v in worst.items()})
    assert sc2["psnr_ours"].shape == (2,) and out2.color.shape[:2] == (2, 3)
    assert worst["pose"] <= 1e-4 and worst["psnr_ours"] <= 1e-2 and worst["ssim_ours"] <= 1e-4 and worst["lpips_ours"] <= 1e-4, worst
