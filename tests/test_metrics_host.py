"""Host checks of the test step's scores and pose step (styl3r_amd.metrics / evaluation; the restatements in tests/metrics_reference.py)."""
import numpy as np
import pytest
import torch

from tests import metrics_reference as ref


def _pair(shape, seed, lo=0.0, hi=1.0):
    rng = np.random.default_rng(seed)
    return rng.uniform(lo, hi, shape), rng.uniform(lo, hi, shape)


@pytest.mark.parametrize("shape", [(1, 1, 11, 11), (2, 3, 11, 20), (1, 3, 37, 53), (2, 1, 64, 64)])
def test_valid_filter_equals_scipy_reflect_plus_crop(shape):
    pytest.importorskip("scipy")
    x, y = _pair(shape, sum(shape), -0.5, 1.5)
    y = 0.7 * x + 0.3 * y                                   # correlated, so the covariance term matters
    assert np.abs(ref.ssim(x, y) - ref.ssim_scipy(x, y)).max() <= 1e-12


def test_ssim_known_answers():
    x, y = _pair((2, 3, 23, 31), 1)
    assert np.allclose(ref.ssim(x, x), 1.0, rtol=0, atol=1e-15)
    assert np.array_equal(ref.ssim(x, y), ref.ssim(y, x))
    a, b = 0.3, 0.8
    got = ref.ssim(np.full((1, 2, 16, 19), a), np.full((1, 2, 16, 19), b))
    assert abs(got[0] - (2 * a * b + ref.C1) / (a * a + b * b + ref.C1)) <= 1e-12
    # 11 x 11: one kept pixel, the whole image under its window
    x, y = _pair((1, 1, 11, 11), 2)
    w2 = np.outer(ref.window(), ref.window())
    f = lambda t: (w2 * t[0, 0]).sum()
    want = ref._map(f(x), f(y), f(x * x), f(y * y), f(x * y))
    assert abs(ref.ssim(x, y)[0] - want) <= 1e-13
    with pytest.raises(ValueError):
        ref.ssim(np.zeros((1, 1, 10, 40)), np.zeros((1, 1, 10, 40)))


def test_metrics_host_paths_match_the_restatement():
    from styl3r_amd import metrics
    x, y = _pair((3, 3, 29, 41), 3, -0.5, 1.5)
    for dt in (torch.float64, torch.float32):
        gt, pred = torch.tensor(x, dtype=dt), torch.tensor(y, dtype=dt)
        x64, y64 = gt.double().numpy(), pred.double().numpy()
        ssim, psnr = metrics.compute_ssim(gt, pred), metrics.compute_psnr(gt, pred)
        assert ssim.shape == (3,) and ssim.dtype == dt and psnr.dtype == dt
        tol = 1e-12 if dt == torch.float64 else 1e-6
        assert np.abs(ssim.double().numpy() - ref.ssim(x64, y64)).max() <= tol
        assert np.abs(psnr.double().numpy() - (-10 * np.log10(ref.mse(x64, y64)))).max() <= 1e-4
        p2, s2 = metrics.image_scores(gt, pred)
        assert torch.equal(p2, psnr) and torch.equal(s2, ssim)


def test_psnr_clips_and_is_inf_for_identical_images():
    from styl3r_amd import metrics
    x = torch.rand(2, 3, 12, 12, dtype=torch.float64)
    assert torch.isinf(metrics.compute_psnr(x, x.clone())).all()
    over = x.clone(); over[:, :, 0, 0] = 1.7; under = x.clone(); under[:, :, 0, 0] = 1.0
    assert torch.equal(metrics.compute_psnr(over, x), metrics.compute_psnr(under, x))     # 1.7 clips to 1
    assert torch.isinf(metrics.compute_psnr(torch.full_like(x, 2.0), torch.full_like(x, 1.5))).all()
    # small images: PSNR has no window, SSIM raises as skimage does
    s = torch.rand(1, 3, 5, 5, dtype=torch.float64)
    assert torch.isfinite(metrics.compute_psnr(s, s * 0.5)).all()
    with pytest.raises(ValueError):
        metrics.compute_ssim(torch.rand(1, 3, 10, 40), torch.rand(1, 3, 10, 40))
    with pytest.raises(ValueError):
        metrics.image_scores(torch.rand(1, 3, 40, 40), torch.rand(1, 3, 40, 41))


def _torch_pose_steps(c2w, grads, lr_rot, lr_trans):
    """torch.optim.Adam + pose_align.update_pose in float64, as test_step_align runs them"""
    from styl3r_amd.pose_align import update_pose
    n = c2w.shape[0]
    rot = torch.nn.Parameter(torch.zeros(n, 3, dtype=torch.float64))
    trans = torch.nn.Parameter(torch.zeros(n, 3, dtype=torch.float64))
    opt = torch.optim.Adam([{"params": [rot], "lr": lr_rot}, {"params": [trans], "lr": lr_trans}])
    ext, out = torch.as_tensor(c2w, dtype=torch.float64), []
    for g_rot, g_trans in grads:
        rot.grad, trans.grad = torch.as_tensor(g_rot).clone(), torch.as_tensor(g_trans).clone()
        opt.step()
        with torch.no_grad():
            ext = update_pose(trans.detach(), rot.detach(), ext)
            rot.fill_(0); trans.fill_(0)
        out.append(ext.numpy().copy())
    return out


def _cameras(n, seed):
    from styl3r_amd.pose_align import SE3_exp
    g = torch.Generator().manual_seed(seed)
    taus = 0.5 * torch.randn(n, 6, generator=g, dtype=torch.float64)
    return torch.stack([SE3_exp(t).inverse() for t in taus]).numpy()


@pytest.mark.parametrize("lr_rot", [0.005, 2e-6])       # 2e-6: |theta| < 1e-5 after every step, the series branch of SO3_exp / V
def test_pose_adam_restatement_matches_torch_adam_and_update_pose(lr_rot):
    n, steps = 3, 6
    rng = np.random.default_rng(4)
    grads = [(rng.normal(size=(n, 3)), rng.normal(size=(n, 3))) for _ in range(steps)]
    grads[2] = (np.zeros((n, 3)), np.zeros((n, 3)))       # a zero gradient mid-run
    grads[0][0][1:] = 0.0                                 # views 1, 2 get no rotation gradient at step 1: theta = 0
    c2w = _cameras(n, 5)
    want = _torch_pose_steps(c2w, grads, lr_rot, 0.005)
    m, v, ext = np.zeros((n, 6)), np.zeros((n, 6)), c2w.copy()
    for s, (g_rot, g_trans) in enumerate(grads, start=1):
        ext = ref.pose_adam_step(ext, m, v, g_rot, g_trans, s, lr_rot, 0.005)
        assert np.abs(ext - want[s - 1]).max() <= 1e-12 * np.abs(want[s - 1]).max(), s


def test_test_cfg_defaults_are_the_reference_config():
    from styl3r_amd.evaluation import TestCfg
    cfg = TestCfg()
    assert (cfg.align_pose, cfg.pose_align_steps, cfg.rot_opt_lr, cfg.trans_opt_lr, cfg.compute_scores) == (True, 100, 0.005, 0.005, True)
