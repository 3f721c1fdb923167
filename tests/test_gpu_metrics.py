"""gsr_image_scores (SSIM + clipped MSE for PSNR), compute_lpips and gsr_pose_adam_update on the MI355X against the host restatements
(tests/metrics_reference.py)."""
import copy

import numpy as np
import pytest
import torch

from tests import metrics_reference as ref

DEV = torch.device("cuda:0")
# (1, 1, 42, 74): exactly one full strip and one full chunk (64 x 32 outputs); (1, 1, 43, 75): a second strip and a second chunk that own one
# output column and one output row each (the last strip's halo and the last chunk's rows of the squared error)
SHAPES = [(1, 1, 11, 11), (3, 3, 11, 64), (3, 1, 37, 53), (1, 3, 256, 256), (3, 3, 256, 448), (1, 3, 512, 512), (40, 3, 256, 256),
          (1, 1, 42, 74), (1, 1, 43, 75)]
CASES = ["random", "identical", "zeros", "out_of_range", "near_identical", "border_only"]


def _images(case, shape, seed):
    g = torch.Generator().manual_seed(seed)
    r = lambda: torch.rand(shape, generator=g)
    if case == "random":
        gt = r(); pred = 0.6 * gt + 0.4 * r()
    elif case == "identical":
        gt = r(); pred = gt.clone()
    elif case == "zeros":
        gt = torch.zeros(shape); pred = torch.zeros(shape)
    elif case == "out_of_range":                               # SSIM does not clip, PSNR does
        gt = 2 * r() - 0.5; pred = 2 * r() - 0.5
    elif case == "near_identical":                             # flat 0.9 field + 1e-3 noise: E[x^2] - mu^2 cancels
        gt = 0.9 + 1e-3 * torch.randn(shape, generator=g); pred = 0.9 + 1e-3 * torch.randn(shape, generator=g)
    else:                                                      # differences only in the 5-pixel border SSIM crops away
        gt = r(); pred = gt.clone()
        pred[..., :5, :] = r()[..., :5, :]; pred[..., -5:, :] = r()[..., -5:, :]
        pred[..., :, :5] = r()[..., :, :5]; pred[..., :, -5:] = r()[..., :, -5:]
    return gt.float(), pred.float()


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("case", CASES)
def test_image_scores_match_the_float64_restatement(case, shape):
    from styl3r_amd import metrics
    gt, pred = _images(case, shape, seed=sum(shape) + CASES.index(case))
    psnr, ssim = metrics.image_scores(gt.to(DEV), pred.to(DEV))
    ssim, psnr = ssim.cpu().double().numpy(), psnr.cpu().double().numpy()
    x, y = gt.numpy(), pred.numpy()
    s64, s32 = ref.ssim(x, y, "f64"), ref.ssim(x, y, "f32")
    bar = np.maximum(2 * np.abs(s32 - s64), 2e-6)
    err = np.abs(ssim - s64)
    mse = ref.mse(x, y)
    print(f"image_scores {case} {shape}: max |dssim| {err.max():.3g} (f32 restatement {np.abs(s32 - s64).max():.3g}), ", end="")
    if case in ("identical", "zeros"):
        assert np.abs(ssim - 1).max() <= 1e-6 and np.isinf(psnr).all() and (psnr > 0).all(), (ssim, psnr)
        print("psnr inf")
        return
    assert (err <= bar).all(), (err.max(), bar[err.argmax()])
    dpsnr = np.abs(psnr - (-10 * np.log10(mse)))
    print(f"max |dpsnr| {dpsnr.max():.3g} dB")
    assert dpsnr.max() <= 1e-4, dpsnr.max()
    if case == "border_only":                                  # the border SSIM crops away still enters PSNR
        assert (mse > 0).all() and np.isfinite(psnr).all()


@pytest.mark.gpu
def test_image_scores_are_deterministic_and_independent_of_the_batch():
    from styl3r_amd import metrics
    gt, pred = (t.to(DEV) for t in _images("random", (40, 3, 256, 256), 7))
    p1, s1 = metrics.image_scores(gt, pred)
    p2, s2 = metrics.image_scores(gt, pred)
    assert torch.equal(p1, p2) and torch.equal(s1, s2)
    for n in (0, 17, 39):
        pn, sn = metrics.image_scores(gt[n:n + 1], pred[n:n + 1])
        assert torch.equal(pn[0], p1[n]) and torch.equal(sn[0], s1[n]), n
    # non-contiguous inputs: a transposed view and a strided slice
    gt_t, pred_t = gt.transpose(2, 3).contiguous().transpose(2, 3), pred.transpose(2, 3).contiguous().transpose(2, 3)
    assert not gt_t.is_contiguous()
    p3, s3 = metrics.image_scores(gt_t, pred_t)
    assert torch.equal(p3, p1) and torch.equal(s3, s1)
    half = gt[:, :, :, ::2]
    assert torch.equal(metrics.compute_ssim(half, pred[:, :, :, ::2]), metrics.compute_ssim(half.contiguous(), pred[:, :, :, ::2].contiguous()))
    assert torch.equal(metrics.compute_psnr(gt, pred), p1)
    with pytest.raises(ValueError):
        metrics.image_scores(gt, pred[:, :, :, :255])
    with pytest.raises(ValueError):
        metrics.compute_ssim(gt[:, :, :10], pred[:, :, :10])
    # the C ABI refuses a window that does not fit
    import ctypes as C
    from styl3r_amd import _lib
    lib = _lib.load()
    assert lib.gsr_image_scores_scratch_bytes(1, 3, 10, 64) == 0
    out = torch.empty(2, device=DEV)
    assert lib.gsr_image_scores(gt.data_ptr(), pred.data_ptr(), 1, 3, 10, 64, out.data_ptr(), out[1:].data_ptr(), out.data_ptr(),
                                C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)) == -1


def _fixed_lpips(seed):
    from styl3r_amd.losses import LPIPS
    torch.manual_seed(seed)
    m = LPIPS()
    with torch.no_grad():
        for mod in m.net.modules():
            if isinstance(mod, torch.nn.Conv2d):
                mod.weight.normal_(0, (2.0 / mod.weight[0].numel()) ** 0.5)
                mod.bias.normal_(0, 0.01)
        for k in range(5):
            getattr(m, f"lin{k}").model[1].weight.uniform_(0, 1)
    return m.to(DEV).eval().requires_grad_(False)


@pytest.mark.gpu
def test_compute_lpips_matches_the_float64_expression():
    from styl3r_amd import metrics, vit_ops
    m = _fixed_lpips(11)
    ref64 = copy.deepcopy(m).double()
    g = torch.Generator(DEV).manual_seed(3)
    gt = torch.rand(6, 3, 64, 64, device=DEV, generator=g)
    pred = (gt + 0.1 * torch.randn(gt.shape, device=DEV, generator=g)).clamp(0, 1)
    before = vit_ops.CALLS["lpips_hip_fwd"]
    d = metrics.compute_lpips(gt, pred, m)
    assert vit_ops.CALLS["lpips_hip_fwd"] == before + 1 and d.shape == (6,)      # the HIP route
    with torch.no_grad():
        d64 = ref64._forward_expression(2 * gt.double() - 1, 2 * pred.double() - 1)[:, 0, 0, 0]
    rel = float(((d.double() - d64).abs() / d64.abs()).max())
    assert rel <= (1e-3 if vit_ops.LINEAR_MODE == "bf16x3" else 1e-4), rel
    cached = metrics.get_lpips(DEV)
    assert cached is metrics.get_lpips(DEV) and not cached.training and not cached.weights_loaded


def _torch_pose_steps(c2w, grads, lr_rot, lr_trans):
    from styl3r_amd.pose_align import update_pose
    n = c2w.shape[0]
    rot = torch.nn.Parameter(torch.zeros(n, 3, dtype=torch.float64))
    trans = torch.nn.Parameter(torch.zeros(n, 3, dtype=torch.float64))
    opt = torch.optim.Adam([{"params": [rot], "lr": lr_rot}, {"params": [trans], "lr": lr_trans}])
    ext, out = c2w.double(), []
    for g_rot, g_trans in grads:
        rot.grad, trans.grad = g_rot.double().clone(), g_trans.double().clone()
        opt.step()
        with torch.no_grad():
            ext = update_pose(trans.detach(), rot.detach(), ext)
            rot.fill_(0); trans.fill_(0)
        out.append(ext.clone())
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 3, 40])
@pytest.mark.parametrize("lr_rot", [0.005, 2e-6])       # 2e-6: |theta| < 1e-5 after every step (the series branch)
def test_pose_adam_update_matches_torch_adam_and_update_pose(n, lr_rot):
    import ctypes as C
    from styl3r_amd import _lib
    from styl3r_amd.pose_align import SE3_exp
    g = torch.Generator().manual_seed(n)
    c2w0 = torch.stack([SE3_exp(t).inverse() for t in 0.5 * torch.randn(n, 6, generator=g, dtype=torch.float64)]).float()
    grads = [(torch.randn(n, 3, generator=g), torch.randn(n, 3, generator=g)) for _ in range(20)]
    grads[3] = (torch.zeros(n, 3), torch.zeros(n, 3))
    grads[0][0][n // 2:] = 0.0                         # views without a rotation gradient at step 1: theta = 0
    want = _torch_pose_steps(c2w0, grads, lr_rot, 0.005)
    c2w = c2w0.to(DEV).contiguous()
    m, v = torch.zeros(n, 6, device=DEV), torch.zeros(n, 6, device=DEV)
    lib = _lib.load()
    stream = C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
    for s, (g_rot, g_trans) in enumerate(grads, start=1):
        gr, gt = g_rot.to(DEV).contiguous(), g_trans.to(DEV).contiguous()
        _lib.check(lib.gsr_pose_adam_update(c2w.data_ptr(), m.data_ptr(), v.data_ptr(), gr.data_ptr(), gt.data_ptr(), n, s, lr_rot, 0.005,
                                            0.9, 0.999, 1e-8, stream), "gsr_pose_adam_update")
        got = c2w.cpu().double()
        err = float((got - want[s - 1]).abs().max() / want[s - 1].abs().max())
        assert err <= 1e-5, (s, err)
    print(f"pose_adam n={n} lr_rot={lr_rot}: rel err after 20 steps {err:.3g}")
