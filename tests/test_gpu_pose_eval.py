"""Relative-pose evaluation on the MI355X: gsr_ssim_structure_fwd / _bwd against the float64 expression, gsr_pnp_ransac against the
float64 restatement of its stages (styl3r_amd/pose_align.py), and evaluation.estimate_relative_pose end to end."""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest
import torch

from tests.test_gpu_metrics import _fixed_lpips
from tests.test_gpu_test_step import TAUS
from tests.test_pose_eval_host import _pnp_problem, _pose_distance

DEV = torch.device("cuda:0")
ROOT = Path(__file__).resolve().parents[1]
GOLD = np.load(ROOT / "tests/golden/pose_eval_ref.npz")
SWITCH_REL = 1e-4          # a branch is undecided in float64 within this relative distance of its switch
MAX_EXCLUDED = 0.02        # at most this share of a case's pixels may be left out of the gradient comparison


# ---- 1. SSIM structure -------------------------------------------------------------------------------------------------------------------
def _rendered_pair():
    """3 views of a scene (256 x 256) and the same views from perturbed cameras: what the refinement loop compares"""
    from styl3r_amd.decoder import DecoderSplattingCUDACfg, Gaussians, get_decoder
    from styl3r_amd.pose_align import SE3_exp
    from styl3r_amd.scenes import make_scene
    sc = make_scene(n_ctx=1, grid_hw=(96, 96), n_views=3, image_hw=(256, 256), sh_degree=0, seed=5).to(DEV)
    g = Gaussians(sc.means[None], sc.covariances[None], sc.harmonics[None], sc.opacities[None])
    dec = get_decoder(DecoderSplattingCUDACfg("splatting_cuda", [0.0, 0.0, 0.0], True)).to(DEV)
    E = sc.extrinsics[None]
    t = torch.tensor(TAUS, device=DEV)
    E1 = torch.stack([(SE3_exp(t[i]) @ E[0, i].inverse()).inverse() for i in range(3)])[None]
    with torch.no_grad():
        a = dec.forward(g, E, sc.intrinsics[None], sc.near[None], sc.far[None], (256, 256)).color[0]
        b = dec.forward(g, E1, sc.intrinsics[None], sc.near[None], sc.far[None], (256, 256)).color[0]
    return a.contiguous(), b.contiguous()


def _noise_pair(shape, seed):
    """a smooth field plus noise against another phase of it plus other noise (the structure map stays well below its 0.98 clamp)"""
    n, c, h, w = shape
    g = torch.Generator().manual_seed(seed)
    ys, xs = torch.meshgrid(torch.arange(h) / 48.0, torch.arange(w) / 48.0, indexing="ij")
    field = lambda ph: torch.stack([torch.stack([0.5 + 0.3 * torch.sin(6.28 * (1.0 + 0.5 * k) * xs + ph + i) * torch.cos(6.28 * (0.7 + 0.4 * i) * ys + k)
                                                 for k in range(c)]) for i in range(n)])
    x = field(0.0) + 0.05 * torch.randn(shape, generator=g)
    y = field(0.15) + 0.05 * torch.randn(shape, generator=g)
    return x.float().to(DEV), y.float().to(DEV)


def _crop(pair, shape, r0=96, c0=80):
    n, c, h, w = shape
    r0, c0 = min(r0, pair[0].shape[-2] - h), min(c0, pair[0].shape[-1] - w)
    return tuple(t[:n, :c, r0:r0 + h, c0:c0 + w].contiguous() for t in pair)


def undecided_footprint(x64, y64):
    """(H, W)-shaped mask per plane of the input pixels inside the 11 x 11 footprint of a map pixel whose branch is undecided in float64:
    the raw map within SWITCH_REL of 0.98, or -- where the 0.98 clamp does not decide the gradient (zero) anyway -- |sigma12| within
    SWITCH_REL of its cap or a variance within SWITCH_REL of eps^2.  Returns (mask (N, C, H, W) bool, share of the pixels)."""
    from styl3r_amd.losses import SSIM_EPS2, SSIM_STRUCTURE_MAX, ssim_structure_map
    with torch.no_grad():
        _, raw, a12, cap, raw1, raw2 = ssim_structure_map(x64, y64, details=True)
    near = lambda a, b: (a - b).abs() <= SWITCH_REL * torch.maximum(a.abs(), torch.as_tensor(b, dtype=a.dtype, device=a.device).abs())
    top = near(raw, SSIM_STRUCTURE_MAX)
    clamped = (raw > SSIM_STRUCTURE_MAX) & ~top
    und = top | (~clamped & (near(a12, cap) | near(raw1, SSIM_EPS2) | near(raw2, SSIM_EPS2)))
    n, c, ho, wo = und.shape
    foot = torch.nn.functional.max_pool2d(torch.nn.functional.pad(und.float().reshape(n * c, 1, ho, wo), (10, 10, 10, 10)), 11, stride=1)
    foot = foot.reshape(n, c, ho + 10, wo + 10) > 0
    return foot, float(foot.float().mean())


def _structure_three_ways(x, y):
    """(per-image value, gradient of 1 - mean) from the kernels, from the float64 expression (on the host) and from the fp32 expression
    composed of framework ops on the device; all returned on the host"""
    from styl3r_amd.losses import _structure_expression, ssim_structure_per_image

    def run(fn, xx, yy):
        yy = yy.detach().clone().requires_grad_(True)
        per = fn(xx, yy)
        (1 - per.mean()).backward()
        return per.detach(), yy.grad
    (vk, gk), (v32, g32) = run(ssim_structure_per_image, x, y), run(_structure_expression, x, y)
    return (vk.cpu(), gk.cpu()), run(_structure_expression, x.cpu().double(), y.cpu().double()), (v32.cpu(), g32.cpu())


def _check_structure(tag, x, y):
    (vk, gk), (v64, g64), (v32, g32) = _structure_three_ways(x, y)
    assert vk.dtype == torch.float32 and gk.dtype == torch.float32 and gk.shape == y.shape
    d32 = (v32.double() - v64).abs()
    dk = (vk.double() - v64).abs()
    bar = torch.maximum(2 * d32, torch.full_like(d32, 2e-6))
    foot, share = undecided_footprint(x.cpu().double(), y.cpu().double())
    keep = ~foot
    scale = float(g64.abs().max())
    e32 = float(((g32.double() - g64).abs() * keep).max()) / scale if scale > 0 else 0.0
    ek = float(((gk.double() - g64).abs() * keep).max()) / scale if scale > 0 else 0.0
    gbar = max(2 * e32, 2e-6)
    print(f"ssim_structure {tag} {tuple(x.shape)}: value {[round(float(v), 6) for v in v64]} |dv| kernel {float(dk.max()):.3g} fp32 ops "
          f"{float(d32.max()):.3g}; gradient max-abs {scale:.3g}, normalised error kernel {ek:.3g} fp32 ops {e32:.3g}; excluded share {share:.4f}")
    assert share <= MAX_EXCLUDED, share
    assert bool((dk <= bar).all()), (dk, bar)
    assert ek <= gbar, (ek, gbar)
    return share, ek, e32


STRUCTURE_SHAPES = [(3, 3, 256, 256), (2, 3, 75, 131), (1, 1, 11, 11)]
# one full strip x one full chunk of the map, and the same plus a one-column strip and a one-row chunk (2 x 2 tiles in the backward too)
TILE_EDGE_SHAPES = [(1, 1, 42, 74), (1, 1, 43, 75)]
STRUCTURE_CASES = [(c, s) for c in ("rendered", "noise") for s in STRUCTURE_SHAPES] + [("noise", s) for s in TILE_EDGE_SHAPES]


@pytest.mark.gpu
@pytest.mark.parametrize("case,shape", STRUCTURE_CASES, ids=lambda v: v if isinstance(v, str) else "x".join(map(str, v)))
def test_ssim_structure_matches_the_float64_expression(case, shape):
    x, y = _crop(_rendered_pair(), shape) if case == "rendered" else _noise_pair(shape, seed=sum(shape))
    if case == "rendered" and shape[0] == 3:                     # the case the loop sees: both clamps are active
        from styl3r_amd.losses import SSIM_EPS2, ssim_structure_map
        _, raw, _, _, _, raw2 = ssim_structure_map(x.cpu().double(), y.cpu().double(), details=True)
        lo, hi = float((raw2 < SSIM_EPS2).double().mean()), float((raw > 0.98).double().mean())
        print(f"rendered pair: share of map pixels with sigma2^2 < eps^2 {lo:.4f}, above 0.98 {hi:.4f}")
    _check_structure(case, x, y)


@pytest.mark.gpu
@pytest.mark.parametrize("tag", ["smooth", "flat"])
def test_ssim_structure_matches_the_reference_fixture(tag):
    from styl3r_amd.losses import ssim_structure
    x, y = torch.from_numpy(GOLD[f"{tag}_x"]).to(DEV), torch.from_numpy(GOLD[f"{tag}_y"]).to(DEV)
    _check_structure("fixture " + tag, x, y)
    got, want = float(ssim_structure(x, y)), float(GOLD[f"{tag}_scalars"][3])
    assert abs(got - want) <= 1e-5, (got, want)                  # the value the reference returns for these images


@pytest.mark.gpu
def test_ssim_structure_is_deterministic_and_independent_of_the_batch():
    from styl3r_amd import _lib
    from styl3r_amd.losses import LossSsimStructure, ssim_structure_per_image
    x, y = _noise_pair((2, 3, 75, 131), seed=3)

    def run(xx, yy):
        yy = yy.clone().requires_grad_(True)
        per = ssim_structure_per_image(xx, yy)
        (1 - per).sum().backward()
        return per.detach(), yy.grad
    v1, g1 = run(x, y)
    v2, g2 = run(x, y)
    assert torch.equal(v1, v2) and torch.equal(g1, g2)
    for n in range(2):
        vn, gn = run(x[n:n + 1], y[n:n + 1])
        assert torch.equal(vn[0], v1[n]) and torch.equal(gn[0], g1[n]), n
    # without a gradient the forward writes no adjoint maps; the loss module is weight * (1 - mean)
    from types import SimpleNamespace
    with torch.no_grad():
        loss = LossSsimStructure(0.25).forward(SimpleNamespace(color=y[None]), {"target": {"image": x[None]}}, None, 0)
    assert abs(float(loss) - 0.25 * (1 - float(v1.mean()))) <= 1e-7
    lib = _lib.load()
    one = C.c_void_p(256)
    win = (C.c_float * 11)()
    assert lib.gsr_ssim_structure_scratch_bytes(1, 3, 10, 64) == 0
    assert lib.gsr_ssim_structure_fwd(one, one, 1, 3, 10, 64, win, one, None, one, None) == -1
    assert lib.gsr_ssim_structure_fwd(None, one, 1, 3, 16, 64, win, one, None, one, None) == -1
    assert lib.gsr_ssim_structure_bwd(one, one, None, one, 1, 3, 16, 64, win, one, None) == -1


# ---- 2-4. PnP-RANSAC ---------------------------------------------------------------------------------------------------------------------
def _gpu_pnp(pr, **kw):
    from styl3r_amd.pose_align import pnp_pose
    pose, st = pnp_pose(pr["means"].to(DEV), pr["opacity"].to(DEV), pr["K"].to(DEV), pr["hw"], **kw)
    return pose.cpu(), {k: v.cpu() for k, v in st.items()}


def _oracle(pr, pixel_offset=0.0):
    """the float64 Levenberg-Marquardt stage on the TRUE inlier set from the TRUE pose: (c2w, inliers within 5 px among the masked points)"""
    from styl3r_amd.pose_align import pnp_normal_equations, pnp_refine
    H, W = pr["hw"]
    w2c = torch.linalg.inv(pr["c2w"]).numpy()
    idx = np.nonzero(pr["inliers"].reshape(-1).numpy())[0]
    X = pr["means"].reshape(-1, 3).double().numpy()
    uv = lambda i: np.stack([i % W + pixel_offset, i // W + pixel_offset], 1).astype(np.float64)
    Kp = pr["Kp"].numpy()
    R, t = pnp_refine(w2c[:3, :3], w2c[:3, 3], X[idx], uv(idx), Kp, np.inf, iterations=10)
    c2w = np.eye(4); c2w[:3, :3] = R.T; c2w[:3, 3] = -R.T @ t
    masked = np.nonzero((pr["opacity"].reshape(-1) > 0.3).numpy())[0]
    count = int(pnp_normal_equations(R, t, X[masked], uv(masked), Kp, 25.0)[3].sum())
    return torch.from_numpy(c2w), count


@pytest.mark.gpu
def test_pnp_exact_geometry_recovers_the_inlier_set_and_the_least_squares_pose():
    pr = _pnp_problem(128, seed=11)
    pose, st = _gpu_pnp(pr, seed=0)
    assert int(st["code"]) == 0 and int(st["masked"]) == int((pr["opacity"] > 0.3).sum())
    assert torch.equal(st["inlier_mask"], pr["inliers"]) and int(st["inliers"]) == int(pr["inliers"].sum())
    ref, _ = _oracle(pr)
    own_rot, own_trans = _pose_distance(ref, pr["c2w"])
    rot, trans = _pose_distance(pose, ref)
    print(f"pnp exact 128x128: float64 LM on the true set vs ground truth: {own_rot:.3g} rad, {own_trans:.3g}; kernel vs that solution: "
          f"{rot:.3g} rad, {trans:.3g}; winner {int(st['winner'])}, inliers {int(st['inliers'])} of {int(st['masked'])}")
    assert rot <= max(10 * own_rot, 1e-5) and trans <= max(10 * own_trans, 1e-5), (rot, trans, own_rot, own_trans)


def _angles_deg(pose, gt):
    """(rotation error, translation-direction error) in degrees, both well conditioned near zero"""
    pose, gt = pose.double(), gt.double()
    rot = np.degrees(_pose_distance(pose, gt)[0])
    a, b = pose[:3, 3] / pose[:3, 3].norm(), gt[:3, 3] / gt[:3, 3].norm()
    return rot, float(np.degrees(float(2 * torch.asin(((a - b).norm() / 2).clamp(max=1.0)))))


@pytest.mark.gpu
@pytest.mark.parametrize("seed", [0, 1, 2, 3, 4])
def test_pnp_noisy_points_is_as_good_as_the_oracle_inlier_set(seed):
    pr = _pnp_problem(256, seed=100 + seed, noise_px=1.0)
    pose, st = _gpu_pnp(pr, seed=seed)
    ref, ref_count = _oracle(pr)
    e_rot, e_dir = _angles_deg(pose, pr["c2w"])
    o_rot, o_dir = _angles_deg(ref, pr["c2w"])
    print(f"pnp noisy 256x256 seed {seed}: inliers {int(st['inliers'])} (oracle {ref_count}), rotation {e_rot:.4g} deg (oracle {o_rot:.4g}), "
          f"translation direction {e_dir:.4g} deg (oracle {o_dir:.4g})")
    assert int(st["code"]) == 0
    assert int(st["inliers"]) >= 0.95 * ref_count, (int(st["inliers"]), ref_count)
    assert e_rot <= 1.5 * o_rot + 0.02 and e_dir <= 1.5 * o_dir + 0.02, (e_rot, o_rot, e_dir, o_dir)


@pytest.mark.gpu
def test_pnp_plumbing():
    from styl3r_amd import _lib
    from styl3r_amd.pose_align import pnp_pose
    pr = _pnp_problem(64, seed=21)
    p1, s1 = _gpu_pnp(pr, seed=7)
    p2, s2 = _gpu_pnp(pr, seed=7)
    assert torch.equal(p1, p2) and all(torch.equal(s1[k], s2[k]) for k in s1)
    # P = 3 (three different problems) equals three P = 1 calls bitwise
    prs = [pr, _pnp_problem(64, seed=22), _pnp_problem(64, seed=23, noise_px=1.0)]
    stack = lambda k: torch.stack([q[k] for q in prs]).to(DEV)
    p3, s3 = pnp_pose(stack("means"), stack("opacity"), stack("K"), (64, 64), seed=7)
    assert p3.shape == (3, 4, 4) and s3["inlier_mask"].shape == (3, 64, 64)
    for i, q in enumerate(prs):
        pi, si = _gpu_pnp(q, seed=7)
        assert torch.equal(p3[i].cpu(), pi) and all(torch.equal(s3[k][i].cpu(), si[k]) for k in si), i
    # data generated at pixel centres needs pixel_offset 0.5
    pc = _pnp_problem(64, seed=24, pixel_offset=0.5)
    good, sg = _gpu_pnp(pc, pixel_offset=0.5)
    bad, _ = _gpu_pnp(pc, pixel_offset=0.0)
    assert _pose_distance(good, pc["c2w"])[1] <= 1e-5 and torch.equal(sg["inlier_mask"], pc["inliers"])
    assert _pose_distance(bad, pc["c2w"])[1] > 1e-3
    # three masked points: a status, the identity, a clean return
    op = torch.zeros_like(pr["opacity"]); op.view(-1)[[5, 200, 901]] = 0.9
    pose, st = pnp_pose(pr["means"].to(DEV), op.to(DEV), pr["K"].to(DEV), (64, 64))
    torch.cuda.synchronize(DEV)
    assert int(st["code"]) == 1 and int(st["masked"]) == 3 and int(st["inliers"]) == 0 and int(st["winner"]) == -1
    assert torch.equal(pose.cpu(), torch.eye(4)) and not bool(st["inlier_mask"].any())
    with pytest.raises(RuntimeError, match="fewer than 6"):
        pnp_pose(pr["means"].to(DEV), op.to(DEV), pr["K"].to(DEV), (64, 64), strict=True)
    # the raw C ABI validates before any launch
    lib = _lib.load()
    one = C.c_void_p(256)
    args = lambda pts, n: (pts, one, one, 1, 64, 64, n, 0.3, 5.0, 100, 0, 0.0, one, None, one, one, None)
    assert lib.gsr_pnp_ransac(*args(None, 4096)) == -1
    assert lib.gsr_pnp_ransac(*args(one, 4095)) == -1
    assert lib.gsr_pnp_ransac(one, one, one, 1, 64, 64, 4096, 0.3, 5.0, 0, 0, 0.0, one, None, one, one, None) == -1
    assert lib.gsr_pnp_ransac(one, one, one, 1, 64, 64, 4096, 0.3, 5.0, 100, 0, 0.0, one, None, None, one, None) == -1
    assert lib.gsr_pnp_ransac_scratch_bytes(1, 64, 64, 0) == 0 and lib.gsr_pnp_ransac_scratch_bytes(1, 64, 64, 100) > 0


# ---- 5. end to end -----------------------------------------------------------------------------------------------------------------------
HW = 96


class _SceneEncoder(torch.nn.Module):
    """stands in for the encoder: returns the scenes' Gaussians and fills the visualization dump with the per-pixel means / opacities"""

    def __init__(self, g, v):
        super().__init__()
        self.g, self.v = g, v

    def forward(self, context, style, global_step=0, visualization_dump=None):
        b = self.g.means.shape[0]
        if visualization_dump is not None:
            visualization_dump["means"] = self.g.means.reshape(b, self.v, HW, HW, 1, 3)
            visualization_dump["opacities"] = self.g.opacities.reshape(b, self.v, HW, HW, 1, 1)
        return self.g


def _pair_scene(seeds):
    """b = len(seeds) scenes of two context views (camera 2: identity rotation at (1, 0, 0)); the context images are the renders from the
    true cameras, in [-1, 1] as the encoder receives them"""
    from styl3r_amd.decoder import DecoderSplattingCUDACfg, Gaussians, get_decoder
    from styl3r_amd.scenes import make_scene
    scs = [make_scene(n_ctx=2, grid_hw=(HW, HW), n_views=2, image_hw=(HW, HW), sh_degree=0, seed=s).to(DEV) for s in seeds]
    st = lambda f: torch.stack([f(sc) for sc in scs])
    g = Gaussians(st(lambda s: s.means), st(lambda s: s.covariances), st(lambda s: s.harmonics), st(lambda s: s.opacities))
    dec = get_decoder(DecoderSplattingCUDACfg("splatting_cuda", [0.0, 0.0, 0.0], True)).to(DEV)
    b = len(seeds)
    E = torch.eye(4, device=DEV).repeat(b, 2, 1, 1)
    E[:, 1, 0, 3] = 1.0
    K, n, f = st(lambda s: s.intrinsics), st(lambda s: s.near), st(lambda s: s.far)
    with torch.no_grad():
        image = dec.forward(g, E, K, n, f, (HW, HW)).color
    ctx = {"image": image * 2 - 1, "extrinsics": E, "intrinsics": K, "near": n, "far": f}
    return g, dec, {"context": ctx}, image


def _losses(lp):
    from styl3r_amd.losses import LossLpips, LossMse
    return [LossMse(), LossLpips(lpips=lp)]


@pytest.mark.gpu
def test_end_to_end_pnp_initialisation_finds_the_second_context_camera():
    from styl3r_amd import evaluation
    g, dec, batch, _ = _pair_scene([5])
    cfg = evaluation.PoseEvalCfg(steps=2, pixel_offset=0.5)
    out = evaluation.estimate_relative_pose(_SceneEncoder(g, 2), dec, batch, _losses(_fixed_lpips(11)), cfg)
    gt = batch["context"]["extrinsics"][0, 1]
    rot, trans = _pose_distance(out["pose_init"][0, 0].cpu(), gt.cpu())
    bound = 1e-5 * 128 / HW                                     # the exact-geometry bound, scaled by the grid's side
    print(f"end to end: pose_init vs the true camera: {rot:.3g} rad, {trans:.3g}; PnP inliers {int(out['pnp_status']['inliers'])} of "
          f"{int(out['pnp_status']['masked'])}; e_R {float(out['e_R_ours']):.3g} deg, e_t {float(out['e_t_ours']):.3g} deg after 2 steps")
    assert int(out["pnp_status"]["code"]) == 0 and int(out["pnp_status"]["inliers"]) == int(out["pnp_status"]["masked"])
    assert rot <= bound and trans <= bound, (rot, trans)
    assert out["pose"].shape == (1, 1, 4, 4) and len(out["losses"]) == 2 and out["e_pose_ours"].shape == (1, 1)


@pytest.mark.gpu
def test_end_to_end_refinement_recovers_a_perturbed_camera_and_follows_align_poses():
    """the bars of test_gpu_test_step.py for the same loop with the structure term added.  The objective has a floor -- the structure map is
    clamped at 0.98, so 1 - structure >= 0.02 -- and still falls below a tenth of its start (measured: 0.428 -> 0.0201 in 120 steps)."""
    from styl3r_amd import evaluation
    from styl3r_amd.losses import _structure_expression, mse_loss
    from styl3r_amd.pose_align import SE3_exp, align_poses
    g, dec, batch, image = _pair_scene([5])
    lp = _fixed_lpips(11)
    losses = _losses(lp)
    ctx = batch["context"]
    gt = ctx["extrinsics"][:, 1:]
    tau = torch.tensor(TAUS[0], device=DEV)
    init = (SE3_exp(tau) @ gt[0, 0].inverse()).inverse()[None, None]
    cfg = evaluation.PoseEvalCfg(steps=120, rot_lr=0.003, trans_lr=0.003, pixel_offset=0.5)
    out = evaluation.estimate_relative_pose(_SceneEncoder(g, 2), dec, batch, losses, cfg, init_pose=init)
    hist = out["losses"]
    err0, err1 = float((init - gt).abs().max()), float((out["pose"] - gt).abs().max())
    # the host loop with the same objective composed of framework ops
    w = losses[1].cfg.weight
    target = ctx["image"][:, 1:] * 0.5 + 0.5
    flat = lambda t: t.reshape(-1, 3, HW, HW)
    obj = lambda pred, t: mse_loss(pred, t) + w * lp(flat(pred), flat(t), normalize=True).mean() + (1 - _structure_expression(flat(t), flat(pred)).mean())
    E_ref, hist_ref = align_poses(dec, g, target, init, ctx["intrinsics"][:, 1:], ctx["near"][:, 1:], ctx["far"][:, 1:], steps=120, rot_lr=0.003,
                                  trans_lr=0.003, loss_fn=obj)
    err_ref = float((E_ref - gt).abs().max())
    rel = [abs(a - b) / abs(b) for a, b in zip(hist[:10], hist_ref[:10])]
    print(f"refinement [mse, lpips, ssim-structure]: loss {hist[0]:.4g} -> {hist[-1]:.4g} (framework ops {hist_ref[0]:.4g} -> {hist_ref[-1]:.4g}), "
          f"pose err {err0:.3g} -> {err1:.3g} (framework ops {err_ref:.3g}), first 10 losses within {max(rel):.3g} rel of align_poses; "
          f"e_R {float(out['e_R_ours']):.3g} deg e_t {float(out['e_t_ours']):.3g} deg")
    assert len(hist) == 120 and max(rel) <= 1e-3, list(zip(hist[:10], hist_ref[:10]))
    assert err1 < 0.35 * err0, (err0, err1)
    assert hist[-1] < 0.1 * hist[0], (hist[0], hist[-1], hist_ref[-1])


@pytest.mark.gpu
def test_end_to_end_two_scenes_equal_two_single_scene_calls():
    from styl3r_amd import evaluation
    lp = _fixed_lpips(11)
    cfg = evaluation.PoseEvalCfg(steps=40, pixel_offset=0.5)
    g2, dec, batch2, _ = _pair_scene([5, 6])
    out2 = evaluation.estimate_relative_pose(_SceneEncoder(g2, 2), dec, batch2, _losses(lp), cfg)
    worst = 0.0
    for b, seed in enumerate([5, 6]):
        g1, _, batch1, _ = _pair_scene([seed])
        out1 = evaluation.estimate_relative_pose(_SceneEncoder(g1, 2), dec, batch1, _losses(lp), cfg)
        assert torch.equal(out1["pose_init"][0], out2["pose_init"][b])                  # PnP: bitwise
        worst = max(worst, float((out1["pose"][0] - out2["pose"][b]).abs().max()))
    print(f"estimate_relative_pose b = 2 vs two b = 1 calls: poses within {worst:.3g}")
    assert out2["pose"].shape == (2, 1, 4, 4) and out2["e_pose_ours"].shape == (2, 1) and worst <= 1e-4, worst
