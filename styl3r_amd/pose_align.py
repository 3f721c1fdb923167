"""Test-time pose alignment through the rasterizer's pose gradient.

Mirrors `ModelWrapperStyle.test_step_align` (src/model/model_wrapper_style.py:391-447) and
`update_pose` / `SE3_exp` / `SO3_exp` / `V` (src/misc/cam_utils.py:67-137): per target view two
3-vectors `cam_rot_delta`, `cam_trans_delta` stay at zero, receive dL/d(theta, rho) from the decoder
(`theta` / `rho` of the rasterizer), take an Adam step, and are folded into the camera as a LEFT
multiplication of the world->camera matrix, T_w2c' = exp(tau) T_w2c, then reset to zero.
Losses: the reference sums its configured losses (MSE + LPIPS); the default here is MSE and any callable
loss can be passed -- LPIPS included (`losses.LossLpips`, on the HIP kernels for device images; its learned
weights load with `LPIPS.load_lpips_weights` when the files are available).
"""
from __future__ import annotations

from typing import Callable, Optional

import torch
from torch import Tensor


def _skew(x: Tensor) -> Tensor:
    z = torch.zeros((), dtype=x.dtype, device=x.device)
    return torch.stack([torch.stack([z, -x[2], x[1]]), torch.stack([x[2], z, -x[0]]), torch.stack([-x[1], x[0], z])])


def SO3_exp(theta: Tensor) -> Tensor:
    W = _skew(theta); W2 = W @ W
    angle = torch.norm(theta)
    I = torch.eye(3, device=theta.device, dtype=theta.dtype)
    if angle < 1e-5:
        return I + W + 0.5 * W2
    return I + (torch.sin(angle) / angle) * W + ((1 - torch.cos(angle)) / (angle ** 2)) * W2


def V_mat(theta: Tensor) -> Tensor:
    W = _skew(theta); W2 = W @ W
    angle = torch.norm(theta)
    I = torch.eye(3, device=theta.device, dtype=theta.dtype)
    if angle < 1e-5:
        return I + 0.5 * W + (1.0 / 6.0) * W2
    return I + W * ((1.0 - torch.cos(angle)) / (angle ** 2)) + W2 * ((angle - torch.sin(angle)) / (angle ** 3))


def SE3_exp(tau: Tensor) -> Tensor:
    rho, theta = tau[:3], tau[3:]
    T = torch.eye(4, device=tau.device, dtype=tau.dtype)
    T[:3, :3] = SO3_exp(theta)
    T[:3, 3] = V_mat(theta) @ rho
    return T


def update_pose(cam_trans_delta: Tensor, cam_rot_delta: Tensor, extrinsics: Tensor) -> Tensor:
    """(n,3), (n,3), c2w (n,4,4) -> new c2w  (cam_utils.py:118-137)."""
    tau = torch.cat([cam_trans_delta, cam_rot_delta], dim=-1)
    w2c = extrinsics.inverse()
    new = torch.stack([SE3_exp(tau[i]) @ w2c[i] for i in range(tau.shape[0])], dim=0)
    return new.inverse()


def align_poses(decoder, gaussians, target_image: Tensor, extrinsics: Tensor, intrinsics: Tensor, near: Tensor, far: Tensor,
                steps: int = 100, rot_lr: float = 0.005, trans_lr: float = 0.005,
                loss_fn: Optional[Callable[[Tensor, Tensor], Tensor]] = None):
    """extrinsics (b,v,4,4) initial target poses; returns (aligned extrinsics, list of per-step losses)."""
    b, v = extrinsics.shape[:2]
    h, w = target_image.shape[-2:]
    dev = extrinsics.device
    loss_fn = loss_fn or (lambda pred, tgt: ((pred - tgt) ** 2).mean())
    rot = torch.nn.Parameter(torch.zeros((b, v, 3), device=dev))
    trans = torch.nn.Parameter(torch.zeros((b, v, 3), device=dev))
    opt = torch.optim.Adam([{"params": [rot], "lr": rot_lr}, {"params": [trans], "lr": trans_lr}])
    extrinsics = extrinsics.clone()
    history = []
    for _ in range(steps):
        opt.zero_grad()
        out = decoder.forward(gaussians, extrinsics, intrinsics, near, far, (h, w), cam_rot_delta=rot, cam_trans_delta=trans)
        loss = loss_fn(out.color, target_image)
        loss.backward()
        history.append(float(loss.detach()))
        with torch.no_grad():
            opt.step()
            new = update_pose(trans.reshape(b * v, 3), rot.reshape(b * v, 3), extrinsics.reshape(b * v, 4, 4))
            rot.data.fill_(0); trans.data.fill_(0)
            extrinsics = new.reshape(b, v, 4, 4)
    return extrinsics, history


# ---------------------------------------------------------------------------
# Initial pose from the predicted geometry: `get_pnp_pose` (src/misc/cam_utils.py:158-178).  Device tensors go through
# libgsr_hip.so's gsr_pnp_ransac (csrc/gsr_pose.hip); CPU tensors take the float64 restatement of the same three stages
# below (same counter-based sample stream), which is also what the tests measure the kernels against.
# ---------------------------------------------------------------------------
PNP_SAMPLE, PNP_REFINE = 6, 10
PNP_STATUS = {0: "ok", 1: "fewer than 6 points above the opacity threshold", 2: "no valid hypothesis"}
_M64 = (1 << 64) - 1


def _mix64(z: int) -> int:
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def pnp_draw(seed: int, hypothesis: int, draw: int, m: int) -> int:
    """index in [0, m) of draw `draw` of hypothesis `hypothesis`: a pure function of its arguments (the problem's index is not among
    them: a problem's result must not depend on its place in a batch)"""
    key = ((hypothesis << 8) | draw) & _M64
    z = _mix64((seed & _M64) ^ _mix64((key + 0x9E3779B97F4A7C15) & _M64))
    return ((z >> 32) * m) >> 32


def _se3_left_np(d, R, t):
    """(R, t) <- SE3_exp(d) (R, t), d = (rho, theta), float64 numpy"""
    import numpy as np
    rho, th = d[:3], d[3:]
    W = np.array([[0, -th[2], th[1]], [th[2], 0, -th[0]], [-th[1], th[0], 0]])
    W2 = W @ W
    a = float(np.linalg.norm(th))
    I = np.eye(3)
    if a < 1e-5:
        E, V = I + W + 0.5 * W2, I + 0.5 * W + W2 / 6.0
    else:
        E = I + np.sin(a) / a * W + (1 - np.cos(a)) / a ** 2 * W2
        V = I + (1 - np.cos(a)) / a ** 2 * W + (a - np.sin(a)) / a ** 3 * W2
    return E @ R, E @ t + V @ rho


def pnp_normal_equations(R, t, X, uv, K, bound2):
    """J^T J (6,6), J^T r (6,), truncated cost sum(min(r^2, bound2)) and the inlier mask of the reprojection residuals of world points
    X (n,3) observed at uv (n,2) under the world->camera pose (R, t) and pixel intrinsics K; the update is T <- SE3_exp(d) T."""
    import numpy as np
    xc = X @ R.T + t
    z = xc[:, 2]
    front = z > 1e-9
    iz = 1.0 / np.where(front, z, 1.0)
    fx, sk, cx, fy, cy = K[0, 0], K[0, 1], K[0, 2], K[1, 1], K[1, 2]
    ru = (fx * xc[:, 0] + sk * xc[:, 1]) * iz + cx - uv[:, 0]
    rv = fy * xc[:, 1] * iz + cy - uv[:, 1]
    r2 = ru * ru + rv * rv
    with np.errstate(invalid="ignore"):
        inl = front & (r2 <= bound2)
    cost = float(np.where(inl, r2, bound2).sum()) if np.isfinite(bound2) else float(r2[inl].sum())
    x, y, zz, iz = xc[inl, 0], xc[inl, 1], xc[inl, 2], iz[inl]
    a0, a1, a2 = fx * iz, sk * iz, -(fx * x + sk * y) * iz * iz
    b1, b2 = fy * iz, -fy * y * iz * iz
    J0 = np.stack([a0, a1, a2, -a1 * zz + a2 * y, a0 * zz - a2 * x, -a0 * y + a1 * x], 1)
    J1 = np.stack([np.zeros_like(a0), b1, b2, -b1 * zz + b2 * y, -b2 * x, b1 * x], 1)
    H = J0.T @ J0 + J1.T @ J1
    g = J0.T @ ru[inl] + J1.T @ rv[inl]
    return H, g, cost, inl


def pnp_refine(R, t, X, uv, K, bound2, iterations: int = PNP_REFINE):
    """the Levenberg-Marquardt stage: a candidate is accepted iff the truncated cost falls; `bound2 = inf` refines on all of X"""
    import numpy as np
    cur, cand = (R, t), (R, t)
    cost_cur, lam, H, g = np.inf, 1e-3, None, None
    for it in range(iterations):
        Hc, gc, cost, inl = pnp_normal_equations(cand[0], cand[1], X, uv, K, bound2)
        if cost < cost_cur and inl.sum() >= PNP_SAMPLE:
            cur, H, g, cost_cur, lam = cand, Hc, gc, cost, max(lam * 0.2, 1e-12)
        else:
            lam = min(lam * 10.0, 1e12)
        if it == iterations - 1 or H is None:
            continue
        try:
            d = np.linalg.solve(H + lam * np.diag(np.diag(H)), -g)
        except np.linalg.LinAlgError:
            continue
        if np.isfinite(d).all():
            cand = _se3_left_np(d, cur[0], cur[1])
    return cur


def _pnp_hypothesis(X, uv, K):
    """six points -> (R, t) or None: DLT with p34 = 1 on centred / scaled points (11 of the 12 equations), polar factor, Gauss-Newton"""
    import numpy as np
    vn = (uv[:, 1] - K[1, 2]) / K[1, 1]
    un = (uv[:, 0] - K[0, 2] - K[0, 1] * vn) / K[0, 0]
    c = X.mean(0)
    sc = float(np.sqrt(((X - c) ** 2).sum() / PNP_SAMPLE))
    if not (sc > 1e-12) or not np.isfinite(sc):
        return None
    Xn = (X - c) / sc
    A, rhs = np.zeros((11, 11)), np.zeros(11)
    for r in range(11):
        d, isv = r >> 1, r & 1
        o = vn[d] if isv else un[d]
        A[r, 4 * isv:4 * isv + 3] = Xn[d]; A[r, 4 * isv + 3] = 1.0
        A[r, 8:11] = -o * Xn[d]
        rhs[r] = o
    if not np.isfinite(A).all() or np.linalg.matrix_rank(A, tol=1e-9) < 11:
        return None
    th = np.linalg.solve(A, rhs)
    Am = np.stack([th[0:3], th[4:7], th[8:11]]) / sc
    bv = np.array([th[3], th[7], 1.0]) - Am @ c
    det = np.linalg.det(Am)
    if not (det > 1e-300) or not np.isfinite(det):
        return None
    mu = 1.0 / np.cbrt(det)
    R, t = mu * Am, mu * bv
    for _ in range(12):
        if not abs(np.linalg.det(R)) > 1e-12:
            return None
        R = 0.5 * (R + np.linalg.inv(R).T)
    unit = np.eye(3)
    obs = np.stack([un, vn], 1)
    for _ in range(5):
        H, g, _, inl = pnp_normal_equations(R, t, X, obs, unit, np.inf)
        if inl.sum() < PNP_SAMPLE:
            return None
        try:
            d = np.linalg.solve(H + 1e-9 * np.diag(np.diag(H)), -g)
        except np.linalg.LinAlgError:
            return None
        if not np.isfinite(d).all():
            return None
        R, t = _se3_left_np(d, R, t)
    if not (np.isfinite(R).all() and np.isfinite(t).all() and ((X @ R.T + t)[:, 2] > 1e-9).all()):
        return None
    return R, t


def pnp_ransac_host(pts3d, opacity, K, W: int, opacity_threshold: float = 0.3, iterations: int = 100, reprojection_error: float = 5.0,
                    seed: int = 0, pixel_offset: float = 0.0):
    """one problem in float64 numpy: pts3d (N,3), opacity (N,), pixel-unit K (3,3) -> (c2w (4,4), inlier mask (N,) bool, status (4,) int:
    masked points, inliers, winning hypothesis, code)"""
    import numpy as np
    pts3d, opacity, K = np.asarray(pts3d, np.float64), np.asarray(opacity, np.float64), np.asarray(K, np.float64)
    n = pts3d.shape[0]
    idx = np.nonzero(opacity > opacity_threshold)[0]
    m = len(idx)
    fail = lambda code: (np.eye(4), np.zeros(n, bool), np.array([m, 0, -1, code]))
    if m < PNP_SAMPLE:
        return fail(1)
    X = pts3d[idx]
    uv = np.stack([idx % W + pixel_offset, idx // W + pixel_offset], 1).astype(np.float64)
    bound2 = float(reprojection_error) ** 2
    best, best_count, best_h = None, -1, -1
    for h in range(iterations):
        pick = [pnp_draw(seed, h, d, m) for d in range(PNP_SAMPLE)]
        if len(set(pick)) < PNP_SAMPLE:
            continue
        with np.errstate(all="ignore"):
            hyp = _pnp_hypothesis(X[pick], uv[pick], K)
            if hyp is None:
                continue
            count = int(pnp_normal_equations(hyp[0], hyp[1], X, uv, K, bound2)[3].sum())
        if count > best_count:
            best, best_count, best_h = hyp, count, h
    if best is None or best_count < PNP_SAMPLE:
        return fail(2)
    with np.errstate(all="ignore"):
        R, t = pnp_refine(best[0], best[1], X, uv, K, bound2)
        inl = pnp_normal_equations(R, t, X, uv, K, bound2)[3]
    mask = np.zeros(n, bool)
    mask[idx[inl]] = True
    c2w = np.eye(4)
    c2w[:3, :3], c2w[:3, 3] = R.T, -R.T @ t
    return c2w, mask, np.array([m, int(inl.sum()), best_h, 0])


def pnp_pose(means: Tensor, opacities: Tensor, intrinsics: Tensor, image_hw, opacity_threshold: float = 0.3, iterations: int = 100,
             reprojection_error: float = 5.0, seed: int = 0, pixel_offset: float = 0.0, strict: bool = False):
    """`get_pnp_pose` for any number of problems: means (..., h, w, 3), opacities (..., h, w), normalised intrinsics (..., 3, 3) (row 0 is
    scaled by w, row 1 by h), `image_hw = (h, w)`.  Pixel (row y, column x) is observed at (x + pixel_offset, y + pixel_offset);
    0 is the reference's integer grid.  Returns (c2w (..., 4, 4) fp32, status): status holds tensors on the inputs' device -- `masked`,
    `inliers`, `winner`, `code` (..., ) int32 (code: PNP_STATUS) and `inlier_mask` (..., h, w) bool.  Nothing is read back unless `strict`,
    which raises where the reference's `assert success` would."""
    h, w = int(image_hw[0]), int(image_hw[1])
    if means.shape[-3:] != (h, w, 3) or opacities.shape[-2:] != (h, w) or intrinsics.shape[-2:] != (3, 3):
        raise ValueError(f"pnp_pose: means {tuple(means.shape)}, opacities {tuple(opacities.shape)}, intrinsics {tuple(intrinsics.shape)} do "
                         f"not fit image_hw {(h, w)}")
    lead = means.shape[:-3]
    if opacities.shape[:-2] != lead or intrinsics.shape[:-2] != lead:
        raise ValueError("pnp_pose: means, opacities and intrinsics need the same leading dimensions")
    P, N = 1, h * w
    for s in lead:
        P *= s
    if P < 1:
        raise ValueError("pnp_pose: no problem to solve")
    dev = means.device
    K = intrinsics.detach().reshape(P, 3, 3).float().clone()
    K[:, 0, :] *= w
    K[:, 1, :] *= h
    pts = means.detach().reshape(P, N, 3).float().contiguous()
    op = opacities.detach().reshape(P, N).float().contiguous()
    if pts.is_cuda:
        import ctypes as C
        from . import _lib
        lib = _lib.load()
        c2w = torch.empty((P, 4, 4), dtype=torch.float32, device=dev)
        mask = torch.empty((P, N), dtype=torch.uint8, device=dev)
        status = torch.empty((P, 4), dtype=torch.int32, device=dev)
        scratch = torch.empty(lib.gsr_pnp_ransac_scratch_bytes(P, h, w, int(iterations)), dtype=torch.uint8, device=dev)
        _lib.check(lib.gsr_pnp_ransac(pts.data_ptr(), op.data_ptr(), K.contiguous().data_ptr(), P, h, w, N, float(opacity_threshold),
                                      float(reprojection_error), int(iterations), int(seed) & _M64, float(pixel_offset), c2w.data_ptr(),
                                      mask.data_ptr(), status.data_ptr(), scratch.data_ptr(),
                                      C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)), "gsr_pnp_ransac")
        mask = mask.bool()
    else:
        import numpy as np
        res = [pnp_ransac_host(pts[p].numpy(), op[p].numpy(), K[p].numpy(), w, opacity_threshold, iterations, reprojection_error, seed,
                               pixel_offset) for p in range(P)]
        c2w = torch.from_numpy(np.stack([r[0] for r in res]).astype(np.float32))
        mask = torch.from_numpy(np.stack([r[1] for r in res]))
        status = torch.from_numpy(np.stack([r[2] for r in res]).astype(np.int32))
    out = {"masked": status[:, 0].reshape(lead), "inliers": status[:, 1].reshape(lead), "winner": status[:, 2].reshape(lead),
           "code": status[:, 3].reshape(lead), "inlier_mask": mask.reshape(*lead, h, w)}
    if strict:
        bad = status[:, 3].cpu()
        if bool((bad != 0).any()):
            p = int((bad != 0).nonzero()[0])
            raise RuntimeError(f"pnp_pose: problem {p} of {P} failed: {PNP_STATUS[int(bad[p])]}")
    return c2w.reshape(*lead, 4, 4), out
