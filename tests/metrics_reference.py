"""Restatements the test-step tests compare against (numpy / torch on the host):
  * `ssim`: skimage structural_similarity(gt, hat, win_size=11, gaussian_weights=True, channel_axis=0, data_range=1.0) per image, as the
    valid 11 x 11 filter of the interior.  "f64": all in float64.  "f32": what the reference does with float32 images -- scipy filters in
    float64 and stores float32 moments, the SSIM map is float32 arithmetic, its mean float64.
  * `ssim_scipy`: the same through scipy.ndimage.gaussian_filter(mode="reflect", sigma=1.5, truncate=3.5) of the whole image + skimage's
    crop of 5 (scipy only).
  * `mse`: mean over C*H*W of (clip(gt,0,1) - clip(pred,0,1))^2 in float64.
  * `pose_adam_step`: one gsr_pose_adam_update step in float64 (Adam on zero deltas, then c2w <- (SE3_exp(tau) c2w^-1)^-1).
"""
import numpy as np

R = 5
C1, C2 = 1e-4, 9e-4
COV_NORM = 121.0 / 120.0


def window():
    x = np.arange(-R, R + 1, dtype=np.float64)
    w = np.exp(-0.5 / 1.5 ** 2 * x * x)
    return w / w.sum()


def _valid(a, w):
    """separable valid filter over the last two axes, float64"""
    h, wd = a.shape[-2:]
    t = sum(w[k] * a[..., :, k:wd - 2 * R + k] for k in range(2 * R + 1))
    return sum(w[k] * t[..., k:h - 2 * R + k, :] for k in range(2 * R + 1))


def _map(ux, uy, uxx, uyy, uxy):
    vx, vy, vxy = COV_NORM * (uxx - ux * ux), COV_NORM * (uyy - uy * uy), COV_NORM * (uxy - ux * uy)
    return ((2 * ux * uy + C1) * (2 * vxy + C2)) / ((ux * ux + uy * uy + C1) * (vx + vy + C2))


def ssim(gt, pred, precision="f64"):
    """(N, C, H, W) arrays -> (N,) float64"""
    gt, pred = np.asarray(gt), np.asarray(pred)
    if min(gt.shape[-2:]) < 2 * R + 1:
        raise ValueError("win_size exceeds image extent")
    x, y = gt.astype(np.float64), pred.astype(np.float64)
    w = window()
    mom = [_valid(t, w) for t in (x, y, x * x, y * y, x * y)]
    if precision == "f32":
        x32, y32 = gt.astype(np.float32).astype(np.float64), pred.astype(np.float32).astype(np.float64)
        mom = [_valid(t, w).astype(np.float32) for t in (x32, y32, x32 * x32, y32 * y32, x32 * y32)]
        s = _map(*mom).astype(np.float32)
        return s.astype(np.float64).mean(axis=(2, 3)).mean(axis=1)
    return _map(*mom).mean(axis=(2, 3)).mean(axis=1)


def ssim_scipy(gt, pred):
    from scipy.ndimage import gaussian_filter
    x, y = np.asarray(gt, np.float64), np.asarray(pred, np.float64)
    out = np.zeros(x.shape[0])
    for n in range(x.shape[0]):
        per = []
        for c in range(x.shape[1]):
            f = lambda a: gaussian_filter(a, sigma=1.5, truncate=3.5, mode="reflect")
            a, b = x[n, c], y[n, c]
            s = _map(f(a), f(b), f(a * a), f(b * b), f(a * b))
            per.append(s[R:-R, R:-R].mean())
        out[n] = np.mean(per)
    return out


def mse(gt, pred):
    d = np.clip(np.asarray(gt, np.float64), 0, 1) - np.clip(np.asarray(pred, np.float64), 0, 1)
    return (d * d).reshape(d.shape[0], -1).mean(axis=1)


def _se3_exp(tau):
    rho, th = tau[:3], tau[3:]
    W = np.array([[0, -th[2], th[1]], [th[2], 0, -th[0]], [-th[1], th[0], 0]])
    W2 = W @ W
    a = np.linalg.norm(th)
    I = np.eye(3)
    if a < 1e-5:
        Rm, V = I + W + 0.5 * W2, I + 0.5 * W + W2 / 6.0
    else:
        Rm = I + np.sin(a) / a * W + (1 - np.cos(a)) / a ** 2 * W2
        V = I + (1 - np.cos(a)) / a ** 2 * W + (a - np.sin(a)) / a ** 3 * W2
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = Rm, V @ rho
    return T


def pose_adam_step(c2w, m, v, g_rot, g_trans, step, lr_rot, lr_trans, beta1=0.9, beta2=0.999, eps=1e-8):
    """float64; c2w (n,4,4), m / v (n,6) = (rot, trans) moments, updated in place; returns the new c2w"""
    g = np.concatenate([g_rot, g_trans], axis=1).astype(np.float64)
    m[:] = beta1 * m + (1 - beta1) * g
    v[:] = beta2 * v + (1 - beta2) * g * g
    lr = np.array([lr_rot] * 3 + [lr_trans] * 3)
    delta = -(lr / (1 - beta1 ** step)) * m / (np.sqrt(v) / np.sqrt(1 - beta2 ** step) + eps)
    out = np.empty_like(np.asarray(c2w, np.float64))
    for i in range(out.shape[0]):
        tau = np.concatenate([delta[i, 3:], delta[i, :3]])          # (rho = trans, theta = rot)
        out[i] = np.linalg.inv(_se3_exp(tau) @ np.linalg.inv(np.asarray(c2w[i], np.float64)))
    return out
