"""Inputs and the independent yardstick of the multi-view consistency tests (tests/test_consistency_host.py, tests/test_gpu_consistency.py).

`shift_scene` is the dyadic scene in which the warp is an exact integer shift.  `random_scene` is a seeded V = 3 scene with rotated
cameras, a pair of views that face apart, an occluding block and invalid depth pixels; it ASSERTS that no pixel of any pair whose views
differ lies within a relative `MARGIN` of a validity threshold (image bounds, z > 0, the occlusion test): under that condition the mask
does not depend on the last bits of the arithmetic, and a device must reproduce it exactly.  A pair (i, i) maps every pixel onto itself,
so its border pixels sit ON the bounds by construction; they are left out of the margin, and equality there rests on both sides running
the same IEEE operations.  `loop_reference` is the per-pixel restatement in Python floats, written from include/gsr.h's formulas and
sharing no code with `metrics.warp_consistency_expression`; it also measures the margin."""
import math

import numpy as np
import torch

MARGIN = 1e-9
DEPTH_TOL = 0.05


def summation_bound(H, W):
    """relative bound of the difference of two orderings of the 3 H W non-negative float64 terms of one sse"""
    return 3 * H * W * 2.0 ** -52


def _valid_depth(d):
    return math.isfinite(d) and d > 0


def loop_reference(images, depth, c2w, K, pairs, depth_tol=DEPTH_TOL):
    """images (S,V,3,H,W) fp32, depth (V,H,W) fp32, c2w (V,4,4) / K (V,3,3) float64, pairs (P,2) -- tensors or arrays.  Returns a dict of
    numpy arrays: mask (P,H,W) bool, count (P,), warped (S,P,3,H,W) fp32, sse (S,P) float64 (pixels added in row-major order), and
    `margin` (P,): the least relative distance of any pixel of the pair from a threshold it was tested against."""
    img = np.asarray(images, dtype=np.float32)
    dep = np.asarray(depth, dtype=np.float32)
    E, Kn, pr = np.asarray(c2w, dtype=np.float64), np.asarray(K, dtype=np.float64), np.asarray(pairs)
    if img.ndim == 4:
        img = img[None]
    S, V, _, H, W = img.shape
    P = pr.shape[0]
    mask = np.zeros((P, H, W), dtype=bool)
    warped = np.zeros((S, P, 3, H, W), dtype=np.float32)
    sse = np.zeros((S, P), dtype=np.float64)
    margin = np.full(P, np.inf)
    for p in range(P):
        i, j = int(pr[p, 0]), int(pr[p, 1])
        if not (0 <= i < V and 0 <= j < V):
            continue
        Ri, ti = [[float(E[i, r, c]) for c in range(3)] for r in range(3)], [float(E[i, r, 3]) for r in range(3)]
        Rj, tj = [[float(E[j, r, c]) for c in range(3)] for r in range(3)], [float(E[j, r, 3]) for r in range(3)]
        fxi, fyi, cxi, cyi = float(Kn[i, 0, 0]), float(Kn[i, 1, 1]), float(Kn[i, 0, 2]), float(Kn[i, 1, 2])
        fxj, fyj, cxj, cyj = float(Kn[j, 0, 0]), float(Kn[j, 1, 1]), float(Kn[j, 0, 2]), float(Kn[j, 1, 2])
        acc = [0.0] * S
        near = math.inf
        for y in range(H):
            for x in range(W):
                d = float(dep[j, y, x])
                if not _valid_depth(d):
                    continue
                u, v = (x + 0.5) / W, (y + 0.5) / H
                xc, yc = ((u - cxj) / fxj) * d, ((v - cyj) / fyj) * d
                w = [((Rj[r][0] * xc + Rj[r][1] * yc) + Rj[r][2] * d) + tj[r] for r in range(3)]
                dl = [w[r] - ti[r] for r in range(3)]
                q = [(Ri[0][c] * dl[0] + Ri[1][c] * dl[1]) + Ri[2][c] * dl[2] for c in range(3)]
                z = q[2]
                near = min(near, abs(z) / max(1.0, abs(d)))
                if not z > 0:
                    continue
                px = ((fxi * q[0]) / z + cxi) * W - 0.5
                py = ((fyi * q[1]) / z + cyi) * H - 0.5
                near = min(near, abs(px) / W, abs(px - (W - 1)) / W, abs(py) / H, abs(py - (H - 1)) / H)
                if not (0 <= px <= W - 1 and 0 <= py <= H - 1):
                    continue
                x0, y0 = min(math.floor(px), W - 2), min(math.floor(py), H - 2)
                ax, ay = px - x0, py - y0
                wt = ((1.0 - ax) * (1.0 - ay), ax * (1.0 - ay), (1.0 - ax) * ay, ax * ay)
                at = ((y0, x0), (y0, x0 + 1), (y0 + 1, x0), (y0 + 1, x0 + 1))
                dt = [float(dep[i, a, b]) for a, b in at]
                if not all(_valid_depth(t) for t in dt):
                    continue
                D = ((wt[0] * dt[0] + wt[1] * dt[1]) + wt[2] * dt[2]) + wt[3] * dt[3]
                near = min(near, abs(abs(z - D) - depth_tol * D) / D)
                if not abs(z - D) <= depth_tol * D:
                    continue
                mask[p, y, x] = True
                for s in range(S):
                    e = 0.0
                    for c in range(3):
                        t = [float(img[s, i, c, a, b]) for a, b in at]
                        val = np.float32(((wt[0] * t[0] + wt[1] * t[1]) + wt[2] * t[2]) + wt[3] * t[3])
                        warped[s, p, c, y, x] = val
                        diff = float(val) - float(img[s, j, c, y, x])
                        e = e + diff * diff if c else diff * diff
                    acc[s] += e
        sse[:, p] = acc
        margin[p] = near
    return dict(mask=mask, count=mask.sum(axis=(1, 2)).astype(np.int32), warped=warped, sse=sse, margin=margin)


def shift_scene(k, occluder=None):
    """16 x 16, identity rotations, fx = fy = 1, cx = cy = 0.5, depth 1 everywhere, view 0 (src) moved by -k/16 along x against view 1
    (dst): every quantity is a dyadic rational and a dst pixel (x, y) lands on src pixel (x + k, y) exactly.  Colours are multiples of
    1/256.  `occluder` (y0, y1, x0, x1): a block of depth 0.5 in the src depth.  pairs = [(0, 1)]."""
    H = W = 16
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    src = np.stack([((ys * 16 + xs + 37 * c) % 256) / 256.0 for c in range(3)]).astype(np.float32)
    dst = np.stack([((ys * 5 + xs * 3 + 11 * c) % 128) / 256.0 for c in range(3)]).astype(np.float32)
    depth = np.ones((2, H, W), dtype=np.float32)
    if occluder is not None:
        y0, y1, x0, x1 = occluder
        depth[0, y0:y1, x0:x1] = 0.5
    c2w = np.tile(np.eye(4), (2, 1, 1))
    c2w[0, 0, 3] = -k / 16.0
    K = np.tile(np.array([[1.0, 0, 0.5], [0, 1.0, 0.5], [0, 0, 1.0]]), (2, 1, 1))
    return dict(images=torch.from_numpy(np.stack([src, dst])[None]), depth=torch.from_numpy(depth), c2w=torch.from_numpy(c2w),
                K=torch.from_numpy(K), pairs=torch.tensor([[0, 1]], dtype=torch.int64), k=k)


def _rotation(rng, angle):
    """Rodrigues rotation about a random axis, float64 (orthonormal to rounding)"""
    a = rng.standard_normal(3)
    a /= np.linalg.norm(a)
    A = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + math.sin(angle) * A + (1 - math.cos(angle)) * (A @ A)


ALL_PAIRS = ((0, 1), (1, 0), (1, 1), (0, 2), (2, 1))       # both directions, a view onto itself, and two pairs with the view that faces away


def random_scene(seed, S, H, W, pairs=ALL_PAIRS, invalid=True, check=True):
    """V = 3.  Views 0 and 1 look down +z from nearby positions with small rotations; view 2 is turned by pi about y, so nothing one of
    the others sees lies in front of it (count 0).  Depth is a smooth field around 2 with fp32 noise; view 0 carries a nearer block
    (occlusion), view 1 -- when `invalid` and the image has room -- the four kinds of invalid depth (0, negative, NaN, +inf).
    Returns torch tensors: images (S,3,3,H,W) fp32, depth fp32, c2w / K float64, pairs int64, and `margin` (P,) from `loop_reference`."""
    rng = np.random.default_rng(seed)
    V = 3
    images = np.random.default_rng(seed + 1000).random((S, V, 3, H, W)).astype(np.float32)      # (the geometry does not depend on S)
    ys, xs = np.meshgrid((np.arange(H) + 0.5) / H, (np.arange(W) + 0.5) / W, indexing="ij")
    depth = np.stack([2.0 + 0.3 * np.sin(3 * xs + v) * np.cos(2 * ys - v) + 0.01 * rng.random((H, W)) for v in range(V)]).astype(np.float32)
    if H >= 4 and W >= 4:
        depth[0, H // 4:H // 2 + 1, W // 4:W // 2 + 1] = 1.0
    if invalid and H >= 4 and W >= 4:
        depth[1, 1, 1], depth[1, 1, 2], depth[1, H - 2, 1], depth[1, H - 2, W - 2] = 0.0, -1.5, np.nan, np.inf
    c2w = np.tile(np.eye(4), (V, 1, 1))
    for v in range(V):
        c2w[v, :3, :3] = _rotation(rng, 0.08 * rng.random())
        c2w[v, :3, 3] = 0.15 * (rng.random(3) - 0.5)
    c2w[2, :3, :3] = c2w[2, :3, :3] @ np.diag([-1.0, 1.0, -1.0])
    K = np.tile(np.eye(3), (V, 1, 1))
    K[:, 0, 0], K[:, 1, 1] = 0.9 + 0.3 * rng.random(V), 0.9 + 0.3 * rng.random(V)
    K[:, 0, 2], K[:, 1, 2] = 0.5 + 0.04 * (rng.random(V) - 0.5), 0.5 + 0.04 * (rng.random(V) - 0.5)
    pr = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    scene = dict(images=torch.from_numpy(images), depth=torch.from_numpy(depth), c2w=torch.from_numpy(c2w), K=torch.from_numpy(K),
                 pairs=torch.from_numpy(pr))
    if check:
        ref = loop_reference(images[:1], depth, c2w, K, pr)
        scene["margin"] = ref["margin"]
        scene["ref_count"] = ref["count"]
        for p, (i, j) in enumerate(pr.tolist()):
            assert i == j or ref["margin"][p] > MARGIN, f"seed {seed} {H} x {W}: pair {(i, j)} has a pixel within {ref['margin'][p]:.2e} of a threshold"
    return scene
