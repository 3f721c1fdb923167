"""Plain restatements of what the element-wise pass kernels compute, for tests/test_gpu_pass_paths.py to compare against; each is pinned
on the CPU by tests/test_pass_reference_host.py.

* Philox-4x32-10 in numpy uint64 and the keep decision of vit_relu_dropout_fwd / vit_head_tail_* (csrc/vit_common.h: philox4x32_10).
* The x2 bilinear (align_corners) operator as a (2n, n) float64 matrix whose floor decisions and lambdas are the kernels' float32 ones.
* The patch orders of vit_im2col7 and vit_im2col3_rows, from F.unfold."""
import numpy as np
import torch

_M32 = np.uint64(0xFFFFFFFF)
_PHILOX_M0, _PHILOX_M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_PHILOX_W0, _PHILOX_W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)


def philox4x32_10(ctr, key):
    """Philox-4x32 with 10 rounds (Salmon et al., SC'11).  ctr: four and key: two integers or equally shaped integer arrays of 32-bit
    words; returns the four output words as uint64 arrays holding 32-bit values.  Every product of two 32-bit words fits in uint64."""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & _M32 for c in ctr)
    k0, k1 = (np.asarray(k, dtype=np.uint64) & _M32 for k in key)
    for _ in range(10):
        p0, p1 = _PHILOX_M0 * c0, _PHILOX_M1 * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & _M32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & _M32
        k0, k1 = (k0 + _PHILOX_W0) & _M32, (k1 + _PHILOX_W1) & _M32
    return c0, c1, c2, c3


def keep_threshold(p, kernel="relu_dropout"):
    """The 32-bit threshold a draw is compared against (keep if word < thresh), with keep = 1 - double(float32(p)):
        relu_dropout_fwd:             keep >= 1 ? 0xFFFFFFFF : uint32(keep * 2^32)
        head_tail_fwd / _bwd:         uint32(min(keep * 2^32, 4294967295.0))
    The first saturates on keep itself, the second on the product.  keep * 2^32 is exact in double (a power-of-two scaling) and, for
    keep < 1, is below 2^32, so truncation and the clamp to 4294967295.0 give the same word: the two expressions agree for EVERY p in
    [0, 1).  (What differs at p = 0 is not the threshold: head_tail then runs its no-dropout instantiation and draws nothing, while
    relu_dropout still drops an element whose word is 0xFFFFFFFF.)"""
    keep = 1.0 - float(np.float32(p))
    if kernel == "relu_dropout":
        return 0xFFFFFFFF if keep >= 1.0 else int(keep * 4294967296.0)
    assert kernel == "head_tail", kernel
    return int(min(keep * 4294967296.0, 4294967295.0))


def keep_scale(p):
    """the factor of a kept element: float32(1 / (1 - double(float32(p))))"""
    return np.float32(1.0 / (1.0 - float(np.float32(p))))


def keep(seed, element_index, p, kernel="relu_dropout"):
    """keep decision of the element(s) with flat index `element_index` of a contiguous tensor: counter = (i4 low, i4 high, 0, 0) with
    i4 = index // 4, key = (seed low, seed high), output word = index % 4, keep if word < thresh.  Returns a bool array."""
    idx = np.asarray(element_index, dtype=np.uint64)
    i4 = idx >> np.uint64(2)
    seed = int(seed)
    words = philox4x32_10((i4 & _M32, i4 >> np.uint64(32), 0, 0), (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))
    lane = (idx & np.uint64(3)).astype(np.int64)
    word = np.choose(lane, [np.broadcast_to(w, idx.shape) for w in words])
    return word < np.uint64(keep_threshold(p, kernel))


def upsample_taps(n):
    """(i0, i1, w0, w1) of the 2n outputs of one axis: source cell, clamped neighbour and the float32 weights 1 - lambda / lambda, with
    the kernels' (and the framework's) float32 arithmetic: r = f32(n - 1) / f32(2n - 1), s = r * f32(o), i = int(s), lambda = s - i."""
    f = np.float32
    r = f(n - 1) / f(2 * n - 1) if n > 1 else f(0)
    s = (r * np.arange(2 * n, dtype=np.float32)).astype(np.float32)
    i0 = s.astype(np.int64)
    lam = (s - i0.astype(np.float32)).astype(np.float32)
    i1 = i0 + (i0 < n - 1)
    return i0, i1, (f(1) - lam).astype(np.float32), lam


def upsample_matrix(n):
    """(2n, n) float64 matrix A of the x2 bilinear align_corners=True operator of one axis; forward = A_h X A_w^T, backward = A_h^T G A_w.
    The floor decisions and the float32 weights are the kernel's own (upsample_taps), widened to float64: what remains between A X A^T in
    float64 and a correct kernel is the fp32 rounding of its products and sums."""
    i0, i1, w0, w1 = upsample_taps(n)
    a = np.zeros((2 * n, n), dtype=np.float64)
    o = np.arange(2 * n)
    np.add.at(a, (o, i0), w0.astype(np.float64))
    np.add.at(a, (o, i1), w1.astype(np.float64))          # (at the last cell both weights land on n - 1, as in the kernels)
    return a


def upsample_forward(x):
    """(..., H, W) -> (..., 2H, 2W) in float64"""
    x = np.asarray(x, dtype=np.float64)
    return upsample_matrix(x.shape[-2]) @ x @ upsample_matrix(x.shape[-1]).T


def upsample_backward(g):
    """(..., 2H, 2W) -> (..., H, W) in float64.  Taps of weight zero are SKIPPED, not multiplied: a +-inf in g reaches exactly the input
    pixels that have a non-zero weight on it (inf there), and no 0 * inf = NaN appears anywhere else."""
    g = np.asarray(g, dtype=np.float64)
    ah, aw = upsample_matrix(g.shape[-2] // 2), upsample_matrix(g.shape[-1] // 2)
    inf = np.isinf(g)
    out = ah.T @ np.where(inf, 0.0, g) @ aw
    if inf.any():
        nzh, nzw = (ah.T != 0).astype(np.float64), (aw != 0).astype(np.float64)
        pos, neg = nzh @ (g == np.inf).astype(np.float64) @ nzw > 0, nzh @ (g == -np.inf).astype(np.float64) @ nzw > 0
        out = np.where(pos & neg, np.nan, np.where(pos, np.inf, np.where(neg, -np.inf, out)))
    return out


def im2col7_reference(img):
    """vit_im2col7: (B, 3, H, W) -> (B, 160, H, W) = the 147 rows of unfold(img, 7, padding=3) in (ci, ky, kx) order + 13 zero planes"""
    B, _, H, W = img.shape
    cols = torch.nn.functional.unfold(img, 7, padding=3).reshape(B, 147, H, W)
    return torch.cat((cols, torch.zeros(B, 13, H, W, dtype=img.dtype, device=img.device)), 1)


def im2col3_rows_reference(x, relu):
    """vit_im2col3_rows: (B, Ci, H, W) -> (B H W, 9 Ci), cols[(b, y, x)][(tap, ci)] with tap = 3 dy + dx of unfold(f(x), 3, padding=1)"""
    B, Ci, H, W = x.shape
    u = torch.nn.functional.unfold(torch.relu(x) if relu else x, 3, padding=1)            # (B, Ci * 9, H W), row ci * 9 + tap
    return u.reshape(B, Ci, 9, H * W).permute(0, 3, 2, 1).reshape(B * H * W, 9 * Ci).contiguous()
