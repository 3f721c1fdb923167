"""What each split-arithmetic mode costs on a given input, with no kernel involved (test_gemm_emulation_host.py, test_gpu_gemm_ranges.py).

`emulate(a, b, mode)` is the contraction a (R, C) . b (S, C)^T the way the Linear and convolution kernels form it: each operand's pieces exactly
as the kernel makes them (tests/weight_image_cases._pieces: the one restatement of the split), the mode's partial products --
  bf16x6  all six a_i b_j with i + j <= 2        bf16x3  a0 b0 + a0 b1 + a1 b0        f16x3  h h' + h l' + l h', un-scaled by the two exact scales
-- summed in FLOAT64.  Its distance from the float64 product of the fp32 operands is the price of the ARITHMETIC on this input; a kernel differs
from it only by its fp32 accumulation, which the float32 yardstick (`yardstick`: numpy's a.astype(f32) @ b.T) measures on the same input.

The case generators below build the operand layouts of test_gpu_gemm_ranges.py: one 30 x outlier that sets a tensor's power-of-two scale and two
reduced blocks far below the bulk, whose outputs are judged AT THEIR OWN SCALE (tests/gpu_utils.worst_row_rel_2d).
  L1 rows of x small -> rows of y      L2 rows of dY small -> rows of dX      L3 columns of dY small -> rows of dW, entries of db
  L4 rows of W small -> columns of y (rows of y^T)      L5 x[:, k0] 2^c, W[:, k0] 2^-c -> every row of y, dX, dW at full accuracy
For a convolution the small operand of L1 / L2 is one whole image of the batch and a row of y / dX is one (b, channel) plane.

The bar of the GPU tests, and of the host test that shows it is sharp (`bar`):
    e_kernel <= EMU_MULT x e_emulation + YARD_MULT x e_f32_yardstick + FLOOR        (all three: worst-row errors against float64, same bytes)
FLOOR: the fp32 rounding of the stored output, the attention range file's YARD_FLOOR.  EMU_MULT, YARD_MULT: the smallest powers of two >= 2 x the
worst ratio measured over the 990 judged groups of test_gpu_gemm_ranges.py on an MI355X (profiles/r07_gemm_range_bars.jsonl; the factor 2 is the
run-to-run margin of the split-contraction atomics):
  EMU_MULT   (kernel - yardstick) / emulation where the arithmetic dominates (emulation >= 16 x yardstick): worst 0.99 -- on the f16x3 reduced
             blocks kernel / emulation itself is 0.987 .. 1.005 on EVERY route: fp16 subnormals survive the conversion, the residual and the MFMA
  YARD_MULT  (kernel - EMU_MULT x emulation - FLOOR) / yardstick: worst 3.3 (a bias gradient: fp32 atomics in arrival order against numpy's
             pairwise sum); for the products themselves (kernel - emulation) / yardstick stays below 2.4"""
import numpy as np
import torch

from tests.gpu_utils import worst_row_rel_2d
from tests.weight_image_cases import f16_scale_of, piece_planes, word_of, word_slots

MODES = ("bf16x6", "bf16x3", "f16x3")
PRODUCTS = {"bf16x6": ((0, 0), (0, 1), (1, 0), (0, 2), (1, 1), (2, 0)), "bf16x3": ((0, 0), (0, 1), (1, 0)), "f16x3": ((0, 0), (0, 1), (1, 0))}
OWN_SCALE_BAR = 2e-4                  # the project's figure for rows 2^20 below their tensor's maximum (test_gpu_vit.py, test_gpu_attention_ranges.py)
# emulated worst-row error of full-scale rows.  bf16x3 leaves out a0 b2 + a1 b1 + a2 b0 <= (2^-17 + 2^-18 + 2^-17) |a| |b| = 1.25 x 2^-16 of every
# term; a row's terms sum to up to ~3 x its largest entry on these inputs (few rows of a short contraction): 2^-14
FULL_SCALE_CAP = {"bf16x6": 2.0 ** -20, "f16x3": 2.0 ** -20, "bf16x3": 2.0 ** -14}
EMU_MULT, YARD_MULT, FLOOR = 2.0, 8.0, 2e-6
OUTLIER = 30.0
MUTANTS = ("flush", "scale", "stale")


def bar(e_emulation, e_yardstick):
    return EMU_MULT * e_emulation + YARD_MULT * e_yardstick + FLOOR


def _word(values):
    return word_of(torch.as_tensor(np.ascontiguousarray(values, dtype=np.float32)))


def operand_pieces(values, mode, word=None, mutant=None):
    """float64 planes of the pieces of one operand TENSOR (any shape).  word: the |max| word the launch is handed (default: the tensor's own).
    mutant: a deliberately wrong split, for the sensitivity test --
      "flush"  fp16 subnormal pieces (below 2^-14 in scaled units) read as zero        "scale"  the power of two 2^3 too small
    (the third, a STALE word, is an argument: `word` of another tensor)"""
    v = torch.as_tensor(np.ascontiguousarray(values, dtype=np.float32))
    if mode != "f16x3":
        return [p.numpy() for p in piece_planes(v, mode)]
    word = word_of(v) if word is None else word
    if mutant == "scale":
        word = (word.view(torch.float32) * 8.0).view(torch.int32)          # a maximum 2^3 larger: a scale 2^3 smaller
    planes = [p.numpy() for p in piece_planes(v, mode, word)]
    if mutant == "flush":
        s = f16_scale_of(word_slots(word).max())
        planes = [np.where(np.abs(p * s) < 2.0 ** -14, 0.0, p) for p in planes]
    return planes


def emulate(a, b, mode, word_a=None, word_b=None, mutant=None):
    """a (R, C) . b (S, C)^T in `mode`'s arithmetic, float64 sums"""
    pa, pb = operand_pieces(a, mode, word_a, mutant), operand_pieces(b, mode, word_b, mutant)
    with np.errstate(invalid="ignore", over="ignore"):
        return sum(pa[i] @ pb[j].T for i, j in PRODUCTS[mode])


def exact(a, b):
    return np.asarray(a, np.float64) @ np.asarray(b, np.float64).T


def yardstick(a, b):
    return (np.asarray(a, np.float32) @ np.asarray(b, np.float32).T).astype(np.float64)


def terms(a, b):
    """|a| . |b|^T: the sum of the magnitudes of the terms of every output (the cancellation floor)"""
    return np.abs(np.asarray(a, np.float64)) @ np.abs(np.asarray(b, np.float64)).T


# ---- operand layouts ----
def _groups(R):
    """the outlier's index and the two reduced blocks of a dimension of R entries; the first block straddles entry 128 when there is one (the
    edge of a 128-row tile), both lie past entry 32 and inside ragged tiles"""
    return 5 % R, np.arange(int(0.72 * R), int(0.85 * R)), np.arange(int(0.88 * R), int(0.97 * R))


def _rows(R, a, b):
    full = np.setdiff1d(np.arange(R), np.concatenate([a, b]))
    return {"full": full, "2^-12": a, "small": b}


def linear_case(layout, M, N, K, c=None, seed=0, small=-17):
    """operands of a Linear (x (M, K), W (N, K), bias (N,), residual (M, N), dY (M, N): float32 numpy) in one of the layouts; `judged`: tensor
    name -> row groups {"full": rows judged at full accuracy, "2^-12" / "small": the reduced blocks, judged at their own scale} of "y", "yT",
    "dx", "dw" (db goes with dw).  small: log2 of the second block's factor.  -17: the 30 x outlier's row is the judged tensor's maximum, so
    the block sits 2^-22 below it; at -18 single rows of a 48-wide output already fall under RANGE_FLOOR = 2^-24 of that maximum, at -20 all do.
    bias and residual carry the factors of the rows / columns of y they are added to (L1: the residual's rows; L4: the bias's entries and the
    residual's columns), so that an epilogue leaves a reduced block of y where it is."""
    rng = np.random.default_rng(1000 * seed + 7 * M + 3 * N + K)
    x = rng.standard_normal((M, K)); w = rng.standard_normal((N, K)) / np.sqrt(K); dy = rng.standard_normal((M, N))
    bias = rng.standard_normal(N) * 0.5; res = rng.standard_normal((M, N)) * 0.5
    rowf, colf = np.ones(M), np.ones(N)
    if layout in ("L1", "L2"):
        o, a, b = _groups(M)
        rowf[o], rowf[a], rowf[b] = OUTLIER, 2.0 ** -12, 2.0 ** small
    elif layout in ("L3", "L4"):
        o, a, b = _groups(N)
        colf[o], colf[a], colf[b] = OUTLIER, 2.0 ** -12, 2.0 ** small
    if layout == "L1":
        x *= rowf[:, None]; res *= rowf[:, None]; bias *= 0
        judged = {"y": _rows(M, a, b)}
    elif layout == "L2":
        dy *= rowf[:, None]
        judged = {"dx": _rows(M, a, b)}
    elif layout == "L3":
        dy *= colf[None]
        judged = {"dw": _rows(N, a, b)}
    elif layout == "L4":
        w *= colf[:, None]; bias *= colf; res *= colf[None]
        judged = {"yT": _rows(N, a, b)}
    elif layout == "L5":
        k0 = K // 3                                  # a "massive channel": one sign, little spread; dY with a mean, so that dW[:, k0] is no cancellation
        x[:, k0] = (1.0 + 0.25 * x[:, k0]) * 2.0 ** c; w[:, k0] *= 2.0 ** -c; dy += 0.5
        none = np.arange(0)
        judged = {"y": _rows(M, none, none), "dx": _rows(M, none, none), "dw": _rows(N, none, none)}
    else:
        raise ValueError(layout)
    f32 = lambda t: np.ascontiguousarray(t, dtype=np.float32)
    return dict(layout=layout, x=f32(x), w=f32(w), dy=f32(dy), bias=f32(bias), res=f32(res), judged=judged, outlier=None if layout == "L5" else o)


# the (layout, c) list of the GPU tests, and the Linear shapes every one of them is generated -- and checked on the host -- at:
# M = 160: one full 128-row tile and a ragged one; N = 48 / 208: ragged against 64- and 128-wide tiles (multiples of 16: the input-gradient GEMM
# contracts over N); K = 64 / 272: one slab group and several (272: the forward's split-contraction branch); (24, 48, 1024): small M, long K;
# (150, 128, 256), (150, 256, 256), (190, 64, 3072): what the small-M kernel accepts (N % 64 == 0, K % 256 == 0), 32- and 64-row tiles;
# (300, 208, 272): rows enough for the weight gradient to split them across workgroups; (160, 48, 272): the narrow fc2 of the MLP pair
LAYOUTS = (("L1", None), ("L2", None), ("L3", None), ("L4", None), ("L5", 10), ("L5", 15))
LINEAR_SHAPES = ((160, 48, 64), (160, 208, 272), (24, 48, 1024), (150, 128, 256), (150, 256, 256), (190, 64, 3072), (300, 208, 272), (160, 48, 272))
# 3x3 / 1x1 convolutions (B, Ci, Co, H, W, k): B = 3 (the outlier's image and the two reduced ones), 96 channels (the least the own kernels take)
CONV_SHAPES = ((3, 96, 96, 16, 64, 3), (3, 96, 96, 6, 45, 3), (3, 96, 96, 12, 20, 3), (3, 96, 96, 12, 24, 1))


LINEAR_PRODUCTS = {"y": ("x", "w"), "yT": ("w", "x"), "dx": ("dy", "wT"), "dw": ("dyT", "xT")}       # tensor -> (a, b) of a . b^T


def linear_operand(case, name):
    """the matrix of an operand name and the tensor whose |max| word it is split with (a transposed operand: the same elements)"""
    src = name[:-1] if name.endswith("T") else name
    return (case[src].T if name.endswith("T") else case[src]), src


def stale_word(case, src):
    """the |max| word of operand tensor `src` taken WITHOUT its outlier (the third mutant): the word of the bulk"""
    t = case[src].copy()
    o = case["outlier"]
    if (case["layout"], src) in (("L1", "x"), ("L2", "dy"), ("L4", "w")):
        t[o] = 0
    elif (case["layout"], src) == ("L3", "dy"):
        t[:, o] = 0
    return _word(t)


def linear_tensor(case, name, how, mode=None, mutant=None):
    """tensor `name` of a linear case: how = "exact" | "yardstick" | "terms" | "emulate" (no bias: the products alone)"""
    (a, sa), (b, sb) = (linear_operand(case, n) for n in LINEAR_PRODUCTS[name])
    if how == "emulate":
        wa = wb = None
        if mode == "f16x3":
            wa, wb = (stale_word(case, s) if mutant == "stale" else _word(case[s]) for s in (sa, sb))
        return emulate(a, b, mode, wa, wb, mutant if mutant != "stale" else None)
    return {"exact": exact, "yardstick": yardstick, "terms": terms}[how](a, b)


def group_errors(got, ref, trm, groups):
    """{group: (worst-row error, row)} of one judged tensor against float64, every group on the floors of the WHOLE tensor"""
    return {g: worst_row_rel_2d(got, ref, trm, rows=rows) for g, rows in groups.items() if len(rows)}


def whole_tensor_rel(got, ref):
    """the metric of tests/gpu_utils.assert_close_rel: max |a - e| / max |e| over the whole tensor"""
    with np.errstate(invalid="ignore", over="ignore"):
        return float(np.abs(np.asarray(got, np.float64) - ref).max() / np.abs(ref).max())


# ---- convolutions: the same products on im2col matrices ----
def im2col(x, k):
    """(B, C, H, W) -> (B H W, k k C), column = tap * C + c, zero padding k // 2: the matrix the implicit GEMM contracts with the rearranged
    weight (Co, k k Ci)"""
    B, C, H, W = x.shape
    p = k // 2
    xp = np.zeros((B, C, H + 2 * p, W + 2 * p), x.dtype); xp[:, :, p:p + H, p:p + W] = x
    cols = [xp[:, :, ky:ky + H, kx:kx + W].transpose(0, 2, 3, 1).reshape(B * H * W, C) for ky in range(k) for kx in range(k)]
    return np.concatenate(cols, 1)


def col2im(cols, B, C, H, W, k):
    """the adjoint of `im2col` (float64 sums): (B H W, k k C) -> (B, C, H, W)"""
    p = k // 2
    out = np.zeros((B, C, H + 2 * p, W + 2 * p))
    c4 = cols.reshape(B, H, W, k * k, C)
    for ky in range(k):
        for kx in range(k):
            out[:, :, ky:ky + H, kx:kx + W] += c4[:, :, :, ky * k + kx].transpose(0, 3, 1, 2)
    return out[:, :, p:p + H, p:p + W]


def weight_matrix(w):
    Co, Ci, k, _ = w.shape
    return np.ascontiguousarray(w.transpose(0, 2, 3, 1).reshape(Co, k * k * Ci))


def conv_case(layout, B, Ci, Co, H, W, k, c=None, seed=0, small=-17):
    """operands of a stride-1 'same' convolution (x (B, Ci, H, W), W (Co, Ci, k, k), bias, dY (B, Co, H, W)) in one of the layouts; B >= 3 for
    L1 / L2: image 0 carries the outlier plane, images 1 and 2 are the reduced blocks.  judged: "y" / "dx" as (B C, H W) planes, "yT" as
    (Co, B H W), "dw" as (Co, k k Ci)."""
    rng = np.random.default_rng(2000 * seed + 31 * B + 7 * Ci + 5 * Co + 3 * H + W + k)
    x = rng.standard_normal((B, Ci, H, W)); w = rng.standard_normal((Co, Ci, k, k)) / np.sqrt(k * k * Ci); dy = rng.standard_normal((B, Co, H, W))
    bias = rng.standard_normal(Co) * 0.5
    f = 2.0 ** small
    planes = lambda C: _rows(B * C, np.arange(C, 2 * C), np.arange(2 * C, 3 * C))
    if layout == "L1":
        x[0, 3] *= OUTLIER; x[1] *= 2.0 ** -12; x[2] *= f; bias *= 0
        judged = {"y": planes(Co)}
    elif layout == "L2":
        dy[0, 3] *= OUTLIER; dy[1] *= 2.0 ** -12; dy[2] *= f
        judged = {"dx": planes(Ci)}
    elif layout == "L3":
        o, a, b = _groups(Co); dy[:, o] *= OUTLIER; dy[:, a] *= 2.0 ** -12; dy[:, b] *= f
        judged = {"dw": _rows(Co, a, b)}
    elif layout == "L4":
        o, a, b = _groups(Co); w[o] *= OUTLIER; w[a] *= 2.0 ** -12; w[b] *= f
        bias[o] *= OUTLIER; bias[a] *= 2.0 ** -12; bias[b] *= f
        judged = {"yT": _rows(Co, a, b)}
    elif layout == "L5":
        c0 = Ci // 3
        x[:, c0] = (1.0 + 0.25 * x[:, c0]) * 2.0 ** c; w[:, c0] *= 2.0 ** -c; dy += 0.5
        none = np.arange(0)
        judged = {"y": _rows(B * Co, none, none), "dx": _rows(B * Ci, none, none), "dw": _rows(Co, none, none)}
    else:
        raise ValueError(layout)
    f32 = lambda t: np.ascontiguousarray(t, dtype=np.float32)
    return dict(layout=layout, x=f32(x), w=f32(w), dy=f32(dy), bias=f32(bias), judged=judged, k=k)


def conv_tensor(case, name, how, mode=None):
    """tensor `name` of a convolution case in the 2-D form it is judged in (no bias)"""
    x, w, dy, k = case["x"], case["w"], case["dy"], case["k"]
    B, Ci, H, W = x.shape
    Co = w.shape[0]
    cols, wm, dym = im2col(x, k), weight_matrix(w), dy.transpose(0, 2, 3, 1).reshape(B * H * W, Co)
    words = {n: _word(case[n]) for n in ("x", "w", "dy")} if mode == "f16x3" else {n: None for n in ("x", "w", "dy")}
    if how == "emulate":
        dot = lambda a, na, b, nb: emulate(a, b, mode, words[na], words[nb])
    else:
        fn = {"exact": exact, "yardstick": yardstick, "terms": terms}[how]
        dot = lambda a, na, b, nb: fn(a, b)
    if name in ("y", "yT"):
        y = dot(cols, "x", wm, "w")                                                  # (B H W, Co)
        return y.T if name == "yT" else y.reshape(B, H * W, Co).transpose(0, 2, 1).reshape(B * Co, H * W)
    if name == "dx":
        g = dot(dym, "dy", wm.T, "w")                                               # (B H W, k k Ci): every term of dX, summed by the fold
        return col2im(g, B, Ci, H, W, k).reshape(B * Ci, H * W)
    if name == "dw":
        return dot(dym.T, "dy", cols.T, "x")                                       # (Co, k k Ci)
    raise ValueError(name)
