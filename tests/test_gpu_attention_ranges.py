"""-m gpu: the attention kernels at the edges of their arithmetic -- peaked softmax, subnormal dS tiles, gradients from 1e-8 to 1e4 x,
magnitudes that share one |max| word, ties, long contractions, shape edges, tail rows, non-default scales -- in every arithmetic
(f32, bf16x6, bf16x3, f16x3), forward and backward, against the float64 oracle (oracle/vit_oracle.py) fed the exact fp32 bytes.

Errors are PER ROW (tests/gpu_utils.worst_row_rel: a row is one (b, h, query) of out / dq, one (b, h, key) of dk / dv, judged at its own
max-norm), so a few wrong rows or a head far below the tensor's maximum cannot hide behind the tensor's scale.  Beside the kernel, the same
formulas run in float32 numpy: the yardstick of what fp32 itself achieves on the input.  The rule the Linear tests use:
  f32, bf16x6   worst-row error <= YARD_MULT x the float32 yardstick's + YARD_FLOOR
  bf16x3        the same against BF3_MULT (its operands are good to 2^-16, not 2^-24) + BF3_FLOOR
  f16x3         <= F16_MULT x the larger of bf16x6's and the yardstick's worst-row error on the same input + F16_FLOOR (measured worst
                ratio 2.5: dk of the c = 5 peaked softmax, where the 2^-22 pieces show beside bf16x6's 2^-24-class products)
  streaming sums over 8 192 keys (the tail-row test): LONG_YARD_MULT in place of YARD_MULT -- the kernels add the terms in order, the
                yardstick's BLAS in blocks (measured 15.5 x on the tail row's dq in f32 and bf16x6 alike)
  rows whose operands share a power-of-two scale with tensors 2^12 .. 2^20 larger (f16x3): OWN_SCALE_BAR at their own scale, the bar the
                Linear range test grants.
Two floors keep the row metric meaningful where no arithmetic can do better than its own rounding: a row that is a near-complete
cancellation (|ref| below CANCEL_FLOOR x the sum of the magnitudes of its terms -- dq / dk of a one-hot softmax row, of a single key, of
identical keys, where dS = p (dP - Delta) cancels exactly) is judged against that fraction of its term sum; a row below RANGE_FLOOR x the
judged tensor's maximum (a key no query attends to: dv ~ 1e-30) is judged against that fraction of the maximum.
PARITY_VERBOSE=1 prints every measured value beside its bar."""
import os

import numpy as np
import pytest
import torch

from oracle import vit_oracle as vo
from tests.gpu_utils import worst_row_rel

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MODES = ("f32", "bf16x6", "bf16x3", "f16x3")
CODE = {"f32": 0, "bf16x6": 1, "bf16x3": 2, "f16x3": 3}
NAMES = ("out", "dq", "dk", "dv")
VERBOSE = bool(os.environ.get("PARITY_VERBOSE"))

YARD_MULT, YARD_FLOOR = 8.0, 2e-6
LONG_YARD_MULT = 32.0
BF3_MULT, BF3_FLOOR = 512.0, 1e-4
F16_MULT, F16_FLOOR = 3.0, 2e-6
OWN_SCALE_BAR = 2e-4
CANCEL_FLOOR = 2.0 ** -8
RANGE_FLOOR = 2.0 ** -24
TINY = 2.0 ** -126          # smallest normal fp32


@pytest.fixture(params=MODES)
def arith(request, monkeypatch):
    """the attention arithmetic under test (vit_ops.ATTENTION_ARITH), and the check that the last launch really took that kernel"""
    from styl3r_amd import vit_ops
    monkeypatch.setattr(vit_ops, "ATTENTION_ARITH", request.param)
    yield request.param
    assert vit_ops.load().vit_attention_arith() == CODE[request.param]


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _gpu(monkeypatch, mode, q, k, v, g, scale, pos=None, max_pos=63):
    """memory_efficient_attention forward + backward in `mode` on the fp32 arrays: [out, dq, dk, dv] as float64"""
    from styl3r_amd import vit_ops
    monkeypatch.setattr(vit_ops, "ATTENTION_ARITH", mode)
    qt, kt, vt = (torch.tensor(_f32(a), device=DEV, requires_grad=True) for a in (q, k, v))
    kw = {}
    if pos is not None:
        kw = dict(qpos=torch.tensor(pos[0], device=DEV), kpos=torch.tensor(pos[1], device=DEV), max_pos=max_pos)
    o = vit_ops.memory_efficient_attention(qt, kt, vt, scale=scale, **kw)
    o.backward(torch.tensor(_f32(g), device=DEV))
    return [t.detach().double().cpu().numpy() for t in (o, qt.grad, kt.grad, vt.grad)]


def _ref(q, k, v, g, scale, pos=None, dtype=np.float64, rows=None):
    """the oracle on the same fp32 values (RoPE through vo.rope2d, gradients rotated back); rows: only these queries (out, dq).
    Returns ([out, dq, dk, dv], dS, per-row sums of the magnitudes of each output's terms (float64, shape (B, N, H)))."""
    qr, kr = vo.rope2d(q, pos[0], dtype=dtype) if pos is not None else q, vo.rope2d(k, pos[1], dtype=dtype) if pos is not None else k
    if rows is not None:
        qr, g = qr[:, rows], g[:, rows]
    dq, dk, dv, o, ds = vo.attention_backward(qr, kr, v, scale, g, dtype=dtype, return_ds=True)
    if pos is not None:
        dq = vo.rope2d(dq, pos[0] if rows is None else pos[0][:, rows], fwd=-1.0, dtype=dtype)
        dk = vo.rope2d(dk, pos[1], fwd=-1.0, dtype=dtype)
    terms = None
    if dtype == np.float64:      # out = P V, dq = dS K, dk = dS^T Q, dv = P^T dO, dS = scale P (dO.V - dO.O): the magnitudes of all their terms
        _, p = vo.attention(qr, kr, v, scale)
        a = lambda t: np.abs(np.asarray(t, np.float64)).transpose(0, 2, 1, 3)       # (b,h,n,d)
        back = lambda t: t.max(-1).transpose(0, 2, 1)                                 # (b,h,n,d) -> per row (b,n,h)
        dpa = a(g) @ a(v).swapaxes(-1, -2)
        deltaa = (a(g) * a(o)).sum(-1)[..., None]
        w = abs(scale) * p * (dpa + deltaa)
        terms = [back(p @ a(v)), back(w @ a(kr)), back(w.swapaxes(-1, -2) @ a(qr)), back(p.swapaxes(-1, -2) @ a(g))]
    return [np.asarray(t, np.float64) for t in (o, dq, dk, dv)], ds, terms


def _bar(mode, e_yard, e6, long=False):
    if mode in ("f32", "bf16x6"):
        return (LONG_YARD_MULT if long else YARD_MULT) * e_yard + YARD_FLOOR
    if mode == "bf16x3":
        return BF3_MULT * e_yard + BF3_FLOOR
    return F16_MULT * max(e6, e_yard) + F16_FLOOR


def _judge(what, mode, got, ref, yard, terms, base6=None, names=NAMES, own_scale=(), long=False):
    """every tensor of `names`: worst-row error of the kernel against float64, beside the float32 yardstick's (and bf16x6's for f16x3);
    `own_scale`: tensors judged against OWN_SCALE_BAR in f16x3 (operands that share a scale with much larger values)"""
    fails = []
    for i, n in enumerate(NAMES):
        if n not in names:
            continue
        fl = np.maximum(np.maximum(CANCEL_FLOOR * terms[i], RANGE_FLOOR * np.abs(ref[i]).max()), 1e-300)
        e, at = worst_row_rel(got[i], ref[i], fl)
        ey = worst_row_rel(yard[i], ref[i], fl)[0]
        e6 = worst_row_rel(base6[i], ref[i], fl)[0] if base6 is not None else None
        bar = OWN_SCALE_BAR if (mode == "f16x3" and n in own_scale) else _bar(mode, ey, e6, long)
        if VERBOSE:
            extra = f", bf16x6 {e6:.2e}" if e6 is not None else ""
            print(f"    [rows] {what} {mode} {n}: {e:.2e} at (b,h,n)={at} (f32 yardstick {ey:.2e}{extra}; bar {bar:.2e})")
        if not e <= bar:
            fails.append(f"{n}: worst row {at} err {e:.3e} > bar {bar:.3e} (yardstick {ey:.3e}, bf16x6 {e6})")
    assert not fails, f"{what} [{mode}]: " + "; ".join(fails)


def _case(monkeypatch, mode, what, q, k, v, g, scale, pos=None, max_pos=63, names=NAMES, rows=None, own_scale=(), pre=None, long=False):
    """the common body: bf16x6 first when f16x3 is judged against it (the mode under test runs LAST: the fixture checks its launch)"""
    ref, ds, terms = _ref(q, k, v, g, scale, pos, np.float64, rows)
    if pre is not None:
        pre(ds)
    yard = _ref(q, k, v, g, scale, pos, np.float32, rows)[0]
    base6 = None
    if mode == "f16x3":
        base6 = _gpu(monkeypatch, "bf16x6", q, k, v, g, scale, pos, max_pos)
    got = _gpu(monkeypatch, mode, q, k, v, g, scale, pos, max_pos)
    if rows is not None:       # (out, dq of those queries; dk, dv are not judged)
        got = [t[:, rows] if i < 2 else t for i, t in enumerate(got)]
        base6 = [t[:, rows] if i < 2 else t for i, t in enumerate(base6)] if base6 is not None else None
    _judge(what, mode, got, ref, yard, terms, base6, names, own_scale, long)
    return got


def _pos(rng, B, N, max_pos=63):
    return rng.integers(0, max_pos + 1, (B, N, 2)).astype(np.int64)


# ---- a. peaked softmax: logit spreads from O(1) to a few hundred nats, crossed with dO from 1 to 1e-7 ----
@pytest.mark.parametrize("c", [1.0, 3.0, 5.0])
@pytest.mark.parametrize("gs", [1.0, 1e-4, 1e-7])
def test_peaked_softmax(c, gs, arith, monkeypatch):
    rng = np.random.default_rng(int(c * 100) + int(-np.log10(gs)))
    B, H, Nq, Nk = 2, 3, 160, 320
    q = _f32(rng.standard_normal((B, Nq, H, 64)) * c)
    k = _f32(rng.standard_normal((B, Nk, H, 64)) * c)
    v = _f32(rng.standard_normal((B, Nk, H, 64)))
    g = _f32(rng.standard_normal((B, Nq, H, 64)) * gs)
    for i in range(32):     # queries 0..31 find their row maximum in the LAST key tile (4.8 c^2 nats above the typical logit): the forward's
        k[:, Nk - 1 - i] = 0.6 * q[:, i]      # online softmax rescales from tiles that all underflowed
    _case(monkeypatch, arith, f"peaked c={c} dO={gs:g}", q, k, v, g, 0.125)


# ---- b. a whole 32-row tile whose dS column max is an fp32 subnormal, the lane's other tiles normal (dO ~ 1e-6) ----
def _subnormal_inputs(which, rng):
    """which = "dq": targeted QUERIES (even ones) see keys 32..63 at -80 nats (the dQ pass walks keys in 32-key tiles);
    "dk": targeted KEYS (even ones) see queries 32..63 at -80 nats (the dK / dV pass walks queries in 32-query tiles).
    Targeted rows carry feature 0 only (= 8: their logits are exactly the other side's feature 0); the others are random."""
    B, H, N_lane, N_walk = 1, 2, 64, 96
    lane = np.zeros((B, N_lane, H, 64)); walk = rng.standard_normal((B, N_walk, H, 64))
    lane[:, 1::2] = rng.standard_normal((B, N_lane // 2, H, 64))          # untargeted rows: random
    lane[:, 0::2, :, 0] = 8.0                                              # targeted rows: feature 0 only, scale * 8 = 1
    walk[:, :, :, 0] = rng.uniform(-0.5, 0.5, (B, N_walk, H))
    walk[:, 32:64, :, 0] = -80.0 + rng.uniform(-1.0, 1.0, (B, 32, H))     # the subnormal tile: logits ~ -80 nats, p ~ e^-84
    if which == "dk":
        # a query of the subnormal tile also sees the untargeted keys at O(1) logits (its log-sum-exp stays normal): those keys carry no feature 0
        lane[:, 1::2, :, 0] = 0.0
    v = rng.standard_normal((B, N_lane if which == "dk" else N_walk, H, 64))
    if which == "dq":
        q, k = lane, walk
        g = rng.standard_normal((B, N_lane, H, 64)) * 1e-6
    else:
        q, k = walk, lane
        g = rng.standard_normal((B, N_walk, H, 64)) * 1e-6
    return _f32(q), _f32(k), _f32(v), _f32(g)


@pytest.mark.parametrize("which", ["dq", "dk"])
def test_subnormal_ds_tile(which, arith, monkeypatch):
    rng = np.random.default_rng(7 if which == "dq" else 8)
    q, k, v, g = _subnormal_inputs(which, rng)

    def precondition(ds):     # ds: (B, H, Nq, Nk) in float64
        t = ds if which == "dq" else ds.transpose(0, 1, 3, 2)              # (.., lane, walk)
        lanes = np.abs(t[:, :, 0::2])                                      # the targeted rows
        tile = lanes[..., 32:64].max(-1)
        rest = np.maximum(lanes[..., :32].max(-1), lanes[..., 64:].max(-1))
        assert (tile > 0).all() and (tile < TINY).all(), (tile.min(), tile.max())    # the targeted tile: max |dS| in (0, 2^-126)
        assert (rest >= TINY).all(), rest.min()                                      # the lane's other tiles: normal
    _case(monkeypatch, arith, f"subnormal dS tile ({which} pass)", q, k, v, g, 0.125, pre=precondition)


# ---- c. gradient magnitudes ----
@pytest.mark.parametrize("kind", ["1", "1e-4", "1e-8", "outlier_row", "zero"])
def test_gradient_magnitudes(kind, arith, monkeypatch):
    rng = np.random.default_rng(31)
    B, H, Nq, Nk = 2, 2, 130, 200
    q = _f32(rng.standard_normal((B, Nq, H, 64)) * 1.5); k = _f32(rng.standard_normal((B, Nk, H, 64)) * 1.5)
    v = _f32(rng.standard_normal((B, Nk, H, 64)))
    g = rng.standard_normal((B, Nq, H, 64))
    if kind == "outlier_row":
        g[:, 17] *= 1e4
    elif kind == "zero":
        g[:] = 0.0
    else:
        g *= float(kind)
    g = _f32(g)
    if kind != "zero":
        _case(monkeypatch, arith, f"dO {kind}", q, k, v, g, 0.125)
        return
    # all-zero dO: the forward as usual, every gradient exactly 0, no NaN
    _case(monkeypatch, arith, "dO = 0 (forward)", q, k, v, g, 0.125, names=("out",))
    got = _gpu(monkeypatch, arith, q, k, v, g, 0.125)
    for n, t in zip(NAMES[1:], got[1:]):
        assert np.isfinite(t).all() and not np.any(t), (n, np.abs(t).max())


# ---- d. magnitudes that share one power-of-two scale ----
@pytest.mark.parametrize("where", ["head", "batch"])
def test_one_head_or_batch_entry_far_below_the_others(where, arith, monkeypatch):
    """q, k, v, dO of head 1 (of batch entry 1) at 2^-20 of the rest: f16x3 takes ONE |max| word per tensor across heads and batches"""
    rng = np.random.default_rng(41)
    B, H, Nq, Nk = 2, 3, 160, 192
    q = rng.standard_normal((B, Nq, H, 64)) * 2; k = rng.standard_normal((B, Nk, H, 64)) * 2
    v = rng.standard_normal((B, Nk, H, 64)); g = rng.standard_normal((B, Nq, H, 64)) * 1e-3
    sel = (slice(None), slice(None), 1) if where == "head" else (1,)
    for t in (q, k, v, g):
        t[sel] *= 2.0 ** -20
    q, k, v, g = (_f32(t) for t in (q, k, v, g))
    ref, _, terms = _ref(q, k, v, g, 0.125)
    yard = _ref(q, k, v, g, 0.125, dtype=np.float32)[0]
    base6 = _gpu(monkeypatch, "bf16x6", q, k, v, g, 0.125) if arith == "f16x3" else None
    got = _gpu(monkeypatch, arith, q, k, v, g, 0.125)
    keep = (lambda t: np.delete(t, 1, axis=2)) if where == "head" else (lambda t: t[:1])
    small = (lambda t: t[:, :, 1:2]) if where == "head" else (lambda t: t[1:])
    for part, f, own in (("the others", keep, ()), (f"the {where} at 2^-20", small, NAMES)):
        _judge(f"{where} at 2^-20: {part}", arith, [f(t) for t in got], [f(t) for t in ref], [f(t) for t in yard],
               [f(t[..., None])[..., 0] for t in terms], [f(t) for t in base6] if base6 is not None else None, own_scale=own)


def test_packed_qkv_with_v_far_below_q_and_k(arith, monkeypatch):
    """attention_qkv: the backward reads ONE |max| word for the packed Q, K, V; V at 2^-12 of Q and K, RoPE on"""
    from styl3r_amd import vit_ops
    rng = np.random.default_rng(43)
    B, N, H = 2, 200, 2
    qkv = rng.standard_normal((B, N, 3, H, 64)) * 1.5
    qkv[:, :, 2] *= 2.0 ** -12
    qkv = _f32(qkv)
    g = _f32(rng.standard_normal((B, N, H, 64)) * 1e-3)
    pos = _pos(rng, B, N)
    q, k, v = (np.ascontiguousarray(qkv[:, :, i]) for i in range(3))
    ref, _, terms = _ref(q, k, v, g, 0.125, (pos, pos))
    yard = _ref(q, k, v, g, 0.125, (pos, pos), np.float32)[0]

    def run(mode):
        monkeypatch.setattr(vit_ops, "ATTENTION_ARITH", mode)
        t = torch.tensor(qkv, device=DEV, requires_grad=True)
        o = vit_ops.attention_qkv(t, 0.125, torch.tensor(pos, device=DEV), max_pos=63)
        o.backward(torch.tensor(g, device=DEV))
        d = t.grad.double().cpu().numpy()
        return [o.detach().double().cpu().numpy(), d[:, :, 0], d[:, :, 1], d[:, :, 2]]
    base6 = run("bf16x6") if arith == "f16x3" else None
    _judge("packed qkv, V at 2^-12", arith, run(arith), ref, yard, terms, base6, own_scale=NAMES)


# ---- e. ties and long contractions ----
@pytest.mark.parametrize("kind", ["uniform_4096", "two_tied_maxima"])
def test_ties_and_long_contractions(kind, arith, monkeypatch):
    rng = np.random.default_rng(53)
    if kind == "uniform_4096":
        B, H, Nq, Nk = 1, 2, 64, 4096
        q = rng.standard_normal((B, Nq, H, 64)) * 2
        k = np.broadcast_to(rng.standard_normal((B, 1, H, 64)) * 2, (B, Nk, H, 64))      # every key the same: p = 1 / 4096 exactly
    else:
        B, H, Nq, Nk = 1, 2, 96, 200
        q = rng.standard_normal((B, Nq, H, 64)) * 2
        k = rng.standard_normal((B, Nk, H, 64)) * 2
        for i in range(16):                   # query i: two exactly equal maxima, key i (first tile) and key Nk - 1 - i (last tile)
            k[:, i] = k[:, Nk - 1 - i] = 0.6 * q[:, i]
    v = rng.standard_normal((B, Nk, H, 64)); g = rng.standard_normal((B, Nq, H, 64)) * 1e-2
    q, k, v, g = (_f32(t) for t in (q, k, v, g))
    _case(monkeypatch, arith, kind, q, k, v, g, 0.125)      # (uniform: dq = K sum_j dS = 0 exactly, judged by CANCEL_FLOOR)


# ---- f. shape edges with these distributions ----
@pytest.mark.parametrize("Nk", [1, 31, 32, 33, 63, 64, 65])
@pytest.mark.parametrize("rope", [False, True])
def test_shape_edges(Nk, rope, arith, monkeypatch):
    rng = np.random.default_rng(61 + Nk)
    B, H, Nq = 2, 2, 45
    q = _f32(rng.standard_normal((B, Nq, H, 64)) * 3); k = _f32(rng.standard_normal((B, Nk, H, 64)) * 3)
    v = _f32(rng.standard_normal((B, Nk, H, 64))); g = _f32(rng.standard_normal((B, Nq, H, 64)) * 1e-4)
    pos = (_pos(rng, B, Nq), _pos(rng, B, Nk)) if rope else None
    _case(monkeypatch, arith, f"Nq 45 Nk {Nk} rope {rope}", q, k, v, g, 0.125, pos)      # (Nk = 1: P = 1, dS = 0 exactly)


def test_tail_rows_at_257_tokens(arith, monkeypatch):
    """11 x 16 heads of 257 tokens: the 257th query / key runs on the vector kernels of vit_attention_tail.hip"""
    B, H, N = 11, 16, 257
    rng = np.random.default_rng(71)
    q = _f32(rng.standard_normal((B, N, H, 64)) * 3); k = _f32(rng.standard_normal((B, N, H, 64)) * 3)
    v = _f32(rng.standard_normal((B, N, H, 64))); g = _f32(rng.standard_normal((B, N, H, 64)) * 1e-4)
    pos = _pos(rng, B, N)
    _case(monkeypatch, arith, "257 tokens, 176 heads", q, k, v, g, 0.125, (pos, pos))


@pytest.mark.parametrize("Nk", [8192, 8193])
def test_tail_row_at_the_score_buffer_limit(Nk, arith, monkeypatch):
    """Nq = 8193 at 8 heads: the last query runs on the tail kernel while Nk <= tail::MAXN = 8192 (its LDS score buffer full), on the tiled
    kernels at 8193; out and dq of the rows under test (the tail row, the last tiled row, two others) -- the oracle evaluates those rows only"""
    rng = np.random.default_rng(Nk)
    B, H, Nq = 2, 4, 8193
    q = _f32(rng.standard_normal((B, Nq, H, 64)) * 2); k = _f32(rng.standard_normal((B, Nk, H, 64)) * 2)
    v = _f32(rng.standard_normal((B, Nk, H, 64))); g = _f32(rng.standard_normal((B, Nq, H, 64)) * 1e-4)
    rows = [0, 4000, 8191, 8192]
    _case(monkeypatch, arith, f"Nq 8193 Nk {Nk}", q, k, v, g, 0.125, names=("out", "dq"), rows=rows, long=True)


# ---- g. non-default scale ----
@pytest.mark.parametrize("scale", [0.01, 1.0])
def test_non_default_scale_with_rope(scale, arith, monkeypatch):
    """scale 1.0: Q (forward, dQ pass) and K (dK pass) are split after their multiplication by scale * log2 e; a q pair and a k pair
    (u, w) = (m, m) 2^2 with m = 1.995 (the tensors' |max|) at the position whose rotation angle is closest to 45 degrees grow to
    m sqrt 2 2^2: with a power of two chosen for |max| alone that is 2^15.9 x 1.44 in fp16, past 65 504"""
    from styl3r_amd import vit_ops
    rng = np.random.default_rng(83)
    B, H, N, max_pos = 1, 2, 96, 63
    cos, sin = (t.cpu().numpy() for t in vit_ops.rope_tables(64, max_pos + 1, 100.0, torch.device(DEV)))
    p45, d45 = np.unravel_index(int(np.argmax(cos + sin)), cos.shape)     # cos + sin = sqrt 2 cos(theta - 45 deg)
    assert cos[p45, d45] + sin[p45, d45] > 1.41
    q = rng.standard_normal((B, N, H, 64)); k = rng.standard_normal((B, N, H, 64))
    v = rng.standard_normal((B, N, H, 64)); g = rng.standard_normal((B, N, H, 64)) * 1e-3
    qpos, kpos = _pos(rng, B, N, max_pos), _pos(rng, B, N, max_pos)
    for t, pos, i in ((q, qpos, 5), (k, kpos, 7)):
        t[:, i, :, d45] = t[:, i, :, d45 + 16] = 1.995 * 4.0                # feature pair (d, d + 16) rotates by the y position
        pos[:, i, 0] = p45
    q, k, v, g = (_f32(t) for t in (q, k, v, g))
    assert np.abs(q).max() == np.abs(k).max() == np.float32(1.995 * 4.0)
    _case(monkeypatch, arith, f"scale {scale}", q, k, v, g, scale, (qpos, kpos), max_pos)
