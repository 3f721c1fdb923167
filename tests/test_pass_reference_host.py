"""CPU pins of tests/pass_reference.py, the yardsticks of tests/test_gpu_pass_paths.py: Philox-4x32-10 against the published known answers
and the kernels' keep convention, the x2 bilinear operator against the framework's fp32 CPU interpolation (forward and backward), and the
two patch orders against the index formulas of the kernels' comments."""
import numpy as np
import pytest
import torch

from tests import pass_reference as R

U = 2.0 ** -24            # one unit of the up-sampling bars: half an ulp of 1.0 in float32


def _words(hexes):
    return tuple(int(h, 16) for h in hexes.split())


@pytest.mark.parametrize("ctr,key,want", [
    ("00000000 00000000 00000000 00000000", "00000000 00000000", "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ("ffffffff ffffffff ffffffff ffffffff", "ffffffff ffffffff", "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ("243f6a88 85a308d3 13198a2e 03707344", "a4093822 299f31d0", "d16cfe09 94fdcceb 5001e420 24126ea1"),
])
def test_philox_known_answers(ctr, key, want):
    """the three vectors of the Random123 distribution's kat_vectors for philox4x32 with 10 rounds"""
    got = tuple(int(w) for w in R.philox4x32_10(_words(ctr), _words(key)))
    assert got == _words(want), [f"{w:08x}" for w in got]


def _philox_ints(ctr, key):
    """the round function of csrc/vit_common.h in Python integers (a second, scalar restatement)"""
    c, k = list(ctr), list(key)
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k[0], p1 & 0xFFFFFFFF, (p0 >> 32) ^ c[3] ^ k[1], p0 & 0xFFFFFFFF]
        k = [(k[0] + 0x9E3779B9) & 0xFFFFFFFF, (k[1] + 0xBB67AE85) & 0xFFFFFFFF]
    return c


def test_keep_follows_the_kernels_counter_key_and_lane_convention():
    seed, p = 0x1234_5678_9ABC_DEF1, 0.1
    idx = np.array([0, 1, 2, 3, 4, 7, 1023, 16_777_216 * 4 - 1, 16_777_216 * 4, (1 << 34) + 5, (1 << 40) + 2], dtype=np.uint64)
    got = R.keep(seed, idx, p)
    thresh = R.keep_threshold(p)
    assert thresh == int((1.0 - float(np.float32(0.1))) * 2.0 ** 32)
    for i, g in zip(idx.tolist(), got.tolist()):
        i4 = i // 4
        word = _philox_ints((i4 & 0xFFFFFFFF, i4 >> 32, 0, 0), (seed & 0xFFFFFFFF, seed >> 32))[i % 4]
        assert g == (word < thresh), i
    # vectorised over any shape, and a different seed gives different decisions
    many = np.arange(40_000, dtype=np.uint64)
    k1 = R.keep(seed, many.reshape(100, 400), p)
    assert k1.shape == (100, 400) and abs(k1.mean() - 0.9) < 4 * (0.09 / 40_000) ** 0.5
    assert (R.keep(seed + 1, many, p) != k1.reshape(-1)).any()
    assert float(R.keep_scale(p)) == float(np.float32(1.0 / (1.0 - float(np.float32(0.1)))))


def test_the_two_threshold_expressions_agree_for_every_p():
    ps = [0.0, 1e-45, 2.0 ** -60, 2.0 ** -40, 2.0 ** -33, 2.0 ** -32, 2.0 ** -31, 1e-6, 0.1, 0.25, 0.5, 0.9, float(np.nextafter(np.float32(1), np.float32(0)))]
    for p in ps:
        a, b = R.keep_threshold(p, "relu_dropout"), R.keep_threshold(p, "head_tail")
        assert a == b and 0 < a <= 0xFFFFFFFF, (p, a, b)
    assert R.keep_threshold(0.0) == 0xFFFFFFFF and R.keep_threshold(0.5) == 1 << 31


SHAPES = [(3, 5, 128), (2, 64, 64), (3, 1, 8), (2, 7, 6), (1, 2, 1024), (4, 128, 2)]


@pytest.mark.parametrize("shape", SHAPES)
def test_upsample_operator_against_the_frameworks_fp32_cpu_interpolation(shape):
    """forward within 8 x 2^-24 max|x|, backward within 24 x 2^-24 max|g| (the bars of the GPU test; the framework measures 0.4 - 1.2 and
    1.4 - 3.2 of these units here).  A floor decision that differed from the framework's would show as an error of the order of the
    neighbour difference times lambda, thousands of units."""
    P, H, W = shape
    g = torch.Generator().manual_seed(H * 1000 + W)
    x = torch.randn(1, P, H, W, generator=g, requires_grad=True)
    y = torch.nn.functional.interpolate(x, scale_factor=2, mode="bilinear", align_corners=True)
    gy = torch.randn(y.shape, generator=g)
    y.backward(gy)
    fwd = np.abs(y.detach().numpy()[0] - R.upsample_forward(x.detach().numpy()[0])).max() / (U * float(x.detach().abs().max()))
    bwd = np.abs(x.grad.numpy()[0] - R.upsample_backward(gy.numpy()[0])).max() / (U * float(gy.abs().max()))
    print(f"  {shape}: forward {fwd:.2f} units, backward {bwd:.2f} units")
    assert fwd <= 8 and bwd <= 24, (shape, fwd, bwd)


def test_upsample_matrix_rows_and_edges():
    for n in (1, 2, 3, 8, 64, 128, 1024):
        a = R.upsample_matrix(n)
        assert a.shape == (2 * n, n) and (a >= 0).all() and np.abs(a.sum(1) - 1).max() <= 2 * U
        assert ((a != 0).sum(1) <= 2).all() and a[0, 0] == 1.0 and (n == 1 or a[-1, -1] > 1 - 1e-4)
        nz = [np.nonzero(a[:, i])[0] for i in range(n)]              # the gather of the backward kernels: candidates 2i - 2 .. 2i + 3
        assert all(v.min() >= 2 * i - 2 and v.max() <= 2 * i + 3 for i, v in enumerate(nz))


def test_upsample_backward_skips_zero_weight_taps_of_an_infinite_gradient():
    g = np.random.default_rng(0).standard_normal((2, 8, 12))
    g[0, 0, 0] = g[1, 7, 11] = g[0, 3, 5] = np.inf
    d = R.upsample_backward(g)
    assert not np.isnan(d).any()
    ah, aw = R.upsample_matrix(4), R.upsample_matrix(6)
    want = np.zeros((2, 4, 6), bool)
    for pl, oy, ox in ((0, 0, 0), (1, 7, 11), (0, 3, 5)):
        want[pl] |= np.outer(ah[oy] != 0, aw[ox] != 0)
    assert (np.isposinf(d) == want).all() and want[0, 0, 0] and want[0].sum() == 1 + 4 and want[1].sum() == 1
    g0 = np.where(np.isinf(g), 0.0, g)
    assert np.array_equal(d[~want], R.upsample_backward(g0)[~want])


def test_patch_orders_against_the_index_formulas():
    g = torch.Generator().manual_seed(1)
    img = torch.randn(2, 3, 3, 4, generator=g)
    cols = R.im2col7_reference(img)
    assert cols.shape == (2, 160, 3, 4) and float(cols[:, 147:].abs().max()) == 0.0
    pad = torch.nn.functional.pad(img, (3, 3, 3, 3))
    for ci in range(3):
        for ky in range(7):
            for kx in range(7):
                assert torch.equal(cols[:, ci * 49 + ky * 7 + kx], pad[:, ci, ky:ky + 3, kx:kx + 4])
    x = torch.randn(2, 5, 3, 4, generator=g)
    for relu in (False, True):
        rows = R.im2col3_rows_reference(x, relu)
        assert rows.shape == (2 * 3 * 4, 45)
        src = torch.nn.functional.pad(torch.relu(x) if relu else x, (1, 1, 1, 1))
        for dy in range(3):
            for dx in range(3):
                want = src[:, :, dy:dy + 3, dx:dx + 4].permute(0, 2, 3, 1).reshape(24, 5)      # [(b, y, x)][ci]
                assert torch.equal(rows[:, (3 * dy + dx) * 5:(3 * dy + dx + 1) * 5], want)
