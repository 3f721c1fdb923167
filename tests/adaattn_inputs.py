"""Inputs of the AdaAttN tests (tests/golden/make_adaattn_fixtures.py, test_adaattn_host.py, test_gpu_adaattn.py): the VGG weights, the
images and the synthetic regimes of the two kernels, shared by the generator and the tests so that nothing large is stored.

Every number comes from `numpy.random.default_rng(seed).random()` doubles (bit-stable across numpy versions and platforms) through a few
float64 operations, rounded to fp32 at the end.  The VGG weights are variance-scaled for ReLU (uniform with variance 2 / fan_in), so the
features keep their magnitude through the 16 convolutions."""
import functools

import numpy as np
import torch

# (Sequential index, c_in, c_out, kernel) of the 17 convolutions of the normalised VGG19 (stylizer/vgg.py make_vgg)
VGG_CONVS = ((0, 3, 3, 1), (2, 3, 64, 3), (5, 64, 64, 3), (9, 64, 128, 3), (12, 128, 128, 3), (16, 128, 256, 3), (19, 256, 256, 3),
             (22, 256, 256, 3), (25, 256, 256, 3), (29, 256, 512, 3), (32, 512, 512, 3), (35, 512, 512, 3), (38, 512, 512, 3),
             (42, 512, 512, 3), )
SLICE_ENDS = (4, 11, 18, 31, 44)
CONFIGS = {"yaml": dict(lam=0.3, content_loss_layers=(3,), style_loss_layers=(2, 3), style_loss_stats=("mean", "std")),
           "all": dict(lam=0.3, content_loss_layers=(1, 2, 3), style_loss_layers=(1, 2, 3), style_loss_stats=("mean", "std", "gram"))}
FIXTURE_SHAPE = dict(b=2, v=2, H=32, W=32, hs=32, ws=48)      # the smallest the reference's five slices accept
TAIL_SEED = 7
IMAGE_SEED = 7847        # of 8000 seeds the one whose prediction keeps the largest activation_margin (9.4e-6) through relu3_1
TIE_MARGIN = 1e-4


def _u(rng, shape, lo=0.0, hi=1.0):
    return rng.random(shape) * (hi - lo) + lo


def _f32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64).astype(np.float32))


@functools.lru_cache(maxsize=None)
def vgg_state_dict(seed: int = 11, depth: int = 5) -> dict:
    """the bare nn.Sequential's state dict (`0.weight`, `0.bias`, `2.weight`, ...) in fp32; depth < 5 stops after slice `depth`.  Each
    convolution draws from its own generator, so a shallower dict is a prefix of the full one."""
    sd = {}
    for idx, ci, co, k in VGG_CONVS:
        if idx >= SLICE_ENDS[depth - 1]:
            break
        rng = np.random.default_rng(seed * 1000 + idx)
        if k == 1:                                             # the input map: near the identity, as the real one is a colour remap
            w = np.eye(3).reshape(3, 3, 1, 1) + _u(rng, (co, ci, 1, 1), -0.1, 0.1)
        else:
            a = np.sqrt(6.0 / (ci * k * k))                    # uniform(-a, a): variance 2 / fan_in
            w = _u(rng, (co, ci, k, k), -a, a)
        sd[f"{idx}.weight"] = _f32(w)
        sd[f"{idx}.bias"] = _f32(_u(rng, (co,), -0.05, 0.05))
    return sd


def slice_key(key: str) -> str:
    """`5.weight` -> `slice2.5.weight` (the names of NormalizedVGG's state dict)"""
    idx = int(key.split(".")[0])
    return f"slice{1 + sum(idx >= e for e in SLICE_ENDS)}.{key}"


def images(seed: int = IMAGE_SEED, b: int = 2, v: int = 2, H: int = 32, W: int = 32, hs: int = 32, ws: int = 48):
    """target (b, v, 3, H, W), prediction (the target plus a smooth error and noise, inside [0, 1]), style (b, 3, hs, ws); fp32"""
    rng = np.random.default_rng(seed)
    coarse = _u(rng, (b, v, 3, H // 4, W // 4))
    target = np.clip(np.kron(coarse, np.ones((4, 4))) * 0.7 + 0.3 * _u(rng, (b, v, 3, H, W)), 0, 1)
    pred = np.clip(target + _u(rng, (b, v, 3, H, W), -0.15, 0.15) + np.kron(_u(rng, (b, v, 3, H // 8, W // 8), -0.1, 0.1), np.ones((8, 8))), 0, 1)
    style = np.clip(np.kron(_u(rng, (b, 3, hs // 2, ws // 2)), np.ones((2, 2))) * 0.6 + 0.4 * _u(rng, (b, 3, hs, ws)), 0, 1)
    return _f32(target), _f32(pred), _f32(style)


def activation_margin(net, x) -> float:
    """how far the VGG pass of `x` (float64) stays from a decision an fp32 pass could take the other way: the smallest |pre-activation| in
    front of a ReLU, and the smallest gap between the two largest candidates of a pooling window whose maximum is active.  One unit on the
    other side of its ReLU, or one window handing its gradient to another pixel, moves the image gradient by ~1e-3 of its norm (one of
    ~1e6 units), far above any rounding bar: inputs of a gradient comparison keep this margin above the fp32 error of a pre-activation."""
    import torch.nn.functional as F
    margin = float("inf")
    for k in range(1, net.depth + 1):
        convs = list(getattr(net, f"slice{k}"))
        for i, m in enumerate(convs):
            if k > 1 and i == len(convs) - 1:
                w = F.unfold(x, 2, stride=2).reshape(x.shape[0], x.shape[1], 4, -1).sort(dim=2, descending=True).values
                gap = (w[:, :, 0] - w[:, :, 1])[w[:, :, 0] > 0]
                margin = min(margin, float(gap.min())) if gap.numel() else margin
                x = F.max_pool2d(x, 2, 2)
            if m.kernel_size == (1, 1):
                x = m(x)
                continue
            pre = F.conv2d(F.pad(x, (1, 1, 1, 1), mode="reflect"), m.weight, m.bias)
            margin = min(margin, float(pre.abs().min()))
            x = torch.relu(pre)
    return margin


def _instance_norm64(x):
    mu = x.mean(-1, keepdims=True)
    return (x - mu) / np.sqrt(x.var(-1, keepdims=True) + 1e-5)


# name -> (D, Nq, M, C, q scale, matched)
STATS_REGIMES = {"diffuse": (64, 70, 150, 64, 0.1, False), "layer2": (192, 70, 150, 128, 1.0, False),
                 "configured": (448, 200, 150, 256, 1.0, False), "long": (448, 257, 1000, 256, 1.0, False),
                 "matched": (448, 200, 150, 256, 1.0, True), "one_key": (64, 70, 1, 64, 1.0, False),
                 "one_query": (64, 1, 150, 64, 1.0, False), "flat_channels": (64, 70, 150, 64, 1.0, False)}
STATS_INDEX = (0, 0, 1)
CONST_CHANNEL, ZERO_CHANNEL = 3, 5                                   # of the "flat_channels" regime


def stats_inputs(name: str, seed: int = 5):
    """q_hat (3, D, Nq), k_hat (2, D, M) instance-normalised (in float64, then rounded), s (2, C, M) ReLU-shaped with exact zeros,
    style_index (3,) int32; fp32 CPU tensors"""
    D, Nq, M, C, qscale, matched = STATS_REGIMES[name]
    rng = np.random.default_rng(seed * 100 + sorted(STATS_REGIMES).index(name))
    relu_like = lambda shape: np.maximum(_u(rng, shape) - 0.4, 0.0) * 3.0
    k_hat = _instance_norm64(relu_like((2, D, M)))
    if matched:                                                           # every query is one of its style's keys, slightly disturbed
        cols = (np.arange(Nq) * 7) % M
        q_hat = np.stack([k_hat[i][:, cols] for i in STATS_INDEX]) + _u(rng, (3, D, Nq), -0.05, 0.05)
    else:
        q_hat = _instance_norm64(relu_like((3, D, Nq))) * qscale
    s = relu_like((2, C, M))
    if name == "flat_channels":
        s[:, CONST_CHANNEL] = 0.7
        s[:, ZERO_CHANNEL] = 0.0
    return _f32(q_hat), _f32(k_hat), _f32(s), torch.tensor(STATS_INDEX, dtype=torch.int32)


TAIL_SHAPES = ((3, 64, 70), (3, 256, 200), (2, 64, 1))
N_TIES = 16


def tail_inputs(shape, seed: int = TAIL_SEED):
    """p, c, mean, std (B, C, N) fp32: continuous p, c, mean, std >= 0.1, and sixteen planted exact ties (std = 0, mean = p) at the returned
    flat indices (none for fewer than 64 elements)"""
    rng = np.random.default_rng(seed * 100 + shape[1] + shape[2])
    p, c, mean = _f32(_u(rng, shape, -1, 2)), _f32(_u(rng, shape, 0, 3)), _f32(_u(rng, shape, -1, 2))
    std = _f32(_u(rng, shape, 0.1, 1.5))
    n = p.numel()
    ties = torch.from_numpy(((np.arange(N_TIES) * 2654435761) % n).astype(np.int64)).unique() if n >= 64 else torch.zeros(0, dtype=torch.int64)
    std.view(-1)[ties] = 0.0
    mean.view(-1)[ties] = p.view(-1)[ties]
    return p, c, mean, std, ties
