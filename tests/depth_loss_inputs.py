"""Inputs of the depth-smoothness tests (tests/golden/make_depth_loss_fixtures.py, test_depth_loss_host.py, test_gpu_depth_loss.py) whose
differences have an unambiguous sign in fp32, so that no element has to be set aside in a gradient comparison.

The scaled depth n takes the values 0 (at or below the near bound), 1 (at or beyond the far bound) and k / 13 for k in {1, 3, 4, 9, 10, 12}.
{0, 1, 3, 4, 9, 10, 12, 13} holds no three-term arithmetic progression, so a second difference k2 - 2 k1 + k0 vanishes only where the three
pixels are equal -- and equal pixels of one view hold the same fp32 depth, so their differences are exactly 0.  Every other first or second
difference is at least 1 / 13.  The image lies in [0.2, 0.8]: its signed differences stay below 0.6, the bilateral weight at sigma 10 above
exp(-6), and a weighted difference is either exactly 0 or above 1.9e-4.  `assert_sign_condition` checks exactly that, in float64."""
import torch

LEVELS = (1, 3, 4, 9, 10, 12)
NEAR = (1.0, 0.5, 2.0, 1.5, 0.75, 3.0)
FAR = (20.0, 50.0, 100.0, 10.0, 30.0, 80.0)
SIGN_MARGIN = 1e-4
CONFIGS = {"plain": (None, False), "second": (None, True), "bilateral": (10.0, False), "bilateral_second": (10.0, True)}


def make_inputs(b, v, H, W, seed):
    """depth (b, v, H, W), near / far (b, v), image (b, v, 3, H, W) as fp32 CPU tensors.  View 0 has near = 1 (log near = 0) and exact
    zeros (ties at the bound); every view has pixels beyond both bounds and, from 8 x 12 pixels on, a flat patch; the last of several views
    lies beyond far."""
    g = torch.Generator().manual_seed(seed)
    N = b * v
    near = torch.tensor([NEAR[i % len(NEAR)] for i in range(N)], dtype=torch.float32)
    far = torch.tensor([FAR[i % len(FAR)] for i in range(N)], dtype=torch.float32)
    lo, hi = near.double().log().view(N, 1, 1), far.double().log().view(N, 1, 1)
    k = torch.tensor(LEVELS, dtype=torch.float64)[torch.randint(0, len(LEVELS), (N, H, W), generator=g)]
    if H >= 8 and W >= 12:
        k[:, H // 4:H // 4 + 4, W // 4:W // 4 + 6] = 4.0                                       # a flat patch
    depth = (lo + (hi - lo) * k / 13).float()
    r = torch.rand(N, H, W, generator=g)
    off = 0.25 + torch.rand(N, H, W, generator=g)
    depth = torch.where(r < 0.1, (lo - off).float(), depth)
    depth = torch.where(r > 0.9, (hi + off).float(), depth)
    depth[0] = torch.where((r[0] >= 0.1) & (r[0] < 0.25), torch.zeros(()), depth[0])            # near = 1: depth 0 sits exactly on the bound
    if N > 1:
        depth[-1] = (hi[-1] + off[-1]).float()
    image = torch.randint(51, 205, (N, 3, H, W), generator=g).float() / 255                     # 8-bit levels inside [0.2, 0.8]
    return depth.view(b, v, H, W), near.view(b, v), far.view(b, v), image.view(b, v, 3, H, W)


def weighted_differences(depth, near, far, image, sigma_image, second):
    """the two maps whose absolute values the loss averages, in float64 from the given (fp32) inputs"""
    depth, near, far = depth.double(), near.double(), far.double()
    lo, hi = near.log()[..., None, None], far.log()[..., None, None]
    n = (torch.maximum(torch.minimum(depth, hi), lo) - lo) / (hi - lo)
    dx, dy = n.diff(dim=-1), n.diff(dim=-2)
    if second:
        dx, dy = dx.diff(dim=-1), dy.diff(dim=-2)
    if sigma_image is not None:
        cx, cy = image.double().diff(dim=-1).amax(dim=-3), image.double().diff(dim=-2).amax(dim=-3)
        if second:
            cx, cy = torch.maximum(cx[..., 1:], cx[..., :-1]), torch.maximum(cy[..., 1:, :], cy[..., :-1, :])
        dx, dy = dx * torch.exp(-cx * sigma_image), dy * torch.exp(-cy * sigma_image)
    return dx, dy


def sign_condition_holds(depth, near, far, image) -> bool:
    for sigma, second in CONFIGS.values():
        for t in weighted_differences(depth, near, far, image, sigma, second):
            if bool(((t != 0) & (t.abs() < SIGN_MARGIN)).any()):
                return False
    return True


def assert_sign_condition(depth, near, far, image):
    assert sign_condition_holds(depth, near, far, image), "a weighted difference is neither exactly 0 nor >= 1e-4: its sign is not safe in fp32"


def value_tolerance(weight, sigma_image):
    """each mean within 8 * 2^-24 * max(1, e^sigma) of the float64 value (three roundings in n, a few more in the difference, exp and
    product; the means themselves are accumulated in float64), the loss within weight * 2 x that"""
    import math
    return weight * 2 * 8 * 2.0 ** -24 * max(1.0, math.exp(sigma_image or 0.0))


GRAD_RTOL = 1e-5      # of max |g_ref|: an element is a handful of fp32 operations on exactly determined signs
