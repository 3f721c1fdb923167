"""Inputs, reference and comparison of the Gaussian-adapter tests (test_adapter_host.py, test_gpu_adapter.py).

The adapter kernels (csrc/vit_adapter.hip) take a different branch, or lose a different group of terms to rounding, depending on where a
Gaussian's raw head outputs lie.  One maximum-relative error over a whole `par` gradient hides most of that: the density channel's gradient
is 1e4 times the scale and quaternion channels'.  So every case here puts EVERY Gaussian into one named regime, and `group_errors` takes one
maximum per output tensor and per gradient group (pts, density, scale, quaternion, SH), each relative to the float64 reference's maximum of
that group.  No Gaussian is left out of any comparison.

All inputs are float32 values held in float64 tensors, so the float64 reference, the float32 yardstick and the kernels see the same numbers.
|density| <= 8 everywhere: from about 17 on, the float32 autograd of the opacity map with an exponent below 1 forms inf * 0."""
import functools
import math
from types import SimpleNamespace

import torch
import torch.nn.functional as F

REGIMES = ("normal", "far", "tiny_xyz", "softplus_linear", "tiny_scale", "clamp_all", "clamp_one", "iso", "small_q", "zero_q", "dens_sat")
EXPONENTS = (1.0, 1.7, 0.6)
# name -> (b, v, H, W, sh_degree, separate appearance head).  5 x 7 x 2 x 3 = 210 Gaussians: one workgroup, partly empty; 8 x 16 x 3 = 384:
# two workgroups, the second half empty.  v = 1 passes no `ptsr` / `parr` at all.
LAYOUTS = {"app_b2_v3_5x7_sh2": (2, 3, 5, 7, 2, True), "app_b1_v1_8x16_sh0": (1, 1, 8, 16, 0, True),
           "packed_b1_v3_8x16_sh2": (1, 3, 8, 16, 2, False), "packed_b2_v1_5x7_sh0": (2, 1, 5, 7, 0, False)}
FORWARD = ("means", "cov", "sh", "opac", "scales", "rot")
GRADIENT = ("d_pts", "d_density", "d_scale", "d_quaternion", "d_sh")
FLOOR = {**{n: 2e-6 for n in FORWARD}, **{n: 2e-5 for n in GRADIENT}}      # the bars of the per-tensor test, now per group
YARDSTICK_FACTOR = 4.0                                                   # the kernel orders two to three roundings per quantity differently


def sh_mask_of(sh_degree):
    mask = torch.ones((sh_degree + 1) ** 2, dtype=torch.float32)
    for deg in range(1, sh_degree + 1):
        mask[deg ** 2:(deg + 1) ** 2] = 0.1 * 0.25 ** deg
    return mask


# --------------------------------------------------------------------------- the expression under test
def reference_expression(pts0, ptsr, par0, parr, app, sh_mask, exponent, v):
    """the framework expression in the inputs' precision, same layout conventions as EncoderNoPoSplatMultiTokenStyle.forward"""
    from styl3r_amd.encoder import build_covariance, reg_dense_depth_exp
    b, _, H, W = pts0.shape
    HW = H * W
    per_view = lambda first, rest: first.unsqueeze(1) if rest is None else torch.cat((first.unsqueeze(1), rest.reshape(b, v - 1, *rest.shape[1:])), 1)
    pts = per_view(pts0, ptsr).permute(0, 1, 3, 4, 2).reshape(b, v, HW, 3)
    par = per_view(par0, parr).flatten(3).transpose(2, 3)                     # (b, v, HW, C)
    means = reg_dense_depth_exp(pts)
    p = par[..., 0].sigmoid()
    opac = p if exponent == 1 else 0.5 * (1 - (1 - p) ** exponent + p ** (1 / exponent))
    scales = (0.001 * F.softplus(par[..., 1:4])).clamp_max(0.3)
    rot = par[..., 4:8] / (par[..., 4:8].norm(dim=-1, keepdim=True) + 1e-8)
    d_sh = sh_mask.numel()
    shraw = app.reshape(b, v, 3 * d_sh, HW).transpose(2, 3) if app is not None else par[..., 8:]
    sh = shraw.reshape(b, v, HW, 3, d_sh) * sh_mask
    cov = build_covariance(scales, rot)
    return (means.reshape(b, v * HW, 3), cov.reshape(b, v * HW, 3, 3), sh.reshape(b, v * HW, 3, d_sh), opac.reshape(b, v * HW),
            scales.reshape(b, v * HW, 3), rot.reshape(b, v * HW, 4))


def per_gaussian(first, rest, b, v):
    """(b, C, H, W) of view 0 + (b (v - 1), C, H, W) of the others -> (b, v H W, C), the order of the adapter's outputs"""
    x = first.unsqueeze(1) if rest is None else torch.cat((first.unsqueeze(1), rest.reshape(b, v - 1, *rest.shape[1:])), 1)
    return x.flatten(3).transpose(2, 3).reshape(b, -1, first.shape[1])


def gradient_groups(g_pts0, g_ptsr, g_par0, g_parr, g_app, case):
    """the five input gradients, regrouped per Gaussian: d_pts (b, G, 3), d_density (b, G), d_scale (b, G, 3), d_quaternion (b, G, 4),
    d_sh (b, G, 3 d_sh) -- from the appearance head's gradient, or from the channels behind the 8 structure channels"""
    b, v = case.b, case.v
    par = per_gaussian(g_par0, g_parr, b, v)
    sh = g_app.reshape(b, v, g_app.shape[1], -1).transpose(2, 3).reshape(b, -1, g_app.shape[1]) if g_app is not None else par[..., 8:]
    return dict(d_pts=per_gaussian(g_pts0, g_ptsr, b, v), d_density=par[..., 0], d_scale=par[..., 1:4], d_quaternion=par[..., 4:8], d_sh=sh)


# --------------------------------------------------------------------------- regime builders
def _unit(g, *shape):
    d = torch.randn(*shape, generator=g)
    return d / d.norm(dim=-1, keepdim=True)


def _uniform(g, lo, hi, *shape):
    return lo + (hi - lo) * torch.rand(*shape, generator=g)


def _log_uniform(g, lo, hi, *shape):
    return torch.exp(_uniform(g, math.log(lo), math.log(hi), *shape))


def build_case(regime, layout):
    """-> case with .ins = (pts0, ptsr, par0, parr, app) (float32 values as float64; ptsr / parr None at v = 1, app None when the SH
    coefficients are packed behind the structure channels), .sh_mask, .weights (the upstream gradients of means, cov, sh, opac)"""
    b, v, H, W, sh_degree, separate_app = LAYOUTS[layout]
    g = torch.Generator().manual_seed(1000 * REGIMES.index(regime) + list(LAYOUTS).index(layout))
    d_sh = (sh_degree + 1) ** 2
    N = (b, v, H, W)
    xyz = torch.randn(*N, 3, generator=g) * 0.8
    dens = (torch.randn(*N, generator=g) * 2).clamp(-8.0, 8.0)
    sraw = torch.randn(*N, 3, generator=g) * 2
    q = torch.randn(*N, 4, generator=g) * 2
    shraw = torch.randn(*N, 3 * d_sh, generator=g) * (1.0 if separate_app else 2.0)
    if regime == "far":
        xyz = _unit(g, *N, 3) * _uniform(g, 4.01, 5.99, *N, 1)
    elif regime == "tiny_xyz":
        xyz = _unit(g, *N, 3) * _log_uniform(g, 1.05e-10, 7.6e-9, *N, 1)
        flat = xyz.view(-1, 3)
        flat[[0, 3, flat.shape[0] // 2, flat.shape[0] - 2, flat.shape[0] - 1]] = 0.0
    elif regime == "softplus_linear":
        sraw = _uniform(g, 20.5, 60.0, *N, 3)
    elif regime == "tiny_scale":
        sraw = _uniform(g, -20.0, -10.0, *N, 3)
    elif regime == "clamp_all":
        sraw = _uniform(g, 300.5, 400.0, *N, 3)
    elif regime == "clamp_one":
        axis = torch.randint(0, 3, N, generator=g)
        sraw = torch.where(F.one_hot(axis, 3).bool(), _uniform(g, 300.5, 400.0, *N, 3), sraw)
    elif regime == "iso":
        sraw = sraw[..., :1].expand(*N, 3).contiguous()
    elif regime == "small_q":
        q = _unit(g, *N, 4) * _log_uniform(g, 1.05e-7, 9.5e-6, *N, 1)
    elif regime == "zero_q":
        q = torch.zeros(*N, 4)
    elif regime == "dens_sat":
        dens = _uniform(g, 6.02, 7.98, *N) * (torch.randint(0, 2, N, generator=g) * 2 - 1)
    else:
        assert regime == "normal", regime
    nchw = lambda t: t.permute(0, 1, 4, 2, 3)                                   # (b, v, H, W, C) -> (b, v, C, H, W)
    pts, par = nchw(xyz), nchw(torch.cat((dens.unsqueeze(-1), sraw, q) + (() if separate_app else (shraw,)), -1))
    split = lambda t: (t[:, 0].contiguous().double(), t[:, 1:].reshape(b * (v - 1), *t.shape[2:]).contiguous().double() if v > 1 else None)
    (pts0, ptsr), (par0, parr) = split(pts), split(par)
    app = nchw(shraw).reshape(b * v, 3 * d_sh, H, W).contiguous().double() if separate_app else None
    G = v * H * W
    weights = tuple(torch.randn(*s, generator=g).double() for s in ((b, G, 3), (b, G, 3, 3), (b, G, 3, d_sh), (b, G)))
    return SimpleNamespace(regime=regime, layout=layout, b=b, v=v, H=H, W=W, sh_degree=sh_degree, d_sh=d_sh, separate_app=separate_app,
                           ins=(pts0, ptsr, par0, parr, app), sh_mask=sh_mask_of(sh_degree).double(), weights=weights)


@functools.lru_cache(maxsize=None)
def case_of(regime, layout):
    return build_case(regime, layout)


def raw_values(case, dtype=torch.float32):
    """per Gaussian, (b, G, .): xyz, density, the three scale raws, the quaternion -- what the regime predicates are about"""
    pts0, ptsr, par0, parr, _ = (None if t is None else t.to(dtype) for t in case.ins)
    par = per_gaussian(par0, parr, case.b, case.v)
    return per_gaussian(pts0, ptsr, case.b, case.v), par[..., 0], par[..., 1:4], par[..., 4:8]


def regime_predicate(case):
    """-> bool (b, G): the Gaussian takes the branches its regime is named after -- evaluated in float32, as the kernel sees it"""
    xyz, dens, sraw, q = raw_values(case)
    d, n = xyz.norm(dim=-1), q.norm(dim=-1)
    clamped = torch.tensor(0.001, dtype=torch.float32) * F.softplus(sraw) > torch.tensor(0.3, dtype=torch.float32)
    ok = (dens.abs() <= 8) & torch.isfinite(xyz).all(-1)
    r = case.regime
    if r != "tiny_xyz":
        ok &= d >= 1e-3
    if r not in ("small_q", "zero_q"):
        ok &= n >= 1e-2
    if r not in ("clamp_all", "clamp_one"):
        ok &= ~clamped.any(-1)
    if r not in ("softplus_linear", "clamp_all", "clamp_one"):
        ok &= (sraw <= 20).all(-1)
    if r == "far":
        ok &= (d >= 4) & (d <= 6)
    elif r == "tiny_xyz":
        ok &= (d == 0) | ((d >= 1e-10) & (d <= 8e-9) & (d < torch.tensor(1e-8, dtype=torch.float32)))
    elif r == "softplus_linear":
        ok &= ((sraw > 20) & (sraw <= 60)).all(-1)
    elif r == "tiny_scale":
        ok &= ((sraw >= -20) & (sraw <= -10)).all(-1)
    elif r == "clamp_all":
        ok &= clamped.all(-1)
    elif r == "clamp_one":
        ok &= clamped.sum(-1) == 1
    elif r == "iso":
        ok &= (sraw == sraw[..., :1]).all(-1)
    elif r == "small_q":
        ok &= (n >= 1e-7) & (n <= 1e-5)
    elif r == "zero_q":
        ok &= (q == 0).all(-1)
    elif r == "dens_sat":
        ok &= (dens.abs() >= 6)
    return ok


# --------------------------------------------------------------------------- reference, yardstick, comparison
def evaluate(fn, case, exponent, dtype, device="cpu"):
    """forward outputs and gradient groups of `fn` (the calling convention of `reference_expression`) on the case's inputs in `dtype`"""
    ins = [None if t is None else t.to(device=device, dtype=dtype, copy=True).requires_grad_(True) for t in case.ins]
    out = fn(*ins, case.sh_mask.to(device=device, dtype=dtype), exponent, case.v)
    sum((o * w.to(device=device, dtype=dtype)).sum() for o, w in zip(out[:4], case.weights)).backward()
    res = {n: o.detach() for n, o in zip(FORWARD, out)}
    res.update(gradient_groups(*(None if t is None else t.grad for t in ins), case))
    return res


@functools.lru_cache(maxsize=None)
def reference(regime, layout, exponent):
    """the float64 expression and its autograd: computed once per case, shared by every test, never modified"""
    return evaluate(reference_expression, case_of(regime, layout), exponent, torch.float64)


def conditioning_scale(case):
    """size of the individual terms of the quaternion gradient: max |w_cov| s_max^2 / min |q|.  Where all three scales are equal
    (clamp_all, iso) Sigma = s^2 R R^T does not depend on the rotation; the terms cancel and what is left is rounding."""
    _, _, sraw, q = raw_values(case, torch.float64)
    s_max = (0.001 * F.softplus(sraw)).clamp_max(0.3).max()
    return float(case.weights[1].abs().max() * s_max ** 2 / q.norm(dim=-1).min())


def group_scale(name, want, case):
    if name == "d_quaternion" and case.regime in ("clamp_all", "iso"):
        return conditioning_scale(case)
    return float(want.abs().max())


def group_errors(got, want, case):
    """{tensor or gradient group: max |got - want| / scale}, scale = the float64 reference's max |.| over the group (the conditioning scale
    for the quaternion gradient of clamp_all and iso).  A group whose reference is identically 0 (the clamped scales' gradient, everything
    about a zero quaternion) has the error 0 where `got` is 0 everywhere and inf otherwise; so has any NaN / Inf."""
    errs = {}
    for name, w in want.items():
        a = got[name].detach().to("cpu", torch.float64).reshape(w.shape)
        diff = (a - w).abs()
        if not bool(torch.isfinite(diff).all()):
            errs[name] = math.inf
            continue
        err, scale = float(diff.max()), group_scale(name, w, case)
        errs[name] = err / scale if scale > 0 else (0.0 if err == 0 else math.inf)
    return errs


def exact_zero_groups(regime):
    """gradient groups that are 0 bit for bit: clamp_max passes no gradient above the clamp; at q = 0 every term carries a factor q"""
    return {"clamp_all": ("d_scale",), "zero_q": ("d_quaternion",)}.get(regime, ())


@functools.lru_cache(maxsize=None)
def yardstick(regime, layout, exponent):
    """error of the float32 evaluation of the element-wise expression against float64, on the same inputs, per group"""
    case = case_of(regime, layout)
    return group_errors(evaluate(reference_expression, case, exponent, torch.float32), reference(regime, layout, exponent), case)


def measured_yardstick(regime):
    """max over layouts and exponents, per group -- what YARDSTICK records"""
    rows = [yardstick(regime, layout, e) for layout in LAYOUTS for e in EXPONENTS]
    return {n: max(r[n] for r in rows) for n in FORWARD + GRADIENT}


def bar(regime, name):
    return max(FLOOR[name], YARDSTICK_FACTOR * YARDSTICK[regime][name])


def assert_within_bars(errs, regime, what):
    bad = {n: (e, bar(regime, n)) for n, e in errs.items() if not e <= bar(regime, n)}
    assert not bad, f"{what}: (error, bar) {bad}"


def assert_exact_zeros(got, regime, what):
    for n in exact_zero_groups(regime):
        assert bool((got[n] == 0).all()), f"{what}: {n} must be exactly 0, max |.| = {float(got[n].abs().max())}"


# --------------------------------------------------------------------------- the kernel's backward closed form, float32, in tensor algebra
def closed_form_backward(case, exponent, dtype=torch.float32, radial_below_clip=True):
    """The backward of csrc/vit_adapter.hip as its header states the forward -- m = xyz / max(|xyz|, 1e-8) expm1(|xyz|), the opacity map,
    s = min(0.001 softplus, 0.3), qh = q / (|q| + 1e-8), R = I + u P(qh), Sigma = (R diag s)(R diag s)^T -- differentiated by hand and
    written on whole tensors: P = qv qv^T - |qv|^2 I + w [qv]x gives the rotation chain as matrix-vector products, where the kernel spells
    out 28 scalar terms.  So the formula can be judged against float64 autograd without a GPU.  radial_below_clip=False restates the form
    the kernel had before |xyz| < 1e-8 got its radial term."""
    one = lambda x: torch.tensor(x, dtype=dtype)
    xyz, dens, sraw, q = raw_values(case, dtype)
    gm, gS, gsh, gop = (w.to(dtype) for w in case.weights)
    # means
    d = xyz.norm(dim=-1, keepdim=True)
    f, dn = torch.expm1(d), d.clamp_min(1e-8)
    above = ((f + 1) * dn - f) / (dn * dn) / dn
    below = torch.where(d > 0, (f + 1) / (dn * d), torch.zeros_like(d)) if radial_below_clip else torch.zeros_like(d)
    coef = torch.where(d >= one(1e-8), above, below)
    d_pts = gm * (f / dn) + xyz * ((gm * xyz).sum(-1, keepdim=True) * coef)
    # opacity
    p = torch.sigmoid(dens)
    dodp = torch.ones_like(p) if exponent == 1 else 0.5 * (exponent * (1 - p) ** (exponent - 1) + (1 / exponent) * p ** (1 / exponent - 1))
    d_density = gop * dodp * (p * (1 - p))
    # covariance -> M = R diag(s)
    sp = F.softplus(sraw)
    s = (one(0.001) * sp).clamp_max(0.3)
    n = q.norm(dim=-1, keepdim=True)
    inv = 1 / (n + one(1e-8))
    qh = q * inv
    qv, w = qh[..., :3], qh[..., 3:]
    u = 2 / ((qh * qh).sum(-1, keepdim=True) + one(1e-8))
    cross = torch.zeros(*qv.shape[:-1], 3, 3, dtype=dtype)
    cross[..., 0, 1], cross[..., 0, 2], cross[..., 1, 0] = -qv[..., 2], qv[..., 1], qv[..., 2]
    cross[..., 1, 2], cross[..., 2, 0], cross[..., 2, 1] = -qv[..., 0], -qv[..., 1], qv[..., 0]
    eye = torch.eye(3, dtype=dtype)
    P = qv.unsqueeze(-1) * qv.unsqueeze(-2) - (qv * qv).sum(-1)[..., None, None] * eye + w.unsqueeze(-1) * cross
    R = eye + u.unsqueeze(-1) * P
    gM = (gS + gS.transpose(-1, -2)) @ (R * s.unsqueeze(-2))
    g_s = (gM * R).sum(-2)
    gR = gM * s.unsqueeze(-2)
    passes = (one(0.001) * sp <= one(0.3)).to(dtype)
    d_scale = g_s * passes * one(0.001) * torch.where(sraw > 20, torch.ones_like(sraw), torch.sigmoid(sraw))
    # rotation -> qh -> q
    ax = torch.stack((gR[..., 2, 1] - gR[..., 1, 2], gR[..., 0, 2] - gR[..., 2, 0], gR[..., 1, 0] - gR[..., 0, 1]), -1)
    trace = gR.diagonal(dim1=-2, dim2=-1).sum(-1, keepdim=True)
    g_qv = ((gR + gR.transpose(-1, -2)) @ qv.unsqueeze(-1)).squeeze(-1) - 2 * trace * qv + w * ax
    g_qh = u * torch.cat((g_qv, (qv * ax).sum(-1, keepdim=True)), -1)
    g_qh = g_qh - (gR * P).sum((-2, -1)).unsqueeze(-1) * u * u * qh                                 # du / dqh = -u^2 qh
    back = torch.where(n > 0, (g_qh * q).sum(-1, keepdim=True) * inv * inv / n, torch.zeros_like(n))
    d_quaternion = g_qh * inv - q * back
    # SH
    d_sh = (gsh * case.sh_mask.to(dtype)).flatten(-2)
    return dict(d_pts=d_pts, d_density=d_density, d_scale=d_scale, d_quaternion=d_quaternion, d_sh=d_sh)


# Recorded `measured_yardstick` (CPU, float32 expression against float64), rounded up to two digits; test_adapter_host.py holds it against
# a fresh measurement.  Only entries above FLOOR / YARDSTICK_FACTOR move a bar.
YARDSTICK = {
    "normal": {"means": 1.6e-07, "cov": 4.5e-07, "sh": 1.2e-09, "opac": 2.8e-07, "scales": 1.0e-07, "rot": 1.1e-07,
               "d_pts": 1.2e-07, "d_density": 6.4e-07, "d_scale": 3.2e-07, "d_quaternion": 3.7e-07, "d_sh": 1.2e-09},
    "far": {"means": 3.4e-07, "cov": 4.7e-07, "sh": 1.1e-09, "opac": 2.6e-07, "scales": 1.2e-07, "rot": 1.1e-07,
            "d_pts": 2.4e-07, "d_density": 6.0e-07, "d_scale": 4.2e-07, "d_quaternion": 2.9e-07, "d_sh": 1.1e-09},
    "tiny_xyz": {"means": 9.9e-08, "cov": 4.1e-07, "sh": 1.3e-09, "opac": 2.7e-07, "scales": 1.3e-07, "rot": 9.8e-08,
                 "d_pts": 8.7e-08, "d_density": 3.8e-07, "d_scale": 2.2e-07, "d_quaternion": 3.3e-07, "d_sh": 1.1e-09},
    "softplus_linear": {"means": 1.9e-07, "cov": 4.9e-07, "sh": 1.2e-09, "opac": 3.0e-07, "scales": 7.8e-08, "rot": 1.1e-07,
                        "d_pts": 1.3e-07, "d_density": 5.5e-07, "d_scale": 4.3e-07, "d_quaternion": 6.4e-07, "d_sh": 9.8e-10},
    "tiny_scale": {"means": 1.5e-07, "cov": 4.3e-07, "sh": 1.2e-09, "opac": 1.8e-07, "scales": 1.4e-07, "rot": 9.4e-08,
                   "d_pts": 1.4e-07, "d_density": 3.5e-07, "d_scale": 4.0e-07, "d_quaternion": 4.4e-07, "d_sh": 1.2e-09},
    "clamp_all": {"means": 1.2e-07, "cov": 6.6e-07, "sh": 1.2e-09, "opac": 2.1e-07, "scales": 4.0e-08, "rot": 1.1e-07,
                  "d_pts": 2.0e-07, "d_density": 3.2e-07, "d_scale": 0.0, "d_quaternion": 4.8e-07, "d_sh": 1.1e-09},
    "clamp_one": {"means": 8.7e-08, "cov": 6.0e-07, "sh": 1.1e-09, "opac": 2.2e-07, "scales": 4.0e-08, "rot": 1.0e-07,
                  "d_pts": 1.7e-07, "d_density": 3.5e-07, "d_scale": 2.8e-07, "d_quaternion": 3.7e-07, "d_sh": 9.8e-10},
    "iso": {"means": 1.5e-07, "cov": 4.2e-07, "sh": 1.1e-09, "opac": 1.8e-07, "scales": 1.3e-07, "rot": 9.7e-08,
            "d_pts": 2.3e-07, "d_density": 4.0e-07, "d_scale": 4.4e-07, "d_quaternion": 2.3e-07, "d_sh": 1.1e-09},
    "small_q": {"means": 1.3e-07, "cov": 3.5e-07, "sh": 1.3e-09, "opac": 3.8e-07, "scales": 8.9e-08, "rot": 1.1e-07,
                "d_pts": 1.0e-07, "d_density": 2.7e-07, "d_scale": 3.6e-07, "d_quaternion": 3.5e-07, "d_sh": 1.3e-09},
    "zero_q": {"means": 1.2e-07, "cov": 2.1e-07, "sh": 1.2e-09, "opac": 2.0e-07, "scales": 1.0e-07, "rot": 0.0,
               "d_pts": 1.1e-07, "d_density": 2.5e-07, "d_scale": 1.4e-07, "d_quaternion": 0.0, "d_sh": 1.2e-09},
    "dens_sat": {"means": 1.2e-07, "cov": 3.9e-07, "sh": 1.3e-09, "opac": 6.5e-07, "scales": 1.1e-07, "rot": 9.6e-08,
                 "d_pts": 1.7e-07, "d_density": 3.9e-05, "d_scale": 4.5e-07, "d_quaternion": 5.1e-07, "d_sh": 9.6e-10},
}


def format_yardstick():
    def up(x):                                                    # two significant digits, rounded up
        if x == 0:
            return "0.0"
        step = 10.0 ** (math.floor(math.log10(x)) - 1)
        return f"{math.ceil(x / step) * step:.1e}"
    lines = ["YARDSTICK = {"]
    for r in REGIMES:
        m = measured_yardstick(r)
        lines.append(f'    "{r}": {{' + ", ".join(f'"{n}": {up(m[n])}' for n in FORWARD + GRADIENT) + "},")
    return "\n".join(lines + ["}"])


if __name__ == "__main__":
    print(format_yardstick())
