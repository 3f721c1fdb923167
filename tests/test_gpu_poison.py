"""-m gpu: every kernel chain on poisoned scratch and output memory (tests/poison.py).

A fresh test process hands out memory that is mostly zero; a long training run hands out recycled blocks that hold anything.  Each
case builds its inputs once and runs the op three times, with every `torch.empty` / `empty_like` / `empty_strided` / `new_empty` of the
wrapper filled with zeros, with 0xFF bytes (NaN / -1) and with 0xA5 bytes / 1e30, and asserts:
  1. the poison reached the op: the allocation record holds the op's scratch size or output shape;
  2. finite inputs give finite outputs under every pattern;
  3. the result does not depend on the pattern: bit-identical where the op is documented as deterministic, else every run meets the
     bar the op's own test uses against its float64 reference (sums ordered by atomics);
  4. for direct C-ABI calls on a scratch of exactly the stated size, the canary bytes behind it are intact.
Which entries may be run this way, and why, is docs/SCRATCH_CONTRACTS.md: an entry is here only if every integer its kernels use as an
index, offset, count or ticket is written before it is read or zeroed by a named line.  Nothing here aims at a fault."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests.gpu_utils import assert_close_rel, oracle_single_view
from tests.helpers import random_scene, simple_camera
from tests.poison import PATTERNS, guarded, poisoned_allocations

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, I32, U8 = torch.float32, torch.int32, torch.uint8


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def three_runs(op, expect=(), before=None):
    """op() -> {name: tensor}, run once per pattern with the allocators poisoned.  Asserts (1) and (2); returns {pattern: outputs}.
    `expect`: keyword sets of AllocationRecord.has (nbytes=..., or shape=... with dtype=...) that every run's record must hold."""
    runs = {}
    for pattern in PATTERNS:
        if before is not None:
            before()
        with poisoned_allocations(pattern) as rec:
            out = op()
            torch.cuda.synchronize()
        assert len(rec) > 0, f"{pattern}: no allocation was poisoned"
        for e in expect:
            assert rec.has(**e), (pattern, e, sorted(set(rec), key=str)[:24])
        out = {k: v.detach() for k, v in out.items() if v is not None}
        for k, v in out.items():
            if v.is_floating_point():
                assert bool(torch.isfinite(v).all()), f"{k} is not finite on {pattern}-filled memory"
        runs[pattern] = out
    return runs


def assert_identical(runs, keys=None):
    """(3), deterministic ops: the three runs agree bit for bit"""
    for pattern in PATTERNS[1:]:
        for k in (keys if keys is not None else runs["zero"]):
            a, b = runs[pattern][k], runs["zero"][k]
            assert a.shape == b.shape and torch.equal(a, b), f"{k}: the {pattern}-filled run differs from the zero-filled one"


def rel_err(got, want):
    want = want.detach().double()
    return float((got.detach().double() - want).abs().max() / want.abs().max().clamp_min(1e-300))


def test_the_harness_notices_both_kinds_of_defect_on_the_device():
    """a scratch word read before anything wrote it, and an output element no kernel wrote (gsr_mse_backward asked for n - 1 of the n
    elements of its torch.empty gradient: everything stays in bounds)"""
    from styl3r_amd import _lib
    lib = _lib.load()
    with pytest.raises(AssertionError, match="not finite on ones-filled"):
        three_runs(lambda: dict(total=torch.empty(100, device=DEV).sum()), expect=[dict(shape=(100,), dtype=F32)])
    n = 4 * 256 * 3 + 3
    g = torch.Generator(DEV).manual_seed(1)
    pred, target, one = torch.rand(n, device=DEV, generator=g), torch.rand(n, device=DEV, generator=g), torch.ones(1, device=DEV)

    def op(count):
        grad = torch.empty_like(pred)
        assert lib.gsr_mse_backward(pred.data_ptr(), target.data_ptr(), one.data_ptr(), count, 1.0, grad.data_ptr(), _stream()) == 0
        return dict(grad=grad)
    assert_identical(three_runs(lambda: op(n)))
    with pytest.raises(AssertionError, match="not finite on ones-filled"):
        three_runs(lambda: op(n - 1))
    res = {}
    for pattern in ("zero", "garbage"):
        with poisoned_allocations(pattern) as rec:
            res[pattern] = op(n - 1)["grad"]
        assert rec.has(shape=(n,), dtype=F32)
    assert torch.equal(res["zero"][:n - 1], res["garbage"][:n - 1]) and float(res["zero"][-1]) == 0.0 and float(res["garbage"][-1]) == float(torch.tensor(1e30))


# =====================================================================================================================
# Rasterizer (rasterizer.py: the whole workspace, every output and every gradient are torch.empty)
# =====================================================================================================================
RH, RW, RSH = 33, 40, 1                                   # ragged tiles: 3 x 3 of them, the last row / column 1 / 8 pixels
R_BG = (0.1, 0.3, 0.2)
CAM_C2W = np.array([[0.995, 0, 0.0998, 0.1], [0, 1, 0, -0.05], [-0.0998, 0, 0.995, 0.2], [0, 0, 0, 1]])


class RasterCase:
    """500 Gaussians x 2 views: 420 in the left half of the image (the right tile column stays empty), 40 behind the camera and 40 far
    off screen (culled records, zero gradient rows); the oracle's forward state and gradients, computed once"""

    def __init__(self):
        from styl3r_amd import rasterizer as rz
        m, c6, op, sh = random_scene(420, seed=21, scale=(0.02, 0.08), sh_degree=RSH)
        m[:, 0] = -np.abs(m[:, 0])
        mb, cb, ob, sb = random_scene(40, seed=22, sh_degree=RSH)
        mb[:, 2] *= -1
        mo, co, oo, so = random_scene(40, seed=23, sh_degree=RSH)
        mo[:, 0] += 8 * mo[:, 2]
        self.np = [np.concatenate(x).astype(np.float32) for x in ((m, mb, mo), (c6, cb, co), (op, ob, oo), (sh, sb, so))]
        self.G = self.np[0].shape[0]
        self.cams = [simple_camera(RH, RW), simple_camera(RH, RW, c2w=CAM_C2W)]
        f = lambda k: torch.tensor(np.stack([c[k] for c in self.cams]), dtype=F32, device=DEV)
        t = lambda k: torch.tensor([c[k] for c in self.cams], dtype=F32, device=DEV)
        self.views = rz.pack_views(f("view"), f("proj"), f("proj_raw"), f("campos"), t("tanfovx"), t("tanfovy"),
                                   torch.tensor([R_BG, R_BG], dtype=F32, device=DEV))
        rng = np.random.default_rng(3)
        self.wI = rng.normal(size=(2, 3, RH, RW)).astype(np.float32)
        self.wD = (rng.normal(size=(2, RH, RW)) * 0.3).astype(np.float32)
        self.fwd, self.grads = [], {}
        for prec in ("f32", "f64"):
            tot = {}
            for v, cam in enumerate(self.cams):
                orc, st, ctx = oracle_single_view(prec, *self.np[:3], cam, shs=self.np[3], bg=R_BG, sh_degree=RSH)
                if prec == "f32":
                    self.fwd.append(st)
                g = orc.backward(st, ctx, self.wI[v], self.wD[v], want_tau=True)
                for k in ("means3D", "cov6", "opacities", "shs"):
                    tot[k] = tot.get(k, 0) + g[k]
                for k in ("means2D", "rho", "theta"):
                    tot.setdefault(k, []).append(g[k])
            self.grads[prec] = {k: (np.stack(v) if isinstance(v, list) else v) for k, v in tot.items()}
        lens = [st.ranges[:, 1] - st.ranges[:, 0] for st in self.fwd]
        assert all((l == 0).any() and (l > 0).any() for l in lens), "the scene must leave some tiles empty"
        assert all((st.radii == 0).sum() >= 80 for st in self.fwd), "the scene must hold culled Gaussians"

    def leaves(self, requires_grad=True, means=None):
        src = list(self.np)
        if means is not None:
            src[0] = means
        out = [torch.tensor(a, device=DEV)[None].requires_grad_(requires_grad) for a in src]
        m2d = torch.zeros((2, self.G, 3), device=DEV, requires_grad=requires_grad)
        theta = torch.zeros((2, 3), device=DEV, requires_grad=requires_grad)
        rho = torch.zeros((2, 3), device=DEV, requires_grad=requires_grad)
        return out, m2d, theta, rho


@pytest.fixture(scope="module")
def raster():
    return RasterCase()


@pytest.fixture
def raster_debug():
    from styl3r_amd import rasterizer as rz
    rz.KEEP_DEBUG = True
    yield rz
    rz.KEEP_DEBUG = False
    rz.LAST_DEBUG.clear()


def _ws_words(rz, name, dtype, count):
    """`count` words of a workspace region of the last forward, cloned (a 256-byte aligned slice of the uint8 workspace)"""
    dbg = rz.LAST_DEBUG
    off = getattr(dbg["layout"], name)
    return dbg["ws"][off:off + 4 * count].clone().view(dtype)


def _raster_step(rz, case, backward=True, twice=False, means=None, mse=None):
    (mn, c6, op, sh), m2d, theta, rho = case.leaves(backward, means)
    out = rz.rasterize_views(mn, c6, op, sh, case.views, (RH, RW), 2, sh_degree=RSH, use_sh=True, means2D=m2d, theta=theta, rho=rho,
                             want_n_touched=True, mse=mse)
    R, T = rz.LAST_DEBUG["num_pairs"], 9
    res = dict(image=out.image, depth=out.depth, opacity=out.opacity, radii=out.radii, n_touched=out.n_touched,
               tile_offset=_ws_words(rz, "tile_offset", I32, 2 * T + 1), point_list=_ws_words(rz, "point_list", I32, max(R, 1))[:R],
               n_contrib=_ws_words(rz, "n_contrib", I32, 2 * RH * RW), final_T=_ws_words(rz, "final_T", F32, 2 * RH * RW),
               pairs=torch.tensor([R]))
    if mse is not None:
        res["loss"] = out.loss_mse
    if backward:
        loss = out.loss_mse if mse is not None else \
            (out.image * torch.tensor(case.wI, device=DEV)).sum() + (out.depth * torch.tensor(case.wD, device=DEV)).sum()
        names = ("means3D", "cov6", "opacities", "shs", "means2D", "theta", "rho")
        leaves = (mn, c6, op, sh, m2d, theta, rho)
        for tag in (("", "2nd_") if twice else ("",)):
            g = torch.autograd.grad(loss, leaves, retain_graph=twice and tag == "")
            res.update({tag + "d_" + n: x for n, x in zip(names, g)})
    return res


def _check_raster_forward(case, out):
    """as test_gpu_rasterizer._check_forward, per view of the batched call: integer state exact, images within 1e-4 of the oracle"""
    T, off, start = 9, out["tile_offset"].cpu().numpy().astype(np.int64), 0
    assert int(out["pairs"]) == sum(st.R for st in case.fwd), "R"
    for v, st in enumerate(case.fwd):
        assert np.array_equal(out["radii"][v].cpu().numpy(), st.radii), "radii"
        assert np.array_equal(np.diff(off)[v * T:(v + 1) * T], st.ranges[:, 1] - st.ranges[:, 0]), "range lengths"
        pl = out["point_list"][start:start + st.R].cpu().numpy().view(np.uint32)
        assert np.array_equal(pl & np.uint32(0x0FFFFFFF), st.point_list.astype(np.uint32)), "sorted (tile, id) list"
        start += st.R
        ok = st.fragile == 0
        assert ok.mean() > 0.97
        nc = out["n_contrib"].view(2, RH, RW)[v].cpu().numpy()
        assert np.array_equal(nc[ok], st.n_contrib[ok].astype(np.int32)), "n_contrib"
        assert_close_rel(out["image"][v].cpu().numpy()[:, ok], st.image[:, ok], 1e-4, "image")
        assert_close_rel(out["depth"][v].cpu().numpy()[ok], st.out_depth[ok], 1e-4, "depth")
        assert_close_rel(out["opacity"][v].cpu().numpy()[ok], st.out_opacity[ok], 1e-4, "opacity")
        assert_close_rel(out["final_T"].view(2, RH, RW)[v].cpu().numpy()[ok], st.final_T[ok], 1e-4, "final_T")
        assert (out["n_touched"][v].cpu().numpy() != st.n_touched).sum() <= 2, "n_touched"


def _check_raster_grads(case, out, tag=""):
    """the bars of test_gpu_rasterizer._check_backward: 1e-4 against the fp32 oracle, 2e-4 against the fp64 one; pose 5e-4 / 2e-4"""
    shape = dict(means3D=(case.G, 3), cov6=(case.G, 6), opacities=(case.G,), shs=(case.G, 4, 3), means2D=(2, case.G, 3))
    for k, s in shape.items():
        got = out[tag + "d_" + k].reshape(s).cpu().numpy()
        assert_close_rel(got, case.grads["f32"][k], 1e-4, f"{tag}d{k} vs f32 oracle")
        assert_close_rel(got, case.grads["f64"][k], 2e-4, f"{tag}d{k} vs f64 oracle")
    for k in ("rho", "theta"):
        got = out[tag + "d_" + k].cpu().numpy()
        assert_close_rel(got, case.grads["f32"][k], 5e-4, f"{tag}d{k} vs f32 oracle")
        assert_close_rel(got, case.grads["f64"][k], 2e-4, f"{tag}d{k} vs f64 oracle")
    culled = np.all([st.radii == 0 for st in case.fwd], axis=0)
    for k in ("means3D", "cov6", "opacities", "shs"):
        assert float(out[tag + "d_" + k][0][torch.tensor(culled, device=DEV)].abs().max()) == 0.0, f"{k}: a culled Gaussian has a gradient"


RASTER_STATE = ("image", "depth", "opacity", "radii", "n_touched", "tile_offset", "point_list", "n_contrib", "final_T", "pairs")


def test_rasterizer_forward_and_both_backward_paths(raster, raster_debug):
    """the two-phase forward (PHASE_BIN / PHASE_RENDER, what rasterizer.py issues) and two backwards through one graph: the first trusts
    GSR_FLAG_PREZERO_GRADS, the second finds dirty accumulators and takes the memset path"""
    rz = raster_debug
    from styl3r_amd import _lib
    dims = _lib.GsrDims(1, 2, raster.G, RH, RW, 4, RSH, 0, None)
    total = _lib.workspace_layout(dims, max(4 * 2 * raster.G, 1 << 16)).total
    runs = three_runs(lambda: _raster_step(rz, raster, twice=True),
                      expect=[dict(nbytes=total, dtype=U8), dict(shape=(2, 3, RH, RW), dtype=F32), dict(shape=(2, raster.G), dtype=I32),
                              dict(shape=(1, raster.G, 4, 3), dtype=F32), dict(shape=(2, 6), dtype=F32)])
    assert_identical(runs, RASTER_STATE)
    for pattern in PATTERNS:
        _check_raster_forward(raster, runs[pattern])
        _check_raster_grads(raster, runs[pattern])
        _check_raster_grads(raster, runs[pattern], "2nd_")


def test_rasterizer_with_every_gaussian_culled(raster, raster_debug):
    rz = raster_debug
    behind = raster.np[0].copy()
    behind[:, 2] = -np.abs(behind[:, 2]) - 0.5
    runs = three_runs(lambda: _raster_step(rz, raster, means=behind), expect=[dict(shape=(2, 3, RH, RW), dtype=F32)])
    assert_identical(runs)
    z = runs["zero"]
    assert int(z["pairs"]) == 0 and int(z["radii"].abs().max()) == 0 and int(z["n_contrib"].abs().max()) == 0
    want = torch.tensor(R_BG, device=DEV).view(1, 3, 1, 1).expand(2, 3, RH, RW)
    assert torch.equal(z["image"], want) and float(z["depth"].abs().max()) == 0.0 and float(z["opacity"].abs().max()) == 0.0
    for k, v in z.items():
        if k.startswith("d_"):
            assert float(v.abs().max()) == 0.0, k


def test_rasterizer_capacity_overflow_retry(raster, raster_debug):
    """a first-try capacity far below R: the render phase exits on the overflow flag, the wrapper re-issues everything on a second,
    larger (and again poisoned) workspace"""
    rz = raster_debug
    key = (1, 2, raster.G, RH, RW)
    old = rz._CAP_HINT.copy()
    try:
        want = _raster_step(rz, raster, backward=False)
        caps = []

        def shrink():
            rz._CAP_HINT[key] = 64

        def op():
            out = _raster_step(rz, raster)
            caps.append(rz.LAST_DEBUG["cap"])
            return out
        runs = three_runs(op, expect=[dict(shape=(2, 3, RH, RW), dtype=F32)], before=shrink)
        assert all(c > 64 for c in caps) and int(want["pairs"]) > 64
    finally:
        rz._CAP_HINT.clear(); rz._CAP_HINT.update(old)
    assert_identical(runs, RASTER_STATE)
    for k in RASTER_STATE:
        assert torch.equal(runs["zero"][k], want[k]), k
    for pattern in PATTERNS:
        _check_raster_grads(raster, runs[pattern])


def test_rasterizer_fused_mse(raster, raster_debug):
    """LossMse inside the composite kernels: partial sums, tickets and the image difference live in the poisoned workspace"""
    rz = raster_debug
    from styl3r_amd.losses import mse_loss
    target = torch.rand(2, 3, RH, RW, device=DEV, generator=torch.Generator(DEV).manual_seed(4))
    (mn, c6, op, sh), m2d, theta, rho = raster.leaves()
    out = rz.rasterize_views(mn, c6, op, sh, raster.views, (RH, RW), 2, sh_degree=RSH, use_sh=True)
    ref = torch.autograd.grad(mse_loss(out.image, target, 0.7), (mn, c6, op, sh))            # the stand-alone loss kernels, unpoisoned
    runs = three_runs(lambda: _raster_step(rz, raster, mse=rz.RasterMse(target, 0.7)), expect=[dict(shape=(), dtype=F32)])
    assert_identical(runs, RASTER_STATE + ("loss",))
    want = 0.7 * ((runs["zero"]["image"].double() - target.double()) ** 2).mean()
    assert abs(float(runs["zero"]["loss"]) - float(want)) <= 1e-6 * float(want)
    assert torch.equal(runs["zero"]["image"], out.image.detach())
    for pattern in PATTERNS:                                # (the 2e-5 bar of the fused-vs-stand-alone test: the atomics' order differs)
        for k, r in zip(("means3D", "cov6", "opacities", "shs"), ref):
            assert_close_rel(runs[pattern]["d_" + k].cpu().numpy(), r.cpu().numpy(), 2e-5, f"fused MSE d{k}")


def test_rasterizer_styles(raster, raster_debug):
    """gsr_forward_styles with 3 styles: the side array of the styles' colours is poisoned too"""
    rz = raster_debug
    rng = np.random.default_rng(9)
    styles = [raster.np[3]] + [(rng.normal(size=raster.np[3].shape) * 0.4).astype(np.float32) for _ in range(2)]
    (mn, c6, op, _), *_ = raster.leaves(False)
    cols = [torch.tensor(s, device=DEV)[None] for s in styles]

    def op_():
        o = rz.rasterize_views_styles(mn, c6, op, cols, raster.views, (RH, RW), 2, sh_degree=RSH, use_sh=True)
        return dict(image=o.image, depth=o.depth, opacity=o.opacity, radii=o.radii,
                    n_contrib=_ws_words(rz, "n_contrib", I32, 2 * RH * RW), final_T=_ws_words(rz, "final_T", F32, 2 * RH * RW))
    runs = three_runs(op_, expect=[dict(shape=(3, 2, 3, RH, RW), dtype=F32), dict(nbytes=2 * 2 * raster.G * 16, dtype=U8)])
    assert_identical(runs)
    z = runs["zero"]
    for s, shs in enumerate(styles):
        for v, cam in enumerate(raster.cams):
            st = raster.fwd[v] if s == 0 else oracle_single_view("f32", *raster.np[:3], cam, shs=shs, bg=R_BG, sh_degree=RSH)[1]
            ok = st.fragile == 0
            assert_close_rel(z["image"][s, v].cpu().numpy()[:, ok], st.image[:, ok], 1e-4, f"style {s} view {v}")
    assert np.array_equal(z["radii"].cpu().numpy(), np.stack([st.radii for st in raster.fwd]))


def test_rasterizer_c_abi_single_call_and_memset_backward_with_canaries(raster, raster_debug):
    """gsr_forward without phase flags and gsr_backward without GSR_FLAG_PREZERO_GRADS on a workspace of exactly
    gsr_workspace_layout().total poisoned bytes: the same images as the wrapper's two-phase form, the gradients within the 2e-5 of the
    prezero-vs-memset test, and nothing written behind the workspace"""
    rz = raster_debug
    from styl3r_amd import _lib
    lib = _lib.load()
    want = _raster_step(rz, raster)
    (mn, c6, op, sh), *_ = raster.leaves(False)
    G, V, cap = raster.G, 2, 1 << 16
    gI, gD = torch.tensor(raster.wI, device=DEV), torch.tensor(raster.wD, device=DEV)
    for pattern in PATTERNS[1:]:
        dims = _lib.GsrDims(1, 2, G, RH, RW, 4, RSH, _lib.GSR_FLAG_NTOUCHED, None)
        L = _lib.workspace_layout(dims, cap)
        ws, intact = guarded(L.total, pattern=pattern)
        nan = lambda *s: torch.full(s, float("nan"), device=DEV)
        img, dep, opa = nan(V, 3, RH, RW), nan(V, RH, RW), nan(V, RH, RW)
        radii, ntouch, status = (torch.full(s, -1, dtype=I32, device=DEV) for s in ((V, G), (V, G), (8,)))
        rc = lib.gsr_forward(C.byref(dims), raster.views.data_ptr(), mn.data_ptr(), c6.data_ptr(), op.data_ptr(), sh.data_ptr(), cap,
                             ws.data_ptr(), L.total, img.data_ptr(), dep.data_ptr(), opa.data_ptr(), radii.data_ptr(), ntouch.data_ptr(),
                             status.data_ptr(), _stream())
        assert rc == 0
        d = [nan(1, G, 3), nan(1, G, 6), nan(1, G), nan(1, G, 4, 3), nan(V, G, 3), nan(V, 6)]
        rc = lib.gsr_backward(C.byref(dims), raster.views.data_ptr(), mn.data_ptr(), c6.data_ptr(), sh.data_ptr(), cap, ws.data_ptr(), L.total,
                              gI.data_ptr(), gD.data_ptr(), *(t.data_ptr() for t in d), _stream())
        assert rc == 0
        torch.cuda.synchronize()
        intact()
        assert int(status[1]) == 0 and int(status[0]) == int(want["pairs"])
        for got, k in ((img, "image"), (dep, "depth"), (opa, "opacity"), (radii, "radii"), (ntouch, "n_touched")):
            assert torch.equal(got, want[k]), (pattern, k)
        for got, k in zip(d[:5], ("means3D", "cov6", "opacities", "shs", "means2D")):
            assert bool(torch.isfinite(got).all()), k
            assert_close_rel(got.cpu().numpy(), want["d_" + k].cpu().numpy(), 2e-5, f"C ABI d{k}")
        tau = torch.cat((want["d_rho"], want["d_theta"]), 1)
        assert_close_rel(d[5].cpu().numpy(), tau.cpu().numpy(), 5e-4, "C ABI dtau")
        own = dict(zip(("d_means3D", "d_cov6", "d_opacities", "d_shs", "d_means2D"), d[:5]), d_rho=d[5][:, 0:3], d_theta=d[5][:, 3:6])
        _check_raster_grads(raster, own)                    # ... and against the oracle itself, at the bars of the wrapper's test


# =====================================================================================================================
# Losses
# =====================================================================================================================
@pytest.mark.parametrize("n", [5, 4 * 256 * 3 + 3])
def test_mse_kernels(n):
    """gsr_mse_forward / _backward: a float4 walk with a ragged tail.  The ticket scratch the wrapper keeps is a zero-on-entry contract
    (torch.zeros, re-armed by the kernel) and is not poisoned; the loss scalar and the gradient are."""
    from styl3r_amd.losses import mse_loss
    g = torch.Generator(DEV).manual_seed(n)
    pred, target = torch.rand(n, device=DEV, generator=g).requires_grad_(True), torch.rand(n, device=DEV, generator=g)

    def op():
        loss = mse_loss(pred, target, 0.7)
        return dict(loss=loss, grad=torch.autograd.grad(loss * 1.5, pred)[0])
    runs = three_runs(op, expect=[dict(shape=(), dtype=F32), dict(shape=(n,), dtype=F32)])
    assert_identical(runs)
    want = 0.7 * ((pred.detach().double() - target.double()) ** 2).mean()
    assert abs(float(runs["zero"]["loss"]) - float(want)) <= 2e-6 * float(want)
    assert torch.allclose(runs["zero"]["grad"].double(), 1.5 * 0.7 * 2 / n * (pred.detach().double() - target.double()), rtol=1e-6, atol=1e-12)


@pytest.mark.parametrize("shape", [(1, 1, 43, 75), (3, 1, 11, 11)])
def test_image_scores_and_ssim_structure(shape):
    from styl3r_amd import _lib, metrics
    from styl3r_amd.losses import ssim_structure_per_image
    lib = _lib.load()
    n, c, h, w = shape
    g = torch.Generator(DEV).manual_seed(h)
    gt, pred = torch.rand(shape, device=DEV, generator=g), torch.rand(shape, device=DEV, generator=g).requires_grad_(True)
    wts = torch.randn(n, device=DEV, generator=g)
    nb_scores, nb_ssim = lib.gsr_image_scores_scratch_bytes(n, c, h, w), lib.gsr_ssim_structure_scratch_bytes(n, c, h, w)

    def op():
        ssim, mse = metrics._scores_hip(gt, pred)
        s = ssim_structure_per_image(gt, pred)
        return dict(ssim=ssim, mse=mse, structure=s, grad=torch.autograd.grad((s * wts).sum(), pred)[0])
    runs = three_runs(op, expect=[dict(nbytes=nb_scores, dtype=U8), dict(nbytes=nb_ssim, dtype=U8), dict(shape=(n,), dtype=F32),
                                  dict(shape=(3, n * c * (h - 10) * (w - 10)), dtype=F32), dict(shape=shape, dtype=F32)])
    assert_identical(runs)
    # the C ABI on scratches of exactly the stated sizes
    z = runs["zero"]
    for pattern in PATTERNS[1:]:
        sc, intact = guarded(nb_scores, pattern=pattern)
        ssim, mse = (torch.full((n,), float("nan"), device=DEV) for _ in range(2))
        assert lib.gsr_image_scores(gt.data_ptr(), pred.data_ptr(), n, c, h, w, ssim.data_ptr(), mse.data_ptr(), sc.data_ptr(), _stream()) == 0
        sc2, intact2 = guarded(nb_ssim, pattern=pattern)
        st = torch.full((n,), float("nan"), device=DEV)
        from styl3r_amd.losses import _window_c
        assert lib.gsr_ssim_structure_fwd(gt.data_ptr(), pred.data_ptr(), n, c, h, w, _window_c(), st.data_ptr(), None, sc2.data_ptr(), _stream()) == 0
        torch.cuda.synchronize()
        intact(); intact2()
        assert torch.equal(ssim, z["ssim"]) and torch.equal(mse, z["mse"]) and torch.equal(st, z["structure"])


@pytest.mark.parametrize("second,with_image", [(False, True), (True, True), (True, False)])
def test_depth_smoothness(second, with_image):
    from styl3r_amd import _lib, losses
    H, W = 13, 37                                           # ragged against the 128 x 8 tiles
    g = torch.Generator(DEV).manual_seed(7)
    depth = (torch.rand(1, 2, H, W, device=DEV, generator=g) * 3 + 0.2).requires_grad_(True)
    near, far = torch.tensor([[1.2, 1.5]], device=DEV), torch.tensor([[9.0, 20.0]], device=DEV)
    image = torch.rand(1, 2, 3, H, W, device=DEV, generator=g) if with_image else None
    nb = _lib.load().gsr_depth_smooth_scratch_bytes(2, H, W)

    def op():
        loss = losses.depth_smoothness(depth, near, far, image, 0.25, 1.5 if with_image else None, second)
        return dict(loss=loss, grad=torch.autograd.grad(loss, depth)[0])
    runs = three_runs(op, expect=[dict(nbytes=nb, dtype=U8), dict(shape=(1, 2, H, W), dtype=F32)], before=losses._DEPTH_SCRATCH.clear)
    assert_identical(runs)
    losses._DEPTH_SCRATCH.clear()
    sc, intact = guarded(nb)
    out = torch.full((), float("nan"), device=DEV)
    rc = _lib.load().gsr_depth_smooth_fwd(depth.data_ptr(), image.data_ptr() if with_image else None, near.data_ptr(), far.data_ptr(), 2, H, W,
                                          0.25, 1.5 if with_image else 0.0, int(second), sc.data_ptr(), out.data_ptr(), _stream())
    torch.cuda.synchronize()
    intact()
    assert rc == 0 and torch.equal(out, runs["zero"]["loss"])


@pytest.mark.parametrize("hw,clip", [((20, 30), None), ((90, 100), None), ((20, 30), 2.5)])
def test_regr3d(hw, clip):
    """N = 600: one workgroup per map selects in LDS; N = 9000: the eight launches of the radix selection, whose histograms the host entry
    zeroes.  Invalid pixels (low confidence, outside the quantiles) and one map without any valid point."""
    from styl3r_amd import _lib
    from styl3r_amd.points import regr3d_hip
    B, (h, w) = 2, hw
    N = h * w
    g = torch.Generator(DEV).manual_seed(N)
    R = lambda *s: torch.randn(*s, device=DEV, generator=g)
    gt1, gt2 = R(B, h, w, 3) + 2.0, R(B, h, w, 3) - 1.5
    pr1, pr2 = (gt1 + 0.1 * R(B, h, w, 3)).requires_grad_(True), (gt2 + 0.1 * R(B, h, w, 3)).requires_grad_(True)
    conf1, conf2 = 3.0 + R(B, h, w), 3.0 + R(B, h, w)
    if clip is None:
        conf1[1] = 0.0                                      # view 1, image 1: nothing valid
    else:
        gt1[1] = gt1[1] * 0 + 50.0                          # beyond dist_clip
    nb = _lib.load().gsr_regr3d_scratch_bytes(B, N)

    def op():
        det = {}
        loss = regr3d_hip(gt1, gt2, pr1, pr2, conf1, conf2, True, dist_clip=clip, details=det)
        d1, d2 = torch.autograd.grad(loss * 1.3, (pr1, pr2))
        return dict(loss=loss, d1=d1, d2=d2, **det)
    runs = three_runs(op, expect=[dict(nbytes=nb, dtype=U8), dict(shape=(2, B, 2), dtype=I32), dict(shape=(2, B, N), dtype=U8),
                                  dict(shape=(B, h, w, 3), dtype=F32)])
    assert_identical(runs)
    z = runs["zero"]
    assert int(z["status"][0, 1, 0]) == 0 and int(z["status"][0, 1, 1]) & _lib.GSR_PT_EMPTY_MAP
    assert int(z["status"][0, 0, 0]) > 0 and float(z["d1"][1].abs().max()) == 0.0 and float(z["d1"][0].abs().max()) > 0
    sc, intact = guarded(nb)
    loss, status = torch.full((), float("nan"), device=DEV), torch.full((2, B, 2), -1, dtype=I32, device=DEV)
    rc = _lib.load().gsr_regr3d_fwd(gt1.data_ptr(), gt2.data_ptr(), conf1.data_ptr(), conf2.data_ptr(), pr1.data_ptr(), pr2.data_ptr(), 3 * N, 3 * N,
                                    B, N, 1, 0, float(clip or 0.0), sc.data_ptr(), loss.data_ptr(), status.data_ptr(), None, None, _stream())
    torch.cuda.synchronize()
    intact()
    assert rc == 0 and torch.equal(loss, z["loss"]) and torch.equal(status, z["status"])


def test_pointmap_post():
    from styl3r_amd.points import pointmap_post
    raw = torch.randn(2, 4, 5, 7, device=DEV, generator=torch.Generator(DEV).manual_seed(1))
    runs = three_runs(lambda: pointmap_post(raw), expect=[dict(shape=(2, 5, 7, 3), dtype=F32), dict(shape=(2, 5, 7), dtype=F32)])
    assert_identical(runs)


# =====================================================================================================================
# Scene-level entries
# =====================================================================================================================
def test_view_overlap():
    from styl3r_amd import _lib, views
    V, H, W = 3, 17, 23
    ext = torch.eye(4, device=DEV).repeat(V, 1, 1)
    ext[1, 0, 3], ext[2, 2, 3], ext[2, 0, 3] = 0.4, -0.6, -0.2
    K = torch.tensor([[0.9, 0, 0.5], [0, 0.8, 0.5], [0, 0, 1.0]], device=DEV).repeat(V, 1, 1)
    pairs = torch.tensor([[0, 1], [2, 0], [1, 1], [0, 7], [-1, 2]], dtype=I32, device=DEV)
    nb = _lib.load().gsr_view_overlap_scratch_bytes(V, pairs.shape[0])
    runs = three_runs(lambda: dict(counts=views.view_overlap_device(ext, K, pairs, (H, W))),
                      expect=[dict(nbytes=nb, dtype=torch.float64), dict(shape=(5, 2), dtype=I32)])
    assert_identical(runs)
    z = runs["zero"]["counts"]
    assert z[3:].tolist() == [[-1, -1], [-1, -1]] and int(z[:3].min()) >= 0 and int(z[:3].max()) <= H * W and int(z[:2].max()) > 0
    assert torch.equal(z[:3].cpu(), views.overlap_counts_torch(ext.cpu(), K.cpu(), pairs[:3].cpu(), (H, W)).to(I32))
    sc, intact = guarded(nb)
    counts = torch.full((5, 2), 12345, dtype=I32, device=DEV)
    rc = _lib.load().gsr_view_overlap(ext.data_ptr(), K.data_ptr(), V, pairs.data_ptr(), 5, H, W, sc.data_ptr(), nb, counts.data_ptr(), _stream())
    torch.cuda.synchronize()
    intact()
    assert rc == 0 and torch.equal(counts, z)


def test_pnp_ransac():
    """64 x 64; problem 0 is solvable, problem 1 has fewer than six masked points (code 1: identity, empty mask)"""
    from styl3r_amd import _lib
    from styl3r_amd.pose_align import pnp_pose
    h = w = 64
    g = torch.Generator(DEV).manual_seed(2)
    K = torch.tensor([[0.9, 0, 0.5], [0, 0.9, 0.5], [0, 0, 1.0]], device=DEV).repeat(2, 1, 1)
    ys, xs = torch.meshgrid(torch.arange(h, device=DEV, dtype=F32), torch.arange(w, device=DEV, dtype=F32), indexing="ij")
    depth = 2.0 + torch.rand(2, h, w, device=DEV, generator=g)
    cam = torch.stack(((xs / w - 0.5) / 0.9 * depth, (ys / h - 0.5) / 0.9 * depth, depth), -1)          # identity pose: world = camera
    cam = cam + 0.002 * torch.randn(cam.shape, device=DEV, generator=g)
    opac = torch.rand(2, h, w, device=DEV, generator=g)
    opac[1] = 0.0
    opac[1, 3, :5] = 0.9
    nb = _lib.load().gsr_pnp_ransac_scratch_bytes(2, h, w, 100)

    def op():
        c2w, st = pnp_pose(cam, opac, K, (h, w), seed=5)
        return dict(c2w=c2w, **st)
    runs = three_runs(op, expect=[dict(nbytes=nb, dtype=U8), dict(shape=(2, 4, 4), dtype=F32), dict(shape=(2, h * w), dtype=U8), dict(shape=(2, 4), dtype=I32)])
    assert_identical(runs)
    z = runs["zero"]
    assert z["code"].tolist() == [0, 1] and z["masked"].tolist()[1] == 5 and int(z["winner"][1]) == -1 and int(z["inliers"][0]) > 1000
    assert torch.equal(z["c2w"][1], torch.eye(4, device=DEV)) and not bool(z["inlier_mask"][1].any())
    assert float((z["c2w"][0] - torch.eye(4, device=DEV)).abs().max()) < 5e-2
    Kp = K.clone(); Kp[:, 0] *= w; Kp[:, 1] *= h
    pts, op2 = cam.reshape(2, -1, 3).contiguous(), opac.reshape(2, -1).contiguous()
    sc, intact = guarded(nb, pattern="garbage")
    c2w, status = torch.full((2, 4, 4), float("nan"), device=DEV), torch.full((2, 4), 77, dtype=I32, device=DEV)
    rc = _lib.load().gsr_pnp_ransac(pts.data_ptr(), op2.data_ptr(), Kp.data_ptr(), 2, h, w, h * w, 0.3, 5.0, 100, 5, 0.0, c2w.data_ptr(), None,
                                    status.data_ptr(), sc.data_ptr(), _stream())
    torch.cuda.synchronize()
    intact()
    assert rc == 0 and torch.equal(c2w, z["c2w"]) and status[:, 3].tolist() == [0, 1]


def test_resample_crop_staged_and_direct():
    from styl3r_amd import _lib, inputs
    src = torch.randint(0, 256, (2, 37, 53, 3), dtype=U8, device=DEV, generator=torch.Generator(DEV).manual_seed(3))
    scaled, window = (19, 29), (2, 3, 15, 21)               # 21 output columns: the byte rows between the passes carry 3 pad bytes
    nb = _lib.load().gsr_resample_scratch_bytes(2, 37, 53, 19, 29, 2, 3, 15, 21)

    def op():
        return dict(staged=inputs.resample_crop(src, scaled, window, flip=[True, False]),
                    direct=inputs.resample_crop(src, scaled, window, flip=[True, False], flags=_lib.GSR_RESAMPLE_DIRECT))
    runs = three_runs(op, expect=[dict(nbytes=nb, dtype=U8), dict(shape=(2, 3, 15, 21), dtype=F32)])
    assert_identical(runs)
    z = runs["zero"]
    assert torch.equal(z["staged"], z["direct"])
    assert torch.equal(z["staged"].cpu(), inputs.resample_crop(src.cpu(), scaled, window, flip=[True, False]))
    px, py = inputs._device_plan(53, 29, torch.device(DEV)), inputs._device_plan(37, 19, torch.device(DEV))
    flip = torch.tensor([1, 0], dtype=I32, device=DEV)
    sc, intact = guarded(nb)
    out = torch.full((2, 3, 15, 21), float("nan"), device=DEV)
    rc = _lib.load().gsr_resample_crop(src.data_ptr(), 0, 2, 37, 53, px.data_ptr(), 29, py.data_ptr(), 19, 2, 3, 15, 21, flip.data_ptr(),
                                       sc.data_ptr(), nb, out.data_ptr(), 0, _stream())
    torch.cuda.synchronize()
    intact()
    assert rc == 0 and torch.equal(out, z["staged"])


def test_undistort():
    from styl3r_amd import colmap
    frames = torch.randint(0, 256, (2, 37, 53, 3), dtype=U8, device=DEV, generator=torch.Generator(DEV).manual_seed(4))
    K = np.array([[40.0, 0, 26.2], [0, 41.0, 18.4], [0, 0, 1]])
    cams = [colmap.UndistortCamera(K, np.array([0.12, -0.05, 0.002, -0.001]), new_K=K, roi=(1, 2, 50, 33)), colmap.UndistortCamera(K, roi=(-2, 5, 50, 33))]
    runs = three_runs(lambda: dict(out=colmap.undistort_frames(frames, cams, [0, 1])), expect=[dict(shape=(2, 33, 50, 3), dtype=U8)])
    assert_identical(runs)
    assert torch.equal(runs["zero"]["out"].cpu(), colmap.undistort_frames(frames.cpu(), cams, [0, 1]))


def test_depth_range_and_ply_normalizer():
    from styl3r_amd import _lib, export
    g = torch.Generator(DEV).manual_seed(6)
    depth = torch.randn(5000, device=DEV, generator=g) * 2 + 1.0                        # a third of them negative
    means = torch.randn(4099, 3, device=DEV, generator=g) * torch.tensor([1.0, 5.0, 0.2], device=DEV)
    nb = _lib.load().gsr_outputs_scratch_bytes()

    def op():
        det = {}
        rng = export.depth_range(depth, details=det)
        none = export.depth_range(-depth.abs())                                        # no positive depth: near = 0
        return dict(range=rng, status=det["status"], quantiles=det["quantiles"], no_positive=none[:1], normalizer=export.ply_normalizer(means))
    runs = three_runs(op, expect=[dict(nbytes=nb, dtype=U8), dict(shape=(4,), dtype=F32), dict(shape=(2,), dtype=I32)])
    assert_identical(runs)
    z = runs["zero"]
    want = torch.stack([depth[depth > 0].quantile(0.01).log(), depth.quantile(0.99).log()])
    assert torch.allclose(z["range"], want, rtol=1e-6) and float(z["no_positive"]) == 0.0
    med = means.median(0).values
    assert torch.equal(z["normalizer"][:3], med) and float(z["normalizer"][3]) > 0
    sc, intact = guarded(nb)
    out = torch.full((4,), float("nan"), device=DEV)
    rc = _lib.load().gsr_ply_normalizer(means.data_ptr(), means.shape[0], sc.data_ptr(), out.data_ptr(), _stream())
    torch.cuda.synchronize()
    intact()
    assert rc == 0 and torch.equal(out, z["normalizer"])


# =====================================================================================================================
# ViT kernels
# =====================================================================================================================
@pytest.mark.parametrize("shape", [(5, 256), (33, 768)])
def test_layernorm_forward_backward_and_skip(shape):
    from styl3r_amd import vit_ops
    torch.manual_seed(shape[0])
    M, Cn = shape
    m = vit_ops.LayerNorm(Cn, eps=1e-6).to(DEV)
    with torch.no_grad():
        m.weight.copy_(1 + 0.3 * torch.randn(Cn, device=DEV)); m.bias.copy_(0.2 * torch.randn(Cn, device=DEV))
    x = (3 * torch.randn(shape, device=DEV) + 0.7).requires_grad_(True)
    gy, gs = torch.randn(shape, device=DEV), torch.randn(shape, device=DEV)
    nb = vit_ops.load().vit_layernorm_scratch_bytes(M, Cn)

    def op():
        y = m(x)
        dx, dg, db = torch.autograd.grad((y * gy).sum(), (x, m.weight, m.bias))
        ys, xs = m.forward_skip(x)
        sx, sg, sb = torch.autograd.grad((ys * gy).sum() + (xs * gs).sum(), (x, m.weight, m.bias))
        return dict(y=y, dx=dx, dgamma=dg, dbeta=db, y_skip=ys, dx_skip=sx, dgamma_skip=sg, dbeta_skip=sb)
    runs = three_runs(op, expect=[dict(nbytes=nb, dtype=U8), dict(shape=(2, M), dtype=F32), dict(shape=(2, Cn), dtype=F32), dict(shape=shape, dtype=F32)])
    assert_identical(runs)
    z = runs["zero"]
    xd = x.detach().double().requires_grad_(True)
    wd, bd = m.weight.detach().double().requires_grad_(True), m.bias.detach().double().requires_grad_(True)
    ref = torch.nn.functional.layer_norm(xd, (Cn,), wd, bd, 1e-6)
    (ref * gy.double()).sum().backward()
    assert rel_err(z["y"], ref.detach()) <= 2e-6 and rel_err(z["dx"], xd.grad) <= 5e-6 and rel_err(z["dx_skip"], xd.grad + gs.double()) <= 5e-6
    assert rel_err(z["dgamma"], wd.grad) <= 1e-5 and rel_err(z["dbeta"], bd.grad) <= 1e-5
    # the C ABI of the backward on a scratch of exactly the stated size
    lib = vit_ops.load()
    mean, rstd, y = torch.empty(M, device=DEV), torch.empty(M, device=DEV), torch.empty(shape, device=DEV)
    assert lib.vit_layernorm_fwd(x.data_ptr(), m.weight.data_ptr(), m.bias.data_ptr(), y.data_ptr(), mean.data_ptr(), rstd.data_ptr(), M, Cn, 1e-6, _stream()) == 0
    sc, intact = guarded(nb)
    dx, dg, db = (torch.full(s, float("nan"), device=DEV) for s in (shape, (Cn,), (Cn,)))
    rc = lib.vit_layernorm_bwd(gy.data_ptr(), x.data_ptr(), mean.data_ptr(), rstd.data_ptr(), m.weight.data_ptr(), None, dx.data_ptr(), dg.data_ptr(),
                               db.data_ptr(), sc.data_ptr(), M, Cn, 0, _stream())
    torch.cuda.synchronize()
    intact()
    assert rc == 0 and torch.equal(dx, z["dx"]) and torch.equal(dg, z["dgamma"]) and torch.equal(db, z["dbeta"])


def test_grouped_layernorm_forward():
    from styl3r_amd import vit_ops
    torch.manual_seed(3)
    norms = [vit_ops.LayerNorm(768, eps=1e-6).to(DEV) for _ in range(2)]
    with torch.no_grad():
        for n in norms:
            n.weight.copy_(1 + 0.3 * torch.randn(768, device=DEV)); n.bias.copy_(0.2 * torch.randn(768, device=DEV))
        x = 2 * torch.randn(2, 33, 768, device=DEV) - 0.3
        runs = three_runs(lambda: dict(y=vit_ops.grouped_layernorm(x, norms), y_flip=vit_ops.grouped_layernorm(x, norms, flip=True)),
                          expect=[dict(shape=(2, 33, 768), dtype=F32)])
    assert_identical(runs)
    for g in range(2):
        ref = torch.nn.functional.layer_norm(x[g].double(), (768,), norms[g].weight.double(), norms[g].bias.double(), 1e-6)
        assert rel_err(runs["zero"]["y"][g], ref) <= 2e-6


# The split rules of the host entries, restated (csrc/vit_gemm_x6.hip as of this commit: linear_x6_fwd :1165-1180, wgrad_splits :1211-1226,
# conv_x6_fwd :1275-1297; tiles are 128 rows, slabs 16 deep).  The cases below assert with them that their shapes still reach the
# zero-filled / memset split paths: a heuristic that changes must be changed here too, and a shape that no longer splits fails its test.
def _cdiv(a, b):
    return -(-a // b)


def linear_fwd_splits(M, N, K):
    tm = _cdiv(M, 128)
    narrow = tm * _cdiv(N, 128) < 640
    tiles, S, nk = tm * (_cdiv(N, 64) if narrow else _cdiv(N, 128)), 1, K // 16
    if tiles <= 200:                                        # (act == 0 and no pre-activation store: the cases here)
        while S < 8 and tiles * S * 2 <= 768 and nk // (S * 2) >= 8:
            S *= 2
    return S


def linear_wgrad_splits(M, N, K):
    tiles, nslab, t = _cdiv(N, 128) * _cdiv(K, 128), _cdiv(M, 16), (0.0, 0.95, 1.62, 2.48)      # six products
    best, best_cost = 1, 1e30
    for S in range(1, 65):
        if S > 1 and nslab // S < 8:
            break
        per_cu, chain = tiles * S / 256.0, _cdiv(nslab, S) + 8.0
        c = 1 if per_cu <= 1 else (2 if per_cu <= 2 else 3)
        cost = max(chain * t[c], per_cu * chain * 0.5 * t[2]) + S
        if cost < best_cost:
            best, best_cost = S, cost
    return best


def conv3_fwd_route(B, Ci, Co, H, W):
    """('halo' | 'taps', S) of a 3 x 3 vit_conv_x6_fwd launch"""
    if W >= 32:
        ht, nslab, S = _cdiv(Co, 128) * B * _cdiv(W, 32) * _cdiv(H, 4), Ci // 16, 1
        if ht < 256:
            S = 512 // ht
            while S > 1 and nslab // S < 2:
                S -= 1
            S = min(max(S, 1), 8)
        return "halo", S
    tiles, nslab, S = _cdiv(Co, 128) * _cdiv(B * H * W, 128), 9 * Ci // 16, 1
    if tiles < 256:
        S = 512 // tiles
        while S > 1 and nslab // S < 8:
            S -= 1
        S = min(max(S, 1), 16)
    return "taps", S


def _linear_case(M, N, K, seed):
    g = torch.Generator(DEV).manual_seed(seed)
    x = torch.randn(M, K, device=DEV, generator=g).requires_grad_(True)
    w = (torch.randn(N, K, device=DEV, generator=g) / K ** 0.5).requires_grad_(True)
    b = torch.randn(N, device=DEV, generator=g).requires_grad_(True)
    gy = torch.randn(M, N, device=DEV, generator=g)
    xd, wd, bd = (t.detach().double().requires_grad_(True) for t in (x, w, b))
    ref = torch.nn.functional.linear(xd, wd, bd)
    (ref * gy.double()).sum().backward()
    return x, w, b, gy, dict(y=ref.detach(), dx=xd.grad, dw=wd.grad, db=bd.grad)


@pytest.mark.parametrize("M,N,K", [(130, 80, 80),        # ragged against every tile; unsplit forward, one weight-gradient split
                                   (64, 64, 4096),       # one output tile, 256 K slabs: the forward splits K (zero fill + atomics)
                                   (2048, 80, 80)])      # 128 row slabs on one tile: the weight gradient splits M (memset + atomics)
def test_fused_linear_forward_and_gradients(M, N, K):
    """sums ordered by atomics where a contraction is split: every run meets the bars of test_fused_linear_vs_fp64 against float64"""
    from styl3r_amd import vit_ops
    routes = (linear_fwd_splits(M, N, K), linear_fwd_splits(M, K, N), linear_wgrad_splits(M, N, K))       # forward, dX, dW
    assert routes[:2] == {(130, 80, 80): (1, 1), (64, 64, 4096): (8, 1), (2048, 80, 80): (1, 1)}[(M, N, K)], routes
    assert (routes[2] > 1) == ((M, N, K) == (2048, 80, 80)), routes                                       # (the cost model picks 10 there)
    assert vit_ops._linear_cfg(M, N, K) == 0 and vit_ops._linear_cfg(M, N, K, dx=True) == 0               # vit_linear_x6_fwd, not a ring / small-M kernel
    x, w, b, gy, ref = _linear_case(M, N, K, M + N + K)

    def op():
        y = vit_ops.fused_linear(x, w, b)
        dx, dw, db = torch.autograd.grad((y * gy).sum(), (x, w, b))
        return dict(y=y, dx=dx, dw=dw, db=db)
    runs = three_runs(op, expect=[dict(shape=(M, N), dtype=F32), dict(shape=(M, K), dtype=F32), dict(nbytes=(N * K + N) * 4, dtype=F32)])
    for pattern in PATTERNS:
        for k, bar in (("y", 4e-6), ("dx", 1e-5), ("dw", 1e-5), ("db", 1e-5)):
            err = rel_err(runs[pattern][k], ref[k])
            assert err <= bar, (pattern, k, err)


def test_small_m_kernel_serving_path():
    from styl3r_amd import vit_ops
    M, N, K = 257, 768, 1024
    x, w, b, _, ref = _linear_case(M, N, K, 5)
    assert vit_ops.small_m_kernel(M, N, K)
    with torch.no_grad():
        runs = three_runs(lambda: dict(y=vit_ops.fused_linear(x.detach(), w.detach(), b.detach())), expect=[dict(shape=(M, N), dtype=F32)])
    for pattern in PATTERNS:
        assert rel_err(runs[pattern]["y"], ref["y"]) <= 4e-6, pattern


@pytest.mark.parametrize("M", [130, 2048])                 # one split (dw stored, db memset) / several (memset + atomics)
def test_linear_weight_gradient_c_abi_bias_layouts(M):
    """vit_linear_x6_wgrad: `dbias` right behind `dw` (one memset covers both when M is split) and in a buffer of its own, on poisoned
    outputs; vit_linear_x6_wgrad_acc: adds to a running gradient.  Bars of test_linear_weight_gradient_kernel_ragged_shapes_vs_fp64."""
    from styl3r_amd import vit_ops
    N, K = 80, 80
    assert (linear_wgrad_splits(M, N, K) > 1) == (M == 2048)
    vit_ops._x6()
    lib = vit_ops.load()
    g = torch.Generator(DEV).manual_seed(M)
    x, dy = torch.randn(M, K, device=DEV, generator=g), torch.randn(M, N, device=DEV, generator=g)
    want_w, want_b = dy.double().t() @ x.double(), dy.double().sum(0)
    run_w, run_b = torch.randn(N, K, device=DEV, generator=g), torch.randn(N, device=DEV, generator=g)
    for pattern in PATTERNS:
        for joined in (True, False):
            for acc in (False, True):
                if joined:
                    buf, intact = guarded((N * K + N) * 4, pattern=pattern)
                    dw, db, checks = buf[:N * K * 4].view(F32).view(N, K), buf[N * K * 4:].view(F32), (intact,)
                else:
                    bw, iw = guarded(N * K * 4, pattern=pattern)
                    bb, ib = guarded(N * 4, pattern=pattern)
                    dw, db, checks = bw.view(F32).view(N, K), bb.view(F32), (iw, ib)
                if acc:
                    dw.copy_(run_w); db.copy_(run_b)
                fn = lib.vit_linear_x6_wgrad_acc if acc else lib.vit_linear_x6_wgrad
                assert fn(dy.data_ptr(), x.data_ptr(), dw.data_ptr(), db.data_ptr(), M, N, K, _stream()) == 0
                torch.cuda.synchronize()
                for c in checks:
                    c()
                ew = float((dw.double() - (want_w + (run_w.double() if acc else 0))).abs().max() / want_w.abs().max())
                eb = float((db.double() - (want_b + (run_b.double() if acc else 0))).abs().max() / want_b.abs().max())
                assert ew <= 4e-6 and eb <= 4e-6, (pattern, joined, acc, ew, eb)


def test_linear_x6c_split_workspace_and_tickets():
    """vit_linear_x6c_fwd with 3 K splits: the partial tiles meet in a poisoned workspace, the tickets behind them are zeroed by the entry
    and re-armed by the kernel (two launches on one workspace)"""
    from styl3r_amd import vit_ops
    M, N, K = 300, 200, 96
    x, w, b, _, ref = _linear_case(M, N, K, 9)
    lib = vit_ops.load()
    blk = vit_ops.split_weight_block(w.detach())
    nb = lib.vit_linear_x6c_workspace_bytes(M, N, 3)
    assert nb > 0
    for pattern in PATTERNS:
        ws, intact = guarded(nb, pattern=pattern)
        for rep in range(2):
            out = torch.full((M, N), float("nan"), device=DEV)
            rc = lib.vit_linear_x6c_fwd(x.data_ptr(), blk.data_ptr(), b.data_ptr(), None, out.data_ptr(), None, M, N, K, 0, 3, ws.data_ptr(), nb, _stream())
            torch.cuda.synchronize()
            intact()
            assert rc == 0 and bool(torch.isfinite(out).all()) and rel_err(out, ref["y"]) <= 4e-6, (pattern, rep)


@pytest.mark.parametrize("B,Ci,Co,H,W", [(2, 32, 64, 9, 13),      # tap kernel, 2 output tiles: the K slabs are split in two (zero fill + atomics)
                                         (2, 32, 64, 37, 45),     # halo kernel, ragged patches (H % 4, W % 32 != 0), unsplit
                                         (1, 64, 96, 4, 32)])     # halo kernel, one tile: the channel slabs are split in two
def test_conv_x6_forward_and_gradients(B, Ci, Co, H, W, monkeypatch):
    """forward and input gradient on vit_conv_x6_fwd, the weight gradient of these small maps through vit_im2col3_rows +
    vit_linear_x6_wgrad; bars of test_conv_x6_matches_fp64_forward_and_backward"""
    from styl3r_amd import vit_ops
    monkeypatch.setattr(vit_ops, "_CONV_X6_MIN_ROWS", 16)          # the input gradient on the own kernel at these channel counts
    routes = (conv3_fwd_route(B, Ci, Co, H, W), conv3_fwd_route(B, Co, Ci, H, W))                        # forward, dX (channels exchanged)
    assert routes == {(2, 32, 64, 9, 13): (("taps", 2), ("taps", 4)), (2, 32, 64, 37, 45): (("halo", 1), ("halo", 2)),
                      (1, 64, 96, 4, 32): (("halo", 2), ("halo", 3))}[(B, Ci, Co, H, W)], routes
    torch.manual_seed(B * 100 + Ci)
    conv = torch.nn.Conv2d(Ci, Co, 3, 1, 1).to(DEV)
    x = torch.randn(B, Ci, H, W, device=DEV, requires_grad=True)
    gy = torch.randn(B, Co, H, W, device=DEV)
    xd, wd, bd = (t.detach().double().requires_grad_(True) for t in (x, conv.weight, conv.bias))
    ref = torch.nn.functional.conv2d(xd, wd, bd, padding=1)
    (ref * gy.double()).sum().backward()
    ref = dict(y=ref.detach(), dx=xd.grad, dw=wd.grad, db=bd.grad)
    before = dict(vit_ops.CALLS)

    def op():
        y = vit_ops._ConvX6.apply(x, conv.weight, conv.bias)
        dx, dw, db = torch.autograd.grad((y * gy).sum(), (x, conv.weight, conv.bias))
        return dict(y=y, dx=dx, dw=dw, db=db)
    runs = three_runs(op, expect=[dict(shape=(B, Co, H, W), dtype=F32), dict(shape=(B, Ci, H, W), dtype=F32), dict(shape=(B * H * W, 9 * Ci), dtype=F32),
                                  dict(nbytes=(Co * 9 * Ci + Co) * 4, dtype=F32)])
    took = {k: vit_ops.CALLS[k] - before[k] for k in ("conv_x6_fwd", "conv_x6_dx", "conv_wgrad_via_linear", "library_conv_bwd")}
    assert took == dict(conv_x6_fwd=3, conv_x6_dx=3, conv_wgrad_via_linear=3, library_conv_bwd=0), took
    for pattern in PATTERNS:
        for k, bar in (("y", 5e-6), ("dx", 5e-6), ("dw", 2e-5), ("db", 2e-5)):
            err = rel_err(runs[pattern][k], ref[k])
            assert err <= bar, (pattern, k, err)


def test_conv_split_pixel_weight_gradient_at_its_minimum_pixel_count():
    """16 x 64 x 64 = 65 536 pixels: the first size at which Conv2dX6's backward takes vit_conv_x6_wgrad (memset + atomics)"""
    from styl3r_amd import vit_ops
    B, Ci, Co, H, W = 16, 32, 64, 64, 64
    assert B * H * W == vit_ops._CONV_X6_WGRAD_MIN_PIXELS
    torch.manual_seed(B + Ci)
    conv = torch.nn.Conv2d(Ci, Co, 3, 1, 1).to(DEV)
    x, gy = torch.randn(B, Ci, H, W, device=DEV), torch.randn(B, Co, H, W, device=DEV)
    wd, bd = conv.weight.detach().double().requires_grad_(True), conv.bias.detach().double().requires_grad_(True)
    (torch.nn.functional.conv2d(x.double(), wd, bd, padding=1) * gy.double()).sum().backward()
    before = vit_ops.CALLS["conv_x6_wgrad"]

    def op():
        y = vit_ops._ConvX6.apply(x, conv.weight, conv.bias)
        dw, db = torch.autograd.grad((y * gy).sum(), (conv.weight, conv.bias))
        return dict(dw=dw, db=db)
    runs = three_runs(op, expect=[dict(shape=(Co, Ci, 3, 3), dtype=F32), dict(shape=(Co,), dtype=F32)])
    assert vit_ops.CALLS["conv_x6_wgrad"] - before == 3
    for pattern in PATTERNS:                                # bars of test_conv_x6_weight_gradient_kernel_matches_fp64
        assert rel_err(runs[pattern]["dw"], wd.grad) <= 5e-6 and rel_err(runs[pattern]["db"], bd.grad) <= 5e-6, pattern


@pytest.mark.parametrize("shape", [(3, 4, 1, 2), (2, 16, 64, 64)])       # the generic kernels / the power-of-two and LDS-staged ones
def test_upsample2x_and_add_relu(shape):
    from styl3r_amd import vit_ops
    g = torch.Generator(DEV).manual_seed(shape[1])
    x = torch.randn(shape, device=DEV, generator=g).requires_grad_(True)
    B, Cc, H, W = shape
    c = torch.randn(B, Cc, 2 * H, 2 * W, device=DEV, generator=g).requires_grad_(True)
    gy = torch.randn(B, Cc, 2 * H, 2 * W, device=DEV, generator=g)

    def op():
        y = vit_ops.upsample2x(x)
        out = dict(y=y, dx=torch.autograd.grad((y * gy).sum(), x)[0])
        if W % 4 == 0:
            z = vit_ops._UpsampleAddRelu.apply(x, c)
            zx, zc = torch.autograd.grad((z * gy).sum(), (x, c))
            out.update(z=z, zx=zx, zc=zc)
        return out
    runs = three_runs(op, expect=[dict(shape=(B, Cc, 2 * H, 2 * W), dtype=F32), dict(shape=shape, dtype=F32)])
    assert_identical(runs)
    z = runs["zero"]
    ref = torch.nn.functional.interpolate(x.detach().double(), scale_factor=2, mode="bilinear", align_corners=True)
    assert rel_err(z["y"], ref) <= 1e-5
    if "z" in z:
        assert rel_err(z["z"], ref + torch.relu(c.detach().double())) <= 1e-5


@pytest.mark.parametrize("C_,CO,p", [(128, 3, 0.0), (256, 8, 0.0), (256, 8, 0.1), (256, 3, 0.1)])
def test_head_tail_and_relu_dropout(C_, CO, p):
    """y and dh are written once per element (bit-identical); dW and db are zeroed by the entry and summed with atomics (the bars of
    test_head_tail_kernel_matches_fp64_and_the_separate_relu_dropout_kernel).  The stand-alone ReLU-dropout kernel provides the mask."""
    from styl3r_amd import vit_ops
    torch.manual_seed(7 + C_ + CO)
    B, H, W, seed = 2, 10, 18, 123456789
    conv = torch.nn.Conv2d(C_, CO, 1).to(DEV)
    h = torch.randn(B, C_, H, W, device=DEV, requires_grad=True)
    g = torch.randn(B, CO, H, W, device=DEV)
    gm = torch.randn(B, C_, H, W, device=DEV)

    def op():
        y = vit_ops._HeadTail.apply(h, conv.weight, conv.bias, p, seed)
        dh, dw, db = torch.autograd.grad((y * g).sum(), (h, conv.weight, conv.bias))
        out = dict(y=y, dh=dh, dw=dw, db=db)
        if p > 0:
            hh = h.detach().clone().requires_grad_(True)
            a = vit_ops._ReluDropout.apply(hh * 1.0, p, seed)
            out.update(mask=a, dmask=torch.autograd.grad((a * gm).sum(), hh)[0])
        return out
    runs = three_runs(op, expect=[dict(shape=(B, CO, H, W), dtype=F32), dict(shape=(B, C_, H, W), dtype=F32), dict(shape=(CO, C_), dtype=F32),
                                  dict(shape=(CO,), dtype=F32)])
    assert_identical(runs, ("y", "dh") + (("mask", "dmask") if p > 0 else ()))
    fac = ((runs["zero"]["mask"] > 0).double() / (1 - p)) if p > 0 else (h.detach() > 0).double()
    hd, wd, bd = (t.detach().double().requires_grad_(True) for t in (h, conv.weight, conv.bias))
    ref = torch.nn.functional.conv2d(hd * fac, wd, bd)
    (ref * g.double()).sum().backward()
    for pattern in PATTERNS:
        r = runs[pattern]
        assert rel_err(r["y"], ref.detach()) <= 2e-6 and rel_err(r["dh"], hd.grad) <= 2e-6
        assert rel_err(r["dw"], wd.grad) <= 1e-5 and rel_err(r["db"], bd.grad) <= 1e-5, pattern


def test_maxpool_and_lpips_tail():
    from styl3r_amd import vit_ops
    g = torch.Generator(DEV).manual_seed(8)
    x = torch.randn(2, 3, 6, 10, device=DEV, generator=g).requires_grad_(True)
    gp = torch.randn(2, 3, 3, 5, device=DEV, generator=g)
    sizes = [(64, 9, 13), (128, 4, 6)]
    fa = [torch.randn(2, *s, device=DEV, generator=g).requires_grad_(True) for s in sizes]
    fb = [torch.randn(2, *s, device=DEV, generator=g) for s in sizes]
    ws = [torch.rand(s[0], device=DEV, generator=g) for s in sizes]
    gd = torch.randn(2, device=DEV, generator=g)
    lib = vit_ops.load()
    taps = vit_ops._lpips_table([a.detach() for a in fa], fb, ws)
    nb, ns = lib.vit_lpips_scratch_bytes(taps, 2, 2), lib.vit_lpips_stats_bytes(taps, 2, 2)

    def op():
        y = vit_ops.maxpool2x2(x)
        d = vit_ops.lpips_tail(fa, fb, ws, relu_in=True)
        dfa = torch.autograd.grad((d * gd).sum(), fa)
        return dict(pool=y, dpool=torch.autograd.grad((y * gp).sum(), x)[0], dist=d, dfa0=dfa[0], dfa1=dfa[1])
    runs = three_runs(op, expect=[dict(nbytes=nb, dtype=F32), dict(nbytes=ns, dtype=F32), dict(shape=(2,), dtype=F32), dict(shape=(2, 3, 3, 5), dtype=F32),
                                  dict(shape=(2, 3, 6, 10), dtype=F32)])
    assert_identical(runs)
    z = runs["zero"]
    assert torch.equal(z["pool"], torch.nn.functional.max_pool2d(x.detach(), 2, 2))
    want = 0
    for a, b, w in zip(fa, fb, ws):
        a, b = torch.relu(a.detach().double()), torch.relu(b.double())
        an, bn = a / (a.pow(2).sum(1, keepdim=True).sqrt() + 1e-10), b / (b.pow(2).sum(1, keepdim=True).sqrt() + 1e-10)
        want = want + (w.double().view(1, -1, 1, 1) * (an - bn) ** 2).sum(1).mean((1, 2))
    assert rel_err(z["dist"], want) <= 1e-5
    sc, intact = guarded(nb)
    dist = torch.full((2,), float("nan"), device=DEV)
    rc = lib.vit_lpips_fwd(taps, 2, 2, 1, dist.data_ptr(), sc.data_ptr(), None, _stream())
    torch.cuda.synchronize()
    intact()
    assert rc == 0 and torch.equal(dist, z["dist"])


def test_adaattn_stats_and_l1():
    from styl3r_amd import losses, vit_ops
    g = torch.Generator(DEV).manual_seed(10)
    q, k, s = (torch.randn(*sh, device=DEV, generator=g) for sh in ((2, 64, 37), (2, 64, 50), (2, 64, 50)))
    p = torch.randn(2, 64, 37, device=DEV, generator=g).requires_grad_(True)
    c = torch.randn(2, 64, 37, device=DEV, generator=g)
    nb = vit_ops.load().vit_adaattn_l1_scratch_bytes(2, 64)

    def op():
        mean, std = losses.adaattn_stats(q, k, s)
        det = {}
        loss = losses.adaattn_l1(p, c, mean, std, det)
        return dict(mean=mean, std=std, loss=loss, dp=torch.autograd.grad(loss * 2.0, p)[0], cs=det["cs"], feature_grad=det["feature_grad"])
    runs = three_runs(op, expect=[dict(nbytes=nb, dtype=torch.float64), dict(shape=(2, 64, 37), dtype=F32), dict(shape=(), dtype=F32)])
    assert_identical(runs)
    z = runs["zero"]
    sc, intact = guarded(nb)
    loss, grad = torch.full((), float("nan"), device=DEV), torch.full((2, 64, 37), float("nan"), device=DEV)
    rc = vit_ops.load().vit_adaattn_l1(p.data_ptr(), c.data_ptr(), z["mean"].data_ptr(), z["std"].data_ptr(), 2, 64, 37, sc.data_ptr(), loss.data_ptr(),
                                       grad.data_ptr(), None, _stream())
    torch.cuda.synchronize()
    intact()
    assert rc == 0 and torch.equal(loss, z["loss"]) and torch.equal(grad, z["feature_grad"])


def test_gaussian_adapter():
    from styl3r_amd.vit_ops import gaussian_adapter_hip
    b, v, H, W, d_sh = 1, 2, 8, 8, 4
    g = torch.Generator(DEV).manual_seed(19)
    R = lambda *s: torch.randn(*s, device=DEV, generator=g)
    ins = [t.requires_grad_(True) for t in (R(b, 3, H, W) * 0.8, R(b, 3, H, W) * 0.8, R(b, 8, H, W) * 2, R(b, 8, H, W) * 2, R(b * v, 3 * d_sh, H, W))]
    mask = torch.tensor([1.0, 0.025, 0.025, 0.025], device=DEV)
    G = v * H * W
    wts = [R(b, G, 3), R(b, G, 3, 3), R(b, G, 3, d_sh), R(b, G)]

    def op():
        out = gaussian_adapter_hip(*ins, mask, 1.0, v, True)
        grads = torch.autograd.grad(sum((a * w).sum() for a, w in zip(out[:4], wts)), ins)
        res = dict(zip(("means", "cov", "sh", "opac", "scales", "rot"), out))
        res.update(zip(("d_pts0", "d_ptsr", "d_par0", "d_parr", "d_app"), grads))
        return res
    runs = three_runs(op, expect=[dict(shape=(b, G, 3, 3), dtype=F32), dict(shape=(b, G), dtype=F32), dict(shape=(b, 8, H, W), dtype=F32)])
    assert_identical(runs)


@pytest.mark.parametrize("arith", ["bf16x6", "f16x3"])
@pytest.mark.parametrize("B,H,Nq,Nk", [(1, 1, 5, 1), (1, 2, 130, 771), (11, 16, 257, 257)])
def test_attention_forward_and_backward(B, H, Nq, Nk, arith, monkeypatch):
    """out, lse, dq, dk, dv and the backward's delta buffer are torch.empty.  The RoPE-fused forward output is bit-identical; the gradients
    meet the bars of test_attention_backward_vs_oracle (2e-5, atol 1e-5) against float64, the output the 1e-5 of the forward test."""
    from styl3r_amd import vit_ops
    monkeypatch.setattr(vit_ops, "ATTENTION_ARITH", arith)
    g = torch.Generator(DEV).manual_seed(Nq * 3 + Nk)
    q, k, v = (torch.randn(B, n, H, 64, device=DEV, generator=g).requires_grad_(True) for n in (Nq, Nk, Nk))
    go = torch.randn(B, Nq, H, 64, device=DEV, generator=g)
    qpos = (torch.arange(Nq, device=DEV)[None, :, None].expand(B, -1, 2) % 17).contiguous()
    kpos = (torch.arange(Nk, device=DEV)[None, :, None].expand(B, -1, 2) % 17).contiguous()

    def rot(t, pos):                                        # the rotation of vit_rope2d in float64
        inv = 1.0 / (100.0 ** (torch.arange(0, 16, dtype=torch.float64, device=DEV) / 16))
        parts = []
        for half in (0, 1):
            ang = pos[..., half].double()[..., None] * inv
            cs, sn = ang.cos()[:, :, None, :], ang.sin()[:, :, None, :]
            u, w_ = t[..., 32 * half:32 * half + 16], t[..., 32 * half + 16:32 * half + 32]
            parts += [u * cs - w_ * sn, w_ * cs + u * sn]
        return torch.cat(parts, -1)
    qd, kd, vd = (t.detach().double().requires_grad_(True) for t in (q, k, v))
    att = torch.softmax(torch.einsum("bnhd,bmhd->bhnm", rot(qd, qpos), rot(kd, kpos)) * 0.125, -1)
    od = torch.einsum("bhnm,bmhd->bnhd", att, vd)
    (od * go.double()).sum().backward()
    ref = dict(out=od.detach(), dq=qd.grad, dk=kd.grad, dv=vd.grad)
    del att

    def op():
        o = vit_ops.memory_efficient_attention(q, k, v, scale=0.125, qpos=qpos, kpos=kpos, rope_base=100.0, max_pos=16)
        dq, dk, dv = torch.autograd.grad((o * go).sum(), (q, k, v))
        return dict(out=o, dq=dq, dk=dk, dv=dv)
    runs = three_runs(op, expect=[dict(shape=(B, Nq, H, 64), dtype=F32), dict(shape=(B, H, Nq), dtype=F32), dict(shape=(B, Nk, H, 64), dtype=F32)])
    assert vit_ops.load().vit_attention_arith() == {"bf16x6": 1, "f16x3": 3}[arith]
    assert_identical(runs, ("out",))
    for pattern in PATTERNS:
        assert_close_rel(runs[pattern]["out"].cpu().numpy(), ref["out"].cpu().numpy(), 1e-5, "attention out")
        for n in ("dq", "dk", "dv"):
            assert_close_rel(runs[pattern][n].cpu().numpy(), ref[n].cpu().numpy(), 2e-5, f"{n} on {pattern}-filled memory", atol=1e-5)


# =====================================================================================================================
# Optimizer pass and snapshot: the wrappers allocate nothing uninitialised (torch.zeros moments, a grown torch.zeros staging buffer), so
# the poison is laid by hand: every operand is a view of a `guarded` buffer of exactly its size, poisoned bytes in front of a misaligned
# view and canaries behind everything
# =====================================================================================================================
@pytest.mark.parametrize("n,offset", [(5, 0), (16385, 0), (16385, 4)])      # a scalar tail only / one whole chunk + a one-element chunk / vec = 0
def test_adamw_step_c_abi_ragged_and_misaligned(n, offset):
    """vit_adamw_step on p, g, m, v of n elements that end exactly where their buffers end (a float4 walk with a ragged tail must not
    touch the canary) and, with `offset`, start 4 bytes into them (the scalar route): two steps, bit-identical whatever surrounds the
    operands, the surroundings untouched, and parameters and moments within the 2e-6 of the framework-parity test of a float64 AdamW."""
    from styl3r_amd import optim
    lib = optim._lib()
    lr, b1, b2, eps, wd = 2e-4, 0.9, 0.95, 1e-8, 0.05
    g = torch.Generator(DEV).manual_seed(n + offset)
    p0 = torch.randn(n, device=DEV, generator=g)
    grads = [torch.randn(n, device=DEV, generator=g), 10.0 * torch.randn(n, device=DEV, generator=g)]
    pd, md, vd = p0.double(), torch.zeros(n, dtype=torch.float64, device=DEV), torch.zeros(n, dtype=torch.float64, device=DEV)
    for t, gr in enumerate(grads, 1):
        gd = gr.double()
        pd = pd - lr * wd * pd
        md = md + (1 - b1) * (gd - md)
        vd = b2 * vd + (1 - b2) * gd * gd
        pd = pd - lr / (1 - b1 ** t) * md / (vd.sqrt() / (1 - b2 ** t) ** 0.5 + eps)
    fill = {"zero": 0x00, "ones": 0xFF, "garbage": 0xA5}
    results = {}
    for pattern in PATTERNS:
        bufs, checks, ops = [], [], []
        for _ in range(4):
            b, intact = guarded(offset + 4 * n, pattern=pattern)
            bufs.append(b); checks.append(intact); ops.append(b[offset:].view(F32))
        p, gv, m, v = ops
        assert p.numel() == n and p.data_ptr() % 16 == offset
        p.copy_(p0); m.zero_(); v.zero_()
        step = torch.zeros((), device=DEV)
        rows = [(p.data_ptr() + 4 * o, gv.data_ptr() + 4 * o, m.data_ptr() + 4 * o, v.data_ptr() + 4 * o, step.data_ptr(), min(optim._CHUNK, n - o),
                 int(offset == 0), 0) for o in range(0, n, optim._CHUNK)]
        host = np.array(rows, dtype=optim._CHUNK_DTYPE)
        with poisoned_allocations(pattern) as rec:          # the chunk table itself sits in poisoned memory before it is filled
            table = torch.empty(host.nbytes, dtype=U8, device=DEV)
        assert rec.has(nbytes=host.nbytes, dtype=U8)
        table.copy_(torch.from_numpy(host.view(np.uint8).reshape(-1).copy()))
        for gr in grads:
            gv.copy_(gr); step += 1
            assert lib.vit_adamw_step(table.data_ptr(), len(rows), lr, b1, b2, eps, wd, None, _stream()) == 0
        torch.cuda.synchronize()
        for b, intact in zip(bufs, checks):
            intact()
            assert bool((b[:offset] == fill[pattern]).all()), "the bytes in front of a misaligned operand changed"
        assert torch.equal(gv, grads[-1]), "the gradient is read, never rewritten"
        results[pattern] = dict(p=p.clone(), m=m.clone(), v=v.clone())
        for k, want in (("p", pd), ("m", md), ("v", vd)):
            assert bool(torch.isfinite(results[pattern][k]).all()) and rel_err(results[pattern][k], want) <= 2e-6, (pattern, k)
    assert_identical(results)


def test_snapshot_pack_c_abi_on_poisoned_staging():
    """vit_snapshot_pack into a staging buffer that ends with the last tensor's last byte and partial records of exactly n_chunks x 24
    bytes: the tensors' bytes arrive, the gaps between them keep the poison, the canaries behind both buffers are intact, and the partial
    records (reserved word included) are the same bits under every pattern and fold to the numpy checksums.
    (tests/test_gpu_checkpoint.py::test_kernel_equals_the_numpy_restatement_and_keeps_the_canary makes the 0xA5 run through the wrapper.)"""
    from styl3r_amd import checkpointing as ck
    lib, chunk = ck._lib(), ck.chunk_bytes()
    g = torch.Generator(DEV).manual_seed(12)
    store = torch.randn(chunk // 4 + 6, device=DEV, generator=g)
    store[3] = float("inf"); store[chunk // 4 + 4] = float("nan")
    srcs = [torch.randn(5, device=DEV, generator=g), torch.randn(chunk // 4 + 1, device=DEV, generator=g), store[1:],
            (torch.arange(7, device=DEV) * 37).to(U8), (torch.arange(chunk + 11, device=DEV) % 251).to(U8)[3:]]
    assert srcs[2].data_ptr() % 16 == 4 and srcs[4].data_ptr() % 4 == 3
    items, off = [], 0
    for t in srcs:
        nbytes = t.numel() * t.element_size()
        items.append((t.data_ptr(), off, nbytes, t.dtype == F32))
        end, off = off + nbytes, ck._round_up(off + nbytes, ck.ALIGN)
    table, first, counts = ck._build_table(items, chunk)
    n_chunks = int(counts.sum())
    assert counts.tolist() == [1, 2, 2, 1, 2]
    dev_table = torch.from_numpy(table.view(np.uint8).reshape(-1).copy()).to(DEV)
    fill = {"zero": 0x00, "ones": 0xFF, "garbage": 0xA5}
    seen = {}
    for pattern in PATTERNS:
        staging, intact_s = guarded(end, pattern=pattern)
        partials, intact_p = guarded(n_chunks * ck._PARTIAL_DTYPE.itemsize, pattern=pattern)
        assert lib.vit_snapshot_pack(dev_table.data_ptr(), n_chunks, staging.data_ptr(), partials.data_ptr(), torch.cuda.current_stream().cuda_stream) == 0
        torch.cuda.synchronize()
        intact_s(); intact_p()
        image, used = staging.cpu().numpy(), np.zeros(end, bool)
        for t, (_, o, nbytes, _) in zip(srcs, items):
            assert np.array_equal(image[o:o + nbytes], t.contiguous().cpu().view(-1).view(U8).numpy()), (pattern, tuple(t.shape))
            used[o:o + nbytes] = True
        assert (~used).sum() > 0 and (image[~used] == fill[pattern]).all(), "a byte between two tensors was written"
        seen[pattern] = dict(partials=partials.clone())
        rec = partials.cpu().numpy().view(ck._PARTIAL_DTYPE)
        assert (rec["reserved"] == 0).all()
        with np.errstate(over="ignore"):
            for t, f, k in zip(srcs, first, counts):
                part = rec[f:f + k]
                base = np.arange(k, dtype=np.uint64) * np.uint64(chunk // 4)
                s1 = int(part["s1"].sum(dtype=np.uint64)) & ck._MASK
                s2 = int((part["s2"] + base * part["s1"]).sum(dtype=np.uint64)) & ck._MASK
                host = t.contiguous().cpu()
                assert (s1, s2) == ck.checksum(host) and int(part["nonfinite"].sum()) == ck.count_nonfinite(host), (pattern, tuple(t.shape))
    assert_identical(seen)


# =====================================================================================================================
# Image codecs (image_io.py:453-455,568-577, dataset.py:232-233: scratch, stream buffers and length words are torch.empty).  Their
# scratches hold lengths and offsets (PNG: a meta row per chunk; JPEG encoder: bits per block, bit offsets per segment), every one written
# by the launch in front of its reader: docs/SCRATCH_CONTRACTS.md
# =====================================================================================================================
def test_png_and_jpeg_codecs():
    from io import BytesIO
    from PIL import Image
    from styl3r_amd import _lib, dataset, image_io
    lib = _lib.load()
    N, H, W = 2, 37, 53                                    # ragged against the 8 x 8 blocks and the 16 x 16 MCUs; several segments per picture
    g = torch.Generator(DEV).manual_seed(13)
    yy, xx = torch.meshgrid(torch.arange(H, device=DEV), torch.arange(W, device=DEV), indexing="ij")
    smooth = torch.stack([(3 * xx + 2 * yy) % 256, (5 * yy + xx) % 256, (xx * yy) % 256], -1)[None].expand(N, -1, -1, -1)
    frames = ((smooth + torch.randint(0, 24, (N, H, W, 3), device=DEV, generator=g)) % 256).to(U8).contiguous()
    jpegs = image_io.encode_jpeg(frames.cpu(), 90, "4:2:0")                             # Pillow's files: the decoder's input
    as_t = lambda files: {f"file{i}": torch.frombuffer(bytearray(b), dtype=U8) for i, b in enumerate(files)}

    def op():
        out = {"png_" + k: v for k, v in as_t(image_io.encode_png(frames)).items()}
        out.update({"jpg_" + k: v for k, v in as_t(image_io.encode_jpeg(frames, 90, "4:2:0")).items()})
        out["decoded"] = dataset.decode_jpeg(jpegs, device=DEV)
        return out
    runs = three_runs(op, expect=[dict(nbytes=lib.gsr_png_scratch_bytes(N, H, W, 3), dtype=U8),
                                  dict(nbytes=lib.gsr_jpeg_enc_scratch_bytes(N, H, W, _lib.GSR_JPEG_420), dtype=U8),
                                  dict(nbytes=lib.gsr_jpeg_scratch_bytes(N, H, W), dtype=U8), dict(shape=(N, H, W, 3), dtype=U8)])
    assert_identical(runs)
    z = runs["zero"]
    for i in range(N):
        back = np.asarray(Image.open(BytesIO(bytes(z[f"png_file{i}"].tolist()))).convert("RGB"))
        assert np.array_equal(back, frames[i].cpu().numpy()), "PNG round trip"
        assert bytes(z[f"jpg_file{i}"].tolist()) == jpegs[i], "the encoder's bytes are Pillow's"
    assert torch.equal(z["decoded"].cpu(), dataset.decode_jpeg(jpegs))
