"""-m gpu: the kernels of csrc/gsr_outputs.hip -- gsr_trajectory, gsr_depth_range, gsr_pack_frames, gsr_ply_normalizer / gsr_ply_rows --
against the host restatements of styl3r_amd/trajectory.py and styl3r_amd/export.py (which tests/test_scene_outputs_host.py holds
against the reference), and `render_flythrough` / `export_scene_ply` end to end on a tiny encoder.

Bars: cameras within 1 float32 ulp of the entry's scale (rotation entries: 1; origins: the largest origin coordinate) of the float64
restatement, and bit-independent of the number of pairs in the call; the depth range bit-equal to torch.quantile(...).log() on the
CPU; frame bytes equal to the host path; medians and quantiles of the normaliser bit-equal to torch.median / torch.quantile; table
rows at the host test's bars."""
import numpy as np
import pytest
import torch

from styl3r_amd import _lib
from styl3r_amd import export as ex
from styl3r_amd import trajectory as tj
from tests.test_scene_outputs_host import G, T, check_ply_table

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
D = lambda k: T(k).to(DEV)
ULP1 = 2.0 ** -23
bits = lambda t: t.detach().cpu().contiguous().view(torch.int32)


# ---- gsr_trajectory ----
def _check_cameras(got, want64, what):
    """got fp32 (F,4,4) from the kernel, want64 the float64 restatement"""
    got = got.cpu().double().numpy()
    want = want64.numpy()
    assert np.isfinite(got).all(), what
    scale = max(1.0, float(np.abs(want[:, :3, 3]).max()))
    assert np.abs(got[:, :3, :3] - want[:, :3, :3]).max() <= ULP1, f"{what}: rotation"
    assert np.abs(got[:, :3, 3] - want[:, :3, 3]).max() <= ULP1 * scale, f"{what}: origin"
    assert (got[:, 3] == np.array([0, 0, 0, 1.0])).all(), what


PAIRS = ("generic", "re10k", "identical", "straddle")


@pytest.mark.parametrize("times", ["f60", "f60s", "exag", "f2", "f1"])
def test_trajectory_matches_the_float64_restatement_for_every_pair(times):
    t = T(f"traj_t_{times}")
    for pair in PAIRS:
        a, b = T(f"traj_{pair}_a"), T(f"traj_{pair}_b")
        got = tj.interpolate_extrinsics(a.to(DEV), b.to(DEV), t.to(DEV))
        assert got.shape == (t.shape[0], 4, 4) and got.is_cuda
        _check_cameras(got, tj._interpolate_extrinsics_f64(a, b, t, 1e-4), f"{pair} {times}")


def test_trajectory_is_independent_of_the_number_of_pairs_and_deterministic():
    t = D("traj_t_f60s")
    A = torch.stack([D(f"traj_{p}_a") for p in ("generic", "re10k", "straddle")])
    B = torch.stack([D(f"traj_{p}_b") for p in ("generic", "re10k", "straddle")])
    Ka, Kb = D("traj_Ka").expand(3, 3, 3).contiguous(), D("traj_Kb").expand(3, 3, 3).contiguous()
    c3, k3 = tj.trajectory_hip(A, B, Ka, Kb, t)
    again = tj.trajectory_hip(A, B, Ka, Kb, t)
    assert torch.equal(bits(c3), bits(again[0])) and torch.equal(bits(k3), bits(again[1]))
    for p in range(3):
        c1, k1 = tj.trajectory_hip(A[p:p + 1], B[p:p + 1], Ka[p:p + 1], Kb[p:p + 1], t)
        assert torch.equal(bits(c1[0]), bits(c3[p])) and torch.equal(bits(k1[0]), bits(k3[p])), p
    assert np.array_equal(k3[0].cpu().numpy(), G["traj_K_f60s_ref"])                   # the reference's fp32 expression, bit for bit
    # batched through the reference's signature: (3,4,4) x2 -> (3,F,4,4)
    assert torch.equal(bits(tj.interpolate_extrinsics(A, B, t)), bits(c3))


def test_trajectory_options_wobble_hold_and_time_map(monkeypatch):
    # (the eased frame times come from the host for both paths: cos on the device and on the CPU differ in the last bit)
    host_times = tj.smooth_time
    monkeypatch.setattr(tj, "smooth_time", lambda n, smooth=True, device=None: host_times(n, smooth).to(device))
    a, b, t = T("traj_generic_a"), T("traj_generic_b"), T("traj_t_f60s")
    r = T("wobble_radius")
    got = tj.generate_wobble(a.to(DEV), r.to(DEV), t.to(DEV))
    want = tj._wobble_f64(a.double()[None].expand(60, 4, 4), r, t, 1, True)
    _check_cameras(got, want, "wobble")
    for scaled in (False, True):
        got = tj.generate_wobble_transformation(r.to(DEV), t.to(DEV), 1, scaled)
        _check_cameras(got, tj._wobble_f64(torch.eye(4, dtype=torch.float64).expand(60, 4, 4), r, t, 1, scaled), f"wobble transform {scaled}")
    # the three videos of the wrapper, device against host
    ctx = dict(extrinsics=torch.stack([a, b])[None], intrinsics=torch.stack([T("traj_Ka"), T("traj_Kb")])[None],
               near=torch.tensor([[0.5, 0.6]]), far=torch.tensor([[50.0, 60.0]]))
    dctx = {k: v.to(DEV) for k, v in ctx.items()}
    for kind in ("interpolation", "wobble", "interpolation_exaggerated"):
        e, k, near, far = tj.trajectory_cameras(dctx, kind=kind, num_frames=None if kind != "interpolation_exaggerated" else 40)
        he, hk, hnear, hfar = tj.trajectory_cameras(ctx, kind=kind, num_frames=None if kind != "interpolation_exaggerated" else 40)
        assert e.shape == he.shape and torch.equal(bits(k), bits(hk)) and torch.equal(near.cpu(), hnear) and torch.equal(far.cpu(), hfar), kind
        scale = max(1.0, float(he[0, :, :3, 3].abs().max()))
        assert (e.cpu() - he).abs().max() <= ULP1 * scale, kind            # (fp32 roundings of two float64 values a few 1e-16 apart)
    # hold_a without a wobble hands A back bit for bit
    c, k = tj.trajectory_hip(a[None].to(DEV), b[None].to(DEV), D("traj_Ka")[None], D("traj_Kb")[None], t.to(DEV), hold_a=True)
    assert torch.equal(bits(c[0]), bits(a.expand(60, 4, 4))) and torch.equal(bits(k[0]), bits(T("traj_Ka").expand(60, 3, 3)))


# ---- gsr_depth_range ----
def _depths(n, seed):
    g = torch.Generator().manual_seed(seed)
    d = (torch.rand(n, generator=g) * 7).round(decimals=1)              # heavy ties: 71 distinct values
    if n >= 8:
        d[torch.randperm(n, generator=g)[: n // 8]] = 0.0
        d[torch.randperm(n, generator=g)[: n // 16]] *= -1.0
    if n >= 501:
        d[n // 3] = float("inf")                                       # one +inf, above the 99 % rank
    if n == 2:
        d = torch.tensor([0.25, 3.5])
    return d


def _log_is_unambiguous(q):
    """The yardstick is the CPU's float32 log, which libm does not round correctly near a tie (the same input was seen to give either
    neighbour on two CPUs, 0.06 ulp from the tie); the kernel rounds the float64 log once.  A seeded quantile whose exact log lies within
    an eighth of an ulp of a float32 rounding tie would make the comparison a comparison of libms, so the cases are chosen to have none."""
    x = float(q)
    if not (x > 0 and np.isfinite(x)):
        return True                                    # (-inf / NaN: nothing to round)
    exact = np.log(np.float64(x))
    near = np.float32(exact)
    ulp = float(np.spacing(np.abs(near))) if near != 0 else 2.0 ** -149
    return abs(abs(exact - float(near)) - 0.5 * ulp) >= 0.125 * ulp


@pytest.mark.parametrize("n", [2, 501, 8192, 8193, 40001])
def test_depth_range_is_bit_equal_to_torch_quantile_log(n):
    d = _depths(n, n)
    info = {}
    got = ex.depth_range(d.to(DEV), details=info)
    want_far = d.quantile(0.99).log()
    pos = d[d > 0]
    want_near = pos.quantile(0.01).log()
    assert _log_is_unambiguous(pos.quantile(0.01)) and _log_is_unambiguous(d.quantile(0.99)), "seeded quantile on a log rounding tie"
    print(f"[depth_range n={n}] near {float(got[0])!r} / {float(want_near)!r}  far {float(got[1])!r} / {float(want_far)!r}")
    assert torch.equal(bits(info["quantiles"]), bits(torch.stack([pos.quantile(0.01), d.quantile(0.99)])))
    assert torch.equal(bits(got), bits(torch.stack([want_near, want_far])))
    assert info["status"].tolist() == [pos.numel(), 0]
    assert torch.equal(bits(ex.depth_range(d.to(DEV))), bits(got))                     # two runs, the same bits


def test_depth_range_cut_and_no_positive_depth():
    d = _depths(1500, 7)
    info = {}
    got = ex.depth_range(d.to(DEV), max_elems=1000, details=info)
    head = d[:1000]
    pos = head[head > 0]
    assert _log_is_unambiguous(pos.quantile(0.01)) and _log_is_unambiguous(head.quantile(0.99)), "seeded quantile on a log rounding tie"
    assert torch.equal(bits(got), bits(torch.stack([pos.quantile(0.01).log(), head.quantile(0.99).log()])))
    assert info["status"].tolist() == [pos.numel(), 0] and pos.numel() != int((d > 0).sum())
    neg = -_depths(501, 3).abs()
    neg[neg.isinf()] = -1.0
    info = {}
    got = ex.depth_range(neg.to(DEV), details=info)
    assert info["status"].tolist() == [0, _lib.GSR_DEPTH_NO_POSITIVE] and float(got[0]) == 0.0
    assert torch.equal(bits(got[1:]), bits(neg.quantile(0.99).log()[None]))            # (log of a non-positive quantile: NaN or -inf, as torch)


def test_depth_range_with_a_nan_keeps_the_positive_quantile():
    """a NaN is in "all depths" (q 0.99 and far are NaN, as torch) and not in "the positive ones" (q 0.01, near and the count ignore it)"""
    d = _depths(501, 501)
    d[7] = float("nan")
    pos = d[d > 0]
    assert torch.isfinite(pos.quantile(0.01)) and torch.isnan(d.quantile(0.99)) and _log_is_unambiguous(pos.quantile(0.01))
    info = {}
    got = ex.depth_range(d.to(DEV), details=info).cpu()
    q = info["quantiles"].cpu()
    print(f"[depth_range nan] near {float(got[0])!r} far {float(got[1])!r} quantiles {q.tolist()} status {info['status'].tolist()}")
    assert torch.isnan(q[1]) and torch.isnan(got[1])
    assert torch.equal(bits(q[:1]), bits(pos.quantile(0.01)[None])) and torch.equal(bits(got[:1]), bits(pos.quantile(0.01).log()[None]))
    assert info["status"].tolist() == [int((d > 0).sum()), 0]


# ---- gsr_pack_frames ----
def test_pack_frames_bytes_equal_the_host_path_and_stay_inside_the_output():
    g = torch.Generator().manual_seed(11)
    checked = 0
    for W in (4, 6, 18, 64):
        for H in (1, 5):
            F_max = 5
            rgbs = [torch.rand(F_max, 3, H, W, generator=g) * 1.4 - 0.2 for _ in range(2)]
            rgbs[0].view(-1)[::7] = 1.0
            rgbs[1].view(-1)[::11] = float("nan")
            depths = [torch.rand(F_max, H, W, generator=g) * 4 + 0.5 for _ in range(2)]
            depths[0].view(-1)[::13] = 0.0
            depths[1].view(-1)[::17] = -1.0
            pool = [rgbs[0], depths[0], rgbs[1], depths[1]]
            rng = ex.depth_range(torch.cat([d.reshape(-1) for d in depths]))
            dpool = [p.to(DEV) for p in pool]
            for axis in (0, 1):
                for gap in (0, 8):
                    for n_panels in (1, 2, 3, 4):
                        for F in (1, 2, 3, 5):
                            want = ex.pack_frames([p[:F] for p in pool[:n_panels]], axis=axis, gap=gap, loop_reverse=True, depth_range=rng)
                            n = want.numel()
                            buf = torch.full((n + 64,), 0xA5, dtype=torch.uint8, device=DEV)
                            got = ex.pack_frames([p[:F].contiguous() for p in dpool[:n_panels]], axis=axis, gap=gap, loop_reverse=True,
                                                 depth_range=rng.to(DEV), out=buf)
                            assert got.shape == want.shape == (F + max(F - 2, 0),) + ex.frames_shape(n_panels, F, H, W, axis, gap, True)[1:] + (3,)
                            flat = buf.cpu()
                            assert torch.equal(flat[:n], want.reshape(-1)), (W, H, axis, gap, n_panels, F)
                            assert (flat[n:] == 0xA5).all(), ("canary", W, H, axis, gap, n_panels, F)
                            checked += 1
    assert checked == 4 * 2 * 2 * 2 * 4 * 4
    # without loop_reverse, and the range taken on the device
    want = ex.pack_frames([pool[1][:3]], gap=0, loop_reverse=False)
    got = ex.pack_frames([dpool[1][:3].contiguous()], gap=0, loop_reverse=False)
    assert got.shape[0] == 3 and torch.equal(got.cpu(), want)


# ---- gsr_ply_normalizer / gsr_ply_rows ----
def _gaussians(G_, d_sh, seed):
    g = torch.Generator().manual_seed(seed)
    means = torch.randn(G_, 3, generator=g) * torch.tensor([2.0, 0.5, 1.0]) + torch.tensor([0.3, -1.0, 4.0])
    means = (means * 8).round() / 8 if G_ > 1000 else means                                  # ties among the medians' neighbours
    scales = torch.rand(G_, 3, generator=g) * 0.2 + 1e-3
    rots = torch.randn(G_, 4, generator=g)
    return means, scales, rots, torch.randn(G_, 3, d_sh, generator=g), torch.rand(G_, generator=g)


def _near_tie_rows(rots):
    """rows whose two largest branch quantities (m00, m11, m22, trace) of the quaternion's matrix lie within 1e-6 relative"""
    q = rots.double() / rots.double().norm(dim=1, keepdim=True)
    x, y, z, w = q.unbind(1)
    m = torch.stack([x * x - y * y - z * z + w * w, -x * x + y * y - z * z + w * w, -x * x - y * y + z * z + w * w], 1)
    top = torch.cat([m, m.sum(1, keepdim=True)], 1).sort(dim=1, descending=True).values
    return (top[:, 0] - top[:, 1]).abs() <= 1e-6 * top[:, 0].abs()


@pytest.mark.parametrize("G_", [1, 2, 63, 64, 65, 4099])
@pytest.mark.parametrize("d_sh", [1, 25])
def test_ply_rows_and_normalizer_match_the_host_path(G_, d_sh):
    inp = _gaussians(G_, d_sh, 100 * G_ + d_sh)
    dinp = [t.to(DEV) for t in inp]
    assert not _near_tie_rows(inp[2]).any(), "the seeded quaternions sit on no branch tie"
    shifts = (False, True) if G_ >= 2 else (False,)
    if G_ >= 2:
        means = inp[0]
        med = means.median(dim=0).values
        want = torch.cat([med, (means - med).abs().quantile(0.95, dim=0).max()[None]])
        got = ex.ply_normalizer(dinp[0])
        assert torch.equal(bits(got), bits(want)), (got.cpu(), want)
        assert torch.equal(bits(ex.ply_normalizer(dinp[0])), bits(got))
    for shift in shifts:
        for dc in (True, False):
            want, names = ex.ply_vertex_table(*inp, shift_and_scale=shift, save_sh_dc_only=dc)
            got, dnames = ex.ply_vertex_table(*dinp, shift_and_scale=shift, save_sh_dc_only=dc)
            assert dnames == names and got.is_cuda
            check_ply_table(got.cpu().numpy(), want.numpy(), f"G {G_} d_sh {d_sh} shift{int(shift)} dc{int(dc)}")


def test_ply_normalizer_with_a_nan_on_one_axis():
    """torch: the median of the axis that holds a NaN is NaN and so is the factor (max over the axes); the other two medians do not see it"""
    means = _gaussians(65, 1, 6501)[0]
    means[40, 1] = float("nan")
    want = means.median(dim=0).values
    assert torch.isnan(want[1]) and torch.isfinite(want[[0, 2]]).all() and torch.isnan((means - want).abs().quantile(0.95, dim=0).max())
    got = ex.ply_normalizer(means.to(DEV)).cpu()
    assert torch.equal(bits(got[[0, 2]]), bits(want[[0, 2]])), (got, want)
    assert torch.isnan(got[1]) and torch.isnan(got[3]), got


def test_ply_table_on_the_device_matches_the_reference_fixture():
    for d_sh in (1, 4, 25):
        dinp = [D(f"ply_d{d_sh}_{k}") for k in ("means", "scales", "rotations", "harmonics", "opacities")]
        for dc in (0, 1):
            for shift in (0, 1):
                got, _ = ex.ply_vertex_table(*dinp, shift_and_scale=bool(shift), save_sh_dc_only=bool(dc))
                check_ply_table(got.cpu().numpy(), G[f"ply_d{d_sh}_dc{dc}_shift{shift}_ref"], f"fixture d_sh {d_sh} dc{dc} shift{shift}")


# ---- end to end ----
def test_flythrough_and_ply_export_end_to_end(tmp_path):
    from styl3r_amd.decoder import DecoderSplattingCUDACfg, get_decoder
    from styl3r_amd.inference import export_scene_ply, render_flythrough, stylize_scene
    from styl3r_amd.scenes import recentre_output_heads_
    from tests.helpers import deterministic_init_, e2e_cameras
    from tests.test_encoder import _build
    m = deterministic_init_(_build(1)).to(DEV)
    g = torch.Generator().manual_seed(5)
    h = w = 32
    cams = {k: v.to(DEV) for k, v in e2e_cameras(1).items()}
    ctx = dict(image=(torch.rand(1, 2, 3, h, w, generator=g) * 2 - 1).to(DEV), **cams)
    styles = (torch.rand(2, 3, h, w, generator=g) * 2 - 1).to(DEV)
    recentre_output_heads_(m, ctx, dict(image=styles[:1]))
    dec = get_decoder(DecoderSplattingCUDACfg("splatting_cuda", [0.1, 0.2, 0.3], True)).to(DEV)
    scene = stylize_scene(m, dec, ctx, styles, dict(cams, image_shape=(h, w)))
    assert len(scene.gaussians) == 3
    frames = 5
    video = render_flythrough(dec, scene, ctx, num_frames=frames, panels=("plain", "stylized", 1), axis=1, gap=8)
    assert video.dtype == torch.uint8 and video.shape == (frames + frames - 2, h, 3 * w + 16, 3) and video.is_cuda
    ext, intr, near, far = tj.trajectory_cameras(ctx, num_frames=frames)
    with torch.no_grad():
        renders = [dec.forward(gs, ext, intr, near, far, (h, w)) for gs in scene.gaussians]
    bg = torch.tensor([0.1, 0.2, 0.3], device=DEV)[:, None, None]
    assert float((renders[0].color[0] - bg).abs().max()) > 1e-2, "the recentred tiny encoder must put Gaussians in front of the cameras"
    want = ex.pack_frames([r.color[0] for r in renders], axis=1, gap=8)
    assert torch.equal(video, want)                                                     # byte for byte
    assert (video[:, :, :w] != video[:, :, w + 8:2 * w + 8]).any()                      # the styles differ
    small = render_flythrough(dec, scene, ctx, num_frames=frames, panels=("plain", "stylized", 1), axis=1, gap=8, frames_per_pass=2)
    assert torch.equal(small, video)
    # a depth panel: the range of the whole video, the plain colours above it
    both = render_flythrough(dec, scene.gaussians[0], ctx, num_frames=frames, panels=("plain", "depth"), loop_reverse=False)
    assert both.shape == (frames, 2 * h + 8, w, 3)
    with torch.no_grad():
        one = dec.forward_styles(scene.gaussians[0], [scene.gaussians[0].harmonics], ext, intr, near, far, (h, w))
    want = ex.pack_frames([one.color[0, 0], one.depth[0]], loop_reverse=False, depth_range=ex.depth_range(one.depth[0]))
    assert torch.equal(both, want)
    # the .ply files read back to the Gaussians that were rendered
    paths = export_scene_ply(scene, tmp_path)
    assert [p.name for p in paths] == ["gaussians.ply", "stylized_gaussians_0.ply", "stylized_gaussians_1.ply"]
    dump = scene.visualization_dump
    for p, gs in zip(paths, scene.gaussians):
        tab, names = ex.read_ply(p)
        assert tab.shape == (gs.means.shape[1], 17) and names == ex.attribute_names(0)
        assert np.array_equal(tab[:, :3], gs.means[0].cpu().numpy()) and np.array_equal(tab[:, 6:9], gs.harmonics[0, :, :, 0].cpu().numpy())
        assert np.array_equal(tab[:, 9], gs.opacities[0].cpu().numpy())
        assert np.abs(np.exp(tab[:, 10:13].astype(np.float64)) / dump["scales"][0].reshape(-1, 3).cpu().double().numpy() - 1).max() <= 4 * ULP1 * 16
        want_q = ex._quat_round_trip_host(dump["rotations"][0].reshape(-1, 4).cpu().numpy())
        assert np.abs(tab[:, 13:] - want_q).max() <= 2 * ULP1
