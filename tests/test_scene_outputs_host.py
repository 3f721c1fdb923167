"""CPU: the host restatements of the scene outputs -- styl3r_amd/trajectory.py and styl3r_amd/export.py on CPU tensors -- against what
the reference's own functions returned for the same inputs (tests/golden/scene_outputs.npz, written by
tests/golden/make_scene_output_fixtures.py), the PLY file round trip, and the C ABI of csrc/gsr_outputs.hip as far as it goes without
a device.  These restatements are the yardstick of tests/test_gpu_scene_outputs.py."""
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from styl3r_amd import _lib
from styl3r_amd import export as ex
from styl3r_amd import trajectory as tj

ROOT = Path(__file__).resolve().parent.parent
G = np.load(ROOT / "tests/golden/scene_outputs.npz")
T = lambda k: torch.from_numpy(G[k])

# Trajectories.  The restatement is float64 to the end; the reference rounds the pivot parameters, frame and pivot point to float32
# before its last step (pivot_parameters_to_extrinsics), so the two differ by float32 rounding of quantities of the pose's scale.
# Largest deviation measured over every case below: 3.54e-7 at a pose scale of 1.0 (the straddle pair, 60 linear frames) -- 3 ulps
# of 1.0 in float32 (1.19e-7).  The bar is 4 x that, times the scale of the case's origins where that exceeds 1.
TRAJ_MEASURED = 3.54e-7
TRAJ_CASES = [(p, t) for p in ("generic", "re10k", "identical", "straddle") for t in ("f60", "f60s", "exag")] + [("generic", "f2"), ("generic", "f1")]


@pytest.mark.parametrize("pair,times", TRAJ_CASES)
def test_interpolate_extrinsics_matches_the_reference(pair, times):
    ref = G[f"traj_{pair}_{times}_ref"].astype(np.float64)
    t = T(f"traj_t_{times}")
    got = tj.interpolate_extrinsics(T(f"traj_{pair}_a"), T(f"traj_{pair}_b"), t)
    assert got.dtype == torch.float32 and got.shape == (t.shape[0], 4, 4) and torch.isfinite(got).all()
    scale = max(1.0, float(np.abs(ref[:, :3, 3]).max()))
    dev = np.abs(got.double().numpy() - ref).max()
    print(f"[traj {pair} {times}] max deviation {dev:.3e} at scale {scale:.2f}")
    assert dev <= 4 * TRAJ_MEASURED * scale
    assert np.array_equal(got[:, 3].numpy(), np.tile(np.array([0, 0, 0, 1], np.float32), (t.shape[0], 1)))
    if times in ("f60", "f60s", "f2"):          # the endpoints come back
        for f, end in ((0, "a"), (-1, "b")):
            assert np.abs(got[f].numpy() - G[f"traj_{pair}_{end}"]).max() <= 4 * TRAJ_MEASURED * scale


def test_the_named_branches_are_the_ones_the_cases_take():
    """re10k: parallel looks along (0,0,1) -- the midpoint pivot and the SECOND replacement of b; straddle: twist angles on both sides
    of 0 / 2 pi, so the interpolation must go through 0, not through pi"""
    a, b = T("traj_re10k_a").double(), T("traj_re10k_b").double()
    assert tj._parallel(a[:3, 2], b[:3, 2], 1e-4) and tj._parallel(a[:3, 2], torch.tensor([0.0, 0, 1], dtype=torch.float64), 1e-4)
    a, b = T("traj_straddle_a"), T("traj_straddle_b")
    mid = tj.interpolate_extrinsics(a, b, torch.tensor([0.5]))[0]
    # half way the roll (+0.1 / -0.1 about the look axis) has cancelled: the camera's x axis lies in the world XZ plane again;
    # the long way round would turn it upside down
    assert abs(float(mid[1, 0])) < 1e-3 and float(mid[1, 1]) > 0.99


def test_intrinsics_and_wobble_match_the_reference():
    Ka, Kb = T("traj_Ka"), T("traj_Kb")
    for times in ("f60s", "exag"):
        got = tj.interpolate_intrinsics(Ka, Kb, T(f"traj_t_{times}"))
        assert np.array_equal(got.numpy(), G[f"traj_K_{times}_ref"])                  # the same fp32 expression: bit-equal
    t, r = T("traj_t_f60s"), T("wobble_radius")
    # the reference forms sin(2 pi t) in float32 and multiplies in float32; here float64, rounded once: same bar as the poses
    assert (tj.generate_wobble(T("traj_generic_a"), r, t) - T("wobble_scaled_ref")).abs().max() <= 4 * TRAJ_MEASURED
    for scaled in (False, True):
        got = tj.generate_wobble_transformation(r, t, 1, scaled)
        assert (got - T("wobble_tf_scaled_ref" if scaled else "wobble_tf_unscaled_ref")).abs().max() <= 4 * TRAJ_MEASURED


def test_smooth_time_and_trajectory_cameras_on_the_host():
    t = tj.smooth_time(60)
    assert np.array_equal(t.numpy(), G["traj_t_f60s"]) and np.array_equal(tj.smooth_time(60, False).numpy(), G["traj_t_f60"])
    ctx = dict(extrinsics=torch.stack([T("traj_generic_a"), T("traj_generic_b")])[None], intrinsics=torch.stack([T("traj_Ka"), T("traj_Kb")])[None],
               near=torch.tensor([[0.5, 0.6]]), far=torch.tensor([[50.0, 60.0]]))
    e, k, near, far = tj.trajectory_cameras(ctx, kind="interpolation")
    assert e.shape == (1, 60, 4, 4) and k.shape == (1, 60, 3, 3) and near.shape == far.shape == (1, 60)
    assert (near == 0.5).all() and (far == 50.0).all()
    assert np.abs(e[0].double().numpy() - G["traj_generic_f60s_ref"]).max() <= 4 * TRAJ_MEASURED * 1.2
    assert np.array_equal(k[0].numpy(), G["traj_K_f60s_ref"])
    e, k, _, _ = tj.trajectory_cameras(ctx, kind="wobble")
    delta = (T("traj_generic_a")[:3, 3] - T("traj_generic_b")[:3, 3]).norm()
    assert (e[0] - tj.generate_wobble(T("traj_generic_a"), delta * 0.25, t)).abs().max() <= 2e-7 and (k[0] == T("traj_Ka")).all()
    e, k, _, _ = tj.trajectory_cameras(ctx, kind="interpolation_exaggerated")
    assert e.shape == (1, 300, 4, 4) and torch.isfinite(e).all()
    lin = torch.linspace(0, 1, 300)
    want = tj.interpolate_extrinsics(T("traj_generic_a"), T("traj_generic_b"), lin * 5 - 2) @ tj.generate_wobble_transformation(delta * 0.5, lin, 5, False)
    assert (e[0] - want).abs().max() <= 4 * TRAJ_MEASURED * 4
    # three context views: the second endpoint is target view 0
    ctx3 = {k_: torch.cat([v, v[:, :1]], dim=1) for k_, v in ctx.items()}
    with pytest.raises(ValueError, match="target"):
        tj.trajectory_cameras(ctx3)
    tgt = dict(extrinsics=T("traj_straddle_b")[None, None], intrinsics=T("traj_Kb")[None, None])
    e3 = tj.trajectory_cameras(ctx3, tgt)[0]
    assert (e3[0] - tj.interpolate_extrinsics(T("traj_generic_a"), T("traj_straddle_b"), t)).abs().max() == 0


# ---- frames ----
def _frame_case(case):
    kinds, axis, gap, frames, dname = case.split("|")
    axis, gap, frames = int(axis), int(gap), int(frames)
    rgb = [T("frames_rgb0"), T("frames_rgb1")]
    depth = T("frames_depth") if dname == "depth" else torch.zeros_like(T("frames_depth"))
    panels = [depth[:frames] if k == "d" else rgb[int(k)][:frames] for k in kinds]
    ref = G[f"frames_{kinds}_a{axis}_g{gap}_f{frames}_{dname}_ref"].transpose(0, 2, 3, 1)
    return kinds, axis, gap, frames, panels, ref


def depth_region(kinds, axis, gap, H, W):
    """(rows, cols) slices of every depth panel in the packed frame"""
    out = []
    for i, k in enumerate(kinds):
        if k == "d":
            lo = i * ((H if axis == 0 else W) + gap)
            out.append((slice(lo, lo + H), slice(None)) if axis == 0 else (slice(None), slice(lo, lo + W)))
    return out


@pytest.mark.parametrize("case", list(G["frames_cases"]))
def test_pack_frames_matches_vcat_hcat_vis_depth_map_and_the_cast(case):
    kinds, axis, gap, frames, panels, ref = _frame_case(case)
    got = ex.pack_frames(panels, axis=axis, gap=gap, loop_reverse=True).numpy()
    assert got.dtype == np.uint8 and got.shape == ref.shape and got.shape[0] == frames + max(frames - 2, 0)
    is_depth = np.zeros(got.shape[:3], bool)
    for rows, cols in depth_region(kinds, axis, gap, 5, 6):
        is_depth[:, rows, cols] = True
    assert np.array_equal(got[~is_depth], ref[~is_depth])                   # RGB and gap bytes: equal
    # depth: equal except where the colour index sits on a node boundary -- at most 1 % of the depth pixels, one LUT step away
    if is_depth.any():
        lut = ex.turbo_table().astype(np.int64)
        key = lambda px: (px.astype(np.int64) * (1, 256, 65536)).sum(-1)
        index_of = {int(k): i for i, k in enumerate(key(lut))}
        g, r = key(got[is_depth]), key(ref[is_depth])
        differ = g != r
        assert differ.mean() <= 0.01
        for a, b in zip(g[differ], r[differ]):
            assert abs(index_of[int(a)] - index_of[int(b)]) == 1


def test_pack_frames_edge_values():
    lut = ex.turbo_table()
    assert lut.shape == (256, 3) and tuple(lut[0]) != tuple(lut[255])
    x = torch.tensor([-0.5, 0.0, 0.5, 1.0, 1.5, float("nan"), 0.999999, 1 / 255]).reshape(1, 1, 1, 8).expand(1, 3, 1, 8)
    got = ex.pack_frames([x], gap=0)[0, 0, :, 0].tolist()
    assert got == [0, 0, 127, 255, 255, 0, 254, 1]
    # a zero depth is turbo's last colour; a negative or NaN depth is black
    d = torch.tensor([[[1.0, 2.0, 0.0, 4.0, -1.0, float("nan"), 3.0, 8.0]]])
    out = ex.pack_frames([d], gap=0, depth_range=torch.tensor([0.0, 2.0]))[0, 0]
    assert tuple(out[2].tolist()) == tuple(lut[255]) and out[4].tolist() == [0, 0, 0] and out[5].tolist() == [0, 0, 0]
    assert tuple(out[0].tolist()) == tuple(lut[255]) and tuple(out[7].tolist()) == tuple(lut[0])      # log 1 = near, log 8 > far
    # an all-zero depth: black panel, the "no positive depth" status, near = 0
    info = {}
    z = torch.zeros(2, 3, 4)
    rng = ex.depth_range(z, details=info)
    assert float(rng[0]) == 0.0 and float(rng[1]) == -np.inf and info["status"].tolist() == [0, _lib.GSR_DEPTH_NO_POSITIVE]
    assert int(ex.pack_frames([z], gap=0).max()) == 0
    with pytest.raises(ValueError):
        ex.pack_frames([x] * 5)
    with pytest.raises(ValueError):
        ex.pack_frames([x, torch.zeros(1, 2, 8)])


def test_depth_range_is_vis_depth_maps_range():
    d = T("frames_depth")
    info = {}
    rng = ex.depth_range(d, details=info)
    assert float(rng[1]) == float(d.view(-1).quantile(0.99).log()) and float(rng[0]) == float(d[d > 0].quantile(0.01).log())
    assert info["status"].tolist() == [int((d > 0).sum()), 0]
    cut = ex.depth_range(d, max_elems=50)
    head = d.reshape(-1)[:50]
    assert float(cut[1]) == float(head.quantile(0.99).log()) and float(cut[0]) == float(head[head > 0].quantile(0.01).log())


# ---- PLY ----
def _ulps(a, b):
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


def check_ply_table(tab, ref, what):
    """the bars of the PLY table: copies bit-equal, log within 4 ulp, quaternions within 2 ulp of 1.0 with the reference's sign"""
    n = tab.shape[1]
    assert tab.shape == ref.shape and tab.dtype == np.float32, what
    copies = np.r_[0:n - 7]
    # (with shift_and_scale x y z went through (m - median) / factor: two correctly rounded fp32 operations on either side)
    assert np.array_equal(tab[:, copies].view(np.int32), ref[:, copies].view(np.int32)), f"{what}: copied columns"
    assert _ulps(tab[:, n - 7:n - 4], ref[:, n - 7:n - 4]).max() <= 4, f"{what}: log(scales)"
    assert np.abs(tab[:, n - 4:] - ref[:, n - 4:]).max() <= 2 * 2.0 ** -23, f"{what}: quaternion"


@pytest.mark.parametrize("d_sh", [1, 4, 25])
@pytest.mark.parametrize("dc_only", [0, 1])
@pytest.mark.parametrize("shift", [0, 1])
def test_ply_vertex_table_matches_the_array_the_reference_hands_to_plyfile(d_sh, dc_only, shift):
    inp = [T(f"ply_d{d_sh}_{k}") for k in ("means", "scales", "rotations", "harmonics", "opacities")]
    tab, names = ex.ply_vertex_table(*inp, shift_and_scale=bool(shift), save_sh_dc_only=bool(dc_only))
    assert names == list(G[f"ply_d{d_sh}_dc{dc_only}_names"]) and len(names) == 17 + (0 if dc_only else 3 * (d_sh - 1))
    check_ply_table(tab.numpy(), G[f"ply_d{d_sh}_dc{dc_only}_shift{shift}_ref"], f"d_sh {d_sh} dc{dc_only} shift{shift}")


def test_export_ply_round_trips_bit_for_bit(tmp_path):
    inp = [T(f"ply_d4_{k}") for k in ("means", "scales", "rotations", "harmonics", "opacities")]
    for dc in (True, False):
        path = tmp_path / "sub" / f"g{int(dc)}.ply"
        ex.export_ply(*inp, path, shift_and_scale=True, save_sh_dc_only=dc)
        tab, names = ex.ply_vertex_table(*inp, shift_and_scale=True, save_sh_dc_only=dc)
        back, back_names = ex.read_ply(path)
        assert back_names == names and np.array_equal(back.view(np.int32), tab.numpy().view(np.int32))
        head = path.read_bytes().split(b"end_header\n")[0].decode().split("\n")
        assert head[:3] == ["ply", "format binary_little_endian 1.0", "element vertex 64"]
        assert [l.split()[2] for l in head[3:] if l] == names and all(l.startswith("property float ") for l in head[3:] if l)
        assert path.stat().st_size == len(b"end_header\n") + sum(len(l) + 1 for l in head if l) + 64 * len(names) * 4
    assert names[:9] == ["x", "y", "z", "nx", "ny", "nz", "f_dc_0", "f_dc_1", "f_dc_2"] and names[9] == "f_rest_0" and names[-8] == "opacity"


# ---- ABI ----
NEW = ("gsr_trajectory", "gsr_outputs_scratch_bytes", "gsr_depth_range", "gsr_pack_frames", "gsr_ply_normalizer", "gsr_ply_rows")


def test_new_entry_points_are_declared_exported_and_check_their_arguments():
    _lib.build_library()
    lib = _lib.load()
    header = (ROOT / "include/gsr.h").read_text()
    for name in NEW:
        assert re.search(rf"\b{name}\s*\(", header) and name in _lib.EXPORTS and hasattr(lib, name), name
    assert "gsr_outputs.hip" in _lib._SOURCES and 0 < lib.gsr_outputs_scratch_bytes() < (1 << 16)
    # GSR_EINVAL before any launch (no device needed)
    assert lib.gsr_trajectory(None, None, None, None, None, 1, 1, 1.0, 0.0, 1e-4, 0, 0.0, 1, 1, None, None, None, None) == -1
    assert lib.gsr_depth_range(None, 10, 10, None, None, None, None) == -1
    assert lib.gsr_pack_frames(None, None, 1, 1, 1, 1, 0, 0, 0, None, None, None) == -1
    assert lib.gsr_ply_normalizer(None, 2, None, None, None) == -1
    assert lib.gsr_ply_rows(None, None, None, None, None, 1, 1, 1, None, None, None) == -1
    import ctypes as C
    one = C.c_void_p(256)       # (non-null, never dereferenced: the dimension checks come first)
    assert lib.gsr_trajectory(one, one, one, one, one, 0, 1, 1.0, 0.0, 1e-4, 0, 0.0, 1, 1, None, one, one, None) == -1
    assert lib.gsr_depth_range(one, 0, 10, one, one, one, None) == -1
    assert lib.gsr_ply_normalizer(one, 1, one, one, None) == -1
    assert lib.gsr_ply_rows(one, one, one, one, one, 0, 1, 1, None, one, None) == -1
    ptrs, flags = (C.c_void_p * 1)(256), (C.c_int32 * 1)(1)
    assert lib.gsr_pack_frames(ptrs, flags, 5, 1, 1, 1, 0, 0, 0, one, one, None) == -1          # five panels
    assert lib.gsr_pack_frames(ptrs, flags, 1, 1, 1, 1, 2, 0, 0, one, one, None) == -1          # axis 2
    assert lib.gsr_pack_frames(ptrs, flags, 1, 1, 1, 1, 0, 0, 0, None, one, None) == -1         # a depth panel without a range


def test_device_entry_points_refuse_cpu_tensors_where_there_is_no_host_path():
    with pytest.raises(RuntimeError, match="HIP"):
        tj.trajectory_hip(torch.eye(4)[None], torch.eye(4)[None], torch.eye(3)[None], torch.eye(3)[None], torch.zeros(2))
