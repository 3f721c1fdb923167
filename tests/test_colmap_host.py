"""CPU tests (-m "not gpu") of styl3r_amd/colmap.py and inference.prepare_colmap_scene: the COLMAP readers and the pose sequence
against what the reference's own functions returned for the synthetic model of tests/golden/make_colmap_fixtures.py, view selection,
the refusals, the undistortion arithmetic on known answers that need no oracle, `optimal_new_camera`, the argument checks of
gsr_undistort (they answer before any launch, so no device is needed) and the scene hand-over."""
import dataclasses
import re
import shutil
from pathlib import Path

import numpy as np
import pytest
import torch

from styl3r_amd import _lib, colmap, inference
from styl3r_amd.inputs import InputCfg

ROOT = Path(__file__).resolve().parents[1]
GOLD_DIR = ROOT / "tests/golden/colmap_scene"
GOLD = np.load(ROOT / "tests/golden/colmap_scene.npz")
TEXT, BINARY = GOLD_DIR / "text" / "sparse" / "0", GOLD_DIR / "binary" / "sparse"
OPENCV_DIST = (-0.12, 0.03, 0.002, -0.001)


def sketch_K(W=53, H=37, f=40.0):
    return np.array([[f, 0, W / 2 - 0.3], [0, f * 1.02, H / 2 + 0.4], [0, 0, 1]])


@pytest.fixture(scope="module")
def lib():
    _lib.build_library()
    return _lib.load()


# --------------------------------------------------------------------------- readers
def check_cameras(tag, cams):
    ids = sorted(cams)
    assert ids == GOLD[f"{tag}_cam_ids"].tolist()
    assert [cams[i].model for i in ids] == GOLD[f"{tag}_cam_models"].tolist()
    assert [[cams[i].width, cams[i].height] for i in ids] == GOLD[f"{tag}_cam_sizes"].tolist()
    assert [len(cams[i].params) for i in ids] == GOLD[f"{tag}_cam_nparams"].tolist()
    params = np.concatenate([cams[i].params for i in ids])
    assert params.dtype == np.float64 and np.array_equal(params, GOLD[f"{tag}_cam_params"])
    assert all(cams[i].id == i and isinstance(cams[i].width, int) for i in ids)


def check_images(tag, ims):
    order = list(ims)
    assert order == GOLD[f"{tag}_im_ids"].tolist()                       # file order, as the reference's dict
    assert np.array_equal(np.stack([ims[i].qvec for i in order]), GOLD[f"{tag}_im_qvec"])
    assert np.array_equal(np.stack([ims[i].tvec for i in order]), GOLD[f"{tag}_im_tvec"])
    assert [ims[i].camera_id for i in order] == GOLD[f"{tag}_im_camera_ids"].tolist()
    assert [ims[i].name for i in order] == GOLD[f"{tag}_im_names"].tolist()
    assert [len(ims[i].point3D_ids) for i in order] == GOLD[f"{tag}_im_nobs"].tolist()
    assert all(ims[i].xys.shape == (len(ims[i].point3D_ids), 2) and ims[i].xys.dtype == np.float64 for i in order)
    assert np.array_equal(np.concatenate([ims[i].xys for i in order]), GOLD[f"{tag}_im_xys"])
    assert np.array_equal(np.concatenate([ims[i].point3D_ids for i in order]), GOLD[f"{tag}_im_point3D_ids"])
    assert all(ims[i].id == i for i in order) and 0 in GOLD[f"{tag}_im_nobs"]        # one image without observations


def test_text_readers_equal_the_reference():
    check_cameras("text", colmap.read_cameras_text(TEXT / "cameras.txt"))
    check_images("text", colmap.read_images_text(TEXT / "images.txt"))


def test_binary_readers_equal_the_reference():
    check_cameras("bin", colmap.read_cameras_binary(BINARY / "cameras.bin"))
    check_images("bin", colmap.read_images_binary(BINARY / "images.bin"))
    check_cameras("sample", colmap.read_cameras_binary(GOLD_DIR / "sample_cameras.bin"))


def test_read_model_finds_either_format(tmp_path):
    for d, tag in ((TEXT, "text"), (BINARY, "bin")):
        cams, ims = colmap.read_model(d)
        check_cameras(tag, cams)
        check_images(tag, ims)
    with pytest.raises(ValueError):
        colmap.read_model(tmp_path)
    (tmp_path / "cameras.bin").write_bytes((BINARY / "cameras.bin").read_bytes()[:-3])
    with pytest.raises(ValueError, match="ends inside"):
        colmap.read_cameras_binary(tmp_path / "cameras.bin")


def test_camera_params_and_qvec2rotmat_equal_the_reference():
    cams, ims = colmap.read_model(BINARY)
    keys = ("w", "h", "fl_x", "fl_y", "cx", "cy", "k1", "k2", "p1", "p2")
    for row, model, cid in zip(GOLD["parsed_values"], GOLD["parsed_models"], sorted(cams)):
        got = colmap.camera_params(cams[cid])
        assert list(got) == [*keys, "model"] and got["model"] == model
        assert np.array_equal(np.array([float(got[k]) for k in keys]), row)
    radial = colmap.camera_params(colmap.Camera(7, "RADIAL", 10, 8, np.array([5.0, 4.0, 3.0, 0.1, -0.2])))
    assert [radial[k] for k in keys] == [10, 8, 5.0, 5.0, 4.0, 3.0, 0.1, -0.2, 0.0, 0.0]
    pinhole = colmap.camera_params(colmap.Camera(8, "PINHOLE", 10, 8, np.array([5.0, 6.0, 4.0, 3.0])))
    assert [pinhole[k] for k in keys] == [10, 8, 5.0, 6.0, 4.0, 3.0, 0.0, 0.0, 0.0, 0.0]
    rot = np.stack([colmap.qvec2rotmat(ims[i].qvec) for i in sorted(ims)])
    assert np.array_equal(rot, GOLD["rotmats"])


def test_refused_camera_models_and_orientation_methods():
    for model in ("OPENCV_FISHEYE", "FULL_OPENCV", "FOV", "SIMPLE_RADIAL_FISHEYE", "RADIAL_FISHEYE", "THIN_PRISM_FISHEYE", "NO_SUCH"):
        with pytest.raises(ValueError, match="perspective only"):
            colmap.camera_params(colmap.Camera(1, model, 10, 8, np.zeros(12)))
    poses = GOLD["orient_in"]
    for kwargs in (dict(method="pca"), dict(method="vertical"), dict(center_method="focus")):
        with pytest.raises(NotImplementedError, match="not implemented"):
            colmap.auto_orient_and_center_poses(poses, **kwargs)
    with pytest.raises(ValueError):
        colmap.auto_orient_and_center_poses(poses, method="sideways")
    with pytest.raises(ValueError):
        colmap.auto_orient_and_center_poses(poses, center_method="sideways")


def test_auto_orient_equals_the_reference():
    """the same float64 numpy operations in the same order as the reference: the results come out bit-equal, so that is asserted"""
    poses = GOLD["orient_in"]
    for method, center in (("up", "poses"), ("up", "none"), ("none", "poses"), ("none", "none")):
        out, transform = colmap.auto_orient_and_center_poses(poses, method, center)
        assert out.shape == (12, 3, 4) and transform.shape == (3, 4)
        assert np.array_equal(out, GOLD[f"orient_{method}_{center}"])
        assert np.array_equal(transform, GOLD[f"orient_{method}_{center}_T"])
    R = colmap.rotation_matrix_between(np.array([0.0, 0, 2]), np.array([0.0, 0, -1]))             # anti-parallel: the fallback axis
    assert np.allclose(R @ np.array([0, 0, 1.0]), [0, 0, -1], atol=1e-12) and np.allclose(R @ R.T, np.eye(3), atol=1e-12)


@pytest.fixture(scope="module")
def scenes(tmp_path_factory):
    """both fixture models as captures on disk: git keeps no empty `images` folder, so each is copied next to a fresh one"""
    out = {}
    for tag in ("text", "binary"):
        root = tmp_path_factory.mktemp(tag) / "capture"
        shutil.copytree(GOLD_DIR / tag, root)
        (root / "images").mkdir()
        out[tag] = colmap.load_colmap_scene(root)
    return out


@pytest.mark.parametrize("tag", ["text", "binary"])
def test_load_colmap_scene_equals_the_reference_sequence(scenes, tag):
    sc = scenes[tag]
    assert sc.image_names == GOLD["scene_names"].tolist() and sc.camera_ids == GOLD["scene_camera_ids"].tolist()
    assert [Path(p).name for p in sc.image_paths] == sc.image_names and Path(sc.image_paths[0]).parent.name == "images"
    assert sc.camtoworlds.shape == (12, 4, 4) and sc.transform.shape == (3, 4) and sc.name == "capture"
    # the same float64 numpy operations as the reference's sequence: bit-equal (the issue's fallback bound was 1e-12 absolute)
    assert np.array_equal(sc.camtoworlds, GOLD["scene_camtoworlds"]) and sc.camtoworlds.dtype == np.float64
    assert np.array_equal(sc.transform, GOLD["scene_transform"]) and sc.scale_factor == float(GOLD["scene_scale_factor"])
    assert np.abs(sc.camtoworlds[:, :3, 3]).max() == pytest.approx(1.0, abs=1e-15)
    # cameras: intrinsics and distortion from the parsed dict, the distortion rounded through fp32
    parsed = {cid: row for cid, row in zip((1, 2, 3), GOLD["parsed_values"])}
    assert sorted(sc.Ks) == [1, 2, 3] and sc.sizes == {1: (53, 37), 2: (53, 37), 3: (53, 37)}
    for cid, row in parsed.items():
        w, h, fx, fy, cx, cy = row[:6]
        assert np.array_equal(sc.raw_Ks[cid], np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]]))
    assert sc.dist[1].shape == (0,) and np.array_equal(sc.dist[2], np.float32([0.15, 0, 0, 0]).astype(np.float64))
    assert np.array_equal(sc.dist[3], np.float32(OPENCV_DIST).astype(np.float64)) and sc.dist[3][0] != -0.12
    assert np.array_equal(sc.Ks[1], sc.raw_Ks[1]) and sc.rois[1] == (0, 0, 53, 37)
    for cid in (2, 3):
        new_K, roi = colmap.optimal_new_camera(sc.raw_Ks[cid], sc.dist[cid], (53, 37))
        assert np.array_equal(sc.Ks[cid], new_K) and sc.rois[cid] == roi == (0, 0, 52, 36)
        assert not np.array_equal(sc.Ks[cid], sc.raw_Ks[cid])


def test_load_colmap_scene_refusals(tmp_path):
    with pytest.raises(ValueError, match="does not exist"):
        colmap.load_colmap_scene(tmp_path)
    shutil.copytree(GOLD_DIR / "binary", tmp_path / "c")
    with pytest.raises(ValueError, match="Image folder"):
        colmap.load_colmap_scene(tmp_path / "c")
    fish = tmp_path / "fish" / "sparse"
    fish.mkdir(parents=True)
    (fish / "cameras.txt").write_text("1 OPENCV_FISHEYE 10 8 5 5 5 4 0 0 0 0\n")
    (fish / "images.txt").write_text("1 1 0 0 0 0 0 0 1 a.png\n\n")
    with pytest.raises(ValueError, match="perspective only"):
        colmap.load_colmap_scene(tmp_path / "fish")


# --------------------------------------------------------------------------- view selection
def test_select_colmap_views_known_answers():
    ctx, tgt = colmap.select_colmap_views([1, 9], 4)
    assert ctx.tolist() == [1, 3, 6, 9] and tgt.tolist() == [2, 4, 5, 7, 8] and ctx.dtype == tgt.dtype == torch.int64
    ctx, tgt = colmap.select_colmap_views(torch.tensor([1, 9]), 2)
    assert ctx.tolist() == [1, 9] and tgt.tolist() == [2, 3, 4, 5, 6, 7, 8]
    ctx, tgt = colmap.select_colmap_views([0, 5, 11], 3)
    assert ctx.tolist() == [0, 5, 11] and tgt.tolist() == [1, 2, 3, 4, 6, 7, 8, 9, 10]
    ctx, tgt = colmap.select_colmap_views([2, 4], 3)
    assert ctx.tolist() == [2, 3, 4] and tgt.tolist() == [2, 3]           # nothing left: the whole range [left, right) is rendered
    ctx, tgt = colmap.select_colmap_views([3], 2)                            # one index, two views: taken as it is, an empty range
    assert ctx.tolist() == [3] and tgt.tolist() == []
    with pytest.raises(ValueError, match="more context indices"):
        colmap.select_colmap_views([1, 4, 9], 2)


# --------------------------------------------------------------------------- undistortion: known answers
def known_answer_cases():
    """a 9 x 13 random byte frame, zero distortion: (name, new_K, expected (9,13,3) bytes)"""
    rng = np.random.default_rng(5)
    img = rng.integers(0, 256, size=(9, 13, 3), dtype=np.uint8)
    K = np.array([[11.0, 0, 6.25], [0, 10.5, 4.75], [0, 0, 1]])
    shift = lambda dx, dy: np.array([[11.0, 0, 6.25 + dx], [0, 10.5, 4.75 + dy], [0, 0, 1]])
    wide = img.astype(np.int64)
    right = np.concatenate([wide[:, 1:], np.zeros((9, 1, 3), np.int64)], axis=1)      # the neighbour at x + 1, zero past the edge
    moved = np.zeros_like(img)
    moved[2:, :10] = img[:7, 3:]                                       # out(u, v) = in(u + 3, v - 2)
    return img, K, [("identity", K, img), ("shift", shift(-3, 2), moved),
                    ("half", shift(-0.5, 0), ((wide + right + 1) >> 1).astype(np.uint8)),
                    ("tie_to_even", shift(-1 / 64, 0), img),             # 32 u + 0.5 rounds to the even 32 u: weight 0, not 1/32
                    ("three_64ths", shift(-3 / 64, 0), ((30 * wide + 2 * right + 16) >> 5).astype(np.uint8))]     # 32 u + 1.5 -> 32 u + 2


def test_undistort_known_answers_host():
    img, K, cases = known_answer_cases()
    frames = torch.from_numpy(img[None])
    for name, new_K, want in cases:
        for dist in ((0.0, 0.0, 0.0, 0.0), ()):
            out = colmap.undistort_frames(frames, colmap.UndistortCamera(K, np.array(dist)), [0], new_K=new_K, roi=(0, 0, 13, 9))
            assert out.dtype == torch.uint8 and out.shape == (1, 9, 13, 3)
            assert np.array_equal(out[0].numpy(), want), (name, dist)
    # the tie case told apart from round-half-up: that rule would blend 1/32 of the neighbour into almost every pixel
    half_up = ((31 * img.astype(np.int64) + np.concatenate([img[:, 1:], np.zeros((9, 1, 3), np.uint8)], 1) + 16) >> 5).astype(np.uint8)
    assert (half_up != img).mean() > 0.5
    # no distortion and no new matrix: the copy path, through any window, zero outside the frame
    cam = colmap.UndistortCamera(K)
    assert np.array_equal(colmap.undistort_frames(frames, cam, [0])[0].numpy(), img)
    win = colmap.undistort_frames(frames, cam, [0], roi=(-2, 5, 6, 7))[0].numpy()
    want = np.zeros((7, 6, 3), np.uint8)
    want[:4, 2:] = img[5:, :4]
    assert np.array_equal(win, want)


def test_undistort_frames_refusals():
    img, K, _ = known_answer_cases()
    frames = torch.from_numpy(img[None]).repeat(2, 1, 1, 1)
    cams = {4: colmap.UndistortCamera(K, roi=(0, 0, 13, 9)), 9: colmap.UndistortCamera(K, roi=(1, 1, 12, 8))}
    with pytest.raises(ValueError, match="one ROI size"):
        colmap.undistort_frames(frames, cams, [4, 9])
    with pytest.raises(ValueError, match="not among"):
        colmap.undistort_frames(frames, cams, [4, 5])
    with pytest.raises(ValueError, match="empty ROI"):
        colmap.undistort_frames(frames, cams, [4, 4], roi=(0, 0, 0, 9))
    with pytest.raises(ValueError, match="frame cameras for"):
        colmap.undistort_frames(frames, cams, [4])
    with pytest.raises(ValueError, match="uint8"):
        colmap.undistort_frames(frames.float(), cams, [4, 4])
    with pytest.raises(ValueError, match="their camera is"):
        colmap.undistort_frames(frames, colmap.UndistortCamera(K, size=(14, 9)), [0, 0])
    assert colmap.undistort_frames(frames, cams, [9, 9]).shape == (2, 8, 12, 3)


# --------------------------------------------------------------------------- the new camera
def test_optimal_new_camera_zero_distortion():
    # a power-of-two focal length and grid steps that are exact in fp32: every step of the procedure is exact
    K = np.array([[32.0, 0, 6.25], [0, 64.0, 4.5], [0, 0, 1]])
    new_K, roi = colmap.optimal_new_camera(K, np.zeros(4), (13, 9))
    assert np.array_equal(new_K, K) and roi == (0, 0, 12, 8)
    # any other camera: the grid passes through fp32 once, 2^-24 relative per coordinate; the quotient of a length by a difference
    # of two such coordinates of magnitude <= 1 and distance >= 1 is within 2^-22 relative, cx' = -fx' x0 likewise on its own scale
    K = sketch_K()
    new_K, roi = colmap.optimal_new_camera(K, np.zeros(4), (53, 37))
    assert roi == (0, 0, 52, 36)
    assert np.abs(new_K - K).max() <= 2.0 ** -22 * 53 and new_K[0, 1] == new_K[1, 0] == 0 and new_K[2, 2] == 1
    with pytest.raises(ValueError, match="k1, k2, p1, p2"):
        colmap.optimal_new_camera(K, np.zeros(5), (53, 37))


@pytest.mark.parametrize("dist", [OPENCV_DIST, (0.15, 0.0, 0.0, 0.0)])
def test_optimal_new_camera_roi_maps_into_the_source(dist):
    K, d = sketch_K(), np.float32(dist).astype(np.float64)
    new_K, roi = colmap.optimal_new_camera(K, d, (53, 37))
    assert roi == (0, 0, 52, 36)                                           # from a float64 sketch of the same procedure
    assert new_K[0, 0] != K[0, 0] and np.isfinite(new_K).all()
    table, index, (rw, rh), rois = colmap.undistort_table((37, 53), colmap.UndistortCamera(K, d), [0])
    assert (rw, rh) == (52, 36) and rois == [roi] and index.tolist() == [0] and table.shape == (1, _lib.GSR_UNDISTORT_CAM_DOUBLES)
    mx, my = colmap._source_maps(table[0], rw, rh)
    assert mx.dtype == np.float32 and mx.shape == (36, 52)
    assert mx.min() >= -1 and mx.max() <= 53 and my.min() >= -1 and my.max() <= 37      # the source image extended by one pixel


# --------------------------------------------------------------------------- C ABI
def test_undistort_is_declared_and_exported(lib):
    header = (ROOT / "include/gsr.h").read_text()
    assert "gsr_undistort" in _lib.EXPORTS and re.search(r"\bgsr_undistort\s*\(", header) and hasattr(lib, "gsr_undistort")
    assert "gsr_undistort.hip" in _lib._SOURCES and (ROOT / "styl3r_amd/csrc/gsr_undistort.hip").is_file()
    assert f"#define GSR_UNDISTORT_CAM_DOUBLES {_lib.GSR_UNDISTORT_CAM_DOUBLES}\n" in header
    assert f"#define GSR_UNDISTORT_FRAMES_PER_LAUNCH {_lib.GSR_UNDISTORT_FRAMES_PER_LAUNCH}\n" in header
    source = (ROOT / "styl3r_amd/csrc/gsr_undistort.hip").read_text()
    code = source[source.index("#include"):]
    assert "#pragma clang fp contract(off)" in code and "atomic" not in code.lower() and "__shared__" not in code


def test_undistort_argument_checks_answer_before_any_launch(lib):
    """every refusal is decided on the host before the first launch: the pointers are never followed (they are host buffers here)"""
    src = np.zeros((2, 9, 13, 3), np.uint8)
    dst = np.zeros((2, 9, 13, 3), np.uint8)
    cams = np.zeros((2, _lib.GSR_UNDISTORT_CAM_DOUBLES))
    fc = np.array([0, 1], np.int32)
    p = lambda a: a.ctypes.data

    def call(src_p=p(src), N=2, H=9, W=13, cams_p=p(cams), n_cams=2, fc_a=fc, roi_w=13, roi_h=9, dst_p=p(dst)):
        return lib.gsr_undistort(src_p, N, H, W, cams_p, n_cams, None if fc_a is None else p(fc_a), roi_w, roi_h, dst_p, None)
    bad = [dict(src_p=None), dict(cams_p=None), dict(fc_a=None), dict(dst_p=None), dict(N=0), dict(H=0), dict(W=0), dict(H=32768), dict(W=32768),
           dict(n_cams=0), dict(n_cams=65536), dict(fc_a=np.array([0, 2], np.int32)), dict(fc_a=np.array([-1, 0], np.int32)),
           dict(n_cams=1), dict(roi_w=0), dict(roi_h=0), dict(roi_w=-3), dict(roi_w=32768), dict(roi_h=32768),
           dict(dst_p=p(dst) + 1), dict(cams_p=p(cams) + 4)]
    for kwargs in bad:
        assert call(**kwargs) == -1, kwargs


# --------------------------------------------------------------------------- the scene hand-over
def scene_frames(n=12, seed=11):
    return torch.from_numpy(np.random.default_rng(seed).integers(0, 256, size=(n, 37, 53, 3), dtype=np.uint8))


def test_prepare_colmap_scene_equals_prepare_scene_fed_by_hand(scenes):
    sc = scenes["binary"]
    frames = scene_frames()
    cfg = InputCfg(input_image_shape=(24, 32))
    style = torch.from_numpy(np.random.default_rng(3).integers(0, 256, size=(40, 50, 3), dtype=np.uint8))
    context, styles, target = inference.prepare_colmap_scene(sc, [1, 9], 4, [style], cfg, frames=frames)
    sel = [1, 3, 6, 9, 2, 4, 5, 7, 8]
    cam_ids = [sc.camera_ids[i] for i in sel]
    assert set(cam_ids) == {2, 3}                                          # both cameras with distortion, one ROI size
    und = colmap.undistort_frames(frames[sel], sc, cam_ids)
    assert und.shape == (9, 36, 52, 3)
    K = np.stack([sc.Ks[c] for c in cam_ids])
    want_c, want_s, want_t = inference.prepare_scene(und, torch.from_numpy(K), torch.from_numpy(sc.camtoworlds[sel]), range(4), range(4, 9), [style],
                                                     cfg, pixel_intrinsics=True)
    for got, want, idx in ((context, want_c, sel[:4]), (target, want_t, sel[4:])):
        for key in ("image", "extrinsics", "intrinsics", "near", "far"):
            assert got[key].dtype == want[key].dtype and torch.equal(got[key], want[key]), key
        assert got["index"].tolist() == [idx]
    assert context["image"].shape == (1, 4, 3, 24, 32) and target["image"].shape == (1, 5, 3, 24, 32) and torch.equal(styles[0], want_s[0])
    # a ROI that does not start at (0, 0) moves the principal point
    moved = dataclasses.replace(sc, rois={**sc.rois, 2: (1, 0, 52, 36), 3: (1, 0, 52, 36)})
    c2, _, _ = inference.prepare_colmap_scene(moved, [1, 9], 4, [style], cfg, frames=frames)
    dx = (context["intrinsics"][0, :, 0, 2] - c2["intrinsics"][0, :, 0, 2]) * 52
    assert torch.allclose(dx, torch.ones(4), atol=1e-5) and torch.equal(context["intrinsics"][0, :, 1, 2], c2["intrinsics"][0, :, 1, 2])
    # cameras of different ROI sizes in one selection are refused
    with pytest.raises(ValueError, match="one ROI size"):
        inference.prepare_colmap_scene(sc, [0, 4], 2, [style], cfg, frames=frames)


def test_prepare_colmap_scene_reads_only_the_selected_frames(scenes, tmp_path):
    from PIL import Image as PILImage
    sc = scenes["text"]
    frames = scene_frames()
    sel = [2, 3, 4, 2, 3]                                                  # context [2, 3, 4] leaves no target: the range [2, 4) is rendered
    paths = list(sc.image_paths)
    for i in set(sel):
        paths[i] = str(tmp_path / sc.image_names[i])
        rgba = np.concatenate([frames[i].numpy(), np.full((37, 53, 1), 200, np.uint8)], axis=2) if i == 3 else frames[i].numpy()
        PILImage.fromarray(rgba).save(paths[i])                         # one RGBA file: the first three channels are kept
    on_disk = dataclasses.replace(sc, image_paths=paths)                   # every other path names a file that does not exist
    cfg = InputCfg(input_image_shape=(24, 32))
    style = torch.zeros(3, 30, 30)
    a = inference.prepare_colmap_scene(on_disk, [2, 4], 3, [style], cfg)
    b = inference.prepare_colmap_scene(sc, [2, 4], 3, [style], cfg, frames=frames)
    assert a[0]["index"].tolist() == [[2, 3, 4]] and a[2]["index"].tolist() == [[2, 3]]
    assert torch.equal(a[0]["image"], b[0]["image"]) and torch.equal(a[2]["image"], b[2]["image"])
    assert torch.equal(colmap.read_frames([paths[2], paths[3]]), frames[[2, 3]])
    PILImage.fromarray(np.zeros((5, 6, 3), np.uint8)).save(tmp_path / "small.png")
    with pytest.raises(ValueError, match="read_frames"):
        colmap.read_frames([paths[2], tmp_path / "small.png"])
