"""Generate tests/golden/colmap_scene/ and tests/golden/colmap_scene.npz: a small synthetic COLMAP model written by the REFERENCE's
own write_* functions (src/dataset/colmap_parsing_utils.py), as text and as binary, and what the reference's own functions return
for it -- its readers, parse_colmap_camera_params, qvec2rotmat, auto_orient_and_center_poses (src/dataset/colmap_utils.py) and the
pose sequence of infer_model_colmap.py:401-435 (inverse, sort by name, orient ("up", "poses"), scale by 1 / max |t|).
Data only: two model directories, one 56-byte cameras.bin of the reference's sample scene, and recorded arrays.  The tests read those
and nothing else.

    python tests/golden/make_colmap_fixtures.py          (where the reference checkout of tests/golden/ref_stubs.py is present)

The model: 12 images whose names are NOT in id order, 3 cameras of one size (SIMPLE_PINHOLE, SIMPLE_RADIAL, OPENCV), at most 5
observations per image (one image has none: its second text line is empty).  The images at name-sorted positions 1..9 belong to
the two cameras with distortion, so that a scene test can select them together.

The driver's lines 401-435 are inline code of a script, not a function: they are restated below on the reference's functions.  Its
`cam.k1` lines (RADIAL / OPENCV) cannot run -- `cam` is a dict -- so nothing of them is recorded; the distortion the package derives
is compared with the dict values of parse_colmap_camera_params instead.  OpenCV is not installed: no undistorted pixels, no K_new.
"""
import importlib
import shutil
import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
ROOT = HERE.parents[1]
sys.path.insert(0, str(ROOT))
OUT_DIR = HERE / "colmap_scene"
OUT = HERE / "colmap_scene.npz"
W, H = 53, 37


def main():
    from tests.golden.ref_stubs import REF, install
    install()
    cpu = importlib.import_module("src.dataset.colmap_parsing_utils")
    cu = importlib.import_module("src.dataset.colmap_utils")
    rng = np.random.default_rng(20240611)

    cameras = {
        1: cpu.Camera(1, "SIMPLE_PINHOLE", W, H, np.array([41.5, W / 2 + 0.25, H / 2 - 0.5])),
        2: cpu.Camera(2, "SIMPLE_RADIAL", W, H, np.array([40.0, W / 2 - 0.3, H / 2 + 0.4, 0.15])),
        3: cpu.Camera(3, "OPENCV", W, H, np.array([40.0, 40.8, W / 2 - 0.3, H / 2 + 0.4, -0.12, 0.03, 0.002, -0.001])),
    }
    # name-sorted position of image id i is (i * 7) % 12; positions 0, 10, 11 -> camera 1, odd others -> 3, even others -> 2
    images = {}
    for k, im_id in enumerate([4, 11, 2, 9, 1, 7, 12, 3, 10, 5, 8, 6]):        # file order is not id order either
        pos = (im_id * 7) % 12
        cam = 1 if pos in (0, 10, 11) else (3 if pos % 2 else 2)
        q = np.array([1.0, 0, 0, 0]) + 0.25 * rng.standard_normal(4)
        q /= np.linalg.norm(q)
        t = np.array([0.4 * pos - 2.0, 0.0, 1.5]) + 0.3 * rng.standard_normal(3)
        n_obs = 0 if k == 3 else int(rng.integers(1, 6))
        xys = np.round(rng.uniform([0, 0], [W, H], size=(n_obs, 2)), 3)
        ids = rng.integers(-1, 200, size=n_obs).astype(np.int64)
        images[im_id] = cpu.Image(id=im_id, qvec=q, tvec=t, camera_id=cam, name=f"frame_{pos:03d}.png", xys=xys, point3D_ids=ids)

    if OUT_DIR.exists():
        shutil.rmtree(OUT_DIR)
    text_dir, bin_dir = OUT_DIR / "text" / "sparse" / "0", OUT_DIR / "binary" / "sparse"
    text_dir.mkdir(parents=True)
    bin_dir.mkdir(parents=True)
    cpu.write_cameras_text(cameras, text_dir / "cameras.txt")
    cpu.write_images_text(images, text_dir / "images.txt")
    cpu.write_cameras_binary(cameras, bin_dir / "cameras.bin")
    cpu.write_images_binary(images, bin_dir / "images.bin")
    shutil.copyfile(Path(REF) / "colmap_test_data/scenes/train/sparse/0/cameras.bin", OUT_DIR / "sample_cameras.bin")

    rec = {}

    def record_cameras(tag, cams):
        ids = sorted(cams)
        rec[f"{tag}_cam_ids"] = np.array(ids, dtype=np.int64)
        rec[f"{tag}_cam_models"] = np.array([cams[i].model for i in ids])
        rec[f"{tag}_cam_sizes"] = np.array([[cams[i].width, cams[i].height] for i in ids], dtype=np.int64)
        rec[f"{tag}_cam_nparams"] = np.array([len(cams[i].params) for i in ids], dtype=np.int64)
        rec[f"{tag}_cam_params"] = np.concatenate([np.asarray(cams[i].params, dtype=np.float64) for i in ids])
        assert all(cams[i].id == i for i in ids)

    def record_images(tag, ims):
        order = list(ims)                                                    # the readers keep file order
        rec[f"{tag}_im_ids"] = np.array(order, dtype=np.int64)
        rec[f"{tag}_im_qvec"] = np.stack([ims[i].qvec for i in order]).astype(np.float64)
        rec[f"{tag}_im_tvec"] = np.stack([ims[i].tvec for i in order]).astype(np.float64)
        rec[f"{tag}_im_camera_ids"] = np.array([ims[i].camera_id for i in order], dtype=np.int64)
        rec[f"{tag}_im_names"] = np.array([ims[i].name for i in order])
        rec[f"{tag}_im_nobs"] = np.array([len(ims[i].point3D_ids) for i in order], dtype=np.int64)
        rec[f"{tag}_im_xys"] = np.concatenate([np.asarray(ims[i].xys, dtype=np.float64).reshape(-1, 2) for i in order])
        rec[f"{tag}_im_point3D_ids"] = np.concatenate([np.asarray(ims[i].point3D_ids, dtype=np.int64).reshape(-1) for i in order])
        assert all(ims[i].id == i for i in order)

    cams_t, ims_t = cpu.read_cameras_text(text_dir / "cameras.txt"), cpu.read_images_text(text_dir / "images.txt")
    cams_b, ims_b = cpu.read_cameras_binary(bin_dir / "cameras.bin"), cpu.read_images_binary(bin_dir / "images.bin")
    record_cameras("text", cams_t)
    record_images("text", ims_t)
    record_cameras("bin", cams_b)
    record_images("bin", ims_b)
    record_cameras("sample", cpu.read_cameras_binary(OUT_DIR / "sample_cameras.bin"))

    keys = ("w", "h", "fl_x", "fl_y", "cx", "cy", "k1", "k2", "p1", "p2")
    parsed = {i: cu.parse_colmap_camera_params(cams_b[i]) for i in sorted(cams_b)}
    rec["parsed_values"] = np.array([[float(parsed[i][k]) for k in keys] for i in sorted(parsed)], dtype=np.float64)
    rec["parsed_models"] = np.array([parsed[i]["model"] for i in sorted(parsed)])

    ordered = sorted(ims_b)
    rec["rotmats"] = np.stack([cpu.qvec2rotmat(ims_b[i].qvec) for i in ordered])

    # infer_model_colmap.py:341-346 and 401-435 on the reference's functions
    bottom = np.array([0, 0, 0, 1]).reshape(1, 4)
    w2c = np.stack([np.concatenate([np.concatenate([cpu.qvec2rotmat(ims_b[i].qvec), ims_b[i].tvec.reshape(3, 1)], 1), bottom], axis=0)
                    for i in ordered], axis=0)
    c2w = np.linalg.inv(w2c)
    names = [ims_b[i].name for i in ordered]
    inds = np.argsort(names)
    c2w_sorted = c2w[inds]
    oriented, transform = cu.auto_orient_and_center_poses(c2w_sorted, method="up", center_method="poses")
    rec["orient_in"] = c2w_sorted
    rec["orient_up_poses"], rec["orient_up_poses_T"] = oriented.copy(), transform.copy()
    for method, center in (("up", "none"), ("none", "poses"), ("none", "none")):
        o, t = cu.auto_orient_and_center_poses(c2w_sorted, method=method, center_method=center)
        rec[f"orient_{method}_{center}"], rec[f"orient_{method}_{center}_T"] = o, t
    scale_factor = 1.0
    scale_factor /= float(np.max(np.abs(oriented[:, :3, 3])))
    oriented[:, :3, 3] *= scale_factor
    rec["scene_camtoworlds"] = np.concatenate((oriented, np.repeat(bottom[np.newaxis, :], oriented.shape[0], axis=0)), axis=1).astype(np.float64)
    rec["scene_transform"] = transform
    rec["scene_scale_factor"] = np.float64(scale_factor)
    rec["scene_names"] = np.array([names[i] for i in inds])
    rec["scene_camera_ids"] = np.array([ims_b[ordered[i]].camera_id for i in inds], dtype=np.int64)

    assert list(rec["scene_names"]) == [f"frame_{p:03d}.png" for p in range(12)]
    assert set(rec["scene_camera_ids"][1:10]) == {2, 3} and set(rec["scene_camera_ids"][[0, 10, 11]]) == {1}
    np.savez_compressed(OUT, **rec)
    total = OUT.stat().st_size + sum(p.stat().st_size for p in OUT_DIR.rglob("*") if p.is_file())
    print(f"wrote {OUT} and {OUT_DIR}: {total} bytes")
    assert total < 64 * 1024


if __name__ == "__main__":
    main()
