"""CPU: styl3r_amd/inputs.py on CPU tensors -- the integer restatement of the 8-bit Lanczos resize over the library's host-built axis
plans, the crop / augmentation shims and the camera arithmetic of `prepare_example` -- against what the reference's own functions
returned for the same inputs through PIL (tests/golden/scene_inputs.npz, written by tests/golden/make_scene_input_fixtures.py), and
the C ABI of csrc/gsr_inputs.hip as far as it goes without a device.  Images and intrinsics are compared bit for bit.  This path is
the yardstick of tests/test_gpu_scene_inputs.py."""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest
import torch

from styl3r_amd import _lib
from styl3r_amd import inputs as si

ROOT = Path(__file__).resolve().parent.parent
G = np.load(ROOT / "tests/golden/scene_inputs.npz")
T = lambda k: torch.from_numpy(G[k])
IMAGE_CASES = [str(k) for k in G["image_cases"]]
ULP1 = 2.0 ** -23
bits = lambda t: (t if isinstance(t, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(t))).detach().cpu().contiguous().view(torch.int32)


def same_bits(a, b) -> bool:
    a, b = bits(a), bits(b)
    return a.shape == b.shape and torch.equal(a, b)


def case_input(key, as_bytes=False):
    """the fixture's input: uint8 (H,W,3) as recorded, or the float (3,H,W) image the reference was fed"""
    x = T(key + "_in")
    if x.dtype == torch.uint8 and not as_bytes:
        return x.permute(2, 0, 1).float() / 255
    return x


def run_case(key, x, flags=0):
    """-> (image, intrinsics or None) of fixture case `key` on input `x` (its device decides the path)"""
    kind, size, _ = key.split("_", 2)
    ref = G[key + "_ref"]
    if kind == "rc":
        if flags:
            h, w = si._image_hw(x)
            hs, ws = si.scaled_size(h, w, ref.shape[-2:])
            win = ((hs - ref.shape[-2]) // 2, (ws - ref.shape[-1]) // 2, *ref.shape[-2:])
            return si.resample_crop(x, (hs, ws), win, flags=flags), None
        return si.rescale_and_crop(x, T(key + "_K").to(x.device), tuple(ref.shape[-2:]))
    if kind == "rs":
        return si.resample_crop(x, tuple(ref.shape[-2:]), flags=flags), None
    if flags:
        hs, ws, top, left = (int(v) for v in G[key + "_rule"])
        return si.resample_crop(x, (hs, ws), (top, left, ref.shape[-1], ref.shape[-1]), flags=flags), None
    return si.apply_style_image_augmentation(x, "val", size=ref.shape[-1]), None


@pytest.mark.parametrize("key", IMAGE_CASES)
def test_every_fixture_case_is_bit_equal_to_the_reference(key):
    img, K = run_case(key, case_input(key))
    assert img.dtype == torch.float32 and same_bits(img, G[key + "_ref"]), key
    if K is not None:
        assert same_bits(K, G[key + "_K_ref"]), key
    if key.endswith("_white"):
        assert (img == 1.0).all()
    if key.endswith("_black"):
        assert (img == 0.0).all()
    x = T(key + "_in")
    if x.dtype == torch.uint8:                       # bytes in give what the float image built from them gives
        assert same_bits(run_case(key, x)[0], G[key + "_ref"]), key


def test_style_rule_uses_the_half_to_even_offset():
    assert si.style_scaled_size(20, 31, 32) == (32, 49) and si.style_scaled_size(20, 35, 32) == (32, 56)
    assert list(G["st_20x31_random_rule"]) == [32, 49, 0, 8] and list(G["st_20x35_random_rule"]) == [32, 56, 0, 12]
    assert (49 - 32) // 2 == 8 and int(round((49 - 32) / 2.0)) == 8 and int(round((51 - 32) / 2.0)) == 10 != (51 - 32) // 2
    assert si.style_scaled_size(31, 20, 352) == (int(31 / 20 * 352), 352)


def test_quantisation_of_floats_and_nan():
    x = torch.tensor([-0.5, 0.0, 0.999 / 255, 1.0 / 255, 0.5, 1.0, 1.7, float("nan"), float("inf"), -float("inf")])
    assert si.quantise(x).tolist() == [0, 0, 0, 1, 127, 255, 255, 0, 255, 0]
    every = torch.arange(256, dtype=torch.uint8)
    assert torch.equal(si.quantise(every.float() / 255), every)            # uint8 -> / 255 -> * 255 -> truncate is the identity
    same = si.rescale(torch.full((3, 24, 24), float("nan")), (24, 24))
    assert (same == 0).all()


def test_resample_plan_equals_the_recorded_tables():
    for n, m in G["plan_cases"]:
        k, bounds, coeffs = si.resample_plan(int(n), int(m))
        assert k == 2 * int(np.ceil(3 * max(n / m, 1))) + 1 == coeffs.shape[1]
        assert np.array_equal(bounds, G[f"plan_{n}_{m}_bounds"]) and np.array_equal(coeffs, G[f"plan_{n}_{m}_coeffs"]), (n, m)
        assert (bounds[:, 0] >= 0).all() and (bounds[:, 0] + bounds[:, 1] <= n).all() and (bounds[:, 1] <= k).all()
        assert (np.diff(bounds[:, 0]) >= 0).all() and (np.diff(bounds.sum(1)) >= 0).all()      # the kernel's segment rule
    assert si.resample_plan(130, 16)[0] == 51 and si.resample_plan(97, 12)[0] == 51 and si.resample_plan(360, 256)[0] == 11


def test_flip_is_applied_before_the_rescale():
    frames, K = T("flip_frames"), T("flip_K")
    plain, Kp = si.rescale_and_crop(frames, K, (16, 16))
    assert same_bits(plain, G["flip_plain_ref"]) and same_bits(Kp, G["flip_K_ref"])
    mirrored, _ = si.rescale_and_crop(frames, K, (16, 16), flip=True)
    assert same_bits(mirrored, G["flip_mirrored_ref"])
    assert not same_bits(mirrored, plain.flip(-1))                            # flipping at the store would be another image
    mixed, _ = si.rescale_and_crop(frames, K, (16, 16), flip=[False, True, False])
    assert same_bits(mixed[0], plain[0]) and same_bits(mixed[1], mirrored[1]) and same_bits(mixed[2], plain[2])
    # leading batch axes, as in the reference
    two, K2 = si.rescale_and_crop(frames[None].expand(2, -1, -1, -1, -1), K[None].expand(2, -1, -1, -1), (16, 16))
    assert two.shape == (2, 3, 3, 16, 16) and same_bits(two[1], plain) and same_bits(K2[0], Kp)


def test_center_crop_reflect_and_the_augmentation_draw():
    img, K = si.center_crop(T("cc_in"), T("cc_K"), (4, 5))
    assert same_bits(img, G["cc_ref"]) and same_bits(K, G["cc_K_ref"])
    x = T("flip_frames").permute(0, 3, 1, 2).float() / 255
    views = {"image": x, "extrinsics": T("flip_extrinsics"), "intrinsics": T("flip_K")}
    refl = si.reflect_views(views)
    assert same_bits(refl["image"], G["flip_reflect_image_ref"]) and same_bits(refl["extrinsics"], G["flip_reflect_extrinsics_ref"])
    assert refl["intrinsics"] is views["intrinsics"]
    example = {"context": views, "target": views, "scene": "s"}
    for seed, reflects in enumerate(G["aug_reflects"]):
        got = si.apply_augmentation_shim(example, torch.Generator().manual_seed(seed))
        assert (got is not example) == bool(reflects), seed
        if reflects:
            assert same_bits(got["target"]["extrinsics"], G["flip_reflect_extrinsics_ref"]) and got["scene"] == "s"
    shim = si.apply_crop_shim({"context": views, "target": views, "scene": "s"}, (16, 16))
    assert same_bits(shim["context"]["image"], G["flip_plain_ref"]) and same_bits(shim["target"]["intrinsics"], G["flip_K_ref"])
    assert shim["context"]["extrinsics"] is views["extrinsics"]


def camera_example(tag, device=None, frames_on=None):
    n, (H, W) = G[f"cam_{tag}_E"].shape[0], (37, 53)
    frames = torch.randint(0, 256, (n, H, W, 3), generator=torch.Generator().manual_seed(7), dtype=torch.uint8)
    style = torch.randint(0, 256, (20, 31, 3), generator=torch.Generator().manual_seed(8), dtype=torch.uint8)
    cfg = si.InputCfg(input_image_shape=(16, 16), style_size=16)
    if frames_on is not None:
        frames, style = frames.to(frames_on), style.to(frames_on)
    pixel, flip = tag == "pixel_flip", tag == "pixel_flip"
    ex = si.prepare_example(frames, T(f"cam_{tag}_K"), T(f"cam_{tag}_E"), G[f"cam_{tag}_ci"], G[f"cam_{tag}_ti"], style, cfg, stage="test",
                            pixel_intrinsics=pixel, flip=flip, scene=tag, device=device)
    return ex, frames, cfg


@pytest.mark.parametrize("tag", ["norm", "pixel_flip"])
def test_prepare_example_cameras_and_images(tag):
    ex, frames, cfg = camera_example(tag)
    ci, ti = G[f"cam_{tag}_ci"], G[f"cam_{tag}_ti"]
    pixel = flip = tag == "pixel_flip"
    want = si.prepare_cameras_f64(T(f"cam_{tag}_K"), T(f"cam_{tag}_E"), ci, ti, cfg, (37, 53), pixel, flip)
    for name, idx in (("context", ci), ("target", ti)):
        v = ex[name]
        assert v["image"].shape == (len(idx), 3, 16, 16) and v["index"].tolist() == idx.tolist() and v["index"].dtype == torch.int64
        mine = want[name]
        # the float64 camera path against the generator's independent float64 evaluation (numpy, LAPACK inverse): two float64 routes
        # through a chain of a few dozen operations on values of the poses' scale -- 1e-13 of that scale is 500 ulps of float64
        E64, K64, near64, far64 = (G[f"cam_{tag}_{name}_{f}_f64"] for f in ("extrinsics", "intrinsics", "near", "far"))
        for a, b in zip(mine, (E64, K64, near64, far64)):
            assert np.abs(a - b).max() <= 1e-13 * max(1.0, np.abs(b).max()), (tag, name)
        dist = G[f"cam_{tag}_{name}_dist"]
        for field, w64, d in (("extrinsics", E64, dist[0]), ("intrinsics", K64, dist[1]), ("near", near64, dist[2]), ("far", far64, dist[3])):
            got = v[field]
            assert got.dtype == torch.float32
            # rounded once: within 1 fp32 ulp of the entry's scale of the RECORDED float64 value (half an ulp from the rounding, the
            # rest of the ulp for the 1e-13 between the two float64 routes)
            tol = ULP1 * (max(1.0, np.abs(w64).max()) if field == "extrinsics" else np.abs(w64).max())      # the scale: rotations 1, origins / K / bounds their largest entry
            assert (np.abs(got.double().numpy() - w64) <= tol).all(), (tag, name, field)
            # and within twice the reference's own distance from float64 of the reference's fp32 result
            ref = G[f"cam_{tag}_{name}_{field}_ref"].astype(np.float64)
            dev = np.abs(got.double().numpy() - ref).max()
            print(f"[cam {tag} {name} {field}] distance to the reference {dev:.3e}, the reference's own {d:.3e}")
            assert dev <= 2 * d, (tag, name, field, dev, d)
        # the images are what one rescale_and_crop of the selected frames gives
        imgs, _ = si.rescale_and_crop(frames[torch.as_tensor(idx)], torch.eye(3), (16, 16), flip=flip)
        assert same_bits(v["image"], imgs)
    assert ex["scene"] == tag and ex["style"]["image"].shape == (3, 16, 16)
    if tag == "norm":                                  # the first context view is the identity after camera_normalization
        assert np.abs(ex["context"]["extrinsics"][0].numpy() - np.eye(4)).max() <= ULP1
        a, b = ex["context"]["extrinsics"][0, :3, 3], ex["context"]["extrinsics"][-1, :3, 3]
        assert abs(float((a - b).norm()) - 1.0) <= 4 * ULP1


def test_gates_raise_skip_example_and_the_draw_decides_the_flip():
    tag = "norm"
    frames = torch.zeros(6, 37, 53, 3, dtype=torch.uint8)
    K, E, ci, ti = T(f"cam_{tag}_K"), T(f"cam_{tag}_E"), G[f"cam_{tag}_ci"], G[f"cam_{tag}_ti"]
    cfg = si.InputCfg(input_image_shape=(16, 16))
    scale = float((E[ci[0], :3, 3] - E[ci[-1], :3, 3]).norm())
    for bad in (si.InputCfg(input_image_shape=(16, 16), baseline_min=scale * 1.01), si.InputCfg(input_image_shape=(16, 16), baseline_max=scale * 0.99)):
        with pytest.raises(si.SkipExample, match="baseline"):
            si.prepare_example(frames, K, E, ci, ti, None, bad, stage="test")
    wide = K.clone()
    wide[3, 0, 0] = 0.3                                 # fov_x = 2 atan(0.5 / 0.3) = 118 degrees
    with pytest.raises(si.SkipExample, match="field of view"):
        si.prepare_example(frames, wide, E, ci, ti, None, cfg, stage="test")
    fov = si.get_fov_deg(wide.double().numpy())
    assert abs(fov[3, 0] - np.degrees(2 * np.arctan(0.5 / float(np.float32(0.3))))) < 1e-9 and (fov[:3] < 100).all()
    # stage "train" + augment: the recorded draw decides; other stages never draw
    plain = si.prepare_example(frames, K, E, ci, ti, None, cfg, stage="test")
    for seed, reflects in enumerate(G["aug_reflects"]):
        got = si.prepare_example(frames, K, E, ci, ti, None, cfg, stage="train", generator=torch.Generator().manual_seed(seed))
        want = si.reflect_extrinsics(plain["target"]["extrinsics"]) if reflects else plain["target"]["extrinsics"]
        assert torch.equal(got["target"]["extrinsics"], want), seed
    assert "style" not in plain


def test_collate_and_convert_poses():
    a, _, _ = camera_example("norm")
    b, _, _ = camera_example("pixel_flip")
    batch = si.collate([a, b])
    assert batch["scene"] == ["norm", "pixel_flip"]
    assert batch["context"]["image"].shape == (2, 2, 3, 16, 16) and batch["target"]["image"].shape == (2, 3, 3, 16, 16)
    assert batch["context"]["extrinsics"].shape == (2, 2, 4, 4) and batch["target"]["intrinsics"].shape == (2, 3, 3, 3)
    assert batch["context"]["near"].shape == (2, 2) and batch["target"]["index"].shape == (2, 3) and batch["style"]["image"].shape == (2, 3, 16, 16)
    assert same_bits(batch["target"]["image"][1], b["target"]["image"])
    E = T("cam_norm_E")
    w2c = torch.linalg.inv(E.double())
    rows = torch.cat([torch.tensor([[0.9, 1.1, 0.5, 0.5, 0.0, 0.0]]).expand(6, -1).double(), w2c[:, :3].reshape(6, 12)], 1).float()
    c2w, K = si.convert_poses(rows)
    assert c2w.dtype == K.dtype == torch.float32 and (c2w - E).abs().max() <= 1e-5   # (the rows hold w2c rounded to fp32: 2^-24 relative, times |E|^2 of a few units)
    assert torch.equal(K[2], torch.tensor([[0.9, 0, 0.5], [0, 1.1, 0.5], [0, 0, 1]]))


def test_abi_argument_checks_without_a_device():
    _lib.build_library()
    lib = _lib.load()
    k = C.c_int32(0)
    assert lib.gsr_resample_plan(0, 4, C.byref(k), None, None) == -1 and lib.gsr_resample_plan(4, 0, C.byref(k), None, None) == -1
    assert lib.gsr_resample_plan(4, 4, None, None, None) == -1
    buf = np.zeros(64, np.int32)
    assert lib.gsr_resample_plan(8, 4, C.byref(k), buf.ctypes.data, None) == -1            # bounds without coefficients
    assert lib.gsr_resample_plan(640, 455, C.byref(k), None, None) == 0 and k.value == 11
    assert lib.gsr_resample_plan(20, 32, C.byref(k), None, None) == 0 and k.value == 7
    sb = lib.gsr_resample_scratch_bytes
    assert sb(60, 360, 640, 256, 455, 0, 99, 256, 256) == 60 * 3 * 360 * 256               # every source row, the window's columns
    assert sb(2, 24, 24, 24, 24, 4, 4, 8, 10) == 2 * 3 * 8 * 12                            # no filtering: the window's rows, pitch 12
    assert sb(0, 24, 24, 24, 24, 0, 0, 24, 24) == 0 and sb(1, 24, 24, 12, 12, 0, 0, 13, 12) == 0 and sb(1, 24, 24, 12, 12, -1, 0, 4, 4) == 0
    one = C.c_void_p(256)                                                                  # (validation only, nothing is dereferenced)
    ok = dict(src=one, f32=0, N=1, H=24, W=24, px=one, sw=12, py=one, sh=12, top=0, left=0, oh=12, ow=12, flip=None, scratch=one,
              nbytes=1 << 20, out=one, flags=0, stream=None)
    bad = [dict(src=None), dict(scratch=None), dict(out=None), dict(N=0), dict(H=0), dict(sw=0), dict(px=None), dict(py=None),
           dict(sw=24), dict(sh=24, py=one), dict(oh=13), dict(left=1), dict(top=-1), dict(flags=2), dict(scratch=C.c_void_p(258))]
    for change in bad:
        a = dict(ok, **change)
        assert lib.gsr_resample_crop(*a.values()) == -1, change
    assert lib.gsr_resample_crop(*dict(ok, nbytes=16).values()) == -2                      # GSR_ENOSPACE


def test_twenty_random_shapes_against_the_installed_pil():
    """supplements the fixtures where PIL is installed"""
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(18)
    for _ in range(20):
        H, W, h, w = (int(v) for v in rng.integers(4, 90, 4))
        a = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        ref = np.array(Image.fromarray(a).resize((w, h), Image.LANCZOS))
        want = torch.tensor(ref / 255, dtype=torch.float32).permute(2, 0, 1)
        assert same_bits(si.rescale(torch.from_numpy(a), (h, w)), want), (H, W, h, w)
