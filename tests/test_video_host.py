"""CPU tests (-m "not gpu") of the JPEG / video half of styl3r_amd/image_io.py: `jpeg_header` against the bytes Pillow writes in front of
its scan, the fixture tests/golden/jpeg_encode.npz against live Pillow (where Pillow is linked against libjpeg-turbo, as it was when
the fixture was written) and against what its cases are for, `encode_jpeg` on CPU tensors, `save_video` / `read_avi`, an independent
walk through the AVI container, and the call sites.  No tolerance anywhere: files are compared byte for byte, decoded frames pixel for pixel."""
import struct
from io import BytesIO
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest
import torch
from PIL import Image, features

from styl3r_amd import dataset as ds
from styl3r_amd import image_io as io
from tests.jpeg_encode_cases import CASES, SAMPLINGS, load_fixture, pillow_files, pillow_pixels

ROOT = Path(__file__).resolve().parents[1]
GOLD = load_fixture(ROOT)


def scan_of(data: bytes) -> bytes:
    """what follows the SOS header: walk the marker segments, the way any reader does"""
    at = 2
    while data[at + 1] != 0xDA:
        at += 2 + struct.unpack(">H", data[at + 2:at + 4])[0]
    return data[at + 2 + struct.unpack(">H", data[at + 2:at + 4])[0]:]


# ---- the header ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("subsampling", SAMPLINGS)
def test_jpeg_header_is_what_pillow_writes_in_front_of_its_scan(subsampling):
    sizes = {q: [(33, 25)] for q in range(1, 101)}
    sizes[90] = [(33, 25), (1, 1), (256, 256), (1080, 1920)]
    for q, hw in sizes.items():
        for H, W in hw:
            want = pillow_files(np.zeros((1, H, W, 3), np.uint8), q, subsampling)[0]
            got = io.jpeg_header(H, W, q, subsampling)
            assert want[:len(got)] == got and want[len(got):] == scan_of(want), (q, H, W)


@pytest.mark.parametrize("name", list(CASES))
def test_header_plus_the_fixtures_scan_is_the_fixture_and_parses_in_pillow(name):
    frames, q, s = CASES[name]
    for img, want in zip(frames, GOLD[name]):
        data = io.jpeg_header(img.shape[0], img.shape[1], q, s) + scan_of(want)
        assert data == want
        opened = Image.open(BytesIO(data))
        assert opened.format == "JPEG" and opened.size == (img.shape[1], img.shape[0]) and np.array(opened).shape == img.shape


def test_quant_tables_follow_libjpegs_quality_rule():
    assert io.jpeg_quant_tables(50).tolist() == [list(io.QUANT_BASE[0]), list(io.QUANT_BASE[1])]
    assert (io.jpeg_quant_tables(100) == 1).all() and io.jpeg_quant_tables(1).max() == 255
    assert io.jpeg_quant_tables(90)[0, :4].tolist() == [3, 2, 2, 3] and io.jpeg_quant_tables(20)[1, 0] == (17 * 250 + 50) // 100


# ---- the fixture -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(not features.check_feature("libjpeg_turbo"), reason="the fixture records libjpeg-turbo's bytes; this Pillow is linked against another libjpeg")
@pytest.mark.parametrize("name", list(CASES))
def test_fixture_equals_live_pillow(name):
    frames, q, s = CASES[name]
    assert pillow_files(frames, q, s) == GOLD[name]


def _coefficients(data: bytes):
    """the quantised coefficients of a file through the project's own entropy decoder: [(blocks, 64) natural order] per component"""
    res = ds.jpeg_entropy([data])
    assert res.status[0] == 0 or res.coefs is not None
    d, flat = res.desc[0], res.coefs.numpy()
    out, at = [], int(d.coef_offset)
    for c in range(d.ncomp):
        n = d.bw[c] * d.bh[c]
        out.append(flat[at:at + 64 * n].reshape(n, 64))
        at += 64 * n
    return out


def test_the_fixture_reaches_what_its_cases_are_named_for():
    for s in ("444", "422", "420"):
        assert b"\xff\x00" in scan_of(GOLD[f"noise_64x48-{s}"][0])                      # stuffed bytes in the densest stream
        y = _coefficients(GOLD[f"one_coefficient_16x16-{s}"][0])[0]
        assert (y[:, 63] != 0).all() and (y[:, 1:63] == 0).all()                        # 62 zeros in front of coefficient 63: three 0xF0 codes
        flat = _coefficients(GOLD[f"flat_32x32-{s}"][0])
        assert all((c[:, 1:] == 0).all() for c in flat) and all((c[1:, 0] == c[0, 0]).all() for c in flat)
        big = _coefficients(GOLD[f"stripes_16x16-{s}"][0])[0]
        assert np.abs(big[:, 1:]).max() >= 512                                          # AC category 10, the largest there is
    assert len({len(f) for f in GOLD["five_40x56-420"]}) > 1 and len(set(GOLD["five_40x56-420"])) == 5


# ---- encode_jpeg on the host -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_encode_jpeg_of_cpu_tensors_is_pillow_and_equals_the_fixture(name):
    frames, q, s = CASES[name]
    before = dict(io.CALLS)
    got = io.encode_jpeg(torch.from_numpy(frames), q, s)
    assert [len(g) for g in got] == [len(w) for w in GOLD[name]] and got == GOLD[name]
    assert io.CALLS["jpeg_enc_host"] == before["jpeg_enc_host"] + frames.shape[0]
    assert io.CALLS["jpeg_enc_hip"] == before["jpeg_enc_hip"] and io.CALLS["jpeg_enc_fallback"] == before["jpeg_enc_fallback"]


def test_encode_jpeg_of_float_frames_converts_as_prep_image_does():
    x = torch.rand(2, 3, 9, 7, generator=torch.Generator().manual_seed(3)) * 1.4 - 0.2
    x[0, 0, 0, :3] = torch.tensor([float("nan"), float("inf"), float("-inf")])
    want = torch.stack([io.prep_image(f) for f in x])
    assert io.encode_jpeg(x) == io.encode_jpeg(want) == pillow_files(want.numpy(), 90, 2)


def test_encode_jpeg_refuses_what_it_does_not_write():
    ok = torch.zeros((1, 8, 8, 3), dtype=torch.uint8)
    for bad in (ok[0], ok.float(), ok.permute(0, 3, 1, 2).contiguous(), torch.zeros((1, 8, 8, 4), dtype=torch.uint8), torch.zeros((1, 4, 8, 8)),
                torch.zeros((0, 8, 8, 3), dtype=torch.uint8), ok.to(torch.int16), ok.numpy()):
        with pytest.raises(ValueError):
            io.encode_jpeg(bad)
    for q in (0, 101, 90.0, "90", None, True):
        with pytest.raises(ValueError):
            io.encode_jpeg(ok, quality=q)
    for s in ("4:1:1", "420", 2, None):
        with pytest.raises(ValueError):
            io.encode_jpeg(ok, subsampling=s)
    with pytest.raises(ValueError):
        io.jpeg_header(70000, 8)


# ---- save_video / read_avi -------------------------------------------------------------------------------------------------------------
def _video_frames(n=4, h=20, w=28, seed=5):
    return torch.rand(n, 3, h, w, generator=torch.Generator().manual_seed(seed))


@pytest.mark.parametrize("form", ["list", "float", "bytes"])
def test_save_video_round_trip_for_every_input_form(tmp_path, form):
    x = _video_frames()
    as_bytes = torch.stack([io.prep_image(f) for f in x])
    images = {"list": [f for f in x], "float": x, "bytes": as_bytes}[form]
    before = dict(io.CALLS)
    io.save_video(images, tmp_path / "deep" / "er" / "clip.avi", fps=24, quality=85, subsampling="4:2:2")
    assert io.CALLS["jpeg_enc_host"] == before["jpeg_enc_host"] + 4
    fps, files = io.read_avi(tmp_path / "deep" / "er" / "clip.avi")
    assert fps == 24 and len(files) == 4
    want = pillow_files(as_bytes.numpy(), 85, 1)
    assert files == want
    for got, w in zip(files, want):
        assert np.array_equal(pillow_pixels(got), pillow_pixels(w))


def _chunks(data: bytes, at: int, end: int):
    """[(fourcc, payload offset, payload size)] of the RIFF chunks in data[at:end]"""
    out = []
    while at < end:
        kind, n = data[at:at + 4], struct.unpack("<I", data[at + 4:at + 8])[0]
        assert at + 8 + n <= end, "a chunk runs over its parent"
        out.append((kind, at + 8, n))
        at += 8 + n + (n & 1)
    assert at == end, "padding to even length, and nothing else, between chunks"
    return out


@pytest.mark.parametrize("fps, rate, scale", [(30, 30, 1), (23.976, 23976, 1000)])
def test_avi_structure_walk(tmp_path, fps, rate, scale):
    """written here, without read_avi: the sizes, the header fields, the index"""
    frames = torch.from_numpy(np.random.default_rng(2).integers(0, 256, (5, 17, 23, 3), dtype=np.uint8))   # noise: odd and even file lengths
    io.save_video(frames, tmp_path / "walk.avi", fps=fps)
    data = (tmp_path / "walk.avi").read_bytes()
    files = pillow_files(frames.numpy(), 90, 2)
    assert {len(f) & 1 for f in files} == {0, 1}
    assert data[:4] == b"RIFF" and struct.unpack("<I", data[4:8])[0] == len(data) - 8 and data[8:12] == b"AVI "
    top = _chunks(data, 12, len(data))
    assert [k for k, _, _ in top] == [b"LIST", b"LIST", b"idx1"]
    (_, hdrl_at, hdrl_n), (_, movi_at, movi_n), (_, idx_at, idx_n) = top
    assert data[hdrl_at:hdrl_at + 4] == b"hdrl" and data[movi_at:movi_at + 4] == b"movi"
    hdrl = _chunks(data, hdrl_at + 4, hdrl_at + hdrl_n)
    assert [k for k, _, _ in hdrl] == [b"avih", b"LIST"] and hdrl[0][2] == 56
    avih = struct.unpack("<14I", data[hdrl[0][1]:hdrl[0][1] + 56])
    assert avih[0] == round(1e6 * scale / rate) and avih[3] & 0x10 and avih[4] == 5 and avih[6] == 1 and avih[8:10] == (23, 17)
    assert avih[7] >= max(len(f) for f in files)
    assert data[hdrl[1][1]:hdrl[1][1] + 4] == b"strl"
    strl = _chunks(data, hdrl[1][1] + 4, hdrl[1][1] + hdrl[1][2])
    assert [k for k, _, _ in strl] == [b"strh", b"strf"] and strl[0][2] == 56 and strl[1][2] == 40
    strh = data[strl[0][1]:strl[0][1] + 56]
    assert strh[:8] == b"vidsMJPG"
    assert struct.unpack("<II", strh[20:28]) == (scale, rate) and struct.unpack("<II", strh[28:36]) == (0, 5)
    assert struct.unpack("<4h", strh[48:56]) == (0, 0, 23, 17)
    size, w, h, planes, depth, codec, image = struct.unpack("<IiiHH4sI", data[strl[1][1]:strl[1][1] + 24])
    assert (size, w, h, planes, depth, codec, image) == (40, 23, 17, 1, 24, b"MJPG", 23 * 17 * 3)
    movi = _chunks(data, movi_at + 4, movi_at + movi_n)
    assert [k for k, _, _ in movi] == [b"00dc"] * 5 and [data[a:a + n] for _, a, n in movi] == files
    assert idx_n == 16 * 5
    for i, (_, a, n) in enumerate(movi):
        kind, flags, offset, length = struct.unpack("<4sIII", data[idx_at + 16 * i:idx_at + 16 * i + 16])
        assert kind == b"00dc" and flags & 0x10 and length == n
        assert movi_at + offset == a - 8 and data[movi_at + offset:movi_at + offset + 4] == b"00dc"     # from the `movi` fourcc to the chunk header
    assert io.read_avi(tmp_path / "walk.avi") == (rate / scale, files)


def test_save_video_refuses_other_suffixes_and_files_of_two_gib(tmp_path, monkeypatch):
    x = _video_frames(2)
    for name in ("clip.mp4", "clip", "clip.avi.mp4", "clip.mov"):
        with pytest.raises(ValueError, match="Motion-JPEG AVI"):
            io.save_video(x, tmp_path / name)
    assert list(tmp_path.iterdir()) == []
    for bad in ([], [torch.zeros(1, 3, 4, 4)], torch.zeros(2, 4, 8, 8)):
        with pytest.raises(ValueError):
            io.save_video(bad, tmp_path / "clip.avi")
    with pytest.raises(ValueError):
        io.save_video(x, tmp_path / "clip.avi", fps=0)
    monkeypatch.setattr(io, "AVI_LIMIT", 4096)
    with pytest.raises(ValueError, match="2 GiB"):
        io.save_video(torch.from_numpy(np.random.default_rng(1).integers(0, 256, (4, 32, 32, 3), dtype=np.uint8)), tmp_path / "big.avi")
    assert not (tmp_path / "big.avi").exists()
    io.save_video(x, tmp_path / "CLIP.AVI")
    assert len(io.read_avi(tmp_path / "CLIP.AVI")[1]) == 2


def test_read_avi_refuses_other_files(tmp_path):
    (tmp_path / "x.avi").write_bytes(b"RIFF\x04\x00\x00\x00WAVE")
    with pytest.raises(ValueError):
        io.read_avi(tmp_path / "x.avi")


# ---- the call sites --------------------------------------------------------------------------------------------------------------------
def test_save_image_of_cpu_tensors_stays_with_pillow(tmp_path):
    image = torch.rand(3, 19, 21, generator=torch.Generator().manual_seed(4))
    before = dict(io.CALLS)
    io.save_image(image, tmp_path / "a" / "style.jpg")
    assert io.CALLS == before
    buf = BytesIO()
    Image.fromarray(io.prep_image(image).numpy()).save(buf, format="JPEG")
    assert (tmp_path / "a" / "style.jpg").read_bytes() == buf.getvalue()


class _Fixed:
    def __init__(self, color):
        self.color = color

    def __call__(self, context, style, global_step):
        return "gaussians"

    def forward(self, gaussians, *cameras):
        return SimpleNamespace(color=self.color)


def test_test_step_writes_the_named_video_only_when_asked(tmp_path):
    from styl3r_amd import evaluation
    assert evaluation.TestCfg().save_video is False
    color = torch.rand(2, 3, 3, 16, 24, generator=torch.Generator().manual_seed(6))
    target = {"image": color, "extrinsics": None, "intrinsics": None, "near": None, "far": None, "index": torch.tensor([[5, 6, 7], [1, 2, 3]])}
    batch = {"context": {"image": color[:, :2], "index": torch.tensor([[3, 40], [0, 9]])}, "target": target, "scene": ["0a1b", "ffee"]}
    model = _Fixed(color)
    quiet = evaluation.TestCfg(align_pose=False, compute_scores=False, output_path=tmp_path / "off")
    evaluation.test_step(model, model, batch, [], quiet)
    assert not (tmp_path / "off").exists()
    cfg = evaluation.TestCfg(align_pose=False, compute_scores=False, save_video=True, output_path=tmp_path / "on")
    evaluation.test_step(model, model, batch, [], cfg)
    files = sorted(str(p.relative_to(tmp_path / "on")) for p in (tmp_path / "on").rglob("*") if p.is_file())
    assert files == ["video/0a1b_frame_3_40.avi", "video/ffee_frame_0_9.avi"]
    for i, name in enumerate(files):
        fps, frames = io.read_avi(tmp_path / "on" / name)
        assert fps == 30 and frames == io.encode_jpeg(color[i])
    del batch["context"]["index"]
    batch["scene"], model.color = "lone", color[:1]
    written = evaluation.save_color_videos(cfg, batch, model)
    assert written == [tmp_path / "on" / "video" / "lone.avi"] and written[0].exists()


def test_save_flythrough_names_the_container_before_it_renders(tmp_path):
    from styl3r_amd.inference import save_flythrough
    with pytest.raises(ValueError, match="Motion-JPEG AVI"):
        save_flythrough(tmp_path / "fly.mp4", None, None, None)
