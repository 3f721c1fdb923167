"""-m gpu: the kernels of csrc/gsr_jpeg_enc.hip (k_jpeg_enc_transform / _scan / _code / _assemble behind gsr_jpeg_enc_scans) through
styl3r_amd/image_io.py and straight through the C ABI, byte for byte against the files Pillow (libjpeg-turbo) wrote
(tests/golden/jpeg_encode.npz, which tests/test_video_host.py holds to live Pillow).  Every device buffer is filled with 0xA5 before the
launches, so that a byte the kernels did not write shows.  No tolerance anywhere."""
import ctypes as C
from io import BytesIO
from pathlib import Path

import numpy as np
import pytest
import torch
from PIL import Image

from styl3r_amd import _lib
from styl3r_amd import dataset as ds
from styl3r_amd import image_io as io
from styl3r_amd.export import _rgb_bytes_host
from tests.jpeg_encode_cases import CASES, SAMPLINGS, load_fixture, pillow_files, pillow_pixels
from tests.test_video_host import _coefficients, scan_of

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
GOLD = load_fixture(Path(__file__).resolve().parents[1])


@pytest.fixture(autouse=True)
def prefilled_buffers(monkeypatch):
    monkeypatch.setattr(io, "DEBUG_FILL", 0xA5)


@pytest.mark.parametrize("name", list(CASES))
def test_device_files_equal_pillows(name):
    frames, q, s = CASES[name]
    before = dict(io.CALLS)
    got = io.encode_jpeg(torch.from_numpy(frames).to(DEV), q, s)
    assert io.CALLS["jpeg_enc_hip"] == before["jpeg_enc_hip"] + frames.shape[0]
    assert io.CALLS["jpeg_enc_fallback"] == before["jpeg_enc_fallback"] and io.CALLS["jpeg_enc_host"] == before["jpeg_enc_host"]
    assert [len(g) for g in got] == [len(w) for w in GOLD[name]]
    assert got == GOLD[name]
    assert io.encode_jpeg(torch.from_numpy(frames).to(DEV), q, s) == got                # two runs, the same bytes


@pytest.mark.parametrize("subsampling", SAMPLINGS)
def test_one_frame_per_call_equals_five_frames_in_one_call(subsampling):
    frames = torch.from_numpy(CASES["five_40x56-420"][0]).to(DEV)
    together = io.encode_jpeg(frames, 90, subsampling)
    assert [io.encode_jpeg(frames[i:i + 1], 90, subsampling)[0] for i in range(5)] == together and len(set(together)) == 5


def test_frames_beyond_the_memory_budget_go_in_batches(monkeypatch):
    frames, q, s = CASES["five_40x56-420"]
    lib = _lib.load()
    one = ((lib.gsr_jpeg_enc_stream_bound(40, 56, _lib.GSR_JPEG_420) + 15) & ~15) + lib.gsr_jpeg_enc_scratch_bytes(1, 40, 56, _lib.GSR_JPEG_420)
    for budget in (2 * one, 1):                                  # two frames per call (2 + 2 + 1), then one per call whatever the budget
        monkeypatch.setattr(io, "JPEG_BATCH_BYTES", budget)
        before = dict(io.CALLS)
        assert io.encode_jpeg(torch.from_numpy(frames).to(DEV), q, s) == GOLD["five_40x56-420"]
        assert io.CALLS["jpeg_enc_hip"] == before["jpeg_enc_hip"] + 5 and io.CALLS["jpeg_enc_fallback"] == before["jpeg_enc_fallback"]


@pytest.mark.parametrize("subsampling", SAMPLINGS)
def test_float_planar_frames_convert_in_the_load(subsampling):
    x = torch.from_numpy(np.random.default_rng(12).random((2, 3, 19, 23)).astype(np.float32) * 1.4 - 0.2)
    x[0, 0, 0, :7] = torch.tensor([-0.1, 0.0, 0.5 / 255, float(np.float32(1 / 255) - np.float32(1e-9)), 1.0, 1.5, float("nan")])
    x[1, 2, 18, :3] = torch.tensor([float("inf"), float("-inf"), 254.999 / 255])
    want_bytes = _rgb_bytes_host(x).contiguous()
    got = io.encode_jpeg(x.to(DEV), 90, subsampling)
    assert got == io.encode_jpeg(want_bytes.to(DEV), 90, subsampling)
    assert got == pillow_files(want_bytes.numpy(), 90, io.JPEG_SAMPLING[subsampling][3])
    assert got == io.encode_jpeg(want_bytes, 90, subsampling)


def _abi(frames: torch.Tensor, quality: int, subsampling: str, tail: int = 64):
    """one gsr_jpeg_enc_scans call with an out stride of exactly the bound; (out bytes, lengths, scratch, bound)"""
    lib, code = _lib.load(), io.JPEG_SAMPLING[subsampling][0]
    N, H, W, _ = frames.shape
    nbytes, bound = lib.gsr_jpeg_enc_scratch_bytes(N, H, W, code), lib.gsr_jpeg_enc_stream_bound(H, W, code)
    assert nbytes and bound
    scratch = torch.full((nbytes,), 0xA5, dtype=torch.uint8, device=DEV)
    out = torch.full((N * bound + tail,), 0xA5, dtype=torch.uint8, device=DEV)
    lengths = torch.full((N,), -1, dtype=torch.int32, device=DEV)
    quant = np.ascontiguousarray(io.jpeg_quant_tables(quality))
    s = C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
    _lib.check(lib.gsr_jpeg_enc_scans(frames.data_ptr(), _lib.GSR_JPEG_ENC_SRC_U8, N, H, W, code, quant.ctypes.data, scratch.data_ptr(), nbytes,
                                      out.data_ptr(), bound, lengths.data_ptr(), s), "gsr_jpeg_enc_scans")
    return out.cpu().numpy(), lengths.cpu().tolist(), scratch.cpu(), bound


@pytest.mark.parametrize("name", ["five_40x56-444", "five_40x56-422", "five_40x56-420", "noise_64x48-420", "noise_1x1-420"])
def test_nothing_is_written_beyond_the_scan_length(name):
    """straight through the C ABI with an out stride of exactly the bound: the bytes behind each scan, and behind the last image, keep 0xA5"""
    frames, q, s = CASES[name]
    got, sizes, _, bound = _abi(torch.from_numpy(frames).to(DEV), q, s)
    N = frames.shape[0]
    for i, n in enumerate(sizes):
        assert got[i * bound:i * bound + n].tobytes() == scan_of(GOLD[name][i])
        assert (got[i * bound + n:(i + 1) * bound] == 0xA5).all()
    assert (got[N * bound:] == 0xA5).all()


def test_bad_arguments_are_refused_before_any_launch():
    lib = _lib.load()
    N, H, W, code = 2, 9, 17, _lib.GSR_JPEG_420
    frames = torch.zeros((N, H, W, 3), dtype=torch.uint8, device=DEV)
    nbytes, bound = lib.gsr_jpeg_enc_scratch_bytes(N, H, W, code), lib.gsr_jpeg_enc_stream_bound(H, W, code)
    blocks = 2 * 1 * 6
    assert bound == 2 * ((blocks * (22 + 63 * 26) + 7) // 8) + 2 and nbytes >= N * blocks * 128
    assert lib.gsr_jpeg_enc_stream_bound(0, 8, code) == 0 and lib.gsr_jpeg_enc_stream_bound(8, 65536, code) == 0
    assert lib.gsr_jpeg_enc_stream_bound(8, 8, 0) == 0 and lib.gsr_jpeg_enc_scratch_bytes(0, 8, 8, code) == 0
    scratch = torch.full((nbytes + 16,), 0xA5, dtype=torch.uint8, device=DEV)
    out = torch.full((N * bound + 16,), 0xA5, dtype=torch.uint8, device=DEV)
    lengths = torch.full((N + 1,), -1, dtype=torch.int32, device=DEV)
    quant = np.ascontiguousarray(io.jpeg_quant_tables(90))
    zero_q, big_q = quant.copy(), quant.copy()
    zero_q[1, 63], big_q[0, 0] = 0, 256
    s = C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
    ok = [frames.data_ptr(), _lib.GSR_JPEG_ENC_SRC_U8, N, H, W, code, quant.ctypes.data, scratch.data_ptr(), nbytes, out.data_ptr(), bound,
          lengths.data_ptr(), s]
    table = ((0, None), (6, None), (7, None), (9, None), (11, None), (1, 2), (1, -1), (2, 0), (2, (1 << 24) + 1), (3, 0), (4, 0), (3, 65536),
             (4, 65536), (5, 0), (5, 4), (6, zero_q.ctypes.data), (6, big_q.ctypes.data), (7, scratch.data_ptr() + 4), (11, lengths.data_ptr() + 2),
             (10, bound - 1), (10, 1 << 31))
    for k, v in table:
        bad = list(ok)
        bad[k] = v
        assert lib.gsr_jpeg_enc_scans(*bad) == -1, (k, v)
    bad = list(ok)
    bad[8] = nbytes - 1
    assert lib.gsr_jpeg_enc_scans(*bad) == -2
    bad = list(ok)
    bad[0], bad[1] = frames.data_ptr() + 1, _lib.GSR_JPEG_ENC_SRC_F32_PLANAR
    assert lib.gsr_jpeg_enc_scans(*bad) == -1
    torch.cuda.synchronize()
    assert bool((scratch == 0xA5).all()) and bool((out == 0xA5).all()) and bool((lengths == -1).all())      # nothing ran
    assert lib.gsr_jpeg_enc_scans(*ok) == 0
    torch.cuda.synchronize()
    assert lengths[:N].tolist() == [len(scan_of(f)) for f in pillow_files(frames.cpu().numpy(), 90, 2)]


def test_a_picture_of_too_many_blocks_is_refused_with_a_status_and_goes_to_pillow():
    lib = _lib.load()
    H = W = 7400                                                 # 925 x 925 MCUs of 3 blocks at 4:4:4: above 2 500 000
    assert lib.gsr_jpeg_enc_scratch_bytes(1, H, W, _lib.GSR_JPEG_444) == 0 and lib.gsr_jpeg_enc_stream_bound(H, W, _lib.GSR_JPEG_444) == 0
    assert lib.gsr_jpeg_enc_stream_bound(H, W, _lib.GSR_JPEG_420) > 0
    frames = torch.zeros((1, H, W, 3), dtype=torch.uint8, device=DEV)
    frames[0, :64, :64] = 200
    small = torch.full((1024,), 0xA5, dtype=torch.uint8, device=DEV)
    lengths = torch.full((1,), -1, dtype=torch.int32, device=DEV)
    quant = np.ascontiguousarray(io.jpeg_quant_tables(90))
    s = C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
    rc = lib.gsr_jpeg_enc_scans(frames.data_ptr(), _lib.GSR_JPEG_ENC_SRC_U8, 1, H, W, _lib.GSR_JPEG_444, quant.ctypes.data, small.data_ptr(), 1024,
                                small.data_ptr(), 1 << 30, lengths.data_ptr(), s)
    torch.cuda.synchronize()
    assert rc == _lib.GSR_JPEG_ENC_TOO_LARGE and bool((small == 0xA5).all()) and int(lengths[0]) == -1
    before = dict(io.CALLS)
    files = io.encode_jpeg(frames, 90, "4:4:4")
    assert io.CALLS["jpeg_enc_fallback"] == before["jpeg_enc_fallback"] + 1 and io.CALLS["jpeg_enc_hip"] == before["jpeg_enc_hip"]
    opened = Image.open(BytesIO(files[0]))
    assert opened.size == (W, H)


@pytest.mark.parametrize("name", ["noise_37x50-444", "noise_37x50-422", "noise_37x50-420", "noise_40x24-420", "gradient_33x25_q20-420",
                                  "noise_200x72-420"])
def test_transform_stage_coefficients_equal_the_entropy_decoders(name):
    """the scratch begins with the quantised coefficients (include/gsr.h): coding order, zig-zag, DC as differences.  Undone here, they are
    what the project's own gsr_jpeg_entropy reads from Pillow's file -- dummy blocks included, which carry the DC in front of them."""
    frames, q, s = CASES[name]
    _, hs, vs, _ = io.JPEG_SAMPLING[s]
    H, W = frames.shape[1:3]
    mx, my, ny = -(-W // (8 * hs)), -(-H // (8 * vs)), hs * vs
    bpm, mcus = ny + 2, mx * my
    _, _, scratch, _ = _abi(torch.from_numpy(frames).to(DEV), q, s)
    coef = scratch[:mcus * bpm * 128].view(torch.int16).numpy().reshape(mcus, bpm, 64).astype(np.int32)
    natural = np.zeros_like(coef)
    natural[:, :, list(io.ZIGZAG)] = coef
    groups = [natural[:, :ny], natural[:, ny:ny + 1], natural[:, ny + 1:]]
    want = _coefficients(GOLD[name][0])
    for c, (g, w) in enumerate(zip(groups, want)):
        g = g.copy()
        g[:, :, 0] = np.cumsum(g[:, :, 0].reshape(-1)).reshape(g.shape[:2])               # differences -> values, in coding order
        fh, fv = (hs, vs) if c == 0 else (1, 1)
        grid = g.reshape(my, mx, fv, fh, 64).transpose(0, 2, 1, 3, 4).reshape(my * fv * mx * fh, 64)
        assert np.array_equal(grid, w.astype(np.int32)), (name, c)


@pytest.mark.parametrize("name", ["rendered_256x256-420", "rendered_256x256-444", "five_40x56-422", "gradient_33x25_q75-420", "noise_9x17-420"])
def test_round_trip_through_the_device_decoder(name):
    frames, q, s = CASES[name]
    files = io.encode_jpeg(torch.from_numpy(frames).to(DEV), q, s)
    before = dict(ds.CALLS)
    back = ds.decode_jpeg(files, device=DEV)
    assert ds.CALLS["jpeg_hip"] == before["jpeg_hip"] + len(files) and ds.CALLS["jpeg_fallback"] == before["jpeg_fallback"]
    assert back.is_cuda and tuple(back.shape) == frames.shape
    for got, gold in zip(back.cpu().numpy(), GOLD[name]):
        assert np.array_equal(got, pillow_pixels(gold))


def test_save_image_of_a_device_tensor_writes_pillows_default_jpeg(tmp_path):
    g = torch.Generator().manual_seed(8)
    for k, image in enumerate((torch.rand(3, 37, 50, generator=g) * 1.2 - 0.1, torch.rand(1, 20, 24, generator=g), torch.rand(2, 3, 16, 12, generator=g))):
        before = dict(io.CALLS)
        io.save_image(image.to(DEV), tmp_path / "deep" / f"style{k}.jpg")
        assert io.CALLS["jpeg_enc_hip"] == before["jpeg_enc_hip"] + 1
        buf = BytesIO()
        Image.fromarray(io.prep_image(image).numpy()).save(buf, format="JPEG")
        assert (tmp_path / "deep" / f"style{k}.jpg").read_bytes() == buf.getvalue()
    io.save_image(torch.rand(3, 9, 9, generator=g).to(DEV), tmp_path / "x.JPEG")
    assert Image.open(tmp_path / "x.JPEG").format == "JPEG"
    with pytest.raises(OSError):
        io.save_image(torch.rand(4, 9, 9, generator=g).to(DEV), tmp_path / "rgba.jpg")     # Pillow's refusal, as before


def _scene():
    from styl3r_amd.decoder import DecoderSplattingCUDACfg, Gaussians, get_decoder
    from styl3r_amd.scenes import make_scene
    sc = make_scene(n_ctx=1, grid_hw=(32, 32), n_views=2, image_hw=(32, 32), sh_degree=0, seed=4).to(DEV)
    g = Gaussians(sc.means[None], sc.covariances[None], sc.harmonics[None], sc.opacities[None])
    dec = get_decoder(DecoderSplattingCUDACfg("splatting_cuda", [0.0, 0.0, 0.0], True)).to(DEV)
    cams = {"extrinsics": sc.extrinsics[None], "intrinsics": sc.intrinsics[None], "near": sc.near[None], "far": sc.far[None]}
    return g, dec, cams


def test_save_flythrough_writes_the_frames_render_flythrough_returns(tmp_path):
    from styl3r_amd.inference import render_flythrough, save_flythrough
    g, dec, cams = _scene()
    ctx = dict(image=torch.zeros((1, 2, 3, 32, 32), device=DEV), **cams)
    before = dict(io.CALLS)
    frames = save_flythrough(tmp_path / "out" / "fly.avi", dec, g, ctx, num_frames=5, panels=("plain",), fps=12, quality=80)
    assert frames.is_cuda and frames.dtype == torch.uint8 and frames.shape == (8, 32, 32, 3)
    assert io.CALLS["jpeg_enc_hip"] == before["jpeg_enc_hip"] + 8 and io.CALLS["jpeg_enc_host"] == before["jpeg_enc_host"]
    assert torch.equal(frames, render_flythrough(dec, g, ctx, num_frames=5, panels=("plain",)))
    assert int(frames.max()) > 0
    fps, files = io.read_avi(tmp_path / "out" / "fly.avi")
    assert fps == 12 and files == pillow_files(frames.cpu().numpy(), 80, 2)


class _FixedGaussians(torch.nn.Module):
    def __init__(self, g):
        super().__init__()
        self.g = g

    def forward(self, context, style, global_step):
        return self.g


def test_test_step_saves_the_video_from_device_tensors(tmp_path):
    from styl3r_amd import evaluation
    g, dec, cams = _scene()
    with torch.no_grad():
        target = dec.forward(g, cams["extrinsics"], cams["intrinsics"], cams["near"], cams["far"], (32, 32)).color
    batch = {"context": {"image": target[:, :1], "index": torch.tensor([[3, 17]], device=DEV)}, "scene": ["scene_7"],
             "target": dict(cams, image=target, index=torch.tensor([[3, 17]], device=DEV))}
    cfg = evaluation.TestCfg(align_pose=False, compute_scores=False, save_video=True, output_path=tmp_path)
    before = dict(io.CALLS)
    out, _ = evaluation.test_step(_FixedGaussians(g), dec, batch, [], cfg)
    assert io.CALLS["jpeg_enc_hip"] == before["jpeg_enc_hip"] + 2
    files = sorted(str(p.relative_to(tmp_path)) for p in tmp_path.rglob("*") if p.is_file())
    assert files == ["video/scene_7_frame_3_17.avi"]
    fps, frames = io.read_avi(tmp_path / files[0])
    assert fps == 30 and frames == pillow_files(torch.stack([io.prep_image(c) for c in out.color[0]]).cpu().numpy(), 90, 2)
