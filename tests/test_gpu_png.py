"""-m gpu: the kernels of csrc/gsr_png.hip (k_png_chunks, k_png_assemble behind gsr_png_chunks / gsr_png_assemble) through
styl3r_amd/image_io.py, byte for byte against the CPU restatement of the same module (which tests/test_png_host.py holds to Pillow and
zlib) and, again, against Pillow and zlib directly.  Every device buffer is filled with 0xA5 before the launches, so that a byte the
kernels did not write shows.  No tolerance anywhere."""
import ctypes as C
from io import BytesIO

import numpy as np
import pytest
import torch
from PIL import Image

from styl3r_amd import _lib
from styl3r_amd import image_io as io
from styl3r_amd.export import _rgb_bytes_host
from tests.test_png_host import CASES, check_files, check_scene_tree, encoded, prep_cases, scene_batch, _gradient, _prep_reference

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


@pytest.fixture(autouse=True)
def prefilled_buffers(monkeypatch):
    monkeypatch.setattr(io, "DEBUG_FILL", 0xA5)


@pytest.mark.parametrize("name", list(CASES))
def test_device_bytes_equal_the_restatement_and_decode_in_pillow(name):
    frames, filt, _ = CASES[name]
    before = dict(io.CALLS)
    got = io.encode_png(torch.from_numpy(frames).to(DEV), filt)
    assert io.CALLS["png_hip"] == before["png_hip"] + frames.shape[0] and io.CALLS["png_fallback"] == before["png_fallback"]
    want = encoded(name)[0]
    assert [len(g) for g in got] == [len(w) for w in want]
    assert got == want
    check_files(got, frames)
    assert io.encode_png(torch.from_numpy(frames).to(DEV), filt) == got          # two runs, the same bytes


def test_one_frame_per_call_equals_five_frames_in_one_call():
    frames = torch.from_numpy(CASES["five_frames"][0]).to(DEV)
    together = io.encode_png(frames)
    assert [io.encode_png(frames[i:i + 1])[0] for i in range(5)] == together and len(set(together)) == 5


def test_float_planar_frames_convert_in_the_load():
    x = torch.from_numpy(np.random.default_rng(12).random((2, 3, 9, 7)).astype(np.float32) * 1.4 - 0.2)
    x[0, 0, 0, :7] = torch.tensor([-0.1, 0.0, 0.5 / 255, float(np.float32(1 / 255) - np.float32(1e-9)), 1.0, 1.5, float("nan")])
    x[1, 2, 8, :3] = torch.tensor([float("inf"), float("-inf"), 254.999 / 255])
    for frames in (x, torch.cat([x, x[:, :1]], dim=1), torch.from_numpy(_gradient(120, 100, 3, 31)).permute(2, 0, 1)[None].float() / 255):
        want_bytes = _rgb_bytes_host(frames).contiguous()
        got = io.encode_png(frames.to(DEV))
        assert got == io.encode_png(want_bytes) and got == io.encode_png(want_bytes.to(DEV))
        check_files(got, want_bytes.numpy())


def test_a_row_wider_than_a_chunk_is_refused_with_a_status_and_goes_to_pillow():
    lib = _lib.load()
    frames = torch.from_numpy(_gradient(2, 5462, 3, 13)[None]).to(DEV)
    assert lib.gsr_png_scratch_bytes(1, 2, 5462, 3) == 0 and lib.gsr_png_stream_bound(2, 5462, 3) == 0
    scratch = torch.full((1024,), 0xA5, dtype=torch.uint8, device=DEV)
    s = C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
    assert lib.gsr_png_chunks(frames.data_ptr(), _lib.GSR_PNG_SRC_U8, 1, 2, 5462, 3, 0, scratch.data_ptr(), 1024, s) == _lib.GSR_PNG_ROW_TOO_WIDE
    torch.cuda.synchronize()
    assert bool((scratch == 0xA5).all())
    before = dict(io.CALLS)
    files = io.encode_png(frames)
    assert io.CALLS["png_fallback"] == before["png_fallback"] + 1 and io.CALLS["png_hip"] == before["png_hip"]
    assert np.array_equal(np.asarray(Image.open(BytesIO(files[0]))), frames[0].cpu().numpy())


def test_bad_arguments_are_einval_before_any_launch():
    lib = _lib.load()
    N, H, W, ch = 2, 5, 3, 3
    frames = torch.zeros((N, H, W, ch), dtype=torch.uint8, device=DEV)
    nbytes, bound = lib.gsr_png_scratch_bytes(N, H, W, ch), lib.gsr_png_stream_bound(H, W, ch)
    assert nbytes == 16 * ((N * 16 + 15) // 16) + N * _lib.GSR_PNG_SLOT_BYTES and bound == 2 + H * (1 + W * ch) + 5 + 5 + 4
    scratch = torch.empty(nbytes + 16, dtype=torch.uint8, device=DEV)
    out = torch.empty(N * bound + 16, dtype=torch.uint8, device=DEV)
    lengths = torch.empty(N + 1, dtype=torch.int32, device=DEV)
    s = C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
    ok = [frames.data_ptr(), _lib.GSR_PNG_SRC_U8, N, H, W, ch, 0, scratch.data_ptr(), nbytes, s]
    assert lib.gsr_png_chunks(*ok) == 0
    for k, v in ((0, None), (7, None), (1, 2), (2, 0), (2, (1 << 24) + 1), (3, 0), (4, 0), (3, (1 << 20) + 1), (5, 2), (5, 5), (6, 2), (7, scratch.data_ptr() + 4)):
        bad = list(ok)
        bad[k] = v
        assert lib.gsr_png_chunks(*bad) == -1, (k, v)
    bad = list(ok)
    bad[8] = nbytes - 1
    assert lib.gsr_png_chunks(*bad) == -2
    bad = list(ok)
    bad[0], bad[1] = frames.data_ptr() + 1, _lib.GSR_PNG_SRC_F32_PLANAR
    assert lib.gsr_png_chunks(*bad) == -1
    ok = [scratch.data_ptr(), nbytes, N, H, W, ch, out.data_ptr(), bound, lengths.data_ptr(), s]
    assert lib.gsr_png_assemble(*ok) == 0
    for k, v in ((0, None), (6, None), (8, None), (0, scratch.data_ptr() + 8), (8, lengths.data_ptr() + 2), (2, 0), (3, 0), (4, 0), (5, 1), (7, bound - 1)):
        bad = list(ok)
        bad[k] = v
        assert lib.gsr_png_assemble(*bad) == -1, (k, v)
    bad = list(ok)
    bad[1] = nbytes - 1
    assert lib.gsr_png_assemble(*bad) == -2
    torch.cuda.synchronize()


def test_nothing_is_written_beyond_the_stream_length():
    """straight through the C ABI with an out stride of exactly the bound: the bytes behind each stream, and behind the last image, keep 0xA5"""
    lib = _lib.load()
    frames = torch.from_numpy(CASES["five_frames"][0]).to(DEV)
    N, H, W, ch = frames.shape
    nbytes, bound = lib.gsr_png_scratch_bytes(N, H, W, ch), lib.gsr_png_stream_bound(H, W, ch)
    scratch = torch.full((nbytes,), 0xA5, dtype=torch.uint8, device=DEV)
    out = torch.full((N * bound + 64,), 0xA5, dtype=torch.uint8, device=DEV)
    lengths = torch.full((N,), -1, dtype=torch.int32, device=DEV)
    s = C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
    _lib.check(lib.gsr_png_chunks(frames.data_ptr(), _lib.GSR_PNG_SRC_U8, N, H, W, ch, 0, scratch.data_ptr(), nbytes, s), "gsr_png_chunks")
    _lib.check(lib.gsr_png_assemble(scratch.data_ptr(), nbytes, N, H, W, ch, out.data_ptr(), bound, lengths.data_ptr(), s), "gsr_png_assemble")
    got, sizes = out.cpu().numpy(), lengths.cpu().tolist()
    want = encoded("five_frames")[0]
    for i, n in enumerate(sizes):
        assert got[i * bound:i * bound + n].tobytes() == io.idat_payload(want[i])
        assert (got[i * bound + n:(i + 1) * bound] == 0xA5).all()
    assert (got[N * bound:] == 0xA5).all()


def test_prep_image_on_the_device():
    for image, as_chw in prep_cases(DEV):
        got = io.prep_image(image)
        assert got.is_cuda and got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), _prep_reference(as_chw))


def test_save_scene_images_writes_the_reference_tree_from_device_tensors(tmp_path):
    from styl3r_amd.inference import save_scene_images
    batch, output, stylized = scene_batch(DEV)
    before = dict(io.CALLS)
    written = save_scene_images(tmp_path, "0a1b2c", "wave.jpg", batch, output, stylized)
    assert io.CALLS["png_hip"] == before["png_hip"] + 9 and io.CALLS["png_host"] == before["png_host"]
    check_scene_tree(tmp_path, written, batch, output, stylized)


class _FixedGaussians(torch.nn.Module):
    def __init__(self, g):
        super().__init__()
        self.g = g

    def forward(self, context, style, global_step):
        return self.g


def test_test_step_saves_the_rendered_views_when_asked(tmp_path):
    from styl3r_amd import evaluation
    from styl3r_amd.decoder import DecoderSplattingCUDACfg, Gaussians, get_decoder
    from styl3r_amd.scenes import make_scene
    sc = make_scene(n_ctx=1, grid_hw=(32, 32), n_views=2, image_hw=(32, 32), sh_degree=0, seed=4).to(DEV)
    g = Gaussians(sc.means[None], sc.covariances[None], sc.harmonics[None], sc.opacities[None])
    dec = get_decoder(DecoderSplattingCUDACfg("splatting_cuda", [0.0, 0.0, 0.0], True)).to(DEV)
    with torch.no_grad():
        target = dec.forward(g, sc.extrinsics[None], sc.intrinsics[None], sc.near[None], sc.far[None], (32, 32)).color
    batch = {"context": {"image": target[:, :1]}, "scene": ["scene_7"],
             "target": {"image": target, "extrinsics": sc.extrinsics[None], "intrinsics": sc.intrinsics[None], "near": sc.near[None],
                        "far": sc.far[None], "index": torch.tensor([[3, 17]], device=DEV)}}
    quiet = evaluation.TestCfg(align_pose=False, compute_scores=False, output_path=tmp_path / "off")
    evaluation.test_step(_FixedGaussians(g), dec, batch, [], quiet)
    assert not (tmp_path / "off").exists()                                       # the default writes nothing
    cfg = evaluation.TestCfg(align_pose=False, compute_scores=False, save_image=True, output_path=tmp_path / "on")
    out, _ = evaluation.test_step(_FixedGaussians(g), dec, batch, [], cfg)
    files = sorted(str(p.relative_to(tmp_path / "on")) for p in (tmp_path / "on").rglob("*") if p.is_file())
    assert files == ["scene_7/color/000003.png", "scene_7/color/000017.png"]
    for name, color in zip(files, out.color[0]):
        assert np.array_equal(np.asarray(Image.open(tmp_path / "on" / name)), io.prep_image(color).cpu().numpy())
    assert float(out.color.abs().sum()) > 0
