"""-m gpu: the kernels of csrc/gsr_jpeg.hip (k_jpeg_idct, k_jpeg_colour behind gsr_jpeg_pixels) through styl3r_amd/dataset.py, byte for
byte against what Pillow decoded (tests/golden/jpeg_frames.npz) and against the numpy restatement of the same module (which
tests/test_jpeg_host.py holds to the same fixtures); then ChunkDataset on the device against the CPU path.  No tolerance anywhere."""
import ctypes as C

import numpy as np
import pytest
import torch

from styl3r_amd import _lib
from styl3r_amd import dataset as ds
from styl3r_amd import inputs as si
from tests.test_dataset_host import make_dataset, same_tree
from tests.test_jpeg_host import CASES, SIZES, Z, stream

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_decode_on_the_device_equals_pillow_bytes(size):
    """every fast-path fixture of a size, one image per call (N = 1) and five per call (N = 5: sampling classes, tables and restart
    intervals mixed in a call, the last call of a size possibly shorter); not one image through the fallback"""
    here = [c for c in CASES if (c["W"], c["H"]) == size]
    before = dict(ds.CALLS)
    for per_call in (1, 5):
        for at in range(0, len(here), per_call):
            group = here[at:at + per_call]
            out = ds.decode_jpeg([stream(c["name"]) for c in group], device=DEV)
            assert out.is_cuda and out.dtype == torch.uint8 and tuple(out.shape) == (len(group), size[1], size[0], 3)
            for c, got in zip(group, out.cpu().numpy()):
                assert np.array_equal(got, Z["rgb_" + c["name"]]), (c["name"], per_call)
    assert ds.CALLS["jpeg_fallback"] == before["jpeg_fallback"] and ds.CALLS["jpeg_hip"] == before["jpeg_hip"] + 2 * len(here)


def random_image(rng, sampling, H, W, at):
    """seeded coefficient blocks inside the gate, with their descriptor: three coefficients of up to +-110 per block (one of them the DC)
    times table entries of up to 16 keep every column below 3 * 1760 = 5280 <= GSR_JPEG_MAX_COLUMN_L1; a DC of +-1760 alone is a flat
    block of +-220, far outside the byte range, so the range limit saturates both ways"""
    mw, mh = (16 if sampling in (_lib.GSR_JPEG_422, _lib.GSR_JPEG_420) else 8), (16 if sampling == _lib.GSR_JPEG_420 else 8)
    mx, my = -(-W // mw), -(-H // mh)
    nc = 1 if sampling == _lib.GSR_JPEG_GRAY else 3
    d = _lib.GsrJpegDesc()
    d.sampling, d.ncomp, d.coef_offset = sampling, nc, at
    count = 0
    for c in range(nc):
        d.bw[c], d.bh[c] = (mx * (mw // 8), my * (mh // 8)) if c == 0 else (mx, my)
        count += d.bw[c] * d.bh[c] * 64
        for k, q in enumerate(rng.integers(1, 17, 64)):
            d.quant[c][k] = int(q)
    d.coef_count = count
    blocks = np.zeros((count // 64, 64), np.int16)
    for b in blocks:
        pos = np.concatenate([[0], rng.choice(np.arange(1, 64), 2, replace=False)])
        b[pos] = rng.integers(-110, 111, 3)
    return blocks.reshape(-1), d


def pixels_on_device(coefs, desc, H, W):
    lib, n = _lib.load(), len(desc)
    arr = (_lib.GsrJpegDesc * n)(*desc)
    coefs_dev = torch.from_numpy(coefs).to(DEV)
    desc_dev = torch.frombuffer(arr, dtype=torch.uint8).to(DEV)
    nbytes = lib.gsr_jpeg_scratch_bytes(n, H, W)
    scratch = torch.full((nbytes,), 0xA5, dtype=torch.uint8, device=DEV)
    out = torch.full((n, H, W, 3), 0xA5, dtype=torch.uint8, device=DEV)
    stream_ = C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
    rc = lib.gsr_jpeg_pixels(coefs_dev.data_ptr(), desc_dev.data_ptr(), n, H, W, scratch.data_ptr(), nbytes, out.data_ptr(), stream_)
    _lib.check(rc, "gsr_jpeg_pixels")
    return out.cpu().numpy()


@pytest.mark.parametrize("size", [(1, 1), (3, 5), (17, 23), (33, 50)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_pixels_kernel_equals_the_numpy_restatement_on_random_coefficients(size):
    """gsr_jpeg_pixels fed directly, no encoder in between: all four sampling classes in ONE call (plus one image marked as not decoded,
    which must come out as zeros), coefficients that saturate the range limit, and at 1 x 1 and 3 x 5 the replication rule of chroma
    planes of at most two columns.  Two runs give identical bytes."""
    W, H = size
    rng = np.random.default_rng(1000 * W + H)
    classes = [_lib.GSR_JPEG_420, _lib.GSR_JPEG_GRAY, _lib.GSR_JPEG_422, _lib.GSR_JPEG_444, _lib.GSR_JPEG_420]
    coefs, desc, at = [], [], 0
    for s in classes:
        c, d = random_image(rng, s, H, W, at)
        coefs.append(c)
        desc.append(d)
        at += len(c)
    bad = _lib.GsrJpegDesc()
    bad.sampling, bad.coef_offset = -1, at
    desc.insert(2, bad)
    coefs = np.concatenate(coefs)
    want = np.stack([ds.pixels_host(coefs, d, H, W) for d in desc])
    assert not want[2].any() and (W * H < 100 or ((want[3:] == 0).any() and (want == 255).any()))          # saturated both ways
    got = pixels_on_device(coefs, desc, H, W)
    assert np.array_equal(got, want)
    assert np.array_equal(pixels_on_device(coefs, desc, H, W), got)


def test_descriptors_that_disagree_with_the_size_are_written_as_zeros():
    """a descriptor is the caller's: grids that are not those of (class, H, W), an offset off the 64-value grid or beyond the buffer
    give zeros for that image, and its neighbours are untouched"""
    W, H = 17, 23
    rng = np.random.default_rng(3)
    coefs, desc, at = [], [], 0
    for s in (_lib.GSR_JPEG_444, _lib.GSR_JPEG_420, _lib.GSR_JPEG_422, _lib.GSR_JPEG_444, _lib.GSR_JPEG_420):
        c, d = random_image(rng, s, H, W, at)
        coefs.append(c)
        desc.append(d)
        at += len(c)
    coefs = np.concatenate(coefs)
    want = np.stack([ds.pixels_host(coefs, d, H, W) for d in desc])
    desc[1].bw[0] += 2
    desc[2].coef_offset += 8
    desc[3].coef_offset = 1 << 40
    desc[4].sampling = 9
    got = pixels_on_device(coefs, desc, H, W)
    assert np.array_equal(got[0], want[0]) and not got[1:].any()


def test_bad_arguments_are_einval_before_any_launch():
    lib = _lib.load()
    coefs, d = random_image(np.random.default_rng(0), _lib.GSR_JPEG_444, 8, 8, 0)
    arr = (_lib.GsrJpegDesc * 1)(d)
    c = torch.from_numpy(coefs).to(DEV)
    dd = torch.frombuffer(arr, dtype=torch.uint8).to(DEV)
    nbytes = lib.gsr_jpeg_scratch_bytes(1, 8, 8)
    scratch, out = torch.empty(nbytes + 16, dtype=torch.uint8, device=DEV), torch.empty((1, 8, 8, 3), dtype=torch.uint8, device=DEV)
    s = C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
    ok = [c.data_ptr(), dd.data_ptr(), 1, 8, 8, scratch.data_ptr(), nbytes, out.data_ptr(), s]
    assert lib.gsr_jpeg_pixels(*ok) == 0
    for k, v in ((0, None), (1, None), (5, None), (7, None), (2, 0), (3, 0), (4, 65536), (0, c.data_ptr() + 2), (5, scratch.data_ptr() + 4),
                 (7, out.data_ptr() + 1)):
        bad = list(ok)
        bad[k] = v
        assert lib.gsr_jpeg_pixels(*bad) == -1, (k, v)
    bad = list(ok)
    bad[6] = nbytes - 1
    assert lib.gsr_jpeg_pixels(*bad) == -2
    torch.cuda.synchronize()


def test_fallback_images_share_a_device_call_with_decoded_ones():
    name = [c["name"] for c in CASES if (c["W"], c["H"], c["sampling"]) == (33, 50, "420")][0]
    names = ["fb_progressive", name, "fb_cmyk"]
    before = dict(ds.CALLS)
    out = ds.decode_jpeg([stream(n) for n in names], device=DEV).cpu().numpy()
    for n, got in zip(names, out):
        assert np.array_equal(got, Z["rgb_" + n]), n
    assert ds.CALLS["jpeg_fallback"] == before["jpeg_fallback"] + 2 and ds.CALLS["jpeg_hip"] == before["jpeg_hip"] + 1


def test_chunk_dataset_on_the_device_equals_the_cpu_path():
    """images equal as bytes / 255 (fp32 bits), cameras bit-equal, indices and scenes equal; batches through the prefetch thread too"""
    torch.manual_seed(0)
    host = list(make_dataset())
    torch.manual_seed(0)
    before = dict(ds.CALLS)
    dev = list(make_dataset(device=DEV))
    assert len(dev) == len(host) == 3 and ds.CALLS["jpeg_hip"] == before["jpeg_hip"] + 12 and ds.CALLS["jpeg_fallback"] == before["jpeg_fallback"]
    for a, b in zip(dev, host):
        assert a["context"]["image"].is_cuda and a["context"]["extrinsics"].is_cuda and a["style"]["image"].is_cuda
        same_tree(a, b)
    torch.manual_seed(0)
    batches = list(ds.iter_batches(make_dataset(device=DEV), 2, prefetch=1))
    same_tree(batches[0], si.collate(host[:2]))
    same_tree(batches[1], si.collate(host[2:]))


def test_decoded_frames_through_rescale_and_crop_equal_pillow_frames_through_it():
    here = [c for c in CASES if (c["W"], c["H"]) == (200, 120)]
    frames = ds.decode_jpeg([stream(c["name"]) for c in here], device=DEV)
    pil = torch.from_numpy(np.stack([Z["rgb_" + c["name"]] for c in here])).to(DEV)
    K = torch.eye(3, device=DEV).repeat(len(here), 1, 1)
    got, Kg = si.rescale_and_crop(frames, K, (64, 64))
    want, Kw = si.rescale_and_crop(pil, K, (64, 64))
    assert got.shape == (len(here), 3, 64, 64) and torch.equal(got.view(torch.int32), want.view(torch.int32)) and torch.equal(Kg, Kw)
