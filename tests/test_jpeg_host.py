"""styl3r_amd.dataset.decode_jpeg on the CPU: the host entropy stage (csrc/gsr_jpeg_entropy.h through gsr_jpeg_probe / gsr_jpeg_entropy)
plus the numpy restatement of the device stage, byte for byte against what Pillow decoded from the same streams
(tests/golden/jpeg_frames.npz, written by tests/golden/make_jpeg_fixtures.py).  No tolerance anywhere: every comparison is
np.array_equal on bytes.  Needs the library (the entropy stage is host code inside it), no GPU."""
import ctypes as C
import json
from pathlib import Path

import numpy as np
import pytest
import torch

from styl3r_amd import _lib
from styl3r_amd import dataset as ds

Z = np.load(Path(__file__).resolve().parent / "golden" / "jpeg_frames.npz")
CASES = json.loads(str(Z["cases"]))
FALLBACK = json.loads(str(Z["fallback"]))
SIZES = sorted({(c["W"], c["H"]) for c in CASES})
CLASS = {"gray": _lib.GSR_JPEG_GRAY, "444": _lib.GSR_JPEG_444, "422": _lib.GSR_JPEG_422, "420": _lib.GSR_JPEG_420}


def stream(name: str) -> bytes:
    return Z["jpg_" + name].tobytes()


def test_the_fixture_holds_what_the_issue_lists():
    assert SIZES == sorted([(1, 1), (2, 2), (3, 5), (8, 8), (16, 16), (17, 23), (33, 50), (64, 40), (200, 120)])
    for W, H in SIZES:
        here = [c for c in CASES if (c["W"], c["H"]) == (W, H)]
        assert {c["sampling"] for c in here} >= {"444", "422", "420"}, (W, H)
        assert {c["kind"] for c in here} == {"photo", "noise"}, (W, H)
        if (W, H) != (200, 120):
            assert {(c["sampling"], c["quality"]) for c in here} >= {(s, q) for s in ("444", "422", "420") for q in (30, 75, 100)}, (W, H)
            assert {c["variant"] for c in here} == {"plain", "optimize", "restart"}, (W, H)
    assert any(c["sampling"] == "gray" for c in CASES)
    assert any(c["kind"] == "noise" and c["quality"] == 100 and (c["W"], c["H"]) == (200, 120) for c in CASES)


def test_every_fixture_is_a_baseline_stream_of_its_class():
    """gsr_jpeg_probe: GSR_OK, the size, the component count, the sampling class and the restart interval of every fast-path fixture"""
    for c in CASES:
        rc, info = ds.jpeg_probe(stream(c["name"]))
        assert rc == 0, c["name"]
        assert (info.width, info.height) == (c["W"], c["H"]), c["name"]
        assert info.sampling == CLASS[c["sampling"]] and info.components == (1 if c["sampling"] == "gray" else 3), c["name"]
        assert (info.restart_interval > 0) == (c["variant"] == "restart"), c["name"]
    assert ds.jpeg_probe(stream("fb_progressive"))[0] == _lib.GSR_JPEG_UNSUPPORTED
    assert ds.jpeg_probe(stream("fb_cmyk"))[0] == _lib.GSR_JPEG_UNSUPPORTED
    assert ds.jpeg_probe(b"")[0] == _lib.GSR_JPEG_CORRUPT and ds.jpeg_probe(b"\xff\xd8\xff")[0] == _lib.GSR_JPEG_CORRUPT


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_decode_equals_pillow_bytes(size):
    """one call per size over ALL its fixtures: sampling classes, tables, Huffman variants and restart intervals mixed in one batch"""
    here = [c for c in CASES if (c["W"], c["H"]) == size]
    before = dict(ds.CALLS)
    out = ds.decode_jpeg([stream(c["name"]) for c in here])
    assert out.dtype == torch.uint8 and tuple(out.shape) == (len(here), size[1], size[0], 3) and not out.is_cuda
    for c, got in zip(here, out.numpy()):
        assert np.array_equal(got, Z["rgb_" + c["name"]]), c["name"]
    assert ds.CALLS["jpeg_fallback"] == before["jpeg_fallback"]                   # not one image left to PIL
    assert ds.CALLS["jpeg_host"] == before["jpeg_host"] + len(here) and ds.CALLS["jpeg_hip"] == before["jpeg_hip"]


def test_single_images_and_tensor_blobs():
    for name in ("17x23_420_q75_plain_photo", "3x5_422_q100_restart_noise", "64x40_gray_q75_plain_photo"):
        exp = Z["rgb_" + name]
        assert np.array_equal(ds.decode_jpeg([stream(name)])[0].numpy(), exp), name
        assert np.array_equal(ds.decode_jpeg([torch.from_numpy(Z["jpg_" + name].copy())])[0].numpy(), exp), name


def test_fallback_streams_go_to_pillow_and_are_counted():
    mixed = ["33x50_420_q75_" + v for v in ("plain_photo", "optimize_photo", "restart_photo")]
    mixed = [n for n in mixed if "jpg_" + n in Z][:1]
    names = ["fb_progressive", mixed[0], "fb_cmyk"]
    before = dict(ds.CALLS)
    out = ds.decode_jpeg([stream(n) for n in names]).numpy()
    for n, got in zip(names, out):
        assert np.array_equal(got, Z["rgb_" + n]), n
    assert ds.CALLS["jpeg_fallback"] == before["jpeg_fallback"] + 2 and ds.CALLS["jpeg_host"] == before["jpeg_host"] + 1


def test_truncated_stream_raises_what_pillow_raised():
    rc, _ = ds.jpeg_probe(stream("fb_truncated"))
    assert rc == 0                                       # the markers are whole: the entropy stage finds the end
    res_status = entropy([stream("fb_truncated")], 40, 64)[2]
    assert res_status[0] == _lib.GSR_JPEG_CORRUPT
    assert FALLBACK["fb_truncated"]["error"] == "OSError"
    with pytest.raises(OSError) as err:
        ds.decode_jpeg([stream("fb_truncated")])
    assert str(err.value) == FALLBACK["fb_truncated"]["message"]


def test_mixed_sizes_raise_value_error_naming_them():
    with pytest.raises(ValueError, match=r"\(23, 17\).*\(50, 33\)"):
        ds.decode_jpeg([stream("17x23_420_q75_plain_photo"), stream([c["name"] for c in CASES if (c["W"], c["H"]) == (33, 50)][0])])
    with pytest.raises(ValueError):
        ds.decode_jpeg([])


def entropy(blobs, H, W, threads=1):
    """gsr_jpeg_entropy directly -> (coefficient prefix, descriptors, status, return code)"""
    lib, n = _lib.load(), len(blobs)
    nbytes = lib.gsr_jpeg_coef_bytes(n, H, W)
    coefs = np.full(nbytes // 2, 0x5a5a, np.int16)
    desc = (_lib.GsrJpegDesc * n)()
    status = np.full(n, -7, np.int32)
    ptrs = (C.c_void_p * n)(*[C.cast(C.c_char_p(b), C.c_void_p) for b in blobs])
    lens = (C.c_size_t * n)(*[len(b) for b in blobs])
    rc = lib.gsr_jpeg_entropy(ptrs, lens, n, H, W, coefs.ctypes.data, C.addressof(desc), status.ctypes.data, threads)
    used = max(int(d.coef_offset + d.coef_count) for d in desc) if rc == 0 else 0
    return coefs[:used].copy(), desc, status, rc


def test_thread_counts_give_identical_coefficients():
    here = [c for c in CASES if (c["W"], c["H"]) == (33, 50)]
    blobs = [stream(c["name"]) for c in here] + [stream("fb_progressive"), stream("17x23_420_q75_plain_photo")]
    ref = None
    for threads in (0, 1, 16, 1000):
        coefs, desc, status, rc = entropy(blobs, 50, 33, threads)
        assert rc == 0 and status[:len(here)].tolist() == [0] * len(here)
        assert status[-2:].tolist() == [_lib.GSR_JPEG_UNSUPPORTED] * 2             # progressive; a picture of another size
        assert desc[len(here)].sampling == -1 and desc[len(here)].coef_count == 0
        got = (coefs.tobytes(), bytes(desc), status.tobytes())
        ref = ref or got
        assert got == ref, threads


def test_bad_arguments_are_einval_before_any_work():
    lib = _lib.load()
    blob = stream("8x8_444_q75_plain_photo")
    ptrs, lens = (C.c_void_p * 1)(C.cast(C.c_char_p(blob), C.c_void_p)), (C.c_size_t * 1)(len(blob))
    coefs, desc, status = np.zeros(4096, np.int16), (_lib.GsrJpegDesc * 1)(), np.full(1, -7, np.int32)
    args = lambda **kw: [kw.get("ptrs", ptrs), kw.get("lens", lens), kw.get("n", 1), kw.get("H", 8), kw.get("W", 8),
                         kw.get("coefs", coefs.ctypes.data), kw.get("desc", C.addressof(desc)), kw.get("status", status.ctypes.data), 1]
    assert lib.gsr_jpeg_entropy(*args()) == 0 and status[0] == 0
    status[0] = -7
    for bad in (dict(ptrs=None), dict(lens=None), dict(coefs=None), dict(desc=None), dict(status=None), dict(n=0), dict(H=0), dict(W=0),
                dict(H=65536), dict(W=1 << 20)):
        assert lib.gsr_jpeg_entropy(*args(**bad)) == -1, bad
    assert status[0] == -7
    assert lib.gsr_jpeg_coef_bytes(0, 8, 8) == 0 and lib.gsr_jpeg_coef_bytes(1, 0, 8) == 0 and lib.gsr_jpeg_scratch_bytes(1, 8, 70000) == 0
    assert lib.gsr_jpeg_coef_bytes(2, 8, 8) == 2 * 6 * 64 * 2                      # 4:2:0 pads 8 x 8 to one 16 x 16 MCU: six blocks
    assert lib.gsr_jpeg_probe(None, 0, C.byref(_lib.GsrJpegInfo())) == -1


def test_no_prefix_and_no_single_byte_change_crashes_the_entropy_stage():
    """every proper prefix of one 17 x 23 4:2:0 stream, and the stream with each of its first 700 bytes set to 0x00 and to 0xFF: each is
    answered with a status (and whatever it is, the coefficient count stays inside the buffer); the guard words behind the used
    prefix are untouched"""
    base = stream("17x23_420_q100_plain_noise" if "jpg_17x23_420_q100_plain_noise" in Z else
                  [c["name"] for c in CASES if (c["W"], c["H"], c["sampling"]) == (17, 23, "420")][0])
    assert len(base) > 700
    variants = [base[:k] for k in range(len(base))]
    for k in range(700):
        for v in (0x00, 0xFF):
            if base[k] != v:
                variants.append(base[:k] + bytes([v]) + base[k + 1:])
    lib = _lib.load()
    n = len(variants)
    coefs = np.full(lib.gsr_jpeg_coef_bytes(n, 23, 17) // 2 + 64, 0x5a5a, np.int16)
    desc = (_lib.GsrJpegDesc * n)()
    status = np.full(n, -7, np.int32)
    ptrs = (C.c_void_p * n)(*[C.cast(C.c_char_p(b), C.c_void_p) for b in variants])
    lens = (C.c_size_t * n)(*[len(b) for b in variants])
    assert lib.gsr_jpeg_entropy(ptrs, lens, n, 23, 17, coefs.ctypes.data, C.addressof(desc), status.ctypes.data, 4) == 0
    assert set(status.tolist()) <= {0, _lib.GSR_JPEG_UNSUPPORTED, _lib.GSR_JPEG_CORRUPT}
    # no proper prefix is a whole picture: the one that lost only (part of) the EOI marker is left to Pillow too, which refuses it
    assert base[-2:] == b"\xff\xd9" and (status[:len(base)] != 0).all()
    with pytest.raises(OSError):
        ds.decode_jpeg([base[:-1]])
    assert (status == 0).any() and (status == _lib.GSR_JPEG_CORRUPT).any()
    assert (coefs[-64:] == 0x5a5a).all()
    per_image = 6 * 2 * 2 * 64                                                     # 17 x 23 at 4:2:0: 2 x 2 MCUs of six blocks
    for d, s in zip(desc, status):
        assert d.coef_count == (per_image if s == 0 else 0) and 0 <= d.coef_offset <= (n - 1) * per_image
    for b in variants[::97]:
        info = _lib.GsrJpegInfo()
        assert lib.gsr_jpeg_probe(b, len(b), C.byref(info)) in (0, _lib.GSR_JPEG_UNSUPPORTED, _lib.GSR_JPEG_CORRUPT)


def test_coefficient_gate_sends_large_blocks_to_the_fallback():
    """a stream whose quantisation table is scaled up far enough leaves the gate: UNSUPPORTED, never a wrong picture"""
    base = bytearray(stream("16x16_444_q100_plain_noise"))
    at = base.find(b"\xff\xdb")
    assert at > 0 and base[at + 4] == 0                                           # 8-bit table 0
    for k in range(64):
        base[at + 5 + k] = 255
    coefs, desc, status, rc = entropy([bytes(base)], 16, 16)
    assert rc == 0 and status[0] == _lib.GSR_JPEG_UNSUPPORTED and desc[0].sampling == -1
    from PIL import Image
    from io import BytesIO
    before = ds.CALLS["jpeg_fallback"]
    got = ds.decode_jpeg([bytes(base)])[0].numpy()
    assert ds.CALLS["jpeg_fallback"] == before + 1
    assert np.array_equal(got, np.asarray(Image.open(BytesIO(bytes(base))).convert("RGB")))
