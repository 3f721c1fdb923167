"""styl3r_amd/image_io.py on the host: the integer restatement of csrc/gsr_png.hip (what tests/test_gpu_png.py holds the kernels to, byte
for byte) against Pillow and zlib -- every file loads (so Pillow has checked the CRCs), decodes to exactly the input bytes, and its
IDAT payload inflates to H * (1 + W * C) bytes; no tolerance.  Then the two size conditions the format gives, the one measured
comparison against zlib's own Z_RLE on the same filtered bytes and chunks, and the reference's functions around the encoder."""
import zlib
from io import BytesIO

import numpy as np
import pytest
import torch
from PIL import Image

from styl3r_amd import image_io as io
from styl3r_amd.export import _rgb_bytes_host

CHUNK = io.CHUNK_BYTES


def _rng(seed):
    return np.random.default_rng(seed)


def _gradient(H, W, C, seed, noise=6.0):
    y, x = np.mgrid[0:H, 0:W]
    base = (x * (200.0 / max(W - 1, 1)) + y * (55.0 / max(H - 1, 1)))[..., None] + np.arange(C) * 9.0
    return np.clip(base + _rng(seed).normal(0, noise, (H, W, C)), 0, 255).astype(np.uint8)


def _blob(H, W, C=3):
    y, x = np.mgrid[0:H, 0:W]
    g = 255 * np.exp(-((x - 0.5 * W) ** 2 + (y - 0.45 * H) ** 2) / (0.014 * H * W))
    return (g[..., None] * np.array([1.0, 0.7, 0.4, 1.0])[:C]).astype(np.uint8)


def _edge_filters(C):
    """a 3 x 5 picture (W = 3, H = 5) whose adaptive choice is Average on the first row and Paeth on a later one, found by a seeded
    search: the two predictors that read the missing left / upper neighbours as zeros are then really used at those edges"""
    rng = _rng(100 + C)
    for _ in range(4000):
        img = np.zeros((5, 3, C), np.int64)
        img[0, 0] = rng.integers(128, 256, C)
        img[0, 1], img[0, 2] = img[0, 0] // 2 + rng.integers(0, 2, C), img[0, 0] // 4 + rng.integers(0, 2, C)      # x ~ a / 2: Average
        for r in range(1, 5):
            for p in range(3):
                a = img[r, p - 1] if p else np.zeros(C, np.int64)
                b, c = img[r - 1, p], (img[r - 1, p - 1] if p else np.zeros(C, np.int64))
                pick = rng.integers(0, 3)
                img[r, p] = np.clip((a, b, a + b - c)[pick] + rng.integers(-1, 2, C) * (rng.random() < 0.3) + (40 if pick == 0 and p == 1 else 0), 0, 255)
        img = img.astype(np.uint8)
        f = io.filter_rows(img.reshape(5, 3 * C), C, 0)[:, 0]
        if f[0] == 3 and 4 in f[1:]:
            return img
    raise AssertionError("no 3 x 5 picture with Average on the first row and Paeth below it")


def _fibonacci_row():
    """filter none, one row of W = 2254 RGB pixels.  The literal / length histogram of its chunk is the Fibonacci sequence over 18
    symbols: the end of block (1), byte 0 -- the filter byte, nowhere else -- (1) and 16 byte values with counts F3 .. F18 = 2, 3, 5 ..
    2584 (6 762 pixel bytes, 6 763 filtered bytes, inside one chunk), no two equal bytes next to each other (so no match).  Every merge
    then joins the running sum with the next leaf: an unlimited Huffman code is 17 bits deep.  (With 18 byte values next to the end of
    block the chain breaks at its first step -- 1, 1, 1, 2, 3 .. -- and the code is 10 bits deep.)"""
    fib = [1, 1]
    while len(fib) < 18:
        fib.append(fib[-1] + fib[-2])
    vals = np.repeat(np.arange(1, 17, dtype=np.uint8) * 7, fib[2:])[::-1].copy()
    row = np.zeros(len(vals), np.uint8)
    half = (len(vals) + 1) // 2
    row[0::2], row[1::2] = vals[:half], vals[half:]
    assert len(row) == 6762 and (row[1:] != row[:-1]).all() and row[0] != 0
    return row.reshape(1, 2254, 3)


def _runs_row():
    """filter none: runs of L = 300 zeros (with the filter byte: 301), 260 (R = 259 = 258 + 1 literal), 261 (258 + 2 literals), 259 (one
    match of 258), 1000, 3 (R = 2: two literals), 4 (R = 3: the shortest match), 2, then 30 distinct bytes"""
    parts = [np.zeros(300, np.uint8)] + [np.full(n, v, np.uint8) for v, n in ((5, 260), (6, 261), (7, 259), (8, 1000), (9, 3), (10, 4), (11, 2))]
    row = np.concatenate(parts + [np.arange(30, 60, dtype=np.uint8)])
    row = np.concatenate([row, np.zeros(-len(row) % 3, np.uint8) + 99])
    return row.reshape(1, -1, 3)


# name -> (uint8 (N,H,W,C), filter, random?)   the smallest shapes that reach each branch (row of W = 100 RGB: 301 bytes, 54 rows a chunk)
CASES = {
    "1x1_rgb": (_rng(1).integers(0, 256, (1, 1, 1, 3), dtype=np.uint8), "adaptive", True),
    "1x1_rgba": (_rng(2).integers(0, 256, (1, 1, 1, 4), dtype=np.uint8), "adaptive", True),
    "3x5_rgb": (_edge_filters(3)[None], "adaptive", True),
    "3x5_rgba": (_edge_filters(4)[None], "adaptive", True),
    "exactly_one_chunk": (_gradient(54, 100, 3, 3)[None], "adaptive", False),
    "three_chunks": (_gradient(120, 100, 3, 4)[None], "adaptive", False),
    "three_chunks_rgba": (_gradient(120, 75, 4, 5)[None], "adaptive", False),
    "wide_1920x3": (_gradient(3, 1920, 3, 6)[None], "adaptive", False),
    "five_frames": (np.stack([_gradient(60, 100, 3, 10 + i, noise=2.0 * i) for i in range(5)]), "adaptive", False),
    "flat": (np.full((1, 120, 100, 3), 77, np.uint8), "adaptive", False),
    "flat_none": (np.full((1, 120, 100, 3), 77, np.uint8), "none", False),
    "run_remainders": (_runs_row()[None], "none", False),
    "blob": (_blob(96, 96)[None], "adaptive", False),
    "random": (_rng(7).integers(0, 256, (1, 120, 100, 3), dtype=np.uint8), "adaptive", True),
    "random_full_chunk": (_rng(8).integers(0, 256, (1, 1, 5461, 3), dtype=np.uint8), "none", True),
    "fibonacci": (_fibonacci_row()[None], "none", False),
    "no_run": (np.tile(np.array([1, 2], np.uint8), 1500).reshape(1, 1, 1000, 3), "none", False),
    "single_run_full_chunk": (np.zeros((1, 1, 5461, 3), np.uint8), "none", False),
}
_ENCODED = {}


def encoded(name):
    """(files, details) of a case through the CPU restatement, computed once and shared (tests/test_gpu_png.py compares against it)"""
    if name not in _ENCODED:
        frames, filt, _ = CASES[name]
        details = {}
        _ENCODED[name] = (io.encode_png(torch.from_numpy(frames), filt, details), details)
    return _ENCODED[name]


def check_files(files, frames):
    """the validity conditions of one call's output"""
    N, H, W, C = frames.shape
    assert len(files) == N
    for png, want in zip(files, frames):
        im = Image.open(BytesIO(png))
        im.load()
        assert im.size == (W, H) and im.mode == ("RGB" if C == 3 else "RGBA")
        assert np.array_equal(np.asarray(im), want)
        assert len(zlib.decompress(io.idat_payload(png))) == H * (1 + W * C)


def n_chunks(H, W, C):
    return -(-H // io.chunk_rows(H, W, C))


def file_bound(H, W, C):
    """8 + 25 + 12 + 2 + sum over the chunks (chunk bytes + 5) + 5 + 4 + 12"""
    return 8 + 25 + 12 + 2 + H * (1 + W * C) + 5 * n_chunks(H, W, C) + 5 + 4 + 12


@pytest.mark.parametrize("name", list(CASES))
def test_files_load_in_pillow_and_decode_to_the_input_bytes(name):
    frames = CASES[name][0]
    files, details = encoded(name)
    check_files(files, frames)
    _, H, W, C = frames.shape
    assert details["chunks"] == frames.shape[0] * n_chunks(H, W, C)


@pytest.mark.parametrize("name", list(CASES))
def test_size_within_the_stored_bound_and_below_the_raw_pixels(name):
    frames, _, is_random = CASES[name]
    _, H, W, C = frames.shape
    for png in encoded(name)[0]:
        assert len(png) <= file_bound(H, W, C)
        if not is_random:
            assert len(png) < H * W * C, (len(png), H * W * C)


def test_the_cases_reach_the_branches_they_are_named_for():
    d = {name: encoded(name)[1] for name in CASES}
    for name in ("random", "random_full_chunk"):
        assert d[name]["stored"] == d[name]["chunks"], name                     # every chunk of random bytes is a stored block
    assert len(encoded("random_full_chunk")[0][0]) == file_bound(1, 5461, 3)     # ... and meets the bound exactly: 16384 + 5 in the slot
    assert d["fibonacci"]["limit_acted"] == 1 and d["fibonacci"]["max_length"] == 15 and d["fibonacci"]["matches"] == 0 \
        and "stored" not in d["fibonacci"]
    hist = np.bincount(np.concatenate([[0], CASES["fibonacci"][0].reshape(-1)]), minlength=286)
    hist[256] = 1
    assert max(io.code_lengths(hist, 32)[0]) == 17                             # what the limit cut down
    assert d["no_run"]["matches"] == 0 and "stored" not in d["no_run"]          # HDIST 1 with a zero length
    assert d["single_run_full_chunk"]["chunks"] == 1 and d["single_run_full_chunk"]["matches"] == 64     # 16383 = 63 * 258 + 129
    assert d["three_chunks"]["chunks"] == 3 and d["exactly_one_chunk"]["chunks"] == 1 and d["wide_1920x3"]["chunks"] == 2
    assert d["flat"]["matches"] >= 3 and d["run_remainders"]["matches"] == 2 + 1 + 1 + 1 + 4 + 1
    filt = io.filter_rows(CASES["three_chunks"][0][0].reshape(120, 300), 3, 0)[:, 0]
    assert filt[54] in (2, 3, 4) and filt[108] in (2, 3, 4)                     # a chunk's first row is filtered against the raw row above it
    for C in (3, 4):
        f = io.filter_rows(CASES["3x5_rgb" if C == 3 else "3x5_rgba"][0][0].reshape(5, 3 * C), C, 0)[:, 0]
        assert f[0] == 3 and 4 in f[1:]


def _png_filter_reference(raw, C):
    """the five PNG filters of the specification, byte by byte"""
    H, WC = raw.shape
    out = np.zeros((5, H, WC), np.uint8)
    for y in range(H):
        for j in range(WC):
            x = int(raw[y, j])
            a = int(raw[y, j - C]) if j >= C else 0
            b = int(raw[y - 1, j]) if y else 0
            c = int(raw[y - 1, j - C]) if y and j >= C else 0
            p = a + b - c
            pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
            pr = a if pa <= pb and pa <= pc else (b if pb <= pc else c)
            out[:, y, j] = [x, (x - a) % 256, (x - b) % 256, (x - (a + b) // 2) % 256, (x - pr) % 256]
    return out


@pytest.mark.parametrize("name", ["1x1_rgb", "3x5_rgb", "3x5_rgba", "blob"])
def test_adaptive_filter_is_the_minimum_sum_of_absolute_differences(name):
    frames = CASES[name][0]
    _, H, W, C = frames.shape
    raw = frames[0].reshape(H, W * C)
    got = io.filter_rows(raw, C, 0)
    cand = _png_filter_reference(raw, C).astype(np.int64)
    cost = np.minimum(cand, 256 - cand).sum(axis=2)
    for y in range(H):
        k = int(got[y, 0])
        assert k == min(range(5), key=lambda f: (cost[f, y], f)) and np.array_equal(got[y, 1:], cand[k, y])
    assert np.array_equal(io.filter_rows(raw, C, 1)[:, 1:], raw) and not io.filter_rows(raw, C, 1)[:, 0].any()


def test_length_limited_code_is_complete_and_keeps_the_order_of_the_counts():
    rng = _rng(11)
    for trial in range(40):
        n, limit = ((286, 15), (19, 7))[trial % 2]
        counts = (rng.integers(0, 2, n) * (2.0 ** rng.uniform(0, 14 if limit == 15 else 9, n))).astype(np.int64)
        counts[rng.integers(0, n)] = 1
        counts[rng.integers(0, n)] += 1
        lens, num, _ = io.code_lengths(counts, limit)
        used = [s for s in range(n) if counts[s]]
        assert all(lens[s] == 0 for s in range(n) if not counts[s]) and all(1 <= lens[s] <= limit for s in used)
        if len(used) > 1:
            assert sum(2.0 ** -lens[s] for s in used) == 1.0                     # Kraft with equality: zlib's inflate refuses anything else
        assert all(lens[s] <= lens[u] for s in used for u in used if counts[s] > counts[u])
        assert num[1:] == [sum(1 for s in used if lens[s] == d) for d in range(1, limit + 1)]


def yardstick(frames, filt):
    """zlib itself on the same filtered stream and the same chunking: raw deflate, strategy Z_RLE, Z_SYNC_FLUSH after each chunk, plus the
    same 11 bytes of framing (zlib header, final empty stored block, Adler-32)"""
    _, H, W, C = frames.shape
    rows = io.chunk_rows(H, W, C)
    total = 0
    for img in frames:
        f = io.filter_rows(img.reshape(H, W * C), C, io.FILTERS[filt])
        z = zlib.compressobj(6, zlib.DEFLATED, -15, 8, zlib.Z_RLE)
        total += 11 + sum(len(z.compress(f[r:r + rows].tobytes())) + len(z.flush(zlib.Z_SYNC_FLUSH)) for r in range(0, H, rows))
    return total


SIZE_FRAMES = {"noisy_gradient": lambda: _gradient(256, 256, 3, 21, noise=8.0), "blob_on_black": lambda: _blob(256, 256), "flat": lambda: np.full((256, 256, 3), 77, np.uint8)}
# measured 1.0000 / 0.9997 / 0.9875 of the yardstick (2 bytes over on the noisy gradient, below it on the other two).  Both
# code the same tokens with optimal Huffman codes, so only the header form can cost anything, per chunk: this encoder always sends
# HLIT = 286 where zlib trims the trailing zero lengths -- one more code-18 token, at most 7 + 7 bits; its greedy choice of repeat codes
# against zlib's own rule -- allowed one more token of at most 7 + 4 bits; and each chunk ends on a byte boundary, so up to 7 bits of a
# difference round up.  14 + 11 + 7 = 32 bits: 4 bytes per chunk, 52 bytes on the 13 chunks of a 256 x 256 RGB frame (0.04 % .. 6 %).
HEADER_MARGIN_PER_CHUNK = 4


@pytest.mark.parametrize("name", list(SIZE_FRAMES))
def test_stream_size_against_zlib_rle_on_the_same_chunks(name):
    frames = SIZE_FRAMES[name]()[None]
    files = io.encode_png(torch.from_numpy(frames))
    check_files(files, frames)
    ours, ref = len(io.idat_payload(files[0])), yardstick(frames, "adaptive")
    print(f"{name}: IDAT payload {ours} B, zlib Z_RLE construction {ref} B, ratio {ours / ref:.4f}, file {len(files[0])} B")
    assert ours <= ref + HEADER_MARGIN_PER_CHUNK * n_chunks(256, 256, 3), (ours, ref)
    assert len(files[0]) < 256 * 256 * 3


def test_float_frames_convert_as_prep_image_does():
    x = torch.from_numpy(_rng(12).random((2, 3, 9, 7)).astype(np.float32) * 1.4 - 0.2)
    x[0, 0, 0, :7] = torch.tensor([-0.1, 0.0, 0.5 / 255, float(np.float32(1 / 255) - np.float32(1e-9)), 1.0, 1.5, float("nan")])
    x[1, 2, 8, :3] = torch.tensor([float("inf"), float("-inf"), 254.999 / 255])
    want = _rgb_bytes_host(x).contiguous()
    assert want[0, 0, :7, 0].tolist() == [0, 0, 0, 0, 255, 255, 0] and want[1, 8, :3, 2].tolist() == [255, 0, 254]
    files = io.encode_png(x)
    assert files == io.encode_png(want)
    check_files(files, want.numpy())
    rgba = torch.cat([x, x[:, :1]], dim=1)
    check_files(io.encode_png(rgba), _rgb_bytes_host(rgba).contiguous().numpy())


def test_a_row_wider_than_a_chunk_goes_to_pillow_and_is_counted():
    frames = _gradient(2, 5462, 3, 13)[None]                                    # 1 + 5462 * 3 = 16387 > 16384
    assert io.chunk_rows(2, 5462, 3) == 0 and io.chunk_rows(2, 5461, 3) == 1
    before = dict(io.CALLS)
    files = io.encode_png(torch.from_numpy(frames))
    assert io.CALLS["png_fallback"] == before["png_fallback"] + 1 and io.CALLS["png_host"] == before["png_host"]
    assert np.array_equal(np.asarray(Image.open(BytesIO(files[0]))), frames[0])
    io.encode_png(torch.from_numpy(CASES["blob"][0]))
    assert io.CALLS["png_host"] == before["png_host"] + 1


def test_encode_png_refuses_what_it_does_not_write():
    for bad in (torch.zeros(4, 4, 3, dtype=torch.uint8), torch.zeros(1, 4, 4, 2, dtype=torch.uint8), torch.zeros(1, 1, 4, 4), torch.zeros(1, 3, 4, 4, dtype=torch.float64),
                torch.zeros(0, 4, 4, 3, dtype=torch.uint8)):
        with pytest.raises(ValueError):
            io.encode_png(bad)
    with pytest.raises(ValueError):
        io.encode_png(torch.zeros(1, 4, 4, 3, dtype=torch.uint8), filter="paeth")


def _prep_reference(image):
    """the last two lines of the reference's prep_image (image_io.py:53-54) on a (C,H,W) tensor"""
    image = (image.detach().clip(min=0, max=1) * 255).type(torch.uint8)
    return image.permute(1, 2, 0).cpu().numpy()


def prep_cases(device="cpu"):
    g = torch.Generator().manual_seed(5)
    r = lambda *s: (torch.rand(*s, generator=g) * 1.2 - 0.1).to(device)
    hw, chw1, chw3, chw4, bchw = r(6, 5), r(1, 6, 5), r(3, 6, 5), r(4, 6, 5), r(3, 3, 6, 5)
    return [(hw, hw[None].expand(3, -1, -1)), (chw1, chw1.expand(3, -1, -1)), (chw3, chw3), (chw4, chw4),
            (bchw, torch.cat(list(bchw), dim=2))]                              # "b c h w -> c h (b w)"


def test_prep_image_takes_the_reference_shapes():
    for image, as_chw in prep_cases():
        got = io.prep_image(image)
        assert got.dtype == torch.uint8 and got.device == image.device and np.array_equal(got.numpy(), _prep_reference(as_chw))
    with pytest.raises(ValueError):
        io.prep_image(torch.zeros(2, 4, 4))


def test_save_image_load_image_and_save_images(tmp_path):
    image = torch.from_numpy(_gradient(20, 30, 3, 14)).permute(2, 0, 1).float() / 255
    io.save_image(image, tmp_path / "a" / "b" / "x.png")
    back = io.load_image(tmp_path / "a" / "b" / "x.png")
    assert back.shape == (3, 20, 30) and torch.equal((back * 255).round().to(torch.uint8), (image * 255).type(torch.uint8))
    assert (tmp_path / "a" / "b" / "x.png").read_bytes()[:8] == io.SIGNATURE
    io.save_image(image[0], tmp_path / "grey.png")                              # (H,W): repeated to three channels
    assert np.array_equal(np.asarray(Image.open(tmp_path / "grey.png")), io.prep_image(image[0]).numpy())
    io.save_image(image, tmp_path / "style.jpg")                                # not .png: Pillow, by the suffix
    assert Image.open(tmp_path / "style.jpg").format == "JPEG"
    frames = torch.stack([image, image.flip(1), image.flip(2)])
    paths = [tmp_path / "many" / f"{i:0>6}.png" for i in range(3)]
    before = io.CALLS["png_host"]
    io.save_images(frames, paths)
    assert io.CALLS["png_host"] == before + 3
    for p, f in zip(paths, frames):
        assert np.array_equal(np.asarray(Image.open(p)), io.prep_image(f).numpy())
    with pytest.raises(ValueError):
        io.save_images(frames, paths[:2])


def scene_batch(device="cpu"):
    """a 2-view 32 x 32 scene as the drivers hold it: context images normalised to [-1, 1], everything else in [0, 1]"""
    g = torch.Generator().manual_seed(9)
    r = lambda *s: torch.rand(*s, generator=g).to(device)
    batch = {"context": {"image": r(1, 2, 3, 32, 32) * 2 - 1, "index": torch.tensor([[3, 40]], device=device)},
             "target": {"image": r(1, 2, 3, 32, 32), "index": torch.tensor([[11, 25]], device=device)},
             "style": {"image": r(1, 3, 24, 24), "image_name": "wave.png"}, "scene": ["0a1b2c"]}
    from types import SimpleNamespace
    return batch, SimpleNamespace(color=r(1, 2, 3, 32, 32) * 1.2 - 0.1), SimpleNamespace(color=r(1, 2, 3, 32, 32))


def check_scene_tree(root, written, batch, output, stylized):
    top = root / "0a1b2c | wave"
    want = {"wave.png": batch["style"]["image"][0]}
    for k, i in enumerate((3, 40)):
        want[f"context/{i:0>6}.png"] = batch["context"]["image"][0, k] * 0.5 + 0.5
    for k, i in enumerate((11, 25)):
        want[f"target/{i:0>6}.png"] = batch["target"]["image"][0, k]
        want[f"color/{i:0>6}.png"] = output.color[0, k]
        want[f"stylized_color/{i:0>6}.png"] = stylized.color[0, k]
    files = sorted(str(p.relative_to(top)) for p in top.rglob("*") if p.is_file())
    assert files == sorted(want) and sorted(str(p.relative_to(top)) for p in written) == files
    for name, tensor in want.items():
        assert np.array_equal(np.asarray(Image.open(top / name)), io.prep_image(tensor).cpu().numpy()), name


def test_save_scene_images_writes_the_reference_tree(tmp_path):
    from styl3r_amd.inference import save_scene_images
    batch, output, stylized = scene_batch()
    written = save_scene_images(tmp_path, "0a1b2c", "wave.jpg", batch, output, stylized)
    check_scene_tree(tmp_path, written, batch, output, stylized)


def test_test_cfg_defaults_write_nothing():
    from styl3r_amd.evaluation import TestCfg
    cfg = TestCfg()
    assert cfg.save_image is False and str(cfg.output_path) == "outputs/test"
    assert (cfg.align_pose, cfg.pose_align_steps, cfg.rot_opt_lr, cfg.trans_opt_lr, cfg.compute_scores) == (True, 100, 0.005, 0.005, True)
