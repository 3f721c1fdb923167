"""The case table of the JPEG encoder's tests (tests/test_video_host.py, tests/test_gpu_jpeg_encode.py) and of the fixture generator
tests/golden/make_jpeg_encode_fixtures.py.  Inputs are rebuilt from seeds; tests/golden/jpeg_encode.npz stores only the files Pillow
(libjpeg-turbo) wrote for them.  Sizes are H x W.  What each case is for:
    noise 1x1, 8x8, 9x17          partial blocks on both axes
    noise 24x8, 40x24 (4:2:0)     H = 8 (mod 16): the last downsampled row is repeated, not the padded input averaged; a dummy row of Y blocks
    noise 37x50                   dummy Y blocks on the right and at the bottom
    stripes 16x16, quality 100    rows of 0 and 255: the largest coefficient categories
    flat 32x32                    nothing but "difference 0" and end of block
    one_coefficient 16x16         only the DC and coefficient 63 of every Y block: runs of 16 zeros (the code 0xF0)
    noise 64x48, quality 100      the densest stream, with stuffed 0xFF bytes
    gradient 33x25, q 1/20/75/95  quantisation tables and rounding
    noise 200x72                  many coding segments: joins that are not byte-aligned
    five 40x56                    five different frames in one call: per-image offsets
    rendered 256x256              a workload-shaped picture
"""
import numpy as np

SAMPLINGS = ("4:4:4", "4:2:2", "4:2:0")
FIXTURE = "tests/golden/jpeg_encode.npz"


def noise(seed, n, h, w):
    return np.random.default_rng(seed).integers(0, 256, (n, h, w, 3), dtype=np.uint8)


def gradient(seed, h, w):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    base = np.stack([x * 255.0 / max(w - 1, 1), y * 255.0 / max(h - 1, 1), (x + y) * 255.0 / max(w + h - 2, 1)], axis=-1)
    return np.clip(base + rng.integers(-12, 13, (h, w, 3)), 0, 255).astype(np.uint8)[None]


def stripes(h, w):
    out = np.zeros((1, h, w, 3), np.uint8)
    out[:, 1::2] = 255
    return out


def one_coefficient(h, w):
    """grey: 128 + 100 times the (7, 7) basis function of the 8 x 8 DCT, tiled"""
    k = np.cos((2 * np.arange(8) + 1) * 7 * np.pi / 16)
    tile = np.rint(128 + 100 * np.outer(k, k)).astype(np.uint8)
    return np.repeat(np.tile(tile, (h // 8, w // 8))[None, :, :, None], 3, axis=3)


def rendered(seed, h, w):
    """smooth coloured blobs over a dark background with a little sensor-like noise: what a rendered frame looks like to the encoder"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    img = np.full((h, w, 3), 0.08)
    for _ in range(12):
        cy, cx, s = rng.uniform(0, h), rng.uniform(0, w), rng.uniform(h / 16, h / 4)
        img += np.exp(-((y - cy) ** 2 + (x - cx) ** 2) / (2 * s * s))[:, :, None] * rng.uniform(0.1, 0.9, 3)
    img += rng.normal(0, 0.004, img.shape)
    return (np.clip(img, 0, 1) * 255).astype(np.uint8)[None]


def _table():
    rows = [("noise_1x1", noise(1, 1, 1, 1), 90, SAMPLINGS), ("noise_8x8", noise(2, 1, 8, 8), 90, SAMPLINGS),
            ("noise_9x17", noise(3, 1, 9, 17), 90, SAMPLINGS), ("noise_24x8", noise(4, 1, 24, 8), 90, ("4:2:0",)),
            ("noise_40x24", noise(5, 1, 40, 24), 90, ("4:2:0",)), ("noise_37x50", noise(6, 1, 37, 50), 90, SAMPLINGS),
            ("stripes_16x16", stripes(16, 16), 100, SAMPLINGS), ("flat_32x32", np.full((1, 32, 32, 3), 128, np.uint8), 90, SAMPLINGS),
            ("one_coefficient_16x16", one_coefficient(16, 16), 50, SAMPLINGS), ("noise_64x48", noise(7, 1, 64, 48), 100, SAMPLINGS)]
    rows += [(f"gradient_33x25_q{q}", gradient(8, 33, 25), q, SAMPLINGS) for q in (1, 20, 75, 95)]
    rows += [("noise_200x72", noise(9, 1, 200, 72), 90, SAMPLINGS), ("five_40x56", noise(10, 5, 40, 56), 90, SAMPLINGS),
             ("rendered_256x256", rendered(11, 256, 256), 90, SAMPLINGS)]
    return {f"{name}-{s.replace(':', '')}": (frames, q, s) for name, frames, q, samplings in rows for s in samplings}


CASES = _table()         # name -> (uint8 (N,H,W,3), quality, subsampling)


def load_fixture(root):
    """name -> [the file Pillow wrote for every frame of the case]"""
    z = np.load(root / FIXTURE)
    return {name: [z[f"{name}/{i}"].tobytes() for i in range(frames.shape[0])] for name, (frames, _, _) in CASES.items()}


def pillow_files(frames, quality, subsampling):
    """`Image.save(format="JPEG", quality=, subsampling=)` with nothing else set, per frame"""
    from io import BytesIO

    from PIL import Image
    out = []
    for img in frames:
        buf = BytesIO()
        Image.fromarray(img).save(buf, format="JPEG", quality=quality, subsampling=subsampling)
        out.append(buf.getvalue())
    return out


def pillow_pixels(data):
    from io import BytesIO

    from PIL import Image
    return np.array(Image.open(BytesIO(data)).convert("RGB"))
