"""Generate tests/golden/jpeg_frames.npz: seeded pictures, the JPEG streams Pillow encodes from them and the RGB bytes Pillow decodes
from those streams (libjpeg-turbo: JDCT_ISLOW, fancy upsampling) -- the oracle of styl3r_amd.dataset.decode_jpeg.  Streams and
recorded results only; the tests read the .npz and nothing else.

    python tests/golden/make_jpeg_fixtures.py            (needs Pillow with libjpeg-turbo)

Two pictures per size: a smooth "photo-like" synthesis (low-frequency waves plus mild grain) and uniform noise, the worst case for
the coefficient range.  Every size is encoded at 4:4:4, 4:2:2 and 4:2:0, at quality 30, 75 and 100 and as three variants (plain,
Huffman tables optimised, a restart marker after every MCU); `keep` thins the combinations of the larger sizes to stay under 1 MB.
Streams for the fallback: one progressive, one CMYK, one truncated at 60 % of its length with the exception Pillow raised for it.
"""
import json
from io import BytesIO
from pathlib import Path

import numpy as np
from PIL import Image

OUT = Path(__file__).resolve().parent / "jpeg_frames.npz"
SIZES = [(1, 1), (2, 2), (3, 5), (8, 8), (16, 16), (17, 23), (33, 50), (64, 40), (200, 120)]      # (W, H)
SUBSAMPLING = {"444": 0, "422": 1, "420": 2}
QUALITIES = [30, 75, 100]
VARIANTS = {"plain": {}, "optimize": {"optimize": True}, "restart": {"restart_marker_blocks": 1}}


def photo(rng, W, H):
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    img = np.zeros((H, W, 3))
    for c in range(3):
        for _ in range(4):
            fx, fy = rng.uniform(0.01, 0.25, 2)
            img[..., c] += rng.uniform(20, 60) * np.sin(fx * x + fy * y + rng.uniform(0, 6.28))
        img[..., c] += 128 + rng.normal(0, 4, (H, W))
    return np.clip(img, 0, 255).astype(np.uint8)


def noise(rng, W, H):
    return rng.integers(0, 256, (H, W, 3), dtype=np.uint8)


def encode(img, **kw):
    buf = BytesIO()
    img.save(buf, "JPEG", **kw)
    return buf.getvalue()


def decode(data):
    return np.asarray(Image.open(BytesIO(data)).convert("RGB"))


def keep(W, H, sub, qi, vi, is_noise):
    """the budget: every combination up to 16 x 16; from 17 x 23 on one variant per (subsampling, quality, picture), in rotation; from
    33 x 50 on noise at one quality per subsampling; the largest size one quality per subsampling for the photo-like picture too, and
    noise at 4:2:0, quality 100 alone"""
    if W * H <= 256:
        return True
    if vi != (qi + sub + is_noise) % 3:
        return False
    if W * H < 1000:
        return True
    if (W, H) != (200, 120):
        return not is_noise or qi == (sub + 2) % 3
    return (sub, qi) == (2, 2) if is_noise else qi == (sub + 1) % 3


def main():
    rng = np.random.default_rng(20240)
    out, cases = {}, []
    for W, H in SIZES:
        pictures = {"photo": photo(rng, W, H), "noise": noise(rng, W, H)}
        for sub, sub_id in SUBSAMPLING.items():
            for quality in QUALITIES:
                for vi, (variant, kw) in enumerate(VARIANTS.items()):
                    for kind, px in pictures.items():
                        if not keep(W, H, sub_id, QUALITIES.index(quality), vi, kind == "noise"):
                            continue
                        name = f"{W}x{H}_{sub}_q{quality}_{variant}_{kind}"
                        data = encode(Image.fromarray(px), quality=quality, subsampling=sub_id, **kw)
                        out["jpg_" + name] = np.frombuffer(data, np.uint8)
                        out["rgb_" + name] = decode(data)
                        cases.append({"name": name, "W": W, "H": H, "sampling": sub, "quality": quality, "variant": variant, "kind": kind})
    gray = Image.fromarray(photo(rng, 64, 40)).convert("L")
    for variant, kw in (("plain", {}), ("restart", {"restart_marker_blocks": 1})):
        name = f"64x40_gray_q75_{variant}_photo"
        data = encode(gray, quality=75, **kw)
        out["jpg_" + name], out["rgb_" + name] = np.frombuffer(data, np.uint8), decode(data)
        cases.append({"name": name, "W": 64, "H": 40, "sampling": "gray", "quality": 75, "variant": variant, "kind": "photo"})
    out["cases"] = np.array(json.dumps(cases))

    base = photo(rng, 33, 50)
    fallback = {}
    data = encode(Image.fromarray(base), quality=75, progressive=True)
    out["jpg_fb_progressive"], out["rgb_fb_progressive"] = np.frombuffer(data, np.uint8), decode(data)
    fallback["fb_progressive"] = {"W": 33, "H": 50}
    data = encode(Image.fromarray(base).convert("CMYK"), quality=75)
    out["jpg_fb_cmyk"], out["rgb_fb_cmyk"] = np.frombuffer(data, np.uint8), decode(data)
    fallback["fb_cmyk"] = {"W": 33, "H": 50}
    data = encode(Image.fromarray(photo(rng, 64, 40)), quality=75)
    data = data[:int(len(data) * 0.6)]
    try:
        decode(data)
        raise SystemExit("Pillow read the truncated stream")
    except OSError as err:
        fallback["fb_truncated"] = {"W": 64, "H": 40, "error": type(err).__name__, "message": str(err)}
    out["jpg_fb_truncated"] = np.frombuffer(data, np.uint8)
    out["fallback"] = np.array(json.dumps(fallback))

    np.savez_compressed(OUT, **out)
    print("wrote", OUT, OUT.stat().st_size, "bytes,", len(cases), "fast-path cases;", fallback["fb_truncated"])
    assert OUT.stat().st_size < 1_000_000, OUT.stat().st_size


if __name__ == "__main__":
    main()
