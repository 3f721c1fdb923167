"""Writes tests/golden/jpeg_encode.npz: for every case of tests/jpeg_encode_cases.py the complete files that Pillow's
`Image.save(format="JPEG", quality=q, subsampling=s)` produces, frame by frame (key `<case>/<frame>`, uint8).  Run it where Pillow is
linked against libjpeg-turbo (`PIL.features.check_feature("libjpeg_turbo")`); the inputs come from seeds and are not stored.

    python tests/golden/make_jpeg_encode_fixtures.py
"""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))

from tests.jpeg_encode_cases import CASES, FIXTURE, pillow_files  # noqa: E402


def main():
    from PIL import features
    if not features.check_feature("libjpeg_turbo"):
        raise SystemExit("this Pillow is not linked against libjpeg-turbo: the fixture would not be the yardstick")
    out = {}
    for name, (frames, quality, subsampling) in CASES.items():
        for i, data in enumerate(pillow_files(frames, quality, subsampling)):
            out[f"{name}/{i}"] = np.frombuffer(data, np.uint8)
    np.savez(ROOT / FIXTURE, **out)
    print(f"{len(CASES)} cases, {len(out)} files, {sum(v.size for v in out.values())} bytes of JPEG -> {FIXTURE}")


if __name__ == "__main__":
    main()
