#!/usr/bin/env python
"""A report, not a test: how far the package's undistortion (styl3r_amd/colmap.py, written after OpenCV's published procedure but never
compared with it) is from OpenCV itself, on the shapes of tools/bench_colmap.py.  Runs only where `import cv2` works.  Prints, per
camera, how many of the 4 K_new entries and 4 ROI entries differ (and by how much), and how many output bytes of the host path differ
from cv2.remap(INTER_LINEAR) + ROI crop -- once with the package's own K_new / ROI and once with OpenCV's passed in through
`new_K=` / `roi=` (which isolates the map and the sampler from the new-camera procedure).  --device also runs the HIP path.
  python tools/compare_undistort_cv2.py [--frames 2] [--device]
"""
import argparse, json, sys
from pathlib import Path
sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import numpy as np
import torch
from styl3r_amd import colmap

try:
    import cv2
except ImportError:
    sys.exit("compare_undistort_cv2: cv2 does not import here; nothing compared")

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=2); ap.add_argument("--device", action="store_true")
args = ap.parse_args()
H, W = 1080, 1920
K = np.array([[1400.0, 0, W / 2 - 0.3], [0, 1410.0, H / 2 + 0.4], [0, 0, 1]])
CAMERAS = {"OPENCV": np.float32([-0.12, 0.03, 0.002, -0.001]), "SIMPLE_RADIAL": np.float32([0.15, 0, 0, 0]), "RADIAL": np.float32([-0.2, 0.05, 0, 0])}
frames = torch.randint(0, 256, (args.frames, H, W, 3), generator=torch.Generator().manual_seed(21), dtype=torch.uint8)
report = {"cv2": cv2.__version__, "frame_hw": [H, W], "frames": args.frames}
for name, dist32 in CAMERAS.items():
    dist = dist32.astype(np.float64)
    ours_K, ours_roi = colmap.optimal_new_camera(K, dist, (W, H))
    cv_K, cv_roi = cv2.getOptimalNewCameraMatrix(K, dist32, (W, H), 0)
    cv_roi = tuple(int(v) for v in cv_roi)
    r = {"K_new_entries_differing": int((ours_K[[0, 1, 0, 1], [0, 1, 2, 2]] != cv_K[[0, 1, 0, 1], [0, 1, 2, 2]]).sum()),
         "K_new_max_abs_difference": float(np.abs(ours_K - cv_K).max()), "roi_entries_differing": int(sum(a != b for a, b in zip(ours_roi, cv_roi))),
         "roi_ours": list(ours_roi), "roi_cv2": list(cv_roi)}
    for tag, new_K, roi in (("own_new_camera", ours_K, ours_roi), ("cv2_new_camera_passed_in", cv_K, cv_roi)):
        mapx, mapy = cv2.initUndistortRectifyMap(K, dist32, None, new_K, (W, H), cv2.CV_32FC1)
        x, y, w, h = roi
        theirs = np.stack([cv2.remap(f, mapx, mapy, cv2.INTER_LINEAR)[y:y + h, x:x + w] for f in frames.numpy()])
        cam = colmap.UndistortCamera(K, dist, (W, H), new_K, roi)
        ours = colmap.undistort_frames(frames, cam, [0] * args.frames).numpy()
        diff = np.abs(ours.astype(np.int16) - theirs.astype(np.int16))
        r[tag] = {"bytes": int(diff.size), "bytes_differing": int((diff != 0).sum()), "max_abs_difference": int(diff.max())}
        if args.device:
            dev = colmap.undistort_frames(frames.cuda(), cam, [0] * args.frames).cpu().numpy()
            r[tag]["device_bytes_differing_from_host_path"] = int((dev != ours).sum())
    report[name] = r
print(json.dumps(report, indent=1))
