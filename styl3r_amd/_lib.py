"""Loader / builder of the HIP C-ABI library (include/gsr.h).

The library is plain C ABI (no torch types) and is bound here with ctypes --
the same stub a maintainer of the reference would add.
There is NO fallback: if the library is missing the import of the product
path fails loudly.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess
from pathlib import Path

_PKG = Path(__file__).resolve().parent
_CSRC = _PKG / "csrc"
_LIBDIR = _PKG / "lib"
# GSR_LIB_NAME / GSR_HIPCC_EXTRA: kernel-experiment builds (tools/ only); the product is libgsr_hip.so
LIB_PATH = _LIBDIR / os.environ.get("GSR_LIB_NAME", "libgsr_hip.so")

_SOURCES = ["gsr_forward.hip", "gsr_backward.hip", "gsr_api.hip", "gsr_loss.hip", "gsr_ssim.hip", "gsr_styles.hip", "gsr_pose.hip", "gsr_points.hip", "gsr_outputs.hip", "gsr_inputs.hip", "gsr_views.hip", "gsr_draw.hip", "gsr_undistort.hip", "gsr_depth.hip", "gsr_jpeg.hip", "gsr_png.hip", "gsr_jpeg_enc.hip", "gsr_consistency.hip"]
_HEADERS = ["gsr_common.h", "gsr_select.h", "gsr_turbo_lut.h", "gsr_jpeg_entropy.h", "../../include/gsr.h"]

HIPCC_FLAGS = [
    "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared",
    "-fhip-fp32-correctly-rounded-divide-sqrt", "-fvisibility=hidden",
    # hipcc's SLP vectoriser packs independent fp32 ops of the composite loops into v_pk_*_f32 plus the
    # v_mov shuffles that feed them: measured -22 % on k_composite_bwd without it (2.11 -> 1.65 ms)
    "-fno-slp-vectorize",
]


def _hipcc() -> str:
    for cand in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    return "hipcc"


def sources_digest(paths, cmd) -> str:
    """sha256 over the command line and the bytes of every source / header: the build stamp (a stale shipped .so whose
    sources changed -- even with a newer mtime -- is rebuilt) and the key that ties a PMC profile to the build it measured."""
    import hashlib
    h = hashlib.sha256(" ".join(map(str, cmd)).encode())
    for q in sorted(map(str, paths)):
        h.update(Path(q).name.encode())
        h.update(Path(q).read_bytes())
    return h.hexdigest()[:16]


def _build_cmd():
    srcs = [_CSRC / s for s in _SOURCES]
    deps = srcs + [(_CSRC / h).resolve() for h in _HEADERS]
    # the command is recorded with repo-relative paths so that the digest is the same here and on the GPU box
    cmd = ["hipcc", *HIPCC_FLAGS, *os.environ.get("GSR_HIPCC_EXTRA", "").split(), *_SOURCES, "-o", LIB_PATH.name]
    return srcs, deps, cmd


def build_digest() -> str:
    """digest of the sources + flags the CURRENT tree would build libgsr_hip.so from"""
    _, deps, cmd = _build_cmd()
    return sources_digest(deps, cmd)


def built_digest() -> str:
    """digest recorded when the shipped libgsr_hip.so was built ('' if unknown)"""
    stamp = LIB_PATH.with_suffix(".stamp")
    return stamp.read_text().strip() if stamp.exists() and LIB_PATH.exists() else ""


def build_library(force: bool = False, verbose: bool = False) -> Path:
    """Compile csrc/*.hip for gfx950 into styl3r_amd/lib/libgsr_hip.so (cross-compiles without a GPU).  The library is
    rebuilt whenever the digest of (sources, headers, command line) differs from the one stamped next to it."""
    srcs, deps, cmd = _build_cmd()
    _LIBDIR.mkdir(exist_ok=True)
    want = sources_digest(deps, cmd)
    if not force and built_digest() == want:
        return LIB_PATH
    real = [_hipcc(), *cmd[1:-2], "-o", str(LIB_PATH)]
    if verbose:
        print(" ".join(real))
    subprocess.run(real, check=True, cwd=str(_CSRC))
    LIB_PATH.with_suffix(".stamp").write_text(want)
    return LIB_PATH


class GsrDims(C.Structure):
    _fields_ = [("B", C.c_int32), ("Vt", C.c_int32), ("G", C.c_int32), ("H", C.c_int32), ("W", C.c_int32),
                ("M", C.c_int32), ("sh_degree", C.c_int32), ("flags", C.c_int32), ("profile", C.c_void_p)]


class GsrLayout(C.Structure):
    _fields_ = [(n, C.c_size_t) for n in ("records", "tile_count", "tile_offset", "tile_cursor", "pairs", "point_list",
                                          "final_T", "n_contrib", "grad_rec", "status", "tile_order", "pairs_alt", "loss_partial", "loss_ticket", "loss_diff", "final_C", "ckpt", "unit_order", "geo", "opac", "scan",
                                          "total")]


class GsrFused(C.Structure):
    """include/gsr.h GsrFused: persistent tile counters + LossMse fused into the composite kernels"""
    _fields_ = [("tile_count", C.c_void_p), ("mse_target", C.c_void_p), ("mse_weight", C.c_float), ("mse_loss", C.c_void_p),
                ("mse_grad_loss", C.c_void_p)]


class GsrJpegInfo(C.Structure):
    """include/gsr.h gsr_jpeg_info: what gsr_jpeg_probe reads from the markers in front of the scan"""
    _fields_ = [(n, C.c_int32) for n in ("width", "height", "components", "sampling", "restart_interval")]


class GsrJpegDesc(C.Structure):
    """include/gsr.h gsr_jpeg_desc: sampling class, block grids, coefficient region and quantisation tables of one decoded image"""
    _fields_ = [("sampling", C.c_int32), ("ncomp", C.c_int32), ("bw", C.c_int32 * 3), ("bh", C.c_int32 * 3),
                ("coef_offset", C.c_int64), ("coef_count", C.c_int64), ("quant", (C.c_uint16 * 64) * 3)]


GSR_FLAG_NTOUCHED = 1
GSR_FLAG_COV9 = 2
GSR_FLAG_PHASE_BIN = 4
GSR_FLAG_PHASE_RENDER = 8
GSR_FLAG_PREZERO_GRADS = 16
GSR_FLAG_BIN_BALLOT = 32
GSR_FLAG_K6_SWAP_SUM = 64    # composite backward, no depth gradient: permlane-swap reduction instead of the LDS transpose (A/B, parity test)
GSR_RESAMPLE_DIRECT = 1      # gsr_resample_crop: horizontal pass without the LDS staging (the large-support path, forced; parity test)
GSR_ID_MASK = 0x0FFFFFFF
GSR_QUAD_SHIFT = 28
GSR_FLAG_SORT_KEYS_SHIFT = 8
GSR_FLAG_STYLES_CHUNK_SHIFT = 13   # gsr_forward_styles: most styles per composite launch, 2..4 (0 = 4)
GSR_FLAG_SEG_SHIFT = 10      # 1..5: depth segments of 64 / 128 / 192 / 256 / 384 entries, 7: one per tile, 0: by size
GSR_STATUS_WORDS = 8
GSR_ST_UNITS = 4
GSR_VIEW_FLOATS = 64
GSR_N_STAGES = 7
GSR_PT_EMPTY_MAP, GSR_PT_NAN, GSR_PT_EMPTY_VIEW = 1, 2, 4     # status bits of gsr_regr3d_fwd
GSR_DRAW_RECORD_DOUBLES, GSR_DRAW_CHUNK = 16, 32                    # gsr_draw_layers: doubles per record, records per LDS chunk
GSR_DRAW_BUTT, GSR_DRAW_ROUND, GSR_DRAW_SQUARE, GSR_DRAW_POINT = 0, 1, 2, 3
GSR_UNDISTORT_CAM_DOUBLES, GSR_UNDISTORT_FRAMES_PER_LAUNCH = 16, 1024     # gsr_undistort: doubles per camera row, frames per launch
GSR_JPEG_UNSUPPORTED, GSR_JPEG_CORRUPT = 1, 2                  # status of gsr_jpeg_probe / gsr_jpeg_entropy (GSR_OK = 0)
GSR_JPEG_GRAY, GSR_JPEG_444, GSR_JPEG_422, GSR_JPEG_420 = 0, 1, 2, 3
GSR_JPEG_MAX_COLUMN_L1, GSR_JPEG_MAX_BLOCK_L1 = 5888, 14080     # the coefficient gate
GSR_PNG_CHUNK_BYTES = 16384                                   # filtered bytes per chunk of gsr_png_chunks (include/gsr.h)
GSR_PNG_SLOT_BYTES = GSR_PNG_CHUNK_BYTES + 8                  # bytes of scratch per chunk payload
GSR_PNG_SRC_U8, GSR_PNG_SRC_F32_PLANAR = 0, 1
GSR_PNG_ROW_TOO_WIDE = 1                                      # status of gsr_png_chunks / gsr_png_assemble (GSR_OK = 0)
GSR_JPEG_ENC_SRC_U8, GSR_JPEG_ENC_SRC_F32_PLANAR = 0, 1
GSR_JPEG_ENC_TOO_LARGE = 1                                    # status of gsr_jpeg_enc_scans (GSR_OK = 0)
GSR_CONSISTENCY_MAX_SETS, GSR_CONSISTENCY_TILE_W, GSR_CONSISTENCY_TILE_H = 8, 32, 8   # gsr_warp_consistency: sets per call, pixels per workgroup
GSR_DEPTH_NO_POSITIVE = 1                                     # status[1] of gsr_depth_range
STAGE_NAMES = ("preprocess", "scan_tiles", "scatter", "tile_sort", "composite_fwd", "composite_bwd", "preprocess_bwd")
EXPORTS = ("gsr_workspace_layout", "gsr_forward", "gsr_backward", "gsr_forward_fused", "gsr_backward_fused", "gsr_version", "gsr_profile_create",
           "gsr_profile_destroy", "gsr_profile_read", "gsr_profile_set_stages", "gsr_last_error", "gsr_build_views", "gsr_mse_scratch_bytes",
           "gsr_mse_forward", "gsr_mse_backward", "gsr_image_scores_scratch_bytes", "gsr_image_scores", "gsr_pose_adam_update", "gsr_forward_styles", "gsr_styles_extra_bytes",
           "gsr_pnp_ransac_scratch_bytes", "gsr_pnp_ransac", "gsr_ssim_structure_scratch_bytes", "gsr_ssim_structure_fwd", "gsr_ssim_structure_bwd",
           "gsr_pointmap_post", "gsr_regr3d_scratch_bytes", "gsr_regr3d_fwd", "gsr_regr3d_bwd",
           "gsr_k6_blocks_per_cu", "gsr_test_reduce9",
           "gsr_trajectory", "gsr_outputs_scratch_bytes", "gsr_depth_range", "gsr_pack_frames", "gsr_ply_normalizer", "gsr_ply_rows",
           "gsr_resample_plan", "gsr_resample_scratch_bytes", "gsr_resample_crop",
           "gsr_view_overlap_scratch_bytes", "gsr_view_overlap", "gsr_draw_layers", "gsr_undistort",
           "gsr_depth_smooth_scratch_bytes", "gsr_depth_smooth_fwd", "gsr_depth_smooth_bwd",
           "gsr_jpeg_probe", "gsr_jpeg_coef_bytes", "gsr_jpeg_entropy", "gsr_jpeg_scratch_bytes", "gsr_jpeg_pixels",
           "gsr_png_scratch_bytes", "gsr_png_stream_bound", "gsr_png_chunks", "gsr_png_assemble",
           "gsr_jpeg_enc_scratch_bytes", "gsr_jpeg_enc_stream_bound", "gsr_jpeg_enc_scans",
           "gsr_warp_consistency_scratch_bytes", "gsr_warp_consistency")
ERRORS = {-1: "GSR_EINVAL (bad dimension / null pointer / unsupported degree)",
          -2: "GSR_ENOSPACE (workspace too small)", -3: "GSR_ELAUNCH (kernel launch failed)"}

_lib = None


def load() -> C.CDLL:
    """dlopen the library and declare the prototypes.  Raises if it is not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not LIB_PATH.exists():
        raise RuntimeError(
            f"{LIB_PATH} is missing: the HIP rasterizer has not been built. "
            "Run `python -c 'import __graft_entry__ as g; g.build()'` (needs hipcc). There is no CPU fallback.")
    # The library must share ONE HIP runtime with the process that owns the device pointers and
    # streams it is handed.  torch wheels bundle their own libamdhip64 (same SONAME as /opt/rocm's):
    # load torch's first so the loader resolves our NEEDED entry to it instead of a second copy
    # (two runtimes => hipErrorNoDevice inside the library).
    import torch  # noqa: F401
    lib = C.CDLL(str(LIB_PATH))
    vp, i64, sz = C.c_void_p, C.c_int64, C.c_size_t
    lib.gsr_workspace_layout.argtypes = [C.POINTER(GsrDims), i64, C.POINTER(GsrLayout)]
    lib.gsr_workspace_layout.restype = C.c_int
    lib.gsr_forward.argtypes = [C.POINTER(GsrDims), vp, vp, vp, vp, vp, i64, vp, sz, vp, vp, vp, vp, vp, vp, vp]
    lib.gsr_forward.restype = C.c_int
    lib.gsr_backward.argtypes = [C.POINTER(GsrDims), vp, vp, vp, vp, i64, vp, sz, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.gsr_backward.restype = C.c_int
    lib.gsr_forward_fused.argtypes = [C.POINTER(GsrDims), vp, vp, vp, vp, vp, i64, vp, sz, vp, vp, vp, vp, vp, vp, C.POINTER(GsrFused), vp]
    lib.gsr_forward_fused.restype = C.c_int
    lib.gsr_backward_fused.argtypes = [C.POINTER(GsrDims), vp, vp, vp, vp, i64, vp, sz, vp, vp, vp, vp, vp, vp, vp, vp, C.POINTER(GsrFused), vp]
    lib.gsr_backward_fused.restype = C.c_int
    lib.gsr_forward_styles.argtypes = [C.POINTER(GsrDims), C.c_int32, vp, vp, vp, vp, C.POINTER(vp), i64, vp, sz, vp, sz, vp, vp, vp, vp, vp, vp, vp]
    lib.gsr_forward_styles.restype = C.c_int
    lib.gsr_styles_extra_bytes.argtypes = [C.POINTER(GsrDims), C.c_int32]
    lib.gsr_styles_extra_bytes.restype = C.c_size_t
    lib.gsr_version.restype = C.c_char_p
    lib.gsr_build_views.argtypes = [vp, vp, vp, vp, vp, C.c_int32, C.c_int32, vp, vp]
    lib.gsr_build_views.restype = C.c_int
    lib.gsr_last_error.restype = C.c_char_p
    lib.gsr_mse_scratch_bytes.argtypes = []
    lib.gsr_mse_scratch_bytes.restype = C.c_size_t
    lib.gsr_mse_forward.argtypes = [vp, vp, i64, C.c_float, vp, vp, vp]
    lib.gsr_mse_forward.restype = C.c_int
    lib.gsr_mse_backward.argtypes = [vp, vp, vp, i64, C.c_float, vp, vp]
    lib.gsr_mse_backward.restype = C.c_int
    lib.gsr_image_scores_scratch_bytes.argtypes = [i64, C.c_int, C.c_int, C.c_int]
    lib.gsr_image_scores_scratch_bytes.restype = C.c_size_t
    lib.gsr_image_scores.argtypes = [vp, vp, i64, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp]
    lib.gsr_image_scores.restype = C.c_int
    lib.gsr_pose_adam_update.argtypes = [vp, vp, vp, vp, vp, i64, C.c_int, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float, vp]
    lib.gsr_pose_adam_update.restype = C.c_int
    lib.gsr_pnp_ransac_scratch_bytes.argtypes = [i64, C.c_int, C.c_int, C.c_int]
    lib.gsr_pnp_ransac_scratch_bytes.restype = C.c_size_t
    lib.gsr_pnp_ransac.argtypes = [vp, vp, vp, i64, C.c_int, C.c_int, i64, C.c_float, C.c_float, C.c_int, C.c_uint64, C.c_float, vp, vp, vp, vp, vp]
    lib.gsr_pnp_ransac.restype = C.c_int
    lib.gsr_ssim_structure_scratch_bytes.argtypes = [i64, C.c_int, C.c_int, C.c_int]
    lib.gsr_ssim_structure_scratch_bytes.restype = C.c_size_t
    lib.gsr_ssim_structure_fwd.argtypes = [vp, vp, i64, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_float), vp, vp, vp, vp]
    lib.gsr_ssim_structure_fwd.restype = C.c_int
    lib.gsr_ssim_structure_bwd.argtypes = [vp, vp, vp, vp, i64, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_float), vp, vp]
    lib.gsr_ssim_structure_bwd.restype = C.c_int
    lib.gsr_pointmap_post.argtypes = [vp, i64, C.c_int, C.c_int, vp, vp, vp]
    lib.gsr_pointmap_post.restype = C.c_int
    lib.gsr_regr3d_scratch_bytes.argtypes = [C.c_int, i64]
    lib.gsr_regr3d_scratch_bytes.restype = C.c_size_t
    lib.gsr_regr3d_fwd.argtypes = [vp, vp, vp, vp, vp, vp, i64, i64, C.c_int, i64, C.c_int, C.c_int, C.c_float, vp, vp, vp, vp, vp, vp]
    lib.gsr_regr3d_fwd.restype = C.c_int
    lib.gsr_regr3d_bwd.argtypes = [vp, vp, vp, vp, i64, i64, C.c_int, i64, C.c_int, C.c_int, vp, vp, vp, vp, vp]
    lib.gsr_regr3d_bwd.restype = C.c_int
    lib.gsr_k6_blocks_per_cu.argtypes = [C.c_int]
    lib.gsr_k6_blocks_per_cu.restype = C.c_int
    lib.gsr_test_reduce9.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, vp]
    lib.gsr_test_reduce9.restype = C.c_int
    f32 = C.c_float
    lib.gsr_trajectory.argtypes = [vp, vp, vp, vp, vp, C.c_int, C.c_int, f32, f32, f32, C.c_int, f32, C.c_int, C.c_int, vp, vp, vp, vp]
    lib.gsr_trajectory.restype = C.c_int
    lib.gsr_outputs_scratch_bytes.argtypes = []
    lib.gsr_outputs_scratch_bytes.restype = C.c_size_t
    lib.gsr_depth_range.argtypes = [vp, i64, i64, vp, vp, vp, vp]
    lib.gsr_depth_range.restype = C.c_int
    lib.gsr_pack_frames.argtypes = [C.POINTER(vp), C.POINTER(C.c_int32), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp]
    lib.gsr_pack_frames.restype = C.c_int
    lib.gsr_ply_normalizer.argtypes = [vp, i64, vp, vp, vp]
    lib.gsr_ply_normalizer.restype = C.c_int
    lib.gsr_ply_rows.argtypes = [vp, vp, vp, vp, vp, i64, C.c_int, C.c_int, vp, vp, vp]
    lib.gsr_ply_rows.restype = C.c_int
    lib.gsr_resample_plan.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_int32), vp, vp]
    lib.gsr_resample_plan.restype = C.c_int
    lib.gsr_resample_scratch_bytes.argtypes = [i64] + [C.c_int] * 8
    lib.gsr_resample_scratch_bytes.restype = C.c_size_t
    lib.gsr_resample_crop.argtypes = [vp, C.c_int, i64, C.c_int, C.c_int, vp, C.c_int, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, sz, vp,
                                      C.c_int, vp]
    lib.gsr_resample_crop.restype = C.c_int
    lib.gsr_view_overlap_scratch_bytes.argtypes = [C.c_int, i64]
    lib.gsr_view_overlap_scratch_bytes.restype = C.c_size_t
    lib.gsr_view_overlap.argtypes = [vp, vp, C.c_int, vp, i64, C.c_int, C.c_int, vp, sz, vp, vp]
    lib.gsr_view_overlap.restype = C.c_int
    lib.gsr_draw_layers.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, vp, vp, vp, C.c_int, vp, i64, vp]
    lib.gsr_draw_layers.restype = C.c_int
    lib.gsr_undistort.argtypes = [vp, i64, C.c_int, C.c_int, vp, C.c_int, vp, C.c_int, C.c_int, vp, vp]
    lib.gsr_undistort.restype = C.c_int
    lib.gsr_depth_smooth_scratch_bytes.argtypes = [i64, C.c_int, C.c_int]
    lib.gsr_depth_smooth_scratch_bytes.restype = C.c_size_t
    lib.gsr_depth_smooth_fwd.argtypes = [vp, vp, vp, vp, i64, C.c_int, C.c_int, f32, f32, C.c_int, vp, vp, vp]
    lib.gsr_depth_smooth_fwd.restype = C.c_int
    lib.gsr_depth_smooth_bwd.argtypes = [vp, vp, vp, vp, vp, i64, C.c_int, C.c_int, f32, f32, C.c_int, vp, vp]
    lib.gsr_depth_smooth_bwd.restype = C.c_int
    lib.gsr_jpeg_probe.argtypes = [vp, sz, C.POINTER(GsrJpegInfo)]
    lib.gsr_jpeg_probe.restype = C.c_int
    lib.gsr_jpeg_coef_bytes.argtypes = [i64, C.c_int, C.c_int]
    lib.gsr_jpeg_coef_bytes.restype = C.c_size_t
    lib.gsr_jpeg_entropy.argtypes = [C.POINTER(vp), C.POINTER(sz), i64, C.c_int, C.c_int, vp, vp, vp, C.c_int]
    lib.gsr_jpeg_entropy.restype = C.c_int
    lib.gsr_jpeg_scratch_bytes.argtypes = [i64, C.c_int, C.c_int]
    lib.gsr_jpeg_scratch_bytes.restype = C.c_size_t
    lib.gsr_jpeg_pixels.argtypes = [vp, vp, i64, C.c_int, C.c_int, vp, sz, vp, vp]
    lib.gsr_jpeg_pixels.restype = C.c_int
    lib.gsr_png_scratch_bytes.argtypes = [i64, C.c_int, C.c_int, C.c_int]
    lib.gsr_png_scratch_bytes.restype = C.c_size_t
    lib.gsr_png_stream_bound.argtypes = [C.c_int, C.c_int, C.c_int]
    lib.gsr_png_stream_bound.restype = C.c_size_t
    lib.gsr_png_chunks.argtypes = [vp, C.c_int, i64, C.c_int, C.c_int, C.c_int, C.c_int, vp, sz, vp]
    lib.gsr_png_chunks.restype = C.c_int
    lib.gsr_png_assemble.argtypes = [vp, sz, i64, C.c_int, C.c_int, C.c_int, vp, sz, vp, vp]
    lib.gsr_png_assemble.restype = C.c_int
    lib.gsr_jpeg_enc_scratch_bytes.argtypes = [i64, C.c_int, C.c_int, C.c_int]
    lib.gsr_jpeg_enc_scratch_bytes.restype = C.c_size_t
    lib.gsr_jpeg_enc_stream_bound.argtypes = [C.c_int, C.c_int, C.c_int]
    lib.gsr_jpeg_enc_stream_bound.restype = C.c_size_t
    lib.gsr_jpeg_enc_scans.argtypes = [vp, C.c_int, i64, C.c_int, C.c_int, C.c_int, vp, vp, sz, vp, sz, vp, vp]
    lib.gsr_jpeg_enc_scans.restype = C.c_int
    lib.gsr_warp_consistency_scratch_bytes.argtypes = [i64, C.c_int, C.c_int, C.c_int]
    lib.gsr_warp_consistency_scratch_bytes.restype = C.c_size_t
    lib.gsr_warp_consistency.argtypes = [vp, vp, vp, vp, vp, C.c_int, C.c_int, i64, C.c_int, C.c_int, C.c_double, vp, vp, vp, vp, vp, sz, vp]
    lib.gsr_warp_consistency.restype = C.c_int
    lib.gsr_profile_create.argtypes = [C.c_int]
    lib.gsr_profile_create.restype = C.c_void_p
    lib.gsr_profile_destroy.argtypes = [C.c_void_p]
    lib.gsr_profile_destroy.restype = None
    lib.gsr_profile_read.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_int32)]
    lib.gsr_profile_set_stages.argtypes = [C.c_void_p, C.c_uint32]
    lib.gsr_profile_set_stages.restype = C.c_int
    lib.gsr_profile_read.restype = C.c_int
    _lib = lib
    return lib


def check(rc: int, what: str) -> None:
    if rc != 0:
        detail = load().gsr_last_error().decode() if rc == -3 else ""
        raise RuntimeError(f"{what} failed: {ERRORS.get(rc, rc)} {detail}")


def workspace_layout(dims: GsrDims, capacity: int) -> GsrLayout:
    L = GsrLayout()
    check(load().gsr_workspace_layout(C.byref(dims), int(capacity), C.byref(L)), "gsr_workspace_layout")
    return L


class StageProfile:
    """hipEvent stage timer of the library (include/gsr.h GsrProfile); pass `.handle` via rasterizer.PROFILE."""

    def __init__(self, max_calls: int):
        self.handle = load().gsr_profile_create(int(max_calls))
        if not self.handle:
            raise RuntimeError("gsr_profile_create failed")

    def set_stages(self, names=None):
        """time only the named stages (None = all): every timed stage costs two event records between otherwise back-to-back kernels"""
        mask = (1 << GSR_N_STAGES) - 1 if names is None else sum(1 << STAGE_NAMES.index(n) for n in names)
        check(load().gsr_profile_set_stages(self.handle, mask), "gsr_profile_set_stages")

    def read(self) -> dict:
        ms = (C.c_float * GSR_N_STAGES)()
        cnt = (C.c_int32 * GSR_N_STAGES)()
        check(load().gsr_profile_read(self.handle, ms, cnt), "gsr_profile_read")
        return {STAGE_NAMES[i]: (float(ms[i]), int(cnt[i])) for i in range(GSR_N_STAGES)}

    def close(self):
        if self.handle:
            load().gsr_profile_destroy(self.handle)
            self.handle = None
