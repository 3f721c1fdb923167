"""Host side of libvit_hip.so (include/vit_ops.h): ctypes bindings + autograd functions for the encoder's kernels.

Mirrors the reference operator interfaces:
  * `cuRoPE2D` / `cuRoPE2D_func`   src/model/encoder/backbone/croco/curope/curope2d.py:12-39
    (in-place on the (B,H,N,D) view, backward = same kernel with -F0)                          -> vit_rope2d
  * `memory_efficient_attention(q, k, v, scale=, p=0)` on (B,N,H,64) fp32 tensors, blocks.py:129,195
                                                                                              -> vit_attention_fwd / _bwd
    (bf16x6 split arithmetic on the bf16 MFMA by default, VIT_ATTENTION=f32: exact-f32 MFMA, =bf16x3: three products; fused RoPE in all;
     `attention_qkv`: the packed (B,N,3,H,64) projection of a self-attention, whose backward writes ONE gradient tensor)
  * `nn.Linear` (+ exact GELU, + residual add) of Mlp / Attention / Block, blocks.py:76-82,100,131,149-152
    -> `fused_linear`: vit_linear_x6_fwd (fp32-accurate bf16x6, default) or vit_linear_fwd (exact-f32 MFMA), dX on the
       pre-split transposed weight, dW + db on vit_linear_x6_wgrad (accumulating into all-reduce bucket slices);
       VIT_LINEAR_MODE=bf16x3: three instead of six partial products per launch (~4e-6 per GEMM; third pieces neither computed nor staged);
       `_linear_cfg` is the ONE route (which kernel and weight image a shape takes: forward, dX, serving; LDS-DMA rings `_RING_SHAPES`, small-M /
       narrow-N kernel) and `_launch_linear` the ONE x6 launch (image, |max| words, entry point); `GeluLink`: GELU' in fc2's dX epilogue
  * `nn.LayerNorm(eps=1e-6)`, blocks.py:144-152,205-222                                        -> `LayerNorm` (vit_layernorm_*)
  * `nn.Conv2d` 3x3 / 1x1 stride 1 of the DPT heads and VGG, dpt_block.py:79-218,350-419      -> `Conv2dX6` (vit_conv_x6_*; small 3x3 dW:
    vit_im2col3_rows + vit_linear_x6_wgrad)
  * head tails ReLU [-> Dropout] -> Conv2d(C, 3 | 8, 1), dpt_block.py:319-320,337-339         -> `head_tail` (vit_head_tail_*)
  * `feat_up(path_1) + ReLU(Conv2d(3, 256, 7, 1, 3)(imgs))`, dpt_gs_head.py:113-118,146-148   -> `input_merger_upsample_add`
  * `F.interpolate(scale_factor=2, bilinear, align_corners=True)`                             -> `upsample2x`
  * reg_dense_depth + opacity map + UnifiedGaussianAdapter + build_covariance                 -> `gaussian_adapter_hip`
`CALLS` counts how often each hand-written kernel was taken (the parity tests assert on it).
No CPU / eager fallback for the kernels above on device tensors: a missing library raises; CPU tensors take the framework ops.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess
import threading
from pathlib import Path
from typing import Optional

import torch
from torch import Tensor, nn

from .weak_cache import WeakTensorCache

_PKG = Path(__file__).resolve().parent
_CSRC = _PKG / "csrc"
LIB_PATH = _PKG / "lib" / os.environ.get("VIT_LIB_NAME", "libvit_hip.so")     # VIT_LIB_NAME: kernel-experiment builds (tools/ only); the product is libvit_hip.so
_SOURCES = ["vit_rope.hip", "vit_attention.hip", "vit_attention_tail.hip", "vit_attention_bwd.hip", "vit_gemm.hip", "vit_attention_x6.hip", "vit_attention_bwd_x6.hip", "vit_gemm_x6.hip", "vit_gemm_sm.hip", "vit_gemm_x6r.hip", "vit_weight_image.hip", "vit_resample.hip", "vit_head_tail.hip", "vit_layernorm.hip", "vit_adapter.hip", "vit_optim.hip", "vit_snapshot.hip", "vit_lpips.hip", "vit_adaattn.hip", "vit_adain.hip", "vit_api.hip"]
EXPORTS = ("vit_rope2d", "vit_attention_fwd", "vit_attention_set_arith", "vit_attention_arith", "vit_attention_bwd", "vit_linear_fwd", "vit_split_weight_bytes",
           "vit_split_weight", "vit_x6_set_products", "vit_x6_products", "vit_x6_set_operand_amax", "vit_x6_set_output_amax", "vit_amax", "vit_split_weight_block_bytes", "vit_split_weight_block", "vit_split_weight_pair", "vit_split_conv_weight_pair", "vit_split_weights_many", "vit_linear_x6_fwd", "vit_linear_sm_set", "vit_linear_sm_ok", "vit_linear_sm_grouped", "vit_layernorm_fwd_grouped", "vit_linear_x6r_fwd", "vit_linear_x6c_fwd", "vit_linear_x6c_workspace_bytes", "vit_linear_x6c_choose_splits", "vit_linear_x6_wgrad", "vit_linear_x6_wgrad_acc", "vit_conv_x6_fwd", "vit_conv_x6_wgrad", "vit_upsample2x_fwd", "vit_upsample2x_bwd", "vit_relu_dropout_fwd", "vit_relu_dropout_bwd", "vit_layernorm_scratch_bytes", "vit_layernorm_fwd", "vit_layernorm_bwd",
           "vit_adapter_fwd", "vit_adapter_bwd", "vit_head_tail_fwd", "vit_head_tail_bwd", "vit_im2col7", "vit_im2col3_rows", "vit_upsample2x_add_relu_fwd", "vit_adamw_step", "vit_snapshot_chunk_bytes", "vit_snapshot_pack",
           "vit_lpips_scratch_bytes", "vit_lpips_stats_bytes", "vit_lpips_fwd", "vit_lpips_bwd", "vit_maxpool2x2_fwd", "vit_maxpool2x2_bwd",
           "vit_adaattn_stats", "vit_adaattn_l1_scratch_bytes", "vit_adaattn_l1",
           "vit_adain_scratch_bytes", "vit_adain_fwd", "vit_conv3_rgb_fwd", "vit_version", "vit_last_error")
ERRORS = {-1: "VIT_EINVAL", -3: "VIT_ELAUNCH"}
_lib = None


def _headers() -> list[Path]:
    """every header the kernel sources may include: csrc/*.h and include/vit_ops.h"""
    return sorted(_CSRC.glob("*.h")) + [_PKG.parent / "include" / "vit_ops.h"]


def build_deps() -> list[Path]:
    """the files the library stamp covers: the sources and every header they compile against (editing one rebuilds the library)"""
    return [_CSRC / s for s in _SOURCES] + _headers()


def build_library(force: bool = False, verbose: bool = False) -> Path:
    """hipcc --offload-arch=gfx950 of csrc/vit_*.hip into lib/libvit_hip.so; rebuilt whenever the digest of
    (sources, headers, command line) differs from the stamp written next to the library (same scheme as _lib.py)."""
    from ._lib import sources_digest
    names = list(_SOURCES)               # (a missing kernel file fails the build: nothing is left out quietly)
    deps = build_deps()
    extra = os.environ.get("VIT_HIPCC_EXTRA", "").split()          # kernel-experiment builds (tools/ only, with VIT_LIB_NAME)
    cmd = ["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", "-fvisibility=hidden", *extra, *names, "-o", LIB_PATH.name]
    want = sources_digest(deps, cmd)
    stamp = LIB_PATH.with_suffix(".stamp")
    if not force and LIB_PATH.exists() and stamp.exists() and stamp.read_text().strip() == want:
        return LIB_PATH
    LIB_PATH.parent.mkdir(exist_ok=True)
    hipcc = "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else "hipcc"
    # one object per source, compiled in parallel and kept (keyed by the digest of the source, the headers and the flags) under build/obj/:
    # editing one kernel file recompiles that file only; the link step is a second
    import hashlib
    from concurrent.futures import ThreadPoolExecutor
    objdir = _PKG.parent / "build" / "obj"
    objdir.mkdir(parents=True, exist_ok=True)
    flags = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fvisibility=hidden", *extra]
    headers = _headers()
    hdig = hashlib.sha256(b"".join(h.read_bytes() for h in headers) + " ".join(flags).encode()).hexdigest()

    def compile_one(name):
        dig = hashlib.sha256((_CSRC / name).read_bytes() + hdig.encode()).hexdigest()[:16]
        obj = objdir / f"{Path(name).stem}.{dig}.o"
        if not obj.exists() or force:
            if not extra:       # (experiment objects live beside the product's)
                for stale in objdir.glob(f"{Path(name).stem}.*.o"):
                    stale.unlink()
            c = [hipcc, *flags, "-c", name, "-o", str(obj)]
            if verbose:
                print(" ".join(c), flush=True)
            subprocess.run(c, check=True, cwd=str(_CSRC))
        return str(obj)
    with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as pool:
        objs = list(pool.map(compile_one, names))
    real = [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", *objs, "-o", str(LIB_PATH)]
    if verbose:
        print(" ".join(real))
    subprocess.run(real, check=True, cwd=str(_CSRC))
    stamp.write_text(want)
    return LIB_PATH


class VitAdapterArgs(C.Structure):
    _fields_ = [("b", C.c_int32), ("v", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("d_sh", C.c_int32),
                ("par_channels", C.c_int32), ("opacity_exponent", C.c_float),
                ("pts0", C.c_void_p), ("ptsr", C.c_void_p), ("par0", C.c_void_p), ("parr", C.c_void_p), ("app", C.c_void_p),
                ("sh_mask", C.c_void_p)]


class VitLpipsTap(C.Structure):
    _fields_ = [("fa", C.c_void_p), ("fb", C.c_void_p), ("w", C.c_void_p), ("dfa", C.c_void_p), ("C", C.c_int32), ("H", C.c_int32), ("W", C.c_int32)]


class VitAttnArgs(C.Structure):
    _fields_ = [("B", C.c_int32), ("H", C.c_int32), ("Nq", C.c_int32), ("Nk", C.c_int32), ("scale", C.c_float),
                ("q_sb", C.c_int64), ("q_sn", C.c_int64), ("q_sh", C.c_int64),
                ("k_sb", C.c_int64), ("k_sn", C.c_int64), ("k_sh", C.c_int64),
                ("v_sb", C.c_int64), ("v_sn", C.c_int64), ("v_sh", C.c_int64),
                ("o_sb", C.c_int64), ("o_sn", C.c_int64), ("o_sh", C.c_int64),
                ("qpos", C.c_void_p), ("kpos", C.c_void_p), ("cos_tab", C.c_void_p), ("sin_tab", C.c_void_p),
                ("P", C.c_int32), ("dq_sn", C.c_int64), ("dkv_sn", C.c_int64),
                ("amax_out", C.c_void_p), ("amax_dq", C.c_void_p), ("amax_dk", C.c_void_p), ("amax_dv", C.c_void_p),
                ("amax_q", C.c_void_p), ("amax_k", C.c_void_p), ("amax_v", C.c_void_p), ("amax_g", C.c_void_p)]


def load() -> C.CDLL:
    global _lib
    if _lib is not None:
        return _lib
    if not LIB_PATH.exists():
        raise RuntimeError(f"{LIB_PATH} is missing: build it with __graft_entry__.build(); there is no CPU fallback")
    import torch  # noqa: F401  one shared HIP runtime (see _lib.py)
    lib = C.CDLL(str(LIB_PATH))
    vp, i64 = C.c_void_p, C.c_int64
    lib.vit_rope2d.argtypes = [vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, i64, i64, i64, C.c_float, vp]
    lib.vit_rope2d.restype = C.c_int
    lib.vit_attention_fwd.argtypes = [C.POINTER(VitAttnArgs), vp, vp, vp, vp, vp, vp]
    lib.vit_attention_fwd.restype = C.c_int
    lib.vit_attention_bwd.argtypes = [C.POINTER(VitAttnArgs), vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.vit_attention_bwd.restype = C.c_int
    lib.vit_linear_fwd.argtypes = [vp, vp, vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp]
    lib.vit_linear_fwd.restype = C.c_int
    lib.vit_split_weight_bytes.argtypes = [C.c_int, C.c_int]
    lib.vit_split_weight_bytes.restype = C.c_size_t
    lib.vit_split_weight.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, vp]
    lib.vit_split_weight.restype = C.c_int
    lib.vit_attention_set_arith.argtypes = [C.c_int]
    lib.vit_attention_set_arith.restype = C.c_int
    lib.vit_attention_arith.argtypes = []
    lib.vit_attention_arith.restype = C.c_int
    lib.vit_x6_set_products.argtypes = [C.c_int]
    lib.vit_x6_set_products.restype = C.c_int
    lib.vit_x6_products.argtypes = []
    lib.vit_x6_products.restype = C.c_int
    lib.vit_x6_set_operand_amax.argtypes = [vp, vp]
    lib.vit_x6_set_operand_amax.restype = C.c_int
    lib.vit_amax.argtypes = [vp, i64, vp, vp]
    lib.vit_amax.restype = C.c_int
    lib.vit_x6_set_output_amax.argtypes = [vp]
    lib.vit_x6_set_output_amax.restype = C.c_int
    lib.vit_split_weight_block_bytes.argtypes = [C.c_int, C.c_int, C.c_int]
    lib.vit_split_weight_block_bytes.restype = C.c_size_t
    lib.vit_split_weight_block.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, vp]
    lib.vit_split_weight_block.restype = C.c_int
    lib.vit_split_weight_pair.argtypes = [vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp]
    lib.vit_split_weight_pair.restype = C.c_int
    lib.vit_split_conv_weight_pair.argtypes = [vp, vp, vp, C.c_int, C.c_int, C.c_int, vp]
    lib.vit_split_conv_weight_pair.restype = C.c_int
    lib.vit_split_weights_many.argtypes = [vp, C.c_int, C.c_uint32, vp]
    lib.vit_split_weights_many.restype = C.c_int
    lib.vit_linear_x6c_fwd.argtypes = [vp, vp, vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, C.c_size_t, vp]
    lib.vit_linear_x6c_fwd.restype = C.c_int
    lib.vit_linear_x6c_workspace_bytes.argtypes = [C.c_int, C.c_int, C.c_int]
    lib.vit_linear_x6c_workspace_bytes.restype = C.c_size_t
    lib.vit_linear_x6c_choose_splits.argtypes = [C.c_int, C.c_int, C.c_int]
    lib.vit_linear_x6c_choose_splits.restype = C.c_int
    lib.vit_linear_x6r_fwd.argtypes = [vp, vp, vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp]
    lib.vit_linear_x6r_fwd.restype = C.c_int
    lib.vit_linear_x6_fwd.argtypes = [vp, vp, vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp]
    lib.vit_linear_x6_fwd.restype = C.c_int
    lib.vit_linear_sm_set.argtypes = [C.c_int, C.c_int, C.c_int]
    lib.vit_linear_sm_set.restype = C.c_int
    lib.vit_linear_sm_ok.argtypes = [C.c_int, C.c_int, C.c_int]
    lib.vit_linear_sm_ok.restype = C.c_int
    pp = C.POINTER(C.c_void_p)
    lib.vit_linear_sm_grouped.argtypes = [pp, pp, pp, pp, pp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp]
    lib.vit_linear_sm_grouped.restype = C.c_int
    lib.vit_layernorm_fwd_grouped.argtypes = [pp, pp, pp, pp, C.c_int, C.c_int, C.c_int, C.c_float, vp]
    lib.vit_layernorm_fwd_grouped.restype = C.c_int
    lib.vit_linear_x6_wgrad.argtypes = [vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, vp]
    lib.vit_linear_x6_wgrad.restype = C.c_int
    lib.vit_linear_x6_wgrad_acc.argtypes = [vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, vp]
    lib.vit_linear_x6_wgrad_acc.restype = C.c_int
    lib.vit_conv_x6_fwd.argtypes = [vp, vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp]
    lib.vit_conv_x6_fwd.restype = C.c_int
    lib.vit_conv_x6_wgrad.argtypes = [vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp]
    lib.vit_conv_x6_wgrad.restype = C.c_int
    lib.vit_relu_dropout_fwd.argtypes = [vp, vp, C.c_int64, C.c_float, C.c_uint64, vp]
    lib.vit_relu_dropout_fwd.restype = C.c_int
    lib.vit_relu_dropout_bwd.argtypes = [vp, vp, vp, C.c_int64, C.c_float, vp]
    lib.vit_relu_dropout_bwd.restype = C.c_int
    lib.vit_upsample2x_fwd.argtypes = [vp, vp, C.c_int64, C.c_int, C.c_int, vp]
    lib.vit_upsample2x_fwd.restype = C.c_int
    lib.vit_upsample2x_bwd.argtypes = [vp, vp, C.c_int64, C.c_int, C.c_int, vp]
    lib.vit_upsample2x_bwd.restype = C.c_int
    lib.vit_layernorm_scratch_bytes.argtypes = [C.c_int, C.c_int]
    lib.vit_layernorm_scratch_bytes.restype = C.c_size_t
    lib.vit_layernorm_fwd.argtypes = [vp, vp, vp, vp, vp, vp, C.c_int, C.c_int, C.c_float, vp]
    lib.vit_layernorm_fwd.restype = C.c_int
    lib.vit_layernorm_bwd.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, vp]
    lib.vit_layernorm_bwd.restype = C.c_int
    lib.vit_adapter_fwd.argtypes = [C.POINTER(VitAdapterArgs), vp, vp, vp, vp, vp, vp, vp]
    lib.vit_adapter_fwd.restype = C.c_int
    lib.vit_adapter_bwd.argtypes = [C.POINTER(VitAdapterArgs), vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.vit_adapter_bwd.restype = C.c_int
    lib.vit_head_tail_fwd.argtypes = [vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_float, C.c_uint64, vp]
    lib.vit_head_tail_fwd.restype = C.c_int
    lib.vit_head_tail_bwd.argtypes = [vp, vp, vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_float, C.c_uint64, vp]
    lib.vit_head_tail_bwd.restype = C.c_int
    lib.vit_im2col7.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, vp]
    lib.vit_im2col7.restype = C.c_int
    lib.vit_im2col3_rows.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp]
    lib.vit_im2col3_rows.restype = C.c_int
    lib.vit_upsample2x_add_relu_fwd.argtypes = [vp, vp, vp, C.c_int64, C.c_int, C.c_int, vp]
    lib.vit_upsample2x_add_relu_fwd.restype = C.c_int
    tp = C.POINTER(VitLpipsTap)
    lib.vit_lpips_scratch_bytes.argtypes = [tp, C.c_int, C.c_int]
    lib.vit_lpips_scratch_bytes.restype = C.c_size_t
    lib.vit_lpips_stats_bytes.argtypes = [tp, C.c_int, C.c_int]
    lib.vit_lpips_stats_bytes.restype = C.c_size_t
    lib.vit_lpips_fwd.argtypes = [tp, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp]
    lib.vit_lpips_fwd.restype = C.c_int
    lib.vit_lpips_bwd.argtypes = [tp, C.c_int, C.c_int, C.c_int, vp, vp, vp]
    lib.vit_lpips_bwd.restype = C.c_int
    lib.vit_maxpool2x2_fwd.argtypes = [vp, vp, C.c_int64, C.c_int, C.c_int, vp]
    lib.vit_maxpool2x2_fwd.restype = C.c_int
    lib.vit_maxpool2x2_bwd.argtypes = [vp, vp, vp, C.c_int64, C.c_int, C.c_int, vp]
    lib.vit_maxpool2x2_bwd.restype = C.c_int
    lib.vit_adaattn_stats.argtypes = [vp, vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp]
    lib.vit_adaattn_stats.restype = C.c_int
    lib.vit_adaattn_l1_scratch_bytes.argtypes = [C.c_int, C.c_int]
    lib.vit_adaattn_l1_scratch_bytes.restype = C.c_size_t
    lib.vit_adaattn_l1.argtypes = [vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, vp]
    lib.vit_adaattn_l1.restype = C.c_int
    lib.vit_adain_scratch_bytes.argtypes = [C.c_int, C.c_int, C.c_int]
    lib.vit_adain_scratch_bytes.restype = C.c_size_t
    lib.vit_adain_fwd.argtypes = [vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, i64, i64, C.c_float, C.c_float, vp, vp, vp]
    lib.vit_adain_fwd.restype = C.c_int
    lib.vit_conv3_rgb_fwd.argtypes = [vp, vp, vp, vp, vp, C.c_float, C.c_float, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp]
    lib.vit_conv3_rgb_fwd.restype = C.c_int
    lib.vit_snapshot_chunk_bytes.argtypes = []
    lib.vit_snapshot_chunk_bytes.restype = C.c_size_t
    lib.vit_snapshot_pack.argtypes = [vp, C.c_int, vp, vp, vp]
    lib.vit_snapshot_pack.restype = C.c_int
    lib.vit_version.restype = C.c_char_p
    lib.vit_last_error.restype = C.c_char_p
    _lib = lib
    return lib


def _check(rc: int, what: str):
    if rc != 0:
        raise RuntimeError(f"{what} failed: {ERRORS.get(rc, rc)} {load().vit_last_error().decode()}")


def _device_stream(dev) -> tuple:
    """(device index, raw handle of its current stream).  The raw-stream query is ~10x cheaper than torch.cuda.current_stream(dev).cuda_stream:
    at batch-1 inference the host issues ~900 launches per forward and is the limit (tools/probes/infer_host_time.py)"""
    idx = dev.index if dev.index is not None else torch.cuda.current_device()
    return idx, torch._C._cuda_getCurrentRawStream(idx)


def _stream(dev):
    return C.c_void_p(_device_stream(dev)[1])


def _need_gpu(t: Tensor, what: str):
    if not t.is_cuda:
        raise RuntimeError(f"{what}: styl3r_amd ViT kernels need tensors on an MI355X (HIP) device; there is no CPU path")


# ---------------------------------------------------------------------------
# RoPE
# ---------------------------------------------------------------------------
_ROPE_TABLES: dict = {}


def rope_tables(D: int, P: int, base: float, device) -> tuple:
    """(cos, sin) of shape (P, D/4), built with the reference fallback's own ops (pos_embed.py:121-128)
    so that the kernel reproduces it bit for bit on the same device."""
    key = (D, P, float(base), str(device))
    if key not in _ROPE_TABLES:
        Dh = D // 2
        inv_freq = 1.0 / (base ** (torch.arange(0, Dh, 2).float().to(device) / Dh))
        t = torch.arange(P, device=device, dtype=inv_freq.dtype)
        freqs = torch.einsum("i,j->ij", t, inv_freq)
        _ROPE_TABLES[key] = (freqs.cos().contiguous(), freqs.sin().contiguous())
    return _ROPE_TABLES[key]


def _rope_inplace(tokens_bnhd: Tensor, positions: Tensor, base: float, F0: float, max_pos: int):
    """tokens_bnhd: (B,N,H,D) view with contiguous last dim (may be a view into a qkv buffer)."""
    _need_gpu(tokens_bnhd, "rope_2d")
    B, N, H, D = tokens_bnhd.shape
    assert tokens_bnhd.dtype == torch.float32 and tokens_bnhd.stride(3) == 1 and D % 4 == 0
    assert positions.dtype == torch.int64 and positions.shape == (B, N, 2) and positions.is_contiguous()
    cos, sin = rope_tables(D, max_pos + 1, base, tokens_bnhd.device)
    sign = 1.0 if F0 >= 0 else -1.0
    assert abs(F0) == 1.0, "only F0 = +-1 (the reference uses F0 = 1)"
    rc = load().vit_rope2d(tokens_bnhd.data_ptr(), positions.data_ptr(), cos.data_ptr(), sin.data_ptr(), B, N, H, D,
                           max_pos + 1, tokens_bnhd.stride(0), tokens_bnhd.stride(1), tokens_bnhd.stride(2), sign,
                           _stream(tokens_bnhd.device))
    _check(rc, "vit_rope2d")


class _RoPE2DFunc(torch.autograd.Function):
    """cuRoPE2D_func (curope2d.py:12-29): in place forward, backward = inverse rotation of the incoming grad."""

    @staticmethod
    def forward(ctx, tokens, positions, base, F0, max_pos):
        ctx.save_for_backward(positions)
        ctx.cfg = (base, F0, max_pos)
        _rope_inplace(tokens, positions, base, F0, max_pos)
        ctx.mark_dirty(tokens)
        return tokens

    @staticmethod
    def backward(ctx, grad):
        (positions,) = ctx.saved_tensors
        base, F0, max_pos = ctx.cfg
        grad = grad.contiguous() if grad.stride(3) != 1 else grad
        _rope_inplace(grad, positions, base, -F0, max_pos)
        return grad, None, None, None, None


class RoPE2D(nn.Module):
    """Drop-in for `cuRoPE2D(freq, F0)`; `max_pos` bounds the positions (16 at 256x256 incl. the
    intrinsics token at (16,0)), which replaces the fallback's `int(positions.max())` host sync."""

    def __init__(self, freq: float = 100.0, F0: float = 1.0, max_pos: int = 64):
        super().__init__()
        self.base, self.F0, self.max_pos = freq, F0, max_pos

    def forward(self, tokens: Tensor, positions: Tensor) -> Tensor:
        _RoPE2DFunc.apply(tokens.transpose(1, 2), positions, self.base, self.F0, self.max_pos)
        return tokens


# ---------------------------------------------------------------------------
# attention
# ---------------------------------------------------------------------------
def _attn_args(q, k, v, out, scale, rope):
    B, Nq, H, D = q.shape
    Nk = k.shape[1]
    assert D == 64 and k.shape == (B, Nk, H, D) and v.shape == (B, Nk, H, D)
    for t in (q, k, v, out):
        assert t.dtype == torch.float32 and t.stride(3) == 1
    a = VitAttnArgs()
    a.B, a.H, a.Nq, a.Nk, a.scale = B, H, Nq, Nk, float(scale)
    a.q_sb, a.q_sn, a.q_sh = q.stride(0), q.stride(1), q.stride(2)
    a.k_sb, a.k_sn, a.k_sh = k.stride(0), k.stride(1), k.stride(2)
    a.v_sb, a.v_sn, a.v_sh = v.stride(0), v.stride(1), v.stride(2)
    a.o_sb, a.o_sn, a.o_sh = out.stride(0), out.stride(1), out.stride(2)
    keep = None
    if rope is not None:
        qpos, kpos, base, max_pos = rope
        cos, sin = rope_tables(D, max_pos + 1, base, q.device)
        assert qpos.shape == (B, Nq, 2) and kpos.shape == (B, Nk, 2) and qpos.dtype == torch.int64
        qpos, kpos = qpos.contiguous(), kpos.contiguous()
        a.qpos, a.kpos, a.cos_tab, a.sin_tab, a.P = qpos.data_ptr(), kpos.data_ptr(), cos.data_ptr(), sin.data_ptr(), max_pos + 1
        keep = (qpos, kpos, cos, sin)
    return a, keep


ATTENTION_ARITH = os.environ.get("VIT_ATTENTION", "bf16x6")   # attention contractions, forward and backward: "bf16x6" (split arithmetic on the bf16 MFMA, default) | "bf16x3" (three of the six partial products) | "f32" (exact-f32 MFMA)
_ATTN_MODES = {"f32": 0, "bf16x6": 1, "bf16x3": 2, "f16x3": 3}     # "f16x3" (round 6): two fp16 pieces per operand, three products (rounds 4-5 ran the six-product bf16 form under this name)
ATTENTION_F16 = os.environ.get("VIT_ATTENTION_F16", "1") == "1"     # A/B switch: 0 = "f16x3" runs the six-product bf16 kernels as in rounds 4-5


def _sync_attention_arith(mode: Optional[str] = None) -> None:
    """state the attention arithmetic for the calling thread (thread_local in the library): the module global by default, the mode a
    node's forward ran in when its backward calls this from the autograd engine thread"""
    mode = ATTENTION_ARITH if mode is None else mode
    if mode not in _ATTN_MODES:
        raise ValueError(f"VIT_ATTENTION = {mode!r}: expected f32, bf16x6, bf16x3 or f16x3")
    want = _ATTN_MODES[mode]
    if want == 3 and not ATTENTION_F16:
        want = 1
    lib = load()
    if lib.vit_attention_arith() != want:
        _check(lib.vit_attention_set_arith(want), "vit_attention_set_arith")


def _attn_operand_words(a: "VitAttnArgs", mode: str, q, k, v, g=None, packed=None):
    """attention in "f16x3": the |max| words of the operand tensors (VitAttnArgs.amax_q / _k / _v / _g) -- published by the Linear layers that
    produced them (fused_linear(amax_out=True) / (amax_dx=True)), else one vit_amax pass each.  `packed`: the (B,N,3,H,64) projection q, k, v are
    planes of (one word serves all three).  Returns the words (kept alive by the caller until the launch is enqueued)."""
    if not (mode == "f16x3" and ATTENTION_F16):
        return None
    def word(t):
        return _amax_of(t if t.is_contiguous() else t.contiguous())
    if packed is not None:
        wq = wk = wv = word(packed)
    else:
        wq, wk, wv = word(q), word(k), word(v)
    a.amax_q, a.amax_k, a.amax_v = wq.data_ptr(), wk.data_ptr(), wv.data_ptr()
    wg = None
    if g is not None:
        wg = word(g)
        a.amax_g = wg.data_ptr()
    return (wq, wk, wv, wg)


def _attn_word(a: "VitAttnArgs", field: str, dev) -> Optional[Tensor]:
    """f16x3: hand the attention launch a zeroed |max| word for one of its outputs (VitAttnArgs.amax_*): the Linear layer that consumes the
    output (proj after the forward; qkv / projq / projk / projv after the backward) then needs no vit_amax pass for its operand scale"""
    if not (LINEAR_MODE == "f16x3" and PUBLISH_AMAX):
        return None
    w = _AMAX.word(dev)
    setattr(a, field, w.data_ptr())
    return w


class _Attention(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, v, scale, qpos, kpos, base, max_pos):
        _need_gpu(q, "attention")
        _sync_attention_arith()
        B, Nq, H, D = q.shape
        out = torch.empty((B, Nq, H, D), dtype=torch.float32, device=q.device)
        lse = torch.empty((B, H, Nq), dtype=torch.float32, device=q.device)
        rope = (qpos, kpos, base, max_pos) if qpos is not None else None
        a, keep = _attn_args(q, k, v, out, scale, rope)
        word = _attn_word(a, "amax_out", q.device)
        ctx.words = _attn_operand_words(a, ATTENTION_ARITH, q, k, v)
        _check(load().vit_attention_fwd(C.byref(a), q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(),
                                        lse.data_ptr(), _stream(q.device)), "vit_attention_fwd")
        if word is not None:
            _publish(out, word)
        ctx.save_for_backward(q, k, v, out, lse, qpos, kpos)
        ctx.cfg = (scale, base, max_pos)
        ctx.arith = ATTENTION_ARITH
        return out

    @staticmethod
    def backward(ctx, g):
        q, k, v, out, lse, qpos, kpos = ctx.saved_tensors
        scale, base, max_pos = ctx.cfg
        lib = load()
        _sync_attention_arith(ctx.arith)
        g = g.contiguous()
        dq = torch.empty(q.shape, dtype=torch.float32, device=q.device)
        dk = torch.empty(k.shape, dtype=torch.float32, device=q.device)
        dv = torch.empty(v.shape, dtype=torch.float32, device=q.device)
        rope = (qpos, kpos, base, max_pos) if qpos is not None else None
        a, keep = _attn_args(q, k, v, out, scale, rope)
        delta = torch.empty_like(lse)
        wq, wk, wv = (_attn_word(a, n, q.device) for n in ("amax_dq", "amax_dk", "amax_dv"))       # the projq / projk / projv weight-gradient and dX launches read them
        if ctx.arith == "f16x3" and ATTENTION_F16:      # the forward's words for q, k, v (same tensors), one more for dO
            fw = ctx.words
            a.amax_q, a.amax_k, a.amax_v = fw[0].data_ptr(), fw[1].data_ptr(), fw[2].data_ptr()
            gw = _amax_of(g)
            a.amax_g = gw.data_ptr()
        _check(lib.vit_attention_bwd(C.byref(a), q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(),
                                     lse.data_ptr(), g.data_ptr(), dq.data_ptr(), dk.data_ptr(), dv.data_ptr(),
                                     delta.data_ptr(), _stream(q.device)), "vit_attention_bwd")
        for t, w in ((dq, wq), (dk, wk), (dv, wv)):
            if w is not None:
                _publish(t, w)
        return dq, dk, dv, None, None, None, None, None


class _AttentionQKV(torch.autograd.Function):
    """Self-attention on a PACKED projection qkv (B,N,3,H,64) (blocks.py:100-103: `self.qkv(x).reshape(B, N, 3, H, C // H)`): the same
    kernels as `_Attention` on the three strided planes, but the backward writes dq, dk, dv straight into the planes of ONE
    (B,N,3,H,64) gradient (VitAttnArgs.dq_sn / dkv_sn) -- autograd's select_backward (a zero fill + a copy per plane) and the two adds
    that assembled that tensor from three contiguous gradients were 6.5 ms of a 328 ms C3 step."""

    @staticmethod
    def forward(ctx, qkv, scale, pos, base, max_pos):
        _need_gpu(qkv, "attention")
        _sync_attention_arith()
        qkv = qkv.contiguous()
        B, N, three, H, D = qkv.shape
        assert three == 3
        q, k, v = qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2]
        out = torch.empty((B, N, H, D), dtype=torch.float32, device=qkv.device)
        lse = torch.empty((B, H, N), dtype=torch.float32, device=qkv.device)
        rope = (pos, pos, base, max_pos) if pos is not None else None
        a, keep = _attn_args(q, k, v, out, scale, rope)
        word = _attn_word(a, "amax_out", qkv.device)
        ctx.words = _attn_operand_words(a, ATTENTION_ARITH, q, k, v, packed=qkv)
        _check(load().vit_attention_fwd(C.byref(a), q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(),
                                        lse.data_ptr(), _stream(qkv.device)), "vit_attention_fwd")
        if word is not None:
            _publish(out, word)
        ctx.save_for_backward(qkv, out, lse, pos)
        ctx.cfg = (scale, base, max_pos)
        ctx.arith = ATTENTION_ARITH
        return out

    @staticmethod
    def backward(ctx, g):
        qkv, out, lse, pos = ctx.saved_tensors
        scale, base, max_pos = ctx.cfg
        _sync_attention_arith(ctx.arith)
        g = g.contiguous()
        B, N, _, H, D = qkv.shape
        q, k, v = qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2]
        dqkv = torch.empty_like(qkv)
        rope = (pos, pos, base, max_pos) if pos is not None else None
        a, keep = _attn_args(q, k, v, out, scale, rope)
        a.dq_sn = a.dkv_sn = 3 * H * D
        delta = torch.empty_like(lse)
        base_ptr, plane = dqkv.data_ptr(), H * D * 4
        word = _attn_word(a, "amax_dq", qkv.device)          # ONE word for the packed gradient: both kernels fold into it
        if word is not None:
            a.amax_dk = a.amax_dv = a.amax_dq
        if ctx.arith == "f16x3" and ATTENTION_F16:
            fw = ctx.words
            a.amax_q = a.amax_k = a.amax_v = fw[0].data_ptr()
            gw = _amax_of(g)
            a.amax_g = gw.data_ptr()
        _check(load().vit_attention_bwd(C.byref(a), q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(),
                                        lse.data_ptr(), g.data_ptr(), base_ptr, base_ptr + plane, base_ptr + 2 * plane,
                                        delta.data_ptr(), _stream(qkv.device)), "vit_attention_bwd")
        if word is not None:
            _publish(dqkv, word)
        return dqkv, None, None, None, None


def attention_qkv(qkv: Tensor, scale: float, pos: Optional[Tensor] = None, rope_base: float = 100.0, max_pos: int = 64) -> Tensor:
    """softmax(q k^T scale) v for a packed (B,N,3,H,64) projection, 2-D RoPE on q and k inside the kernel when `pos` is given"""
    return _AttentionQKV.apply(qkv, float(scale), pos, rope_base, max_pos)


def memory_efficient_attention(q: Tensor, k: Tensor, v: Tensor, scale: Optional[float] = None, p: float = 0.0,
                               qpos: Optional[Tensor] = None, kpos: Optional[Tensor] = None, rope_base: float = 100.0,
                               max_pos: int = 64) -> Tensor:
    """xformers-compatible call on (B,N,H,64) fp32 tensors (views into a qkv buffer are fine).  With
    qpos/kpos the 2-D RoPE is applied to q and k inside the kernel (the buffers stay untouched)."""
    if p != 0.0:
        raise NotImplementedError("attention dropout is 0 in every Styl3R config (blocks.py: attn_drop=0.)")
    if scale is None:
        scale = q.shape[-1] ** -0.5
    return _Attention.apply(q, k, v, float(scale), qpos, kpos, rope_base, max_pos)


# ---------------------------------------------------------------------------
# fused Linear (+ GELU / + residual)
# ---------------------------------------------------------------------------
# Arithmetic of the fused Linear (both are fp32-accurate; tests/test_gpu_vit.py measures each against fp64):
#   "f32"    v_mfma_f32_32x32x2_f32, exact fp32 products (157 TF peak)
#   "bf16x6" every operand split exactly into 3 bf16 pieces, 6 leading partial products on v_mfma_f32_32x32x16_bf16
#            with fp32 accumulation (417 TF peak-equivalent); forward and input-gradient GEMMs.  Default: its measured
#            error against fp64 is equal to or below the f32 path's on every shape tested (split error 2^-27, dropped
#            cross terms 3 * 2^-26 relative), at 1.5-1.7x the throughput
#   "bf16x3" the three leading products only (operands good to 2^-16: the reference's TF32 class)
#   "f16x3"  every operand split into TWO fp16 pieces of value x 2^k (k from the operand tensor's |max|), three products on
#            v_mfma_f32_32x32x16_f16: 2^-22 per product at the MFMA count and data path of bf16x3 (csrc/vit_gemm_x6.hip).  Needs the
#            |max| of every activation operand: one `vit_amax` pass per tensor (`_amax_word`), shared by the launches that read it
LINEAR_MODE = os.environ.get("VIT_LINEAR_MODE", "bf16x6")      # "bf16x6" (default) | "bf16x3" | "f16x3" | "f32"
_PRODUCTS = {"bf16x6": 6, "bf16x3": 3, "f16x3": 2}


def _x6() -> bool:
    """True when the bf16 split-arithmetic kernels are selected; keeps the library's products-per-launch (6 / 3) in step with
    LINEAR_MODE (a module global that tests and benchmarks flip at run time)."""
    if LINEAR_MODE == "f32":
        return False
    if LINEAR_MODE not in _PRODUCTS:
        raise ValueError(f"VIT_LINEAR_MODE = {LINEAR_MODE!r}: expected bf16x6, bf16x3, f16x3 or f32")
    _pin_products(LINEAR_MODE)
    return True

def _pin_products(mode: str) -> None:
    """libvit_hip.so keeps the products-per-launch per HOST THREAD (thread_local): autograd runs a node's backward on its own engine
    thread, so every backward re-states the mode its forward ran in before it launches anything (a step never mixes modes, whatever
    LINEAR_MODE has become in the meantime)."""
    if mode in _PRODUCTS:
        want = _PRODUCTS[mode]
        lib = load()
        if lib.vit_x6_products() != want:
            _check(lib.vit_x6_set_products(want), "vit_x6_set_products")
        _sync_small_m()


_SPLIT_CACHE = WeakTensorCache()   # _image_key(weight, layout) -> packed uint8 image of that weight (owner: the weight)


def _f16() -> bool:
    return LINEAR_MODE == "f16x3"


class _AmaxArena:
    """zero-initialised |max| "words" for vit_amax results (one per activation tensor per use).  A word is 64 int32 slots, ONE PER 128-BYTE CACHE
    LINE (8 KiB): producers fold their maxima into slot (workgroup + wave) & 63 -- atomics on one cache line serialise in the L2, thousands of
    them cost tens of microseconds per launch -- and readers take the max over the slots (csrc/vit_common.h amax_word_fold / amax_word_read).  Words
    are handed out in order from a device buffer that is replaced -- one allocation + one fill -- when it runs out; words still referenced
    (saved for a backward) keep their buffer alive"""
    LINE = 64 * 32

    def __init__(self, lines: int = 512):
        self.lines, self.buf, self.next = lines, {}, {}

    def word(self, dev) -> Tensor:
        """one arena per (device, STREAM, capture state), allocated and zero-filled on the stream that asks -- the stream the
        producer's atomics run on -- so the fill is ordered in front of them (a device-wide arena could be refilled on a side stream while
        the main stream already folded maxima into it).  Under hipGraph capture the arena is a fresh buffer of the graph's pool whose fill
        KERNEL (not a memset node: DESIGN R3.6) is captured in front of the producers, so every replay starts from zeroed words; the graph's
        pool keeps the memory for the graph's lifetime.  The stream key is the raw handle (~0.1 us), not torch.cuda.current_stream."""
        key = (*_device_stream(dev), torch.cuda.is_current_stream_capturing())
        i = self.next.get(key, self.lines)
        if i >= self.lines:
            self.buf[key] = torch.empty(self.lines * self.LINE, dtype=torch.int32, device=dev).fill_(0)
            i = 0
        self.next[key] = i + 1
        return self.buf[key][i * self.LINE:(i + 1) * self.LINE]

    def end_capture(self) -> None:
        """drop the arenas opened under a capture: the next capture (or eager code on the same stream handle) must not be handed words of
        a pool whose zero fill it does not replay"""
        for key in [k for k in self.buf if k[2]]:
            del self.buf[key]; del self.next[key]


_AMAX = _AmaxArena()


def _amax_word(t: Tensor) -> Tensor:
    """|max| of a contiguous fp32 device tensor as a |max| word (vit_amax; 64 slots, 8 KiB): its largest entry is the bit pattern of the maximum"""
    w = _AMAX.word(t.device)
    _check(load().vit_amax(t.data_ptr(), t.numel(), w.data_ptr(), _stream(t.device)), "vit_amax")
    return w


# |max| words PUBLISHED by the kernel that produced a tensor (vit_x6_set_output_amax: LayerNorm forward / backward, the GEMM and halo-convolution
# epilogues): the f16x3 consumer of that tensor finds the word here instead of running a vit_amax pass.  Keyed by the tensor's memory; an entry
# holds a WEAK reference to the producing tensor object and is valid only while that object is alive (its memory cannot have been reused), still
# starts at the same address and carries the version it was published with (no in-place write since).  Views / reshapes of the tensor match too:
# the entries and their weak-reference callback are weak_cache's, the lookup rule is `_known_amax`'s own.
_PUBLISHED = WeakTensorCache()        # (data_ptr, numel) -> word (owner: the produced tensor; stream: the raw stream it was published on)


def _publish(t: Tensor, word: Tensor) -> None:
    _PUBLISHED.store((t.data_ptr(), t.numel()), t, word, _device_stream(t.device)[1] if t.is_cuda else 0)


PUBLISH_AMAX = os.environ.get("VIT_PUBLISH_AMAX", "1") == "1"      # A/B switch: 0 = every f16x3 operand scale comes from its own vit_amax pass


def _known_amax(t: Tensor) -> Optional[Tensor]:
    if not PUBLISH_AMAX:
        return None
    hit = _PUBLISHED.entry((t.data_ptr(), t.numel()))
    if hit is None:
        return None
    src = hit()
    if src is None or src.data_ptr() != t.data_ptr() or src._version != hit.version or t._version != hit.version:
        return None
    if t.is_cuda and hit.stream != _device_stream(t.device)[1] and not torch.cuda.is_current_stream_capturing():
        hit.payload.record_stream(torch.cuda.current_stream(t.device))     # word of another stream's arena read here: the allocator must know
    return hit.payload


def _amax_of(t: Tensor) -> Tensor:
    """|max| word of a contiguous fp32 device tensor: the one its producer published, else a vit_amax pass"""
    w = _known_amax(t)
    if w is not None:
        CALLS["amax_published"] += 1
        return w
    CALLS["amax_pass"] += 1
    return _amax_word(t)


def _output_amax_word(dev) -> Tensor:
    """a zeroed |max| word that the NEXT launch on this thread (Linear / halo convolution / LayerNorm) folds the |max| of what it stores into"""
    w = _AMAX.word(dev)
    _check(load().vit_x6_set_output_amax(w.data_ptr()), "vit_x6_set_output_amax")
    return w


def _want_output_amax(dev) -> Optional[Tensor]:
    """f16x3: ask the next launch to publish its output's |max|, unless the A/B switch is off"""
    return _output_amax_word(dev) if (_f16() and PUBLISH_AMAX) else None


_WEIGHT_AMAX = WeakTensorCache()      # id(weight) -> |max| word of the weight's values: one vit_amax pass per weight and optimizer step


def _weight_amax_word(weight: Tensor, values: Tensor) -> Tensor:
    """|max| word of a parameter (`values`: the fp32 tensor whose elements are the parameter's -- any permutation of them), cached like
    its split images: the forward, transposed and convolution images of one weight share it"""
    word = _WEIGHT_AMAX.get(id(weight), weight)
    if word is None:
        word = _amax_word(values)
        _WEIGHT_AMAX.store(id(weight), weight, word)
    return word


def register_weight_amax(weight: Tensor, word: Tensor) -> None:
    """the |max| word of `weight`'s CURRENT values, produced elsewhere (optim.AdamWHIP: csrc/vit_optim.hip folds it while it writes the update)"""
    _WEIGHT_AMAX.store(id(weight), weight, word)


def _announce(a: Optional[Tensor], b: Optional[Tensor] = None) -> None:
    """f16x3: the |max| words of the activation operand(s) of the NEXT x6 launch on this thread (consumed by it)"""
    _check(load().vit_x6_set_operand_amax(a.data_ptr() if a is not None else None, b.data_ptr() if b is not None else None),
           "vit_x6_set_operand_amax")


# layout names of a weight image: MFMA operand order / block layout of the ring kernels (_t: the transposed image the dX GEMM reads), and
# "conv" / "conv_dx" (the rearranged convolution weight / its flipped, channel-transposed form)
_LINEAR_LAYOUTS = ("row", "row_t", "block", "block_t")      # [2 * block + transposed]


def _image_key(weight: Tensor, layout: str) -> tuple:
    """THE key of a weight image in _SPLIT_CACHE: the lazy splits, the pair splits, the one-launch refresh and the staleness probe of _FusedLinear.forward
    all come here, so they cannot disagree (a refresh that spelled another key would find nothing and leave every image to one launch each: correct
    results, ~1 270 launches a step).  The f16x3 image differs (two fp16 pieces of the scaled weight): the mode at call time is part of the key."""
    return (id(weight), layout, "f16") if LINEAR_MODE == "f16x3" else (id(weight), layout)


_SPLIT_JOB_DTYPE = None
_SPLIT_PLAN: dict = {}        # (device index, mode) -> plan of the last refresh: reused while the same buffers serve the same weights


def refresh_split_cache(params) -> int:
    """After an optimizer step: rebuild EVERY cached image of the given 2-D weights (forward / transposed, MFMA-order / block layout, in the
    current arithmetic mode) in ONE launch (vit_split_weights_many) instead of one launch per image at its next use -- ~1 270 launches and
    12 ms of the C3 step.  Images that are not cached yet (first step), conv images (they go through a rearranged copy) and weights whose
    f16x3 |max| word is not current (the optimizer did not publish it) are left to the lazy path.  Returns the number of images rebuilt.
    The job table is built once: later calls only check that every image buffer / |max| word of the plan still serves its weight (identity
    tests, ~1 ms of host time for 1 200 images) and that the weight really changed, then launch."""
    global _SPLIT_JOB_DTYPE
    import numpy as np
    if LINEAR_MODE == "f32" or not _x6():
        return 0
    f16 = _f16()
    params = [p for p in params if p.dim() == 2 and p.is_cuda and p.dtype == torch.float32 and p.is_contiguous()]
    if not params:
        return 0
    dev = params[0].device
    pkey = (dev.index, LINEAR_MODE)
    plan = _SPLIT_PLAN.get(pkey)
    if plan is not None:                                  # fast path
        ok = len(plan["params"]) == len(params) and all(a is b for a, b in zip(plan["params"], params))
        if ok:
            image, weight_word = _SPLIT_CACHE.entry, _WEIGHT_AMAX.entry
            for key, p, packed, word in plan["entries"]:
                hit = image(key)
                if hit is None or hit.payload is not packed or hit.ptr != p.data_ptr() or hit.version == p._version:
                    ok = False; why = ("image", key, hit is None, hit is not None and hit.payload is not packed, hit is not None and hit.version == p._version); break
                if word:                                  # (the optimizer hands in a fresh view of the same word every step: compare addresses)
                    hw = weight_word(id(p))
                    if hw is None or hw.payload.data_ptr() != word or hw.version != p._version:
                        ok = False; why = ("word", key, hw is None, hw is not None and hw.version != p._version); break
            if not ok and os.environ.get("VIT_SPLIT_DEBUG"):
                print("refresh_split_cache: plan dropped:", why, flush=True)
        elif os.environ.get("VIT_SPLIT_DEBUG"):
            print("refresh_split_cache: plan dropped: parameter list changed", len(plan["params"]), len(params), flush=True)
        if ok:
            _check(load().vit_split_weights_many(plan["table"].data_ptr(), plan["njobs"], plan["blocks"], _stream(dev)), "vit_split_weights_many")
            for key, p, packed, word in plan["entries"]:
                _SPLIT_CACHE.renew(key, p)
            CALLS["split_many_images"] += plan["njobs"]
            CALLS["split_plan_reused"] += 1
            return plan["njobs"]
        _SPLIT_PLAN.pop(pkey, None)
    jobs, entries = [], []
    partial = False         # some image of some weight is not part of this refresh: the job table must not become the reusable plan
    for p in params:
        ver, ptr = p._version, p.data_ptr()
        word = None
        if f16:
            word = _WEIGHT_AMAX.get(id(p), p)
            if word is None:
                partial = True
                continue
        N, K = p.shape
        for transposed in (False, True):
            for block in (False, True):
                key = _image_key(p, _LINEAR_LAYOUTS[2 * block + transposed])
                hit = _SPLIT_CACHE.entry(key)
                if hit is None:
                    continue            # (a layout this weight never uses)
                if hit() is not p or hit.ptr != ptr or hit.version == ver:
                    partial = True      # an image that exists but is not refreshed here (already current, or of a replaced tensor)
                    continue
                R, Kc = (K, N) if transposed else (N, K)
                if Kc % 8:
                    continue
                packed = hit.payload
                tail = packed.data_ptr() + packed.numel() - 8192      # the |max| word closes the image (_image_buffer sized it by the library)
                jobs.append((ptr, packed.data_ptr(), word.data_ptr() if word is not None else 0, tail, N, K,
                             (1 if transposed else 0) | (2 if block else 0), (Kc + 63) // 64, (R + 63) // 64))
                entries.append((key, p, packed, word.data_ptr() if word is not None else 0))
    if not jobs:
        return 0
    if _SPLIT_JOB_DTYPE is None:
        _SPLIT_JOB_DTYPE = np.dtype([("w", "u8"), ("packed", "u8"), ("amax", "u8"), ("tail", "u8"), ("rows", "i4"), ("cols", "i4"), ("kind", "i4"),
                                     ("first_block", "u4"), ("nbx", "u4"), ("reserved", "u4")])     # VitSplitJob
    host = np.zeros(len(jobs), dtype=_SPLIT_JOB_DTYPE)
    first = 0
    for i, (w, pk, am, tl, N, K, kind, nbx, nby) in enumerate(jobs):
        host[i] = (w, pk, am, tl, N, K, kind, first, nbx, 0)
        first += nbx * nby
    table = torch.from_numpy(host.view(np.uint8).reshape(-1).copy()).to(dev)
    _check(load().vit_split_weights_many(table.data_ptr(), len(jobs), first, _stream(dev)), "vit_split_weights_many")
    for key, p, packed, word in entries:
        _SPLIT_CACHE.renew(key, p)
    # the plan is reusable only if it covers every cached image of every weight handed in (a table built on an early step, while the
    # cache was still filling or with some images already current, passed every fast-path check afterwards and pinned the rest to lazy launches)
    if not partial:
        _SPLIT_PLAN[pkey] = {"params": list(params), "entries": entries, "table": table, "njobs": len(jobs), "blocks": first}
    CALLS["split_many_images"] += len(jobs)
    return len(jobs)


PAIR_SPLIT = os.environ.get("VIT_PAIR_SPLIT", "1") == "1"      # A/B switch: 0 = one launch per weight image (rounds 2-5)


def _image_buffer(key: tuple, weight: Tensor, block: bool, transposed: bool) -> Tensor:
    """where an image of a Linear `weight` is (re)built: the buffer of its previous image when that was this tensor's and has the size, else a new one"""
    N, K = weight.shape
    nbytes = load().vit_split_weight_block_bytes(N, K, 1 if transposed else 0) if block else load().vit_split_weight_bytes(N, K)
    old = _SPLIT_CACHE.previous(key, weight)
    return old if old is not None and old.numel() == nbytes else torch.empty(nbytes, dtype=torch.uint8, device=weight.device)


def _split_into(key: tuple, weight: Tensor, values: Tensor, packed: Tensor, kernel: str, transposed: bool = False) -> Tensor:
    """the lazy path of every single-image split: `values` (rows, cols) -- the fp32 elements of `weight` as the kernel reads them -- split into
    `packed` by vit_split_weight / vit_split_weight_block and stored under `key`; f16x3: the weight's |max| word is announced first"""
    if _f16():
        _announce(_weight_amax_word(weight, values))
    _check(getattr(load(), kernel)(values.data_ptr(), packed.data_ptr(), *values.shape, 1 if transposed else 0, _stream(weight.device)), kernel)
    _SPLIT_CACHE.store(key, weight, packed)
    return packed


def _linear_image(weight: Tensor, block: bool, transposed: bool) -> Tensor:
    key = _image_key(weight, _LINEAR_LAYOUTS[2 * block + transposed])
    hit = _SPLIT_CACHE.get(key, weight)
    if hit is not None:
        return hit
    return _split_into(key, weight, weight.detach().contiguous().float(), _image_buffer(key, weight, block, transposed),
                       "vit_split_weight_block" if block else "vit_split_weight", transposed)


def split_weight(weight: Tensor, transposed: bool = False) -> Tensor:
    """bf16x3 split of an nn.Linear weight (N,K) in MFMA operand order (include/vit_ops.h vit_split_weight); cached until the parameter is
    modified in place or replaced (weak_cache: weak reference + version counter + address; optimizer steps must bump the version)."""
    return _linear_image(weight, False, transposed)


def split_weight_block(weight: Tensor, transposed: bool = False) -> Tensor:
    """bf16x3 split of a weight (N,K) in the BLOCK layout the ring kernels read (csrc/vit_weight_image.h; vit_split_weight_block; rows padded to a
    multiple of 64 with zeros).  Cached like `split_weight`."""
    return _linear_image(weight, True, transposed)


def split_weight_pair(weight: Tensor, block_fwd: bool, block_t: bool) -> None:
    """Both images of a Linear weight (N,K) -- the forward one and the transposed one its input-gradient GEMM will ask for -- in ONE launch
    (vit_split_weight_pair), each in the layout its kernel wants (block: the LDS-DMA ring kernels; row: vit_linear_x6_fwd).  Called by the
    forward of a layer whose input needs a gradient when the forward image is stale (i.e. once per optimizer step and weight): the
    backward then finds its image in the cache.  Entries are the same as the single-image functions write."""
    N, K = weight.shape
    w = weight.detach().contiguous().float()
    keys = (_image_key(weight, _LINEAR_LAYOUTS[2 * block_fwd]), _image_key(weight, _LINEAR_LAYOUTS[2 * block_t + 1]))
    bufs = (_image_buffer(keys[0], weight, block_fwd, False), _image_buffer(keys[1], weight, block_t, True))
    if _f16():
        _announce(_weight_amax_word(weight, w))
    _check(load().vit_split_weight_pair(w.data_ptr(), bufs[0].data_ptr(), bufs[1].data_ptr(), N, K, 1 if block_fwd else 0, 1 if block_t else 0,
                                        _stream(weight.device)), "vit_split_weight_pair")
    CALLS["split_pair"] += 1
    for key, buf in zip(keys, bufs):
        _SPLIT_CACHE.store(key, weight, buf)


def linear_x6r(x: Tensor, packed_block: Tensor, N: int, bias: Optional[Tensor] = None, residual: Optional[Tensor] = None,
               gelu: bool = False, cfg: int = 3) -> Tensor:
    """out = [residual +] act(x . W^T + bias) on the LDS-DMA ring kernels (vit_linear_x6r_fwd; forward only, experimental).
    `packed_block` = split_weight_block(W) (or of W^T's transposed packing for a dX product), N = its output width."""
    K = x.shape[-1]
    x2 = x.reshape(-1, K).contiguous().float()
    M = x2.shape[0]
    out = torch.empty(M, N, dtype=torch.float32, device=x.device)
    res = residual.reshape(M, N).contiguous().float() if residual is not None else None
    if cfg == 0:
        raise ValueError("linear_x6r: cfg 0 is vit_linear_x6_fwd on the row image, not a ring configuration")
    _launch_linear(x2, None, out, M, N, K, cfg, image=packed_block, bias=bias, residual=res, act=1 if gelu else 0, count=None)
    return out.reshape(*x.shape[:-1], N)


def split_conv_weight(weight: Tensor, for_input_grad: bool = False, want_dx: bool = False) -> Tensor:
    """bf16x3 split of a conv weight (Co,Ci,k,k) rearranged for vit_conv_x6_fwd: (Co, k*k*Ci) with k index = tap*Ci + ci;
    `for_input_grad`: the spatially flipped, channel-transposed weight (Ci, k*k*Co) whose convolution with dY is dX.
    Cached like `split_weight` (weak reference + version counter of the ORIGINAL parameter).
    Round 6: 1x1 / 3x3 weights are rearranged and split by ONE kernel straight from the parameter (vit_split_conv_weight_pair) -- and when
    the forward finds its image stale and says its input needs a gradient (`want_dx`), the dX image comes out of the same launch."""
    key = _image_key(weight, "conv_dx" if for_input_grad else "conv")
    hit = _SPLIT_CACHE.get(key, weight)
    if hit is not None:
        return hit
    lib = load()
    Co, Ci, kh, kw = weight.shape
    both = (want_dx or for_input_grad) and Co % 8 == 0
    # (a dX image of a weight whose Co is not a multiple of 8: the rearranged-copy path below)
    if PAIR_SPLIT and kh == kw and kh in (1, 3) and Ci % 8 == 0 and weight.dtype == torch.float32 and weight.is_contiguous() and (both or not for_input_grad):
        w = weight.detach()
        pf = torch.empty(lib.vit_split_weight_bytes(Co, kh * kw * Ci), dtype=torch.uint8, device=weight.device)
        pd = torch.empty(lib.vit_split_weight_bytes(Ci, kh * kw * Co), dtype=torch.uint8, device=weight.device) if both else None
        if _f16():
            _announce(_weight_amax_word(weight, w))
        _check(lib.vit_split_conv_weight_pair(w.data_ptr(), pf.data_ptr(), pd.data_ptr() if pd is not None else None, Co, Ci, kh,
                                              _stream(weight.device)), "vit_split_conv_weight_pair")
        CALLS["split_pair"] += 1
        _SPLIT_CACHE.store(_image_key(weight, "conv"), weight, pf)
        if pd is not None:
            _SPLIT_CACHE.store(_image_key(weight, "conv_dx"), weight, pd)
        return pd if for_input_grad else pf
    w = weight.detach().float()
    if for_input_grad:
        w2 = w.flip(2, 3).permute(1, 2, 3, 0).reshape(Ci, kh * kw * Co).contiguous()
    else:
        w2 = w.permute(0, 2, 3, 1).reshape(Co, kh * kw * Ci).contiguous()
    packed = torch.empty(lib.vit_split_weight_bytes(*w2.shape), dtype=torch.uint8, device=weight.device)
    return _split_into(key, weight, w2, packed, "vit_split_weight")


def conv_x6_forward(x: Tensor, weight: Tensor, bias: Optional[Tensor] = None, residual: Optional[Tensor] = None,
                    relu_in: bool = False, packed: Optional[Tensor] = None, amax: Optional[Tensor] = None, publish: bool = False,
                    want_dx: bool = False) -> Tensor:
    """out = [residual +] bias + conv2d(relu?(x), weight, padding=k//2) on vit_conv_x6_fwd (no autograd)."""
    B, Ci, H, W = x.shape
    Co, _, k, _ = weight.shape
    x = x.contiguous().float()
    out = torch.empty((B, Co, H, W), dtype=torch.float32, device=x.device)
    wp = packed if packed is not None else split_conv_weight(weight, want_dx=want_dx)
    res = residual.contiguous().float() if residual is not None else None
    if _f16():
        _announce(amax if amax is not None else _amax_of(x))        # (relu_in: |max| of x bounds |max| of relu(x))
    pub = _want_output_amax(x.device) if publish else None
    _check(load().vit_conv_x6_fwd(x.data_ptr(), wp.data_ptr(), bias.data_ptr() if bias is not None else None,
                                  res.data_ptr() if res is not None else None, out.data_ptr(), B, Ci, Co, H, W, k,
                                  1 if relu_in else 0, _stream(x.device)), "vit_conv_x6_fwd")
    if pub is not None:
        _publish(out, pub)
    return out


# the implicit-GEMM convolution walks its K = taps * Ci slabs sequentially (~0.12 ms floor at Ci = 256): it beats the library
# (1.2-1.7x) once the 128 x 128 output tiles fill the chip; with fewer tiles it splits K across workgroups (atomics) and is on par down to ~100 tiles, slower below (measured,
# tools/probes/conv_small.py); smaller problems stay on the library path
_CONV_X6_MIN_TILES = 1     # r03: forward / dX take the bf16x6 kernel at EVERY size (tools/probes/dpt_layers.py, profiles/r03_dpt_layers.md:
#                            on par with or ahead of the library's Winograd down to the 8 x 8 layers once K is split across workgroups)
_CONV_X6_WGRAD_MIN_PIXELS = int(os.environ.get("VIT_CONV_WGRAD_MIN_PIXELS", "65536"))   # 3x3 dW / db on the split-pixel kernel needs this many pixels (below, its 16-pixel slabs of short image
#                                     rows lose 1.3 - 1.9x to the library's NHWC implicit GEMM: the one library kernel family left in the heads); 1x1: any size
SMALL_CONV_WGRAD = os.environ.get("VIT_CONV_SMALL_WGRAD", "linear")   # 3x3 weight gradients below that pixel count: "linear" (own kernels, default) | "library"
_CONV_X6_MIN_ROWS = 96     # output channels (dX: input channels) per 128-row tile: at 64 the tile is half empty and MIOpen wins (82 vs 104 TF)
# how often each hand-written kernel was taken instead of the library / framework path (the parity tests assert on these)
CALLS = {"linear_x6r": 0, "conv_wgrad_via_linear": 0, "head_tail": 0, "input_merger_x6": 0, "conv_x6_fwd": 0, "conv_x6_dx": 0, "conv_x6_wgrad": 0, "layernorm_hip_fwd": 0, "layernorm_hip_bwd": 0,
         "layernorm_framework": 0, "adapter_hip": 0,
         # library / framework routes taken ON DEVICE TENSORS (layers the hand-written kernels do not cover): the end-to-end tests assert that every one of them stays at zero
         "library_conv_fwd": 0, "library_conv_bwd": 0, "framework_upsample": 0, "framework_dropout": 0, "framework_linear": 0,
         "input_merger_library": 0, "framework_maxpool": 0,
         "lpips_hip_fwd": 0, "lpips_hip_bwd": 0, "maxpool_hip_fwd": 0, "maxpool_hip_bwd": 0,
         "amax_pass": 0, "amax_published": 0, "split_many_images": 0, "split_plan_reused": 0, "split_pair": 0}     # f16x3: activation |max| words from a vit_amax pass / from the producing kernel's epilogue     # (the 7x7 input merger on the library: only when the IMAGE needs a gradient, i.e. in parity tests)
LIBRARY_ROUTES = ("library_conv_fwd", "library_conv_bwd", "framework_upsample", "framework_dropout", "layernorm_framework")


def _conv_tiles(out_channels: int, x: Tensor) -> int:
    return ((out_channels + 127) // 128) * ((x.shape[0] * x.shape[2] * x.shape[3] + 127) // 128)


class _ConvX6(torch.autograd.Function):
    """out = [residual +] bias + conv2d(f(x), weight) (3x3 pad 1 / 1x1, stride 1; f = ReLU if relu_in) on the bf16x6
    implicit-GEMM kernels: forward, input gradient (the same kernel on the flipped, channel-transposed weight, with the
    ReLU mask applied in its epilogue) and weight / bias gradients (vit_conv_x6_wgrad, which applies the ReLU while it
    stages the input); small problems fall back to aten::convolution_backward per gradient.  With relu_in and residual a
    ResidualConvUnit (dpt_block.py:79-118: conv2(act(conv1(act(x)))) + x) is two launches forward and no ReLU / add
    passes or ReLU'd copies of the activations in either direction."""

    @staticmethod
    def forward(ctx, x, weight, bias, residual=None, relu_in=False):
        _need_gpu(x, "conv2d")
        x = x.contiguous().float()
        ctx.save_for_backward(x, weight)
        ctx.has_bias, ctx.has_res, ctx.relu_in = bias is not None, residual is not None, bool(relu_in)
        ctx.mode = LINEAR_MODE
        _pin_products(ctx.mode)
        CALLS["conv_x6_fwd"] += 1
        ctx.ax = _amax_of(x) if _f16() else None               # f16x3: the input's |max|, shared with the weight-gradient launch
        # (the 3x3 halo kernel publishes its output's |max| from the epilogue: the next convolution of a residual unit / head needs no pass)
        k_, W_ = weight.shape[2], x.shape[3]
        # (its input needs a gradient and the dX GEMM will take the own kernel: a stale forward image is rebuilt together with the dX image)
        want_dx = bool(ctx.needs_input_grad[0]) and weight.shape[0] % 16 == 0 and weight.shape[1] >= _CONV_X6_MIN_ROWS
        return conv_x6_forward(x, weight, bias, residual, relu_in, amax=ctx.ax, publish=(k_ == 3 and W_ >= 32), want_dx=want_dx)

    @staticmethod
    def backward(ctx, g):
        x, weight = ctx.saved_tensors
        _pin_products(ctx.mode)
        g = g.contiguous().float()
        f16 = ctx.mode == "f16x3"
        ag = _amax_of(g) if f16 else None                      # |max| of dY (published by the producing kernel, else one pass): read by the dX and the dW launch
        k = weight.shape[2]
        need_x, need_w, need_b = ctx.needs_input_grad[0], ctx.needs_input_grad[1], ctx.has_bias and ctx.needs_input_grad[2]
        need_r = ctx.has_res and ctx.needs_input_grad[3]
        xin = None                                          # f(x), materialised only for a library fallback

        def f_x():
            nonlocal xin
            if xin is None:
                xin = torch.relu(x) if ctx.relu_in else x
            return xin

        dx = None
        if need_x:
            if weight.shape[0] % 16 == 0 and weight.shape[1] >= _CONV_X6_MIN_ROWS and _conv_tiles(weight.shape[1], g) >= _CONV_X6_MIN_TILES:
                B, Co, H, W = g.shape
                Ci = weight.shape[1]
                dx = torch.empty((B, Ci, H, W), dtype=torch.float32, device=g.device)
                CALLS["conv_x6_dx"] += 1
                wpt = split_conv_weight(weight, True)
                if f16:
                    _announce(ag)
                pub = _want_output_amax(g.device) if (f16 and k == 3 and W >= 32) else None
                _check(load().vit_conv_x6_fwd(g.data_ptr(), wpt.data_ptr(), None,
                                              x.data_ptr() if ctx.relu_in else None, dx.data_ptr(),
                                              B, Co, Ci, H, W, k, 2 if ctx.relu_in else 0, _stream(g.device)), "vit_conv_x6_fwd (dX)")
                if pub is not None:
                    _publish(dx, pub)
            else:
                CALLS["library_conv_bwd"] += 1
                dx = torch.ops.aten.convolution_backward(g, f_x(), weight, None, [1, 1], [k // 2, k // 2], [1, 1], False, [0, 0], 1,
                                                         [True, False, False])[0]
                if ctx.relu_in:
                    dx = dx * (x > 0)
        dw = db = None
        B_, _, H_, W_ = g.shape
        # dW (+ db) on the bf16x6 split-pixel kernel when there are enough pixels to split (>= 64 x 64 x 16; below that the
        # library's kernel is faster: measured)
        if need_w and W_ % 8 == 0 and (H_ * W_) % 16 == 0 and (k == 1 or B_ * H_ * W_ >= _CONV_X6_WGRAD_MIN_PIXELS):
            dw = torch.empty_like(weight, dtype=torch.float32)
            db = torch.empty((weight.shape[0],), dtype=torch.float32, device=g.device) if need_b else None
            CALLS["conv_x6_wgrad"] += 1
            if f16:
                _announce(ag, ctx.ax)
            _check(load().vit_conv_x6_wgrad(g.data_ptr(), x.data_ptr(), dw.data_ptr(), db.data_ptr() if need_b else None,
                                            B_, weight.shape[1], weight.shape[0], H_, W_, k, 1 if ctx.relu_in else 0,
                                            _stream(g.device)), "vit_conv_x6_wgrad")
        elif need_w and k == 3 and weight.shape[1] % 16 == 0 and _x6() and SMALL_CONV_WGRAD == "linear":
            # 3x3 layers with few pixels (the 8 x 8 .. 64 x 64 stages): the split-pixel kernel's 16-pixel slabs of short image rows
            # lose there, so the gradient goes through the LINEAR weight-gradient kernel instead: dW (Co, 9 Ci) = dY^T (Co, P) . cols (P, 9 Ci)
            # with the pixel-major operands built by vit_im2col3_rows (the nine taps, the ReLU of a residual unit applied on the way) and one
            # channels-last copy of dY.  No library kernel.
            Co, Ci = weight.shape[0], weight.shape[1]
            P = B_ * H_ * W_
            cols = torch.empty((P, 9 * Ci), dtype=torch.float32, device=g.device)
            _check(load().vit_im2col3_rows(x.data_ptr(), cols.data_ptr(), B_, Ci, H_, W_, 1 if ctx.relu_in else 0, _stream(g.device)), "vit_im2col3_rows")
            gt = g.permute(0, 2, 3, 1).reshape(P, Co).contiguous()
            buf = torch.empty(Co * 9 * Ci + (Co if need_b else 0), dtype=torch.float32, device=g.device)
            dwl = buf[:Co * 9 * Ci].view(Co, 9 * Ci)
            db = buf[Co * 9 * Ci:] if need_b else None
            CALLS["conv_wgrad_via_linear"] += 1
            if f16:
                _announce(ag, ctx.ax)                          # (gt is a copy of g; |cols| <= |x|)
            _check(load().vit_linear_x6_wgrad(gt.data_ptr(), cols.data_ptr(), dwl.data_ptr(), db.data_ptr() if need_b else None, P, Co, 9 * Ci,
                                              _stream(g.device)), "vit_linear_x6_wgrad (conv)")
            dw = dwl.view(Co, 3, 3, Ci).permute(0, 3, 1, 2).contiguous()
        elif need_w or need_b:
            CALLS["library_conv_bwd"] += 1
            _, dw, db = torch.ops.aten.convolution_backward(g, f_x(), weight, [weight.shape[0]] if ctx.has_bias else None, [1, 1],
                                                            [k // 2, k // 2], [1, 1], False, [0, 0], 1, [False, bool(need_w), bool(need_b)])
        return dx, dw, db, (g if need_r else None), None


class Conv2dX6(nn.Conv2d):
    """nn.Conv2d whose forward / input gradient run on vit_conv_x6_fwd when the layer qualifies (k in {1, 3}, stride 1,
    padding k // 2, no dilation / groups, Ci % 16 == 0, Co >= 96) and the input is a device fp32 tensor in bf16x6 mode;
    otherwise the stock MIOpen path.  Same parameters / state_dict keys as nn.Conv2d."""

    def _x6_ok(self, x: Tensor) -> bool:
        k = self.kernel_size[0]
        return (_x6() and x.is_cuda and x.dtype == torch.float32 and x.dim() == 4
                and self.kernel_size in ((1, 1), (3, 3)) and self.stride == (1, 1) and self.padding == (k // 2, k // 2)
                and self.dilation == (1, 1) and self.groups == 1 and self.padding_mode == "zeros"
                and self.in_channels % 16 == 0 and self.out_channels >= _CONV_X6_MIN_ROWS
                and _conv_tiles(self.out_channels, x) >= _CONV_X6_MIN_TILES)

    def forward(self, x: Tensor) -> Tensor:
        if self._x6_ok(x):
            return _ConvX6.apply(x, self.weight, self.bias)
        if x.is_cuda:
            CALLS["library_conv_fwd"] += 1
        return super().forward(x)

    def forward_fused(self, x: Tensor, residual: Optional[Tensor] = None) -> Tensor:
        """[residual +] conv(relu(x)): one launch on the bf16x6 kernel when the layer qualifies, the plain sequence otherwise."""
        if self._x6_ok(x):
            return _ConvX6.apply(x, self.weight, self.bias, residual, True)
        if x.is_cuda:
            CALLS["library_conv_fwd"] += 1
        out = super().forward(torch.relu(x))
        return out if residual is None else out + residual


class _Upsample2x(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        B, Cc, H, W = x.shape
        x = x.contiguous().float()
        out = torch.empty((B, Cc, 2 * H, 2 * W), dtype=torch.float32, device=x.device)
        _check(load().vit_upsample2x_fwd(x.data_ptr(), out.data_ptr(), B * Cc, H, W, _stream(x.device)), "vit_upsample2x_fwd")
        ctx.shape = (B, Cc, H, W)
        if _f16():          # bilinear interpolation is a convex combination: |max| of the input bounds |max| of the output (a valid f16x3 scale)
            w = _known_amax(x)
            if w is not None:
                _publish(out, w)
        return out

    @staticmethod
    def backward(ctx, g):
        B, Cc, H, W = ctx.shape
        g = g.contiguous().float()
        din = torch.empty((B, Cc, H, W), dtype=torch.float32, device=g.device)
        _check(load().vit_upsample2x_bwd(g.data_ptr(), din.data_ptr(), B * Cc, H, W, _stream(g.device)), "vit_upsample2x_bwd")
        return din


def upsample2x(x: Tensor) -> Tensor:
    """F.interpolate(x, scale_factor=2, mode="bilinear", align_corners=True); device fp32 NCHW tensors with an even width
    take vit_upsample2x_fwd / vit_upsample2x_bwd, anything else the framework's kernels."""
    if x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and x.shape[-1] % 2 == 0:
        return _Upsample2x.apply(x)
    if x.is_cuda:
        CALLS["framework_upsample"] += 1
    return torch.nn.functional.interpolate(x, scale_factor=2, mode="bilinear", align_corners=True)


class _MaxPool2x2(torch.autograd.Function):
    """nn.MaxPool2d(2, 2) on vit_maxpool2x2_fwd / _bwd: the backward recomputes the argmax from the saved input (no index tensor)"""

    @staticmethod
    def forward(ctx, x):
        B, Cc, H, W = x.shape
        x = _aligned(x)
        out = torch.empty((B, Cc, H // 2, W // 2), dtype=torch.float32, device=x.device)
        CALLS["maxpool_hip_fwd"] += 1
        _check(load().vit_maxpool2x2_fwd(x.data_ptr(), out.data_ptr(), B * Cc, H, W, _stream(x.device)), "vit_maxpool2x2_fwd")
        ctx.save_for_backward(x)
        if _f16():          # every output is one of the inputs: |max| of the input bounds |max| of the output (a valid f16x3 scale)
            w = _known_amax(x)
            if w is not None:
                _publish(out, w)
        return out

    @staticmethod
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        B, Cc, H, W = x.shape
        g = g.contiguous().float()
        din = torch.empty_like(x)
        CALLS["maxpool_hip_bwd"] += 1
        _check(load().vit_maxpool2x2_bwd(x.data_ptr(), g.data_ptr(), din.data_ptr(), B * Cc, H, W, _stream(g.device)), "vit_maxpool2x2_bwd")
        return din


def _aligned(x: Tensor) -> Tensor:
    """contiguous fp32 with a 16-byte aligned base (a view at an odd offset is copied)"""
    x = x.contiguous().float()
    return x if x.data_ptr() % 16 == 0 else x.clone()


def maxpool2x2(x: Tensor) -> Tensor:
    """F.max_pool2d(x, 2, 2); device fp32 NCHW maps with even H and W take vit_maxpool2x2_fwd / _bwd, anything else the framework's
    kernels.  Commutes with ReLU (max(relu(x)) = relu(max(x)), the mask of the ReLU follows at the argmax): LPIPS's VGG pools the
    pre-activations."""
    if x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and x.shape[-1] % 2 == 0 and x.shape[-2] % 2 == 0 and x.numel() > 0:
        return _MaxPool2x2.apply(x)
    if x.is_cuda:
        CALLS["framework_maxpool"] += 1
    return torch.nn.functional.max_pool2d(x, 2, 2)


def _lpips_table(fa, fb, ws, dfa=None):
    taps = (VitLpipsTap * len(fa))()
    for k, (a, b, w) in enumerate(zip(fa, fb, ws)):
        taps[k] = VitLpipsTap(a.data_ptr(), b.data_ptr(), w.data_ptr(), dfa[k].data_ptr() if dfa is not None else None,
                              a.shape[1], a.shape[2], a.shape[3])
    return taps


class _LpipsTail(torch.autograd.Function):
    """dist (N,) = sum_k mean_hw sum_c w_k[c] (a^ - b^)^2 over the five taps (losses.LPIPS.forward's tail) on vit_lpips_fwd; the
    backward is one vit_lpips_bwd for every tap.  The target taps get no gradient (ground truth).  Saved for the backward: the taps
    and 16 B of per-pixel statistics (vit_lpips_stats_bytes)."""

    @staticmethod
    def forward(ctx, relu_in, *args):
        n = len(args) // 3
        fa = [_aligned(t) for t in args[:n]]
        fb = [_aligned(t) for t in args[n:2 * n]]
        ws = [t.detach().reshape(-1).contiguous().float() for t in args[2 * n:]]
        N, dev = fa[0].shape[0], fa[0].device
        for a, b, w in zip(fa, fb, ws):
            assert a.shape == b.shape and a.shape[0] == N and w.numel() == a.shape[1], "lpips tail: matching taps, one weight per channel"
        lib = load()
        taps = _lpips_table(fa, fb, ws)
        part = torch.empty(lib.vit_lpips_scratch_bytes(taps, n, N) // 4, dtype=torch.float32, device=dev)
        want = any(ctx.needs_input_grad[1:1 + n])
        stats = torch.empty(lib.vit_lpips_stats_bytes(taps, n, N) // 4, dtype=torch.float32, device=dev) if want else None
        dist = torch.empty(N, dtype=torch.float32, device=dev)
        CALLS["lpips_hip_fwd"] += 1
        _check(lib.vit_lpips_fwd(taps, n, N, 1 if relu_in else 0, dist.data_ptr(), part.data_ptr(),
                                 stats.data_ptr() if stats is not None else None, _stream(dev)), "vit_lpips_fwd")
        if want:
            ctx.save_for_backward(stats, *fa, *fb, *ws)
        ctx.n, ctx.relu_in = n, bool(relu_in)
        return dist

    @staticmethod
    def backward(ctx, g):
        n = ctx.n
        stats, *rest = ctx.saved_tensors
        fa, fb, ws = rest[:n], rest[n:2 * n], rest[2 * n:]
        g = g.contiguous().float()
        dfa = [torch.empty_like(a) for a in fa]
        taps = _lpips_table(fa, fb, ws, dfa)
        CALLS["lpips_hip_bwd"] += 1
        _check(load().vit_lpips_bwd(taps, n, fa[0].shape[0], 1 if ctx.relu_in else 0, g.data_ptr(), stats.data_ptr(), _stream(g.device)),
               "vit_lpips_bwd")
        return (None, *[d if ctx.needs_input_grad[1 + k] else None for k, d in enumerate(dfa)], *([None] * (2 * n)))


def lpips_tail(fa, fb, weights, relu_in: bool = False) -> Tensor:
    """(N,) LPIPS distances from the taps fa / fb (lists of (N, C_k, H_k, W_k) device fp32 tensors, up to five) and the 1x1 `lin`
    weights (C_k elements each): sum_k mean_hw sum_c w_k[c] (a^_c - b^_c)^2 with a^ = a / (|a|_c + 1e-10) (relu_in: of max(a, 0)).
    The target side `fb` is ground truth: it must not need a gradient (callers keep the torch expression for that case)."""
    for t in (*fa, *fb):
        _need_gpu(t, "lpips_tail")
    assert not any(t.requires_grad for t in fb), "lpips_tail: the target taps are ground truth"
    assert not (torch.is_grad_enabled() and any(w.requires_grad for w in weights)), "lpips_tail: the lin weights get no gradient"
    return _LpipsTail.apply(bool(relu_in), *fa, *fb, *weights)


class _ReluDropout(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, p, seed):
        _need_gpu(x, "relu_dropout")
        ctx.mark_dirty(x)                        # in place, like the reference's ReLU(True): the convolution before it does not keep its output
        _check(load().vit_relu_dropout_fwd(x.data_ptr(), x.data_ptr(), x.numel(), float(p), int(seed), _stream(x.device)), "vit_relu_dropout_fwd")
        ctx.save_for_backward(x)
        ctx.p = float(p)
        return x

    @staticmethod
    def backward(ctx, g):
        (y,) = ctx.saved_tensors
        g = g.contiguous().float()
        dx = torch.empty_like(y)
        _check(load().vit_relu_dropout_bwd(y.data_ptr(), g.data_ptr(), dx.data_ptr(), y.numel(), ctx.p, _stream(g.device)), "vit_relu_dropout_bwd")
        return dx, None, None


_DROPOUT_GEN: dict = {}


def reseed_dropout(seed: Optional[int] = None) -> None:
    """(Re)start the dropout stream from (seed or torch.initial_seed(), RANK).  Called implicitly whenever torch.initial_seed()
    has changed since the last draw; call it explicitly to repeat a run after re-seeding with the SAME value."""
    base = torch.initial_seed() if seed is None else int(seed)
    rank = int(os.environ.get("RANK", "0"))
    g = torch.Generator()
    g.manual_seed((base * 1_000_003 + 7919 * rank + 0x5DEECE66D) % (2 ** 63))
    _DROPOUT_GEN["gen"], _DROPOUT_GEN["key"] = g, (torch.initial_seed(), rank)


def _dropout_generator() -> torch.Generator:
    """one generator per (base seed, rank): re-created when torch.manual_seed changes the base seed"""
    key = (torch.initial_seed(), int(os.environ.get("RANK", "0")))
    if _DROPOUT_GEN.get("gen") is None or _DROPOUT_GEN.get("key") != key:
        reseed_dropout()
    return _DROPOUT_GEN["gen"]


def relu_dropout(x: Tensor, p: float, training: bool) -> Tensor:
    """Dropout(p)(ReLU(x)) of the 'gs_params' DPT heads (dpt_block.py:332-340).  Training on a device fp32 tensor: one HIP pass each
    way, in place, no mask tensor (vit_relu_dropout_fwd / _bwd; the keep decisions come from Philox keyed by a seed drawn from a DEDICATED
    generator -- seeded from (torch.initial_seed(), RANK) at first use, so `torch.manual_seed` before the first step makes a run
    repeatable, ranks draw different masks as under the reference's `seed + global_rank` (src/main_style.py:118), and the default CPU
    generator -- data sampling, shuffles -- is never consumed); otherwise the framework ops."""
    if training and p > 0.0 and x.is_cuda and x.dtype == torch.float32 and x.is_contiguous() and x.numel() % 4 == 0 and not x.is_leaf:
        seed = int(torch.randint(0, 2 ** 62, (1,), generator=_dropout_generator()).item())
        return _ReluDropout.apply(x, p, seed)
    if x.is_cuda and training and p > 0.0:
        CALLS["framework_dropout"] += 1
    return torch.nn.functional.dropout(torch.relu_(x) if not x.is_leaf else torch.relu(x), p, training)


class _HeadTail(torch.autograd.Function):
    """vit_head_tail_fwd / _bwd: ReLU [-> Dropout(p)] -> 1x1 convolution with 3 or 8 output channels, one pass over the activation
    each way; saves the RAW convolution output h (nothing activated, no mask)."""

    @staticmethod
    def forward(ctx, h, weight, bias, p, seed):
        _need_gpu(h, "head_tail")
        h = h.contiguous().float()
        B, Cc, H, W = h.shape
        CO = weight.shape[0]
        w2 = weight.reshape(CO, Cc).contiguous().float()
        y = torch.empty((B, CO, H, W), dtype=torch.float32, device=h.device)
        CALLS["head_tail"] += 1
        _check(load().vit_head_tail_fwd(h.data_ptr(), w2.data_ptr(), bias.data_ptr() if bias is not None else None, y.data_ptr(),
                                        B, Cc, CO, H * W, float(p), int(seed), _stream(h.device)), "vit_head_tail_fwd")
        ctx.save_for_backward(h, w2)
        ctx.meta = (float(p), int(seed), bias is not None, tuple(weight.shape))
        return y

    @staticmethod
    def backward(ctx, g):
        h, w2 = ctx.saved_tensors
        p, seed, has_bias, wshape = ctx.meta
        g = g.contiguous().float()
        B, Cc, H, W = h.shape
        CO = w2.shape[0]
        dh = torch.empty_like(h)
        dw = torch.empty((CO, Cc), dtype=torch.float32, device=h.device)
        db = torch.empty((CO,), dtype=torch.float32, device=h.device) if has_bias else None
        _check(load().vit_head_tail_bwd(h.data_ptr(), w2.data_ptr(), g.data_ptr(), dh.data_ptr(), dw.data_ptr(),
                                        db.data_ptr() if db is not None else None, B, Cc, CO, H * W, p, seed, _stream(h.device)),
               "vit_head_tail_bwd")
        return dh, dw.reshape(wshape), db, None, None


def head_tail(h: Tensor, conv: nn.Conv2d, p: float, training: bool) -> Optional[Tensor]:
    """conv(Dropout(p)(ReLU(h))) for the 1x1 output convolutions of the DPT heads on vit_head_tail_*; None when the layer does not
    qualify (not a device fp32 tensor, output channels other than 3 / 8, C not a multiple of 8 or above 256): the caller then runs the
    separate ReLU / Dropout / convolution kernels."""
    Cc = h.shape[1]
    if not (h.is_cuda and h.dtype == torch.float32 and h.dim() == 4 and conv.kernel_size == (1, 1) and conv.out_channels in (3, 8)
            and Cc % 8 == 0 and Cc <= 256 and (h.shape[2] * h.shape[3]) % 4 == 0):
        return None
    drop = p if training else 0.0
    seed = int(torch.randint(0, 2 ** 62, (1,), generator=_dropout_generator()).item()) if drop > 0.0 else 0
    return _HeadTail.apply(h, conv.weight, conv.bias, drop, seed)


class _UpsampleAddRelu(torch.autograd.Function):
    """out = upsample2x(x) + relu(c) in one pass (vit_upsample2x_add_relu_fwd); backward: (upsample2x_bwd(g), g where c > 0)."""

    @staticmethod
    def forward(ctx, x, c):
        B, Cc, H, W = x.shape
        x = x.contiguous().float(); c = c.contiguous().float()
        out = torch.empty((B, Cc, 2 * H, 2 * W), dtype=torch.float32, device=x.device)
        _check(load().vit_upsample2x_add_relu_fwd(x.data_ptr(), c.data_ptr(), out.data_ptr(), B * Cc, H, W, _stream(x.device)),
               "vit_upsample2x_add_relu_fwd")
        ctx.save_for_backward(c)
        ctx.shape = (B, Cc, H, W)
        return out

    @staticmethod
    def backward(ctx, g):
        (c,) = ctx.saved_tensors
        B, Cc, H, W = ctx.shape
        g = g.contiguous().float()
        dx = dc = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty((B, Cc, H, W), dtype=torch.float32, device=g.device)
            _check(load().vit_upsample2x_bwd(g.data_ptr(), dx.data_ptr(), B * Cc, H, W, _stream(g.device)), "vit_upsample2x_bwd")
        if ctx.needs_input_grad[1]:
            dc = torch.empty_like(c)        # g where the input merger's pre-activation is positive (the ReLU gate), one pass
            _check(load().vit_relu_dropout_bwd(c.data_ptr(), g.data_ptr(), dc.data_ptr(), c.numel(), 0.0, _stream(g.device)), "vit_relu_dropout_bwd (gate)")
        return dx, dc


_DERIVED = WeakTensorCache()      # (id(parameter), tag) -> derived tensor (owner: the parameter)


def derived_weight(param: Optional[Tensor], tag: str, fn):
    """Serving path: a tensor derived from a parameter (a reshaped / permuted convolution weight, a repeated bias) is built ONCE per parameter
    version and keeps its identity, so the split images vit_ops caches per weight tensor stay valid -- without this every forward re-made the
    tensor and with it its copies, its |max| pass and its split launch (5 launches per reassemble layer and head, ~150 per C2 forward).
    With autograd on, the derivation must stay in the graph: computed in place."""
    if param is None:
        return None
    if torch.is_grad_enabled() and param.requires_grad:
        return fn(param)
    key = (id(param), tag)
    d = _DERIVED.get(key, param)
    if d is None:
        with torch.no_grad():
            d = fn(param.detach())
        _DERIVED.store(key, param, d)
    return d


def input_merger_upsample_add(p1: Tensor, imgs: Tensor, conv7: nn.Conv2d) -> Optional[Tensor]:
    """`feat_up(path_1) + ReLU(Conv2d(3, 256, 7, 1, 3)(imgs))` of the 'gs' head (dpt_gs_head.py:113-118,146-148) without the library:
    the 7x7 patches as 160 planes (vit_im2col7), the convolution as a 1x1 convolution over them on the bf16x6 kernels (forward and
    weight gradient), ReLU + add inside the up-sampling pass.  None when the layer does not qualify (the image needs a gradient -- parity
    tests only --, not a device fp32 tensor, other kernel geometry): the caller keeps the framework sequence."""
    if not (_x6() and imgs.is_cuda and imgs.dtype == torch.float32 and not imgs.requires_grad and imgs.shape[1] == 3 and conv7.kernel_size == (7, 7)
            and conv7.stride == (1, 1) and conv7.padding == (3, 3) and imgs.shape[3] % 8 == 0 and (imgs.shape[2] * imgs.shape[3]) % 16 == 0
            and p1.shape[2] * 2 == imgs.shape[2] and p1.shape[3] * 2 == imgs.shape[3] and conv7.out_channels == p1.shape[1]
            and conv7.out_channels >= _CONV_X6_MIN_ROWS):
        return None
    B, _, H, W = imgs.shape
    imgs = imgs.contiguous()
    cols = torch.empty((B, 160, H, W), dtype=torch.float32, device=imgs.device)
    _check(load().vit_im2col7(imgs.data_ptr(), cols.data_ptr(), B, H, W, _stream(imgs.device)), "vit_im2col7")
    Co = conv7.out_channels
    w160 = derived_weight(conv7.weight, "w160", lambda w_: torch.nn.functional.pad(w_.reshape(Co, 147), (0, 13)).reshape(Co, 160, 1, 1))
    CALLS["input_merger_x6"] += 1
    c = _ConvX6.apply(cols, w160, conv7.bias)
    return _UpsampleAddRelu.apply(p1, c)


class _GaussianAdapterHip(torch.autograd.Function):
    """vit_adapter_fwd / vit_adapter_bwd (include/vit_ops.h): DPT head outputs (NCHW, per view group) -> Gaussians in the
    rasterizer's layout, one launch each way (reg_dense_depth + sigmoid / opacity map + UnifiedGaussianAdapter +
    build_covariance + the per-view cat / transposes).  Returns (means, cov, sh, opac[, scales, rot])."""

    @staticmethod
    def forward(ctx, pts0, ptsr, par0, parr, app, sh_mask, exponent, v, want_dump):
        b, _, H, W = pts0.shape
        dev = pts0.device
        c = lambda t: None if t is None else t.contiguous().float()
        pts0, ptsr, par0, parr, app = c(pts0), c(ptsr), c(par0), c(parr), c(app)
        d_sh = sh_mask.numel()
        a = VitAdapterArgs(b, v, H, W, d_sh, par0.shape[1], float(exponent), pts0.data_ptr(), ptsr.data_ptr() if ptsr is not None else None,
                           par0.data_ptr(), parr.data_ptr() if parr is not None else None, app.data_ptr() if app is not None else None,
                           sh_mask.data_ptr())
        G = v * H * W
        means = torch.empty((b, G, 3), dtype=torch.float32, device=dev)
        cov = torch.empty((b, G, 3, 3), dtype=torch.float32, device=dev)
        sh = torch.empty((b, G, 3, d_sh), dtype=torch.float32, device=dev)
        opac = torch.empty((b, G), dtype=torch.float32, device=dev)
        scales = torch.empty((b, G, 3), dtype=torch.float32, device=dev) if want_dump else None
        rot = torch.empty((b, G, 4), dtype=torch.float32, device=dev) if want_dump else None
        _check(load().vit_adapter_fwd(C.byref(a), means.data_ptr(), cov.data_ptr(), sh.data_ptr(), opac.data_ptr(),
                                      scales.data_ptr() if want_dump else None, rot.data_ptr() if want_dump else None,
                                      _stream(dev)), "vit_adapter_fwd")
        CALLS["adapter_hip"] += 1
        ctx.save_for_backward(pts0, ptsr, par0, parr, app, sh_mask)
        ctx.meta = (b, v, H, W, d_sh, float(exponent))
        if want_dump:
            ctx.mark_non_differentiable(scales, rot)
            return means, cov, sh, opac, scales, rot
        return means, cov, sh, opac

    @staticmethod
    def backward(ctx, g_means, g_cov, g_sh, g_opac, *_):
        pts0, ptsr, par0, parr, app, sh_mask = ctx.saved_tensors
        b, v, H, W, d_sh, exponent = ctx.meta
        dev = pts0.device
        G = v * H * W
        z = lambda g, shape: (g.contiguous().float() if g is not None else torch.zeros(shape, dtype=torch.float32, device=dev))
        g_means, g_cov = z(g_means, (b, G, 3)), z(g_cov, (b, G, 3, 3))
        g_sh, g_opac = z(g_sh, (b, G, 3, d_sh)), z(g_opac, (b, G))
        a = VitAdapterArgs(b, v, H, W, d_sh, par0.shape[1], exponent, pts0.data_ptr(), ptsr.data_ptr() if ptsr is not None else None,
                           par0.data_ptr(), parr.data_ptr() if parr is not None else None, app.data_ptr() if app is not None else None,
                           sh_mask.data_ptr())
        e = lambda t: None if t is None else torch.empty_like(t)
        d_pts0, d_ptsr, d_par0, d_parr, d_app = e(pts0), e(ptsr), e(par0), e(parr), e(app)
        p = lambda t: None if t is None else t.data_ptr()
        _check(load().vit_adapter_bwd(C.byref(a), g_means.data_ptr(), g_cov.data_ptr(), g_sh.data_ptr(), g_opac.data_ptr(),
                                      p(d_pts0), p(d_ptsr), p(d_par0), p(d_parr), p(d_app), _stream(dev)), "vit_adapter_bwd")
        return d_pts0, d_ptsr, d_par0, d_parr, d_app, None, None, None, None


def gaussian_adapter_hip(pts0, ptsr, par0, parr, app, sh_mask, exponent: float, v: int, want_dump: bool = False):
    return _GaussianAdapterHip.apply(pts0, ptsr, par0, parr, app, sh_mask, exponent, v, want_dump)


def invalidate_split_cache() -> None:
    _SPLIT_CACHE.clear()
    _WEIGHT_AMAX.clear()
    _SPLIT_PLAN.clear()


# (N, K) -> ring configuration of vit_linear_x6r_fwd for launches of M >= 4096 rows, per arithmetic mode (cfg 3: 256 x 256 tiles, one
# activation split per workgroup, ping-pong wave pairs; cfg 1: 128 x 128 LDS-DMA ring).  Measured with tools/probes/gemm_lab.py at M ~ 5 140
# (profiles/r03_gemm_lab.md; TF default -> ring).  Six products: encoder qkv 168 -> 206, decoder fc1 171 -> 200, decoder qkv 166 -> 177, encoder
# fc2 150 -> 164.  Three products, where the default kernel is bound by its data path, not by the matrix pipes: encoder qkv
# 221 -> 311, fc1 223 -> 276, fc2 164 -> 283, proj 161 -> 224, decoder qkv 210 -> 252, fc1 224 -> 294, fc2 198 -> 234.  In three-product mode the
# same table serves the input-gradient GEMMs (dX = dY . W is the Linear with N and K exchanged).  Outputs are bit-identical to vit_linear_x6_fwd.
_RING_SHAPES = {
    # f16x3: the data path of bf16x3 with fp16 pieces -- same table
    "f16x3": {(3072, 1024): 3, (3072, 768): 3, (2304, 768): 3, (4096, 1024): 1, (1024, 4096): 1, (1024, 1024): 1, (1024, 3072): 1,
              (768, 3072): 1, (768, 2304): 1, (768, 768): 1, (768, 1024): 1},
    "bf16x6": {(3072, 1024): 3, (3072, 768): 3, (2304, 768): 3, (1024, 4096): 1},
    "bf16x3": {(3072, 1024): 3, (3072, 768): 3, (2304, 768): 3, (4096, 1024): 1, (1024, 4096): 1, (1024, 1024): 1, (1024, 3072): 1,
               (768, 3072): 1, (768, 2304): 1, (768, 768): 1, (768, 1024): 1},
}
# 2048 <= M < 4096 (the dual decoders' 2 570-row launches, the style encoder's 2 560 rows at C3): only the wide layers still fill the chip
# (three products, M = 2 570: decoder qkv 155 -> 198, fc1 167 -> 252; the N = 768 layers LOSE there: 118 -> 89, and 1024 x 1024 is a tie).
# Style-encoder shapes at M = 2 560 (tools/probes/gemm_lab.py, r03): three products fc1 209 -> 252 (cfg 3), qkv 179 -> 271, fc2 152 -> 165,
# qkv dX 140 -> 159 (cfg 1); six products (forward only) fc1 154 -> 173 (cfg 3), qkv 139 -> 177 (cfg 1).  tools/probes/linear_shapes.py: these
# four shapes are 20 % of the Linear forward + dX FLOPs of a C3 step.
_RING_SHAPES_MID = {"f16x3": {(2304, 768): 1, (3072, 768): 1, (4096, 1024): 3, (1024, 4096): 1, (3072, 1024): 1, (1024, 3072): 1},
                    "bf16x3": {(2304, 768): 1, (3072, 768): 1, (4096, 1024): 3, (1024, 4096): 1, (3072, 1024): 1, (1024, 3072): 1},
                    "bf16x6": {(4096, 1024): 3, (3072, 1024): 1}}
RING_DISPATCH = os.environ.get("VIT_RING_DISPATCH", "1") == "1"


def _linear_cfg(M: int, N: int, K: int, *, dx: bool = False, serving: bool = False, mode: Optional[str] = None) -> int:
    """THE route of a fused-Linear launch of a layer (N, K) at M rows: 0 = vit_linear_x6_fwd on the ROW image; 1 / 3 (LDS-DMA rings) and 5
    (csrc/vit_gemm_sm.hip) = vit_linear_x6r_fwd on the BLOCK image -- `cfg != 0` is the layout of the image, for the launch, the staleness probe
    and the pair split alike.  "f32" has no x6 launch: 0.
    serving (no grad): the small-M kernel where `small_m_kernel` takes the shape, else 0 -- at EVERY row count, above 2048 too: the serving path
      takes neither the rings nor the narrow-output route (batch-1 serving runs at 257 / 514 rows; larger no-grad launches were never A/B-ed).
    training forward: the narrow-output kernel (5) above SMALL_M_ROWS, else the ring table of the row count (>= 4096 / >= 2048), else 0.
    dx: the input-gradient GEMM (dX = dY . W: the forward rule with N and K exchanged) -- ring kernels in three-product mode only (in six-product
      mode the A/B on the whole step lost 3 ms), the narrow-output kernel in every mode; `mode`: the mode of the node's forward -- once LINEAR_MODE
      has moved on, the row image."""
    if LINEAR_MODE == "f32":
        return 0
    if serving:
        return 5 if small_m_kernel(M, N, K) else 0
    if dx:
        if mode is not None and mode != LINEAR_MODE:
            return 0
        cfg = _linear_cfg(M, K, N)
        return cfg if (cfg == 5 or LINEAR_MODE in ("bf16x3", "f16x3")) else 0
    # csrc/vit_gemm_sm.hip in the AUTOGRAD path: narrow outputs at train-step row counts only.  (Nothing trains at 257 / 514 rows except the parity
    # fixtures, and those were recorded against the summation order of the 128-row kernels: with the small-M kernel in their forward the c3
    # fixture's style-encoder gradients sit in the flip-prone state of DESIGN 9 (3) in EVERY run instead of two runs in five --
    # profiles/r06_c3_stylizer_rows_ab.txt)
    # (tried and dropped: every served shape at 1 024 < M < 2 048 -- the C4 style stage's 1 536-row style encoder, whose 1024-wide layers are
    #  split-contraction launches of the 128-row kernel.  The kernel lab says -9 .. -40 % per launch there, the C4 step says 374.6 -> 378.8 / 384.5 ms:
    #  profiles/r06_mid_rows_ab.jsonl, profiles/r06_small_linear_lab_m1536.txt)
    if M > SMALL_M_ROWS and narrow_n_kernel(M, N, K):
        return 5
    if not RING_DISPATCH or M < 2048:
        return 0
    return (_RING_SHAPES if M >= 4096 else _RING_SHAPES_MID).get(LINEAR_MODE, {}).get((N, K), 0)


def _launch_linear(a2: Tensor, weight: Optional[Tensor], out: Tensor, M: int, N: int, K: int, cfg: int, *, image: Optional[Tensor] = None, transposed: bool = False,
                   bias: Optional[Tensor] = None, residual: Optional[Tensor] = None, pre: Optional[Tensor] = None, act: int = 0,
                   operand_word: Optional[Tensor] = None, want_word: bool = False, count: Optional[str] = "linear_x6r", what: str = "") -> Optional[Tensor]:
    """THE x6 launch of a Linear: out (M, N) = [residual +] act(a2 (M, K) . W^T + bias), M / N / K as the kernel sees them, on the kernel of `cfg`
    (`_linear_cfg`) and the image that kernel reads, in the order the library's per-thread |max| words need (f16x3): the weight image FIRST
    (a lazy split announces and consumes the weight's word itself), then the activation's `operand_word` (None outside f16x3), then --
    `want_word` -- a zeroed word for the |max| of what the epilogue stores (returned: the caller links or publishes it), then the launch.
    transposed: the input-gradient GEMM (a2 = dY, out = dX, residual = the pre-activation of act 2).  image: a block image the caller holds
    (`linear_x6r`).  count: the CALLS key of a block-image launch.  Allocates and reshapes nothing."""
    if want_word and cfg == 2:
        raise ValueError("vit_linear_x6r_fwd cfg 2 cannot publish its output's |max| (include/vit_ops.h)")
    wp = image if image is not None else _linear_image(weight, cfg != 0, transposed)
    if operand_word is not None:
        _announce(operand_word)
    word = _output_amax_word(a2.device) if want_word else None
    b, r, p = bias.data_ptr() if bias is not None else None, residual.data_ptr() if residual is not None else None, pre.data_ptr() if pre is not None else None
    if cfg:
        if count is not None:
            CALLS[count] = CALLS.get(count, 0) + 1
        rc = load().vit_linear_x6r_fwd(a2.data_ptr(), wp.data_ptr(), b, r, out.data_ptr(), p, M, N, K, act, cfg, _stream(a2.device))
    else:
        rc = load().vit_linear_x6_fwd(a2.data_ptr(), wp.data_ptr(), b, r, out.data_ptr(), p, M, N, K, act, _stream(a2.device))
    if rc:
        _check(rc, ("vit_linear_x6r_fwd" if cfg else "vit_linear_x6_fwd") + what)
    return word


class _FusedLinear(torch.autograd.Function):
    """forward on the hand-written MFMA kernels (f32 or bf16x6); backward in bf16x6 mode: dX with the pre-split transposed
    weight, dW = dY^T X and db in one split-M pass (vit_linear_x6_wgrad); in f32 mode the backward GEMMs are plain library
    GEMMs through torch / hipBLASLt."""

    @staticmethod
    def forward(ctx, x, weight, bias, residual, act, link=None, link_in=None, amax_out=False, amax_dx=False):
        _need_gpu(x, "linear")
        shp = x.shape
        x2 = x.reshape(-1, shp[-1]).contiguous().float()
        M, K = x2.shape
        N = weight.shape[0]
        out = torch.empty((M, N), dtype=torch.float32, device=x.device)
        need_pre = act == 1 and (x.requires_grad or weight.requires_grad)
        pre = torch.empty_like(out) if need_pre else None
        res2 = residual.reshape(-1, N).contiguous().float() if residual is not None else None
        b = bias.contiguous().float() if bias is not None else None
        x6 = _x6()
        w = weight.contiguous().float()
        ctx.ax = None
        ctx.amax_dx = bool(amax_dx)
        if x6:
            cfg = _linear_cfg(M, N, K)
            if (PAIR_SPLIT and x.requires_grad and N % 16 == 0 and K % 8 == 0
                    and _SPLIT_CACHE.get(_image_key(weight, _LINEAR_LAYOUTS[2 * (cfg != 0)]), weight) is None):
                # the forward image is stale (the optimizer stepped): the backward's input-gradient GEMM will need the transposed image of the
                # same values -- both in one launch, each in the layout the route of its launch reads
                split_weight_pair(weight, cfg != 0, _linear_cfg(M, N, K, dx=True) != 0)
            # f16x3: |max| of the input (shared with the weight-gradient launch).  An fc2 takes the word its fc1's epilogue filled (GeluLink.ax)
            # instead of a pass over the (M, 4 C) hidden activation; an fc1 asks its own epilogue for that word (to_link).
            # amax_out: the consumer of this layer's output wants its |max| (the attention kernels in f16x3: q, k, v scales) -- the epilogue publishes it
            to_link = to_publish = False
            if _f16():
                ctx.ax = link_in.ax if (link_in is not None and link_in.ax is not None) else _amax_of(x2)
                to_link = link is not None and need_pre
                to_publish = not to_link and amax_out and PUBLISH_AMAX and act == 0
            word = _launch_linear(x2, weight, out, M, N, K, cfg, bias=b, residual=res2, pre=pre, act=int(act), operand_word=ctx.ax,
                                  want_word=to_link or to_publish)
            if to_link:
                link.ax = word
            elif to_publish:
                _publish(out, word)
        else:
            _check(load().vit_linear_fwd(x2.data_ptr(), w.data_ptr(), b.data_ptr() if b is not None else None,
                                         res2.data_ptr() if res2 is not None else None, out.data_ptr(), pre.data_ptr() if pre is not None else None,
                                         M, N, K, int(act), _stream(x.device)), "vit_linear_fwd")
        ctx.save_for_backward(x2, w, pre)
        # GeluLink: `link` (this layer applies the GELU) publishes its pre-activation; `link_in` (this layer consumes that GELU's
        # output) lets the backward run GELU' inside its input-gradient GEMM -- see GeluLink
        ctx.link, ctx.link_in = (link if (x6 and need_pre) else None), (link_in if x6 else None)
        if ctx.link is not None:
            ctx.link.pre, ctx.link.fused = pre, False
        ctx.mode = LINEAR_MODE
        ctx.weight_ref = weight if x6 else None
        ctx.weight_version = weight._version      # dX re-splits the LIVE parameter: it must still be the forward's value
        ctx.bias_ref = bias if x6 else None
        ctx.meta = (shp, bias is not None, residual is not None, act)
        return out.reshape(*shp[:-1], N)

    @staticmethod
    def backward(ctx, g):
        x2, w, pre = ctx.saved_tensors
        shp, has_bias, has_res, act = ctx.meta
        _pin_products(ctx.mode)
        if ctx.weight_ref is not None and ctx.weight_ref._version != ctx.weight_version:
            raise RuntimeError("fused Linear: the weight was modified in place between forward and backward (optimizer step / "
                               "EMA under retain_graph?); dX would be computed with the new value")
        g2 = g.reshape(-1, g.shape[-1])
        g_res = g if has_res else None
        if act == 1 and not (ctx.link is not None and ctx.link.fused):     # (fused: the layer behind already multiplied by GELU')
            g2 = torch.ops.aten.gelu_backward(g2.contiguous(), pre, approximate="none")
        need_x, need_w, need_b = ctx.needs_input_grad[0], ctx.needs_input_grad[1], ctx.needs_input_grad[2]
        f16 = ctx.mode == "f16x3" and ctx.weight_ref is not None
        ag = None                                              # f16x3: |max| of dY, one pass shared by the dX and the dW launch

        if f16 and act == 1 and ctx.link is not None and ctx.link.fused and ctx.link.adx is not None:
            ag = ctx.link.adx                                  # this fc1's dY came out of fc2's input-gradient GEMM, which published its |max|

        def amax_g(t):
            nonlocal ag
            if ag is None:
                ag = _amax_of(t)
            return ag

        dx = None
        if need_x:
            N, K = w.shape
            if ctx.weight_ref is not None and N % 16 == 0:
                g2c = g2.contiguous().float()
                M = g2c.shape[0]
                dx = torch.empty((M, K), dtype=torch.float32, device=g.device)
                lk = ctx.link_in
                gelu_pre = lk.pre if (lk is not None and lk.pre is not None and tuple(lk.pre.shape) == (M, K)) else None
                # f16x3, the |max| of what the epilogue stores: behind a GELU those values ARE fc1's dY (GeluLink.adx); amax_dx: proj's input
                # gradient is the attention backward's dO, whose scale comes from the published word
                want = f16 and (gelu_pre is not None or (ctx.amax_dx and PUBLISH_AMAX))
                word = _launch_linear(g2c, ctx.weight_ref, dx, M, K, N, _linear_cfg(M, N, K, dx=True, mode=ctx.mode), transposed=True,
                                      residual=gelu_pre, act=2 if gelu_pre is not None else 0, operand_word=amax_g(g2c) if f16 else None,
                                      want_word=want, what=" (dX)")
                if gelu_pre is not None:
                    lk.fused = True
                    if want:
                        lk.adx = word
                elif want:
                    _publish(dx, word)
                dx = dx.reshape(shp)
            else:
                dx = (g2 @ w).reshape(shp)
        dw = db = None
        wslot = getattr(ctx.weight_ref, "_grad_slot", None) if ctx.weight_ref is not None else None
        if need_w and wslot is not None:
            # In-place gradients (ddp.BucketedGradReducer.prepare): dW / db are ACCUMULATED straight into the parameter's
            # zeroed slice of its all-reduce bucket -- no per-layer memset, no pack copy afterwards.  The first use of
            # a parameter in this backward hands the slice to autograd as its gradient; later uses (two encoder passes
            # share the weights) have already added into the same memory and return None.
            g2c = g2.contiguous().float()
            N, K = w.shape
            bslot = getattr(ctx.bias_ref, "_grad_slot", None) if (has_bias and need_b and ctx.bias_ref is not None) else None
            if f16:
                _announce(amax_g(g2c), ctx.ax)
            _check(load().vit_linear_x6_wgrad_acc(g2c.data_ptr(), x2.data_ptr(), wslot["view"].data_ptr(),
                                                  bslot["view"].data_ptr() if bslot is not None else None, g2c.shape[0], N, K,
                                                  _stream(g.device)), "vit_linear_x6_wgrad_acc")
            if not wslot["used"]:
                wslot["used"] = True
                dw = wslot["view"].detach()          # a fresh alias: autograd can adopt it as .grad without cloning
            if bslot is not None and not bslot["used"]:
                bslot["used"] = True
                db = bslot["view"].detach()
            if has_bias and need_b and bslot is None:
                db = g2.sum(0)
            return dx, dw, db, g_res, None, None, None, None, None
        if need_w and ctx.weight_ref is not None:         # dW (+ db in the same pass) on the bf16x6 kernel
            g2c = g2.contiguous().float()
            N, K = w.shape
            want_b = has_bias and need_b
            buf = torch.empty(N * K + (N if want_b else 0), dtype=torch.float32, device=g.device)   # db right behind dw: one memset
            dw = buf[:N * K].view(N, K)
            db = buf[N * K:] if want_b else None
            if f16:
                _announce(amax_g(g2c), ctx.ax)
            _check(load().vit_linear_x6_wgrad(g2c.data_ptr(), x2.data_ptr(), dw.data_ptr(), db.data_ptr() if want_b else None,
                                              g2c.shape[0], N, K, _stream(g.device)), "vit_linear_x6_wgrad")
        else:
            dw = g2.t() @ x2 if need_w else None          # frozen layers (style stage) skip the weight GEMM
        if db is None and has_bias and need_b:
            db = g2.sum(0)
        return dx, dw, db, g_res, None, None, None, None, None


SMALL_M_ROWS = int(os.environ.get("VIT_SMALL_M_ROWS", "1024"))      # launches of up to this many rows take csrc/vit_gemm_sm.hip; 0 = the kernel is off at every M (A/B switch)
NARROW_N = int(os.environ.get("VIT_NARROW_N", "768"))               # ... and launches of ANY row count whose output is at most this wide (0 = off): see _linear_cfg
_SMALL_M_SET: dict = {}                                              # host thread -> the max_rows this thread last told the library


def small_m_kernel(M: int, N: int, K: int) -> bool:
    """does this shape run on the small-M kernel (vit_linear_x6r_fwd cfg 5) at batch-1 row counts?  (also keeps the library's per-thread switch in
    step with SMALL_M_ROWS, which tests and benchmarks flip at run time)"""
    _sync_small_m()
    return SMALL_M_ROWS > 0 and M <= SMALL_M_ROWS and bool(load().vit_linear_sm_ok(M, N, K))


def narrow_n_kernel(M: int, N: int, K: int) -> bool:
    """the same kernel at the train step's row counts, for NARROW outputs (the decoders' 768-wide proj / projq / projk / projv / fc2 and the
    input-gradient GEMMs of their qkv / fc1): 128-wide tiles leave the chip under-filled there and the barrier-free kernel is 30 % faster
    (M = 2 570, f16x3: 768 x 768 37 -> 25 us, 768 x 3072 95 -> 67 us; profiles/r06_small_linear_lab_big.jsonl); wider layers stay on the ring kernels"""
    _sync_small_m()
    return SMALL_M_ROWS > 0 and 0 < N <= NARROW_N and M > SMALL_M_ROWS and bool(load().vit_linear_sm_ok(M, N, K))


def _sync_small_m() -> None:
    tid = threading.get_ident()
    if _SMALL_M_SET.get(tid) != SMALL_M_ROWS:
        _check(load().vit_linear_sm_set((1 << 24) if SMALL_M_ROWS > 0 else 0, 0, 0), "vit_linear_sm_set")       # (the row-count policy lives here)
        _SMALL_M_SET[tid] = SMALL_M_ROWS


class GeluLink:
    """Ties the two Linear layers of an Mlp (fc1 -> GELU -> fc2, blocks.py:76-82) together for the backward: fc1's node publishes
    the GELU's pre-activation here, fc2's node -- whose input-gradient GEMM produces exactly the gradient of the GELU's output -- runs
    GELU'(pre) in that GEMM's epilogue (vit_linear_x6_fwd act = 2) and sets `fused`; fc1's node then skips its GeluBackward pass.  Valid
    only when the GELU's output feeds NOTHING but that fc2 (true inside Mlp: the hidden tensor is local to its forward).
    In f16x3 mode the link also carries two |max| words that the producing GEMMs' epilogues fill on the side (vit_x6_set_output_amax): `ax` for
    the hidden activation (fc1 publishes it, fc2 needs it for its input scale) and `adx` for its gradient (fc2's input-gradient GEMM publishes
    it, fc1's backward needs it) -- the two largest operands of a block then cost no vit_amax pass."""
    __slots__ = ("pre", "fused", "ax", "adx")

    def __init__(self):
        self.pre, self.fused, self.ax, self.adx = None, False, None, None


def fused_linear(x: Tensor, weight: Tensor, bias: Optional[Tensor] = None, residual: Optional[Tensor] = None,
                 gelu: bool = False, link: Optional[GeluLink] = None, link_in: Optional[GeluLink] = None,
                 amax_out: bool = False, amax_dx: bool = False) -> Tensor:
    """[residual +] [gelu](x @ weight.T + bias) in one kernel (vit_linear_fwd).  link / link_in: see GeluLink.
    amax_out / amax_dx (f16x3): publish the |max| of the output / of the input gradient from the producing GEMM's epilogue -- the attention
    kernels take their operand scales from those words (qkv, projq / projk / projv outputs; proj's input gradient = the attention's dO)."""
    if not torch.is_grad_enabled() and _x6() and x.is_cuda and x.dtype == torch.float32:
        # serving path: no autograd node, no saved tensors, straight to the kernel
        shp = x.shape
        x2 = x.reshape(-1, shp[-1])
        if not x2.is_contiguous():
            x2 = x2.contiguous()
        M, K = x2.shape
        N = weight.shape[0]
        out = torch.empty((M, N), dtype=torch.float32, device=x.device)
        res2 = None
        if residual is not None:
            res2 = residual.reshape(-1, N)
            if not res2.is_contiguous() or res2.dtype != torch.float32:
                res2 = res2.contiguous().float()
        cfg = _linear_cfg(M, N, K, serving=True)
        # f16x3: the small-M kernel (csrc/vit_gemm_sm.hip) runs the whole epilogue in one launch, GELU included: every output gets its |max| word
        # for free (the next Linear / the attention finds it published); the 128-row kernel publishes un-activated outputs on request
        f16 = _f16()
        ow = _launch_linear(x2, weight, out, M, N, K, cfg, bias=bias, residual=res2, act=1 if gelu else 0, operand_word=_amax_of(x2) if f16 else None,
                            want_word=f16 and PUBLISH_AMAX and ((amax_out and not gelu) or cfg != 0), count="linear_sm",
                            what=" (small M)" if cfg else "")
        if ow is not None:
            _publish(out, ow)
        return out.reshape(*shp[:-1], N)
    return _FusedLinear.apply(x, weight, bias, residual, 1 if gelu else 0, link, link_in, amax_out, amax_dx)


# --------------------------------------------------------------------------- two problems per launch (serving path of the dual decoders)
def _ptr_array(ptrs):
    return (C.c_void_p * len(ptrs))(*[C.c_void_p(p) if p else None for p in ptrs])


def grouped_shape_ok(M: int, N: int, K: int) -> bool:
    """serving path: can two (M, K) x (N, K)^T problems run in one vit_linear_sm_grouped launch?"""
    return not torch.is_grad_enabled() and LINEAR_MODE != "f32" and _x6() and small_m_kernel(M, N, K)


def grouped_ok(x: Tensor, N: int) -> bool:
    """... for a (2, ..., K) stacked device input and N output features"""
    return (x.is_cuda and x.dtype == torch.float32 and x.dim() >= 2 and x.shape[0] == 2 and x.is_contiguous()
            and grouped_shape_ok(x.numel() // (2 * x.shape[-1]), N, x.shape[-1]))


def grouped_linear(x: Tensor, layers, residual: Optional[Tensor] = None, gelu: bool = False, flip: bool = False) -> Tensor:
    """Serving path, no autograd.  x: (2, ..., K) contiguous, the inputs of two layers of ONE shape stacked; group g runs layers[g] on x[g]
    (flip: on x[1 - g] -- the memory of a decoder is the other decoder's features) and writes out[g]: (2, ..., N) = [residual +]
    [gelu](x_g . W_g^T + b_g) in one launch of the small-M kernel (vit_linear_sm_grouped).  f16x3: one |max| word for the stacked input, one
    published for the stacked output."""
    assert grouped_ok(x, layers[0].out_features), "grouped_linear: check grouped_ok first"
    K = x.shape[-1]
    M = x.numel() // (2 * K)
    N = layers[0].out_features
    assert layers[1].out_features == N and layers[0].in_features == K == layers[1].in_features and x.is_contiguous()
    out = torch.empty((2, *x.shape[1:-1], N), dtype=torch.float32, device=x.device)
    res = None
    if residual is not None:
        res = residual if (residual.is_contiguous() and residual.dtype == torch.float32) else residual.contiguous().float()
        assert res.numel() == out.numel()
    wps = [split_weight_block(l.weight) for l in layers]
    ow = None
    if _f16():
        _announce(_amax_of(x))
        if PUBLISH_AMAX:
            ow = _output_amax_word(x.device)
    xb, ob, eb = x.data_ptr(), out.data_ptr(), 4
    xs = [xb + (1 if flip else 0) * M * K * eb, xb + (0 if flip else 1) * M * K * eb]
    os_ = [ob, ob + M * N * eb]
    rs = [res.data_ptr(), res.data_ptr() + M * N * eb] if res is not None else [None, None]
    bs = [l.bias.data_ptr() if l.bias is not None else None for l in layers]
    CALLS["linear_sm_grouped"] = CALLS.get("linear_sm_grouped", 0) + 1
    _check(load().vit_linear_sm_grouped(_ptr_array(xs), _ptr_array([w.data_ptr() for w in wps]), _ptr_array(bs), _ptr_array(rs), _ptr_array(os_),
                                        2, M, N, K, 1 if gelu else 0, _stream(x.device)), "vit_linear_sm_grouped")
    if ow is not None:
        _publish(out, ow)
    return out


def grouped_layernorm(x: Tensor, norms, flip: bool = False) -> Tensor:
    """Serving path.  x: (2, ..., C) contiguous; out[g] = norms[g](x[g]) (flip: of x[1 - g]) in one launch (vit_layernorm_fwd_grouped: the
    arithmetic of vit_layernorm_fwd).  norms[g] may be nn.Identity (both or none)."""
    if isinstance(norms[0], nn.Identity):
        assert isinstance(norms[1], nn.Identity)
        return torch.stack((x[1], x[0])) if flip else x
    Cn = x.shape[-1]
    M = x.numel() // (2 * Cn)
    assert x.is_contiguous() and x.dtype == torch.float32 and x.is_cuda and all(n._hip_ok(x) for n in norms)
    y = torch.empty_like(x)
    pub = _want_output_amax(x.device)
    xb, yb = x.data_ptr(), y.data_ptr()
    xs = [xb + (1 if flip else 0) * M * Cn * 4, xb + (0 if flip else 1) * M * Cn * 4]
    CALLS["layernorm_hip_fwd"] += 1
    _check(load().vit_layernorm_fwd_grouped(_ptr_array(xs), _ptr_array([n.weight.data_ptr() for n in norms]),
                                            _ptr_array([n.bias.data_ptr() if n.bias is not None else None for n in norms]),
                                            _ptr_array([yb, yb + M * Cn * 4]), 2, M, Cn, float(norms[0].eps), _stream(x.device)),
           "vit_layernorm_fwd_grouped")
    if pub is not None:
        _publish(y, pub)
    return y


# --------------------------------------------------------------------------- LayerNorm (E2, E5, E6: norm1..3, norm_y, enc/dec_norm)
class _LayerNormHip(torch.autograd.Function):
    """y = LayerNorm(x) on vit_layernorm_fwd / vit_layernorm_bwd.  with_skip: also returns x itself as a second output for
    the block's residual branch; the backward then receives the skip gradient together with dy and adds it inside the
    kernel (dx = dskip + LN'(dy)) instead of leaving an (M, C) add to the autograd engine."""

    @staticmethod
    def forward(ctx, x, weight, bias, eps, with_skip):
        _need_gpu(x, "layer_norm")
        ctx.set_materialize_grads(False)
        Cn = x.shape[-1]
        xc = x.contiguous().float()
        M = xc.numel() // Cn
        y = torch.empty_like(xc)
        stats = torch.empty((2, M), dtype=torch.float32, device=x.device)
        pub = _want_output_amax(x.device)                     # f16x3: the Linear layers that read y take their scale from this word
        _check(load().vit_layernorm_fwd(xc.data_ptr(), weight.data_ptr(), bias.data_ptr() if bias is not None else None, y.data_ptr(),
                                        stats[0].data_ptr(), stats[1].data_ptr(), M, Cn, float(eps), _stream(x.device)), "vit_layernorm_fwd")
        if pub is not None:
            _publish(y, pub)
        ctx.save_for_backward(xc, weight, stats)
        ctx.has_bias, ctx.with_skip = bias is not None, bool(with_skip)
        if with_skip:
            return y, x.view_as(x)
        return y

    @staticmethod
    def backward(ctx, g, gskip=None):
        xc, weight, stats = ctx.saved_tensors
        Cn = xc.shape[-1]
        M = xc.numel() // Cn
        dev = xc.device
        if g is None:                       # only the skip branch received a gradient
            return gskip, None, None, None, None
        g = g.contiguous().float()
        gs = gskip.contiguous().float() if gskip is not None else None
        CALLS["layernorm_hip_bwd"] += 1
        dx = torch.empty_like(xc)
        dwb = torch.empty((2, Cn), dtype=torch.float32, device=dev)
        scratch = torch.empty(load().vit_layernorm_scratch_bytes(M, Cn), dtype=torch.uint8, device=dev)
        pub = _want_output_amax(dev)                          # f16x3: dx is the dY of the Linear layer in front of this block
        _check(load().vit_layernorm_bwd(g.data_ptr(), xc.data_ptr(), stats[0].data_ptr(), stats[1].data_ptr(), weight.data_ptr(),
                                        gs.data_ptr() if gs is not None else None, dx.data_ptr(), dwb[0].data_ptr(),
                                        dwb[1].data_ptr(), scratch.data_ptr(), M, Cn, 0, _stream(dev)), "vit_layernorm_bwd")
        if pub is not None:
            _publish(dx, pub)
        return dx, dwb[0], (dwb[1] if ctx.has_bias else None), None, None


class LayerNorm(nn.LayerNorm):
    """nn.LayerNorm (same parameters / state_dict keys) whose forward and backward run on the HIP kernels for device fp32
    inputs with C % 256 == 0, C <= 2048 (the trunks' 1024 / 768); anything else takes the framework path.
    `forward_skip(x) -> (LN(x), x)`: the second output is x for the residual branch of a pre-norm block, so that the two
    gradients of x meet inside vit_layernorm_bwd."""

    def _hip_ok(self, x: Tensor) -> bool:
        Cn = x.shape[-1]
        return (x.is_cuda and x.dtype == torch.float32 and len(self.normalized_shape) == 1 and self.weight is not None
                and Cn % 256 == 0 and Cn <= 2048 and x.numel() > 0)

    def forward(self, x: Tensor) -> Tensor:
        if self._hip_ok(x):
            CALLS["layernorm_hip_fwd"] += 1
            if not torch.is_grad_enabled():          # serving path: no autograd node
                xc = x if x.is_contiguous() else x.contiguous()
                Cn = xc.shape[-1]
                M = xc.numel() // Cn
                y = torch.empty_like(xc)
                stats = torch.empty((2, M), dtype=torch.float32, device=x.device)
                pub = _want_output_amax(x.device)
                _check(load().vit_layernorm_fwd(xc.data_ptr(), self.weight.data_ptr(),
                                                self.bias.data_ptr() if self.bias is not None else None, y.data_ptr(),
                                                stats.data_ptr(), stats.data_ptr() + 4 * M, M, Cn, float(self.eps),
                                                _stream(x.device)), "vit_layernorm_fwd")
                if pub is not None:
                    _publish(y, pub)
                return y
            return _LayerNormHip.apply(x, self.weight, self.bias, self.eps, False)
        CALLS["layernorm_framework"] += 1
        return super().forward(x)

    def forward_skip(self, x: Tensor):
        if self._hip_ok(x) and torch.is_grad_enabled() and x.requires_grad:
            CALLS["layernorm_hip_fwd"] += 1
            return _LayerNormHip.apply(x, self.weight, self.bias, self.eps, True)
        return self.forward(x), x
