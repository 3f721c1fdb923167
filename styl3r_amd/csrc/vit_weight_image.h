// vit_weight_image.h -- the packed weight image every Linear and convolution of the split-arithmetic path reads, described ONCE: where its
// bytes lie (host and device), and the device pieces every kernel that writes one is made of (vit_weight_image.hip).
//
// An image holds the pieces of an (R, Kc) fp32 matrix -- R output rows, Kc the contraction length, Kc % 8 == 0 -- in groups of eight
// consecutive k, three 16-byte slots per group: three bf16 pieces ("bf16x6" and "bf16x3": the same image), or two fp16 pieces of
// value x f16_scale_of(|max|) in slots 0 / 1 ("f16x3"; slot 2 is neither written nor read).  Two layouts:
//     row     [row][k / 8][piece][8]                 the MFMA operand order of vit_gemm_x6.hip
//     block   [row / 64][k / 8][piece][row % 64][8]  rows padded to a multiple of 64 with zero pieces: one (k group, piece) plane of 64 rows is
//                                                    1 KiB of contiguous memory, a DMA chunk of vit_gemm_x6r.hip / vit_gemm_sm.hip
// Right behind the pieces sits a copy of the weight's |max| word (vit_common.h: 64 slots, 8 KiB), from which the f16x3 readers take their
// inverse scale.  tests/weight_image_cases.py restates the bytes in torch.
#pragma once
#include "vit_common.h"

namespace vit {
namespace image {
constexpr size_t WORD_BYTES = 64 * AMAX_WORD_STRIDE * sizeof(uint32_t);

__host__ __device__ inline size_t piece_bytes(int R, int Kc, bool block)
{
    return (size_t)(block ? (R + 63) / 64 * 64 : R) * (size_t)Kc * 6;
}
__host__ __device__ inline size_t total_bytes(int R, int Kc, bool block) { return piece_bytes(R, Kc, block) + WORD_BYTES; }
__host__ __device__ inline const uint32_t *tail_word(const void *packed, int R, int Kc, bool block)
{
    return reinterpret_cast<const uint32_t *>(static_cast<const char *>(packed) + piece_bytes(R, Kc, block));
}
__host__ __device__ inline uint32_t *tail_word(void *packed, int R, int Kc, bool block)
{
    return reinterpret_cast<uint32_t *>(static_cast<char *>(packed) + piece_bytes(R, Kc, block));
}

// ---- the writer: F16 = two fp16 pieces of the scaled value, else three bf16 pieces --------------------------------------------------------
// Preamble of every image kernel (all lanes of whole waves call it): the workgroup for which `first` holds copies the announced |max| word
// into the tail(s); returns the scale of the pieces.  (No __restrict__: vit_split_weight's self-computed word IS the tail.)
template <bool F16>
__device__ inline float preamble(const uint32_t *amax, bool first, uint32_t *tail, uint32_t *tail2 = nullptr)
{
    if constexpr (F16) {
        if (first && threadIdx.x < 64) {
            const uint32_t a = amax[threadIdx.x * AMAX_WORD_STRIDE];
            tail[threadIdx.x * AMAX_WORD_STRIDE] = a;
            if (tail2) tail2[threadIdx.x * AMAX_WORD_STRIDE] = a;
        }
        return f16_scale_of(amax_word_read(amax));
    } else {
        return 1.f;
    }
}

// eight values (lo, hi) -> the pieces of k group `kg` of `row`, in an image with KG k groups per row
template <bool F16>
__device__ inline void store_group(uint4 *__restrict__ packed, bool block, int row, int kg, int KG, const float4 &lo, const float4 &hi, float sw)
{
    uint4 q0, q1, q2;
    split8s<F16 ? 2 : 6>(lo, hi, sw, q0, q1, q2);
    uint4 *o = packed + (block ? (((int64_t)(row >> 6) * KG + kg) * 3) * 64 + (row & 63) : ((int64_t)row * KG + kg) * 3);
    const int step = block ? 64 : 1;
    o[0] = q0; o[step] = q1;
    if constexpr (!F16) o[2 * step] = q2;
}

// The 64 x 64 tile of w (rows, cols) at (r0, c0) -> s[row][column], zeros outside w; the index that runs along consecutive threads runs along
// the rows of w (coalesced), four columns per load where the rows are 16-byte aligned.
typedef float Tile[64][65];
__device__ inline void stage_tile(Tile &s, const float *__restrict__ w, int rows, int cols, int r0, int c0)
{
    if ((cols & 3) == 0 && (reinterpret_cast<uintptr_t>(w) & 15) == 0) {
        for (int i = threadIdx.x; i < 64 * 16; i += 256) {
            const int r = i >> 4, c4 = (i & 15) * 4;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (r0 + r < rows && c0 + c4 < cols) v = *reinterpret_cast<const float4 *>(w + (int64_t)(r0 + r) * cols + c0 + c4);
            s[r][c4] = v.x; s[r][c4 + 1] = v.y; s[r][c4 + 2] = v.z; s[r][c4 + 3] = v.w;
        }
    } else {
        for (int i = threadIdx.x; i < 64 * 64; i += 256) {
            const int r = i >> 6, c = i & 63;
            s[r][c] = (r0 + r < rows && c0 + c < cols) ? w[(int64_t)(r0 + r) * cols + c0 + c] : 0.f;
        }
    }
}

// A staged tile -> the 64 rows x 8 k groups of an (R, Kc) image that start at (row0, k group kg0).  transposed = 0: image row = tile row, k
// along the tile's columns; 1: image row = tile column, k along its rows (the image of w^T).  Consecutive threads write consecutive rows of one
// plane (block layout) or consecutive k groups of one row (row layout: 48 contiguous bytes each).  The block layout's padding rows are
// written (the tile holds zeros there), the row layout has none.
template <bool F16>
__device__ inline void emit_tile(const Tile &s, uint4 *__restrict__ packed, bool block, bool transposed, int row0, int kg0, int R, int Kc, float sw)
{
    for (int i = threadIdx.x; i < 8 * 64; i += 256) {
        const int kg = block ? (i >> 6) : (i & 7), r = block ? (i & 63) : (i >> 3), k = kg * 8;
        if ((kg0 + kg) * 8 >= Kc || (!block && row0 + r >= R)) continue;
        const float4 lo = transposed ? make_float4(s[k + 0][r], s[k + 1][r], s[k + 2][r], s[k + 3][r]) : make_float4(s[r][k + 0], s[r][k + 1], s[r][k + 2], s[r][k + 3]);
        const float4 hi = transposed ? make_float4(s[k + 4][r], s[k + 5][r], s[k + 6][r], s[k + 7][r]) : make_float4(s[r][k + 4], s[r][k + 5], s[r][k + 6], s[r][k + 7]);
        store_group<F16>(packed, block, row0 + r, kg0 + kg, Kc >> 3, lo, hi, sw);
    }
}

// One 64-row x 64-k tile (number `local` of the job's nbx x ceil(R / 64)) of one image of one weight: kind bit 0 = the image of w^T, bit 1 =
// the block layout (include/vit_ops.h VitSplitJob).
template <bool F16>
__device__ inline void write_job_tile(const VitSplitJob &jb, uint32_t local, Tile &s)
{
    const bool transposed = jb.kind & 1, block = jb.kind & 2;
    const int k0 = (int)(local % jb.nbx) * 64, row0 = (int)(local / jb.nbx) * 64;          // of the image
    const float sw = preamble<F16>(jb.amax, local == 0, jb.tail);
    stage_tile(s, jb.w, jb.rows, jb.cols, transposed ? k0 : row0, transposed ? row0 : k0);
    __syncthreads();
    emit_tile<F16>(s, static_cast<uint4 *>(jb.packed), block, transposed, row0, k0 >> 3, transposed ? jb.cols : jb.rows,
                   transposed ? jb.rows : jb.cols, sw);
}
}  // namespace image
}  // namespace vit
