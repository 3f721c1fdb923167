// vit_weight_image.hip -- the kernels that write packed weight images and their host entries.  Layout, preamble, store, staging and the emit
// loop are vit_weight_image.h's; a kernel here only says which tiles of which weight go into which image.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vit_internal.h"
#include "vit_weight_image.h"

namespace vit {
namespace image {
// All the weight images of a model in ONE launch (after an optimizer step every weight changed: one launch per image was 1 274 launches and
// 12 ms of a 285 ms train step at 1.4 TB/s -- launch-bound).  A job = one image of one weight; a workgroup = one 64-row x 64-k tile of one job
// (binary search over the jobs' first-block table).
template <bool F16>
__global__ void __launch_bounds__(256) k_split_many(const VitSplitJob *__restrict__ jobs, int njobs)
{
    int lo = 0, hi = njobs - 1;                        // last job whose first_block <= blockIdx.x
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (jobs[mid].first_block <= blockIdx.x) lo = mid; else hi = mid - 1;
    }
    const VitSplitJob jb = jobs[lo];
    __shared__ Tile s;
    write_job_tile<F16>(jb, blockIdx.x - jb.first_block, s);
}

// One image of one weight (the lazy path: first use of a weight, frozen weights, the convolutions' rearranged copies): the same body, the
// job by value.
template <bool F16>
__global__ void __launch_bounds__(256) k_split_one(const VitSplitJob jb)
{
    __shared__ Tile s;
    write_job_tile<F16>(jb, blockIdx.x, s);
}

// BOTH images of one Linear weight in one launch: the forward image (rows = rows of w) and the transposed one for the input-gradient GEMM
// (rows = columns of w), each in its own layout.  After an optimizer step every trainable weight needs both again; a workgroup stages one
// 64 x 64 tile of w -- a tile of either image -- and emits it twice: the fp32 weight is read once.
template <bool F16>
__global__ void __launch_bounds__(256) k_split_pair(const float *__restrict__ w, uint4 *__restrict__ pf, uint4 *__restrict__ pt, int rows, int cols,
                                                    int block_f, int block_t, const uint32_t *amax, uint32_t *tail_f, uint32_t *tail_t)
{
    __shared__ Tile s;
    const int r0 = blockIdx.y * 64, c0 = blockIdx.x * 64;
    const float sw = preamble<F16>(amax, blockIdx.x == 0 && blockIdx.y == 0, tail_f, tail_t);
    stage_tile(s, w, rows, cols, r0, c0);
    __syncthreads();
    emit_tile<F16>(s, pf, block_f, false, r0, c0 >> 3, rows, cols, sw);
    emit_tile<F16>(s, pt, block_t, true, c0, r0 >> 3, cols, rows, sw);
}

// Both operand images of a convolution weight w (Co, Ci, k, k) straight from the parameter, in ONE launch (before: a permute + clone, a flip,
// a second permute + clone and two split launches per weight and optimizer step -- ~290 framework copy launches of a C3 step):
//   forward image  rows = co, column = tap * Ci + ci               value w[co][ci][tap]                 (vit_conv_x6_fwd's weight)
//   dX image       rows = ci, column = tap * Co + co               value w[co][ci][k*k - 1 - tap]       (spatially flipped, channel-transposed)
// both in the row layout.  A workgroup owns 16 output channels x 16 input channels x all taps: each of the two images' 8-wide k groups (8
// consecutive ci at one (co, tap) / 8 consecutive co at one (ci, tap)) lies inside it.  pdx may be null (forward image only).
constexpr int CW_T = 16, CW_TAPS_MAX = 9;
template <bool F16>
__global__ void __launch_bounds__(256) k_split_conv_pair(const float *__restrict__ w, uint4 *__restrict__ pf, uint4 *__restrict__ pdx, int Co, int Ci, int kk,
                                                         const uint32_t *amax, uint32_t *tail_f, uint32_t *tail_dx)
{
    const float sw = preamble<F16>(amax, blockIdx.x == 0 && blockIdx.y == 0, tail_f, tail_dx);           // (tail_dx is null with pdx)
    __shared__ float s[CW_T][CW_T * CW_TAPS_MAX + 1];            // [co][ci * kk + tap]
    const int co0 = blockIdx.y * CW_T, ci0 = blockIdx.x * CW_T, run = CW_T * kk;
    for (int i = threadIdx.x; i < CW_T * run; i += 256) {         // per co: CW_T * kk contiguous floats
        const int co = i / run, e = i - co * run;
        const int ci = e / kk;
        s[co][e] = (co0 + co < Co && ci0 + ci < Ci) ? w[((int64_t)(co0 + co) * Ci + ci0) * kk + e] : 0.f;
    }
    __syncthreads();
    const int items = CW_T * kk * (CW_T / 8);
    for (int i = threadIdx.x; i < items; i += 256) {             // forward image
        const int cg = i % (CW_T / 8), t = (i / (CW_T / 8)) % kk, co = i / ((CW_T / 8) * kk);
        if (co0 + co >= Co || ci0 + cg * 8 >= Ci) continue;
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = s[co][(cg * 8 + j) * kk + t];
        store_group<F16>(pf, false, co0 + co, ((t * Ci + ci0) >> 3) + cg, (kk * Ci) >> 3, make_float4(v[0], v[1], v[2], v[3]), make_float4(v[4], v[5], v[6], v[7]), sw);
    }
    if (!pdx) return;
    for (int i = threadIdx.x; i < items; i += 256) {             // input-gradient image
        const int cg = i % (CW_T / 8), t = (i / (CW_T / 8)) % kk, ci = i / ((CW_T / 8) * kk);
        if (ci0 + ci >= Ci || co0 + cg * 8 >= Co) continue;
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = s[cg * 8 + j][ci * kk + (kk - 1 - t)];
        store_group<F16>(pdx, false, ci0 + ci, ((t * Co + co0) >> 3) + cg, (kk * Co) >> 3, make_float4(v[0], v[1], v[2], v[3]), make_float4(v[4], v[5], v[6], v[7]), sw);
    }
}
}  // namespace image

// The modes differ in the pieces (two fp16 / three bf16), not in the product count: bf16x3 reads the bf16x6 image.
static bool f16_images() { return x6_products() == 2; }

int split_weights_many(const VitSplitJob *jobs_dev, int njobs, uint32_t total_blocks, hipStream_t stream)
{
    if (!jobs_dev || njobs <= 0 || total_blocks == 0) return VIT_EINVAL;
    (void)hipGetLastError();
    for_flag(f16_images(), [&](auto f16) { hipLaunchKernelGGL(image::k_split_many<f16.value>, dim3(total_blocks), dim3(256), 0, stream, jobs_dev, njobs); });
    return launch_status();
}

// one image of w (rows, cols) -- of w^T with `transpose` -- through the one-job kernel; `am`: the weight's |max| word (f16x3)
static int split_one(const float *w, void *packed, int rows, int cols, int transpose, bool block, const uint32_t *am, hipStream_t stream)
{
    const int R = transpose ? cols : rows, Kc = transpose ? rows : cols;
    const VitSplitJob jb{w, packed, am, image::tail_word(packed, R, Kc, block), rows, cols, (transpose ? 1 : 0) | (block ? 2 : 0), 0u, (uint32_t)((Kc + 63) / 64), 0u};
    for_flag(f16_images(), [&](auto f16) { hipLaunchKernelGGL(image::k_split_one<f16.value>, dim3(jb.nbx * (uint32_t)((R + 63) / 64)), dim3(256), 0, stream, jb); });
    return launch_status();
}

int split_weight(const float *w, void *packed, int rows, int cols, int transpose, hipStream_t stream)
{
    if (!w || !packed || rows <= 0 || cols <= 0) return VIT_EINVAL;
    if ((transpose ? rows : cols) % 8 != 0) return VIT_EINVAL;
    (void)hipGetLastError();
    // f16x3: the weight's own scale.  The caller may announce the weight's |max| word (vit_x6_set_operand_amax(word, NULL): one vit_amax pass
    // then serves both images of a weight, forward and transposed); otherwise it is computed here into the word behind the pieces
    const uint32_t *am, *unused;
    x6_take_amax(am, unused);
    if (f16_images() && !am) {
        uint32_t *tail = image::tail_word(packed, rows, cols, false);
        if (!zero_fill(tail, image::WORD_BYTES, stream)) { g_last_hip_error = hipGetLastError(); return VIT_ELAUNCH; }
        const int rc = amax(w, (int64_t)rows * cols, tail, stream);
        if (rc != VIT_OK) return rc;
        am = tail;
    }
    return split_one(w, packed, rows, cols, transpose, false, am, stream);
}

int split_weight_block(const float *w, void *packed, int rows, int cols, int transpose, hipStream_t stream)
{
    if (!w || !packed || rows <= 0 || cols <= 0) return VIT_EINVAL;
    if ((transpose ? rows : cols) % 8 != 0) return VIT_EINVAL;
    (void)hipGetLastError();
    // f16x3: the weight's |max| word must be announced (vit_x6_set_operand_amax(word, NULL)); the image keeps a copy right behind its pieces
    const uint32_t *am, *unused;
    x6_take_amax(am, unused);
    if (f16_images() && !am) return VIT_EINVAL;
    return split_one(w, packed, rows, cols, transpose, true, am, stream);
}

// both images of a Linear weight (rows x cols) in one launch: see k_split_pair.  block_f / block_t: the block layout (1) or the row layout (0)
// of the forward / the transposed image.  f16x3: the weight's |max| word must be announced.
int split_weight_pair(const float *w, void *packed_f, void *packed_t, int rows, int cols, int block_f, int block_t, hipStream_t stream)
{
    if (!w || !packed_f || !packed_t || rows <= 0 || cols <= 0 || (rows % 8) != 0 || (cols % 8) != 0) return VIT_EINVAL;
    (void)hipGetLastError();
    const uint32_t *am, *unused;
    x6_take_amax(am, unused);
    if (f16_images() && !am) return VIT_EINVAL;
    uint32_t *tf = image::tail_word(packed_f, rows, cols, block_f), *tt = image::tail_word(packed_t, cols, rows, block_t);
    const dim3 grid((cols + 63) / 64, (rows + 63) / 64);
    for_flag(f16_images(), [&](auto f16) {
        hipLaunchKernelGGL(image::k_split_pair<f16.value>, grid, dim3(256), 0, stream, w, static_cast<uint4 *>(packed_f), static_cast<uint4 *>(packed_t), rows, cols,
                           block_f, block_t, am, tf, tt);
    });
    return launch_status();
}

// the two images of a convolution weight (Co, Ci, k, k), k in {1, 3}: see k_split_conv_pair.  packed_dx may be null.  Ci % 8 == 0; with a dX image
// also Co % 8 == 0.  f16x3: the weight's |max| word must be announced.
int split_conv_weight_pair(const float *w, void *packed_fwd, void *packed_dx, int Co, int Ci, int ksize, hipStream_t stream)
{
    if (!w || !packed_fwd || Co <= 0 || Ci <= 0 || (ksize != 1 && ksize != 3) || (Ci % 8) != 0 || (packed_dx && (Co % 8) != 0)) return VIT_EINVAL;
    (void)hipGetLastError();
    const int kk = ksize * ksize;
    const uint32_t *am, *unused;
    x6_take_amax(am, unused);
    if (f16_images() && !am) return VIT_EINVAL;
    uint32_t *tf = image::tail_word(packed_fwd, Co, kk * Ci, false), *td = packed_dx ? image::tail_word(packed_dx, Ci, kk * Co, false) : nullptr;
    const dim3 grid((Ci + image::CW_T - 1) / image::CW_T, (Co + image::CW_T - 1) / image::CW_T);
    for_flag(f16_images(), [&](auto f16) {
        hipLaunchKernelGGL(image::k_split_conv_pair<f16.value>, grid, dim3(256), 0, stream, w, static_cast<uint4 *>(packed_fwd), static_cast<uint4 *>(packed_dx), Co, Ci, kk,
                           am, tf, td);
    });
    return launch_status();
}
}  // namespace vit
