// vit_adain.hip -- the two kernels the 2D-AdaIN baseline (src/test/vgg_model.py, AdaIN2D.generate) needs beside the convolutions.
//
// vit_adain_fwd: adaptive instance normalisation of content (B, C, N) by style (Bs, C, M), image b taking style row style_index[b]:
//     t = style_std * (x - c_mean) / c_std + style_mean,   out = alpha * t + (1 - alpha) * x
// with mean = the row mean and std = the UNBIASED standard deviation + eps (calc_mean_std, vgg_model.py:19-27), in the reference's operation
// order, every fp32 operation rounded on its own (no contraction).  Two launches:
//   (1) k_adain_style_stats: one workgroup per style row (Bs x C of them: the views of a scene share one style, whose statistics are computed
//       once) -> scratch[2 row] = mean, scratch[2 row + 1] = std + eps, as floats;
//   (2) k_adain_apply: one workgroup per content row: the row's own statistics, then the output.  The row is read three times (sum, squared
//       deviations, the pass proper); at relu4_1 sizes a row is a few KiB and the second and third reads come out of the cache.
// Statistics accumulate in float64 in ONE order -- thread t sums elements t, t + 256, ... in index order, then one 256-leaf tree in LDS -- and
// the variance is the two-pass form sum (x - mean)^2 / (n - 1).  No atomics, every element written once, bit-identical run to run.
//
// vit_conv3_rgb_fwd: the decoder's output layer (64 -> 3): a 3x3 convolution with at most 4 output channels, for which the 128-row MFMA tile
// of vit_conv_x6_fwd would run 98 % empty.  Plain fp32 weights, one fp32 fma per (ci, ky, kx) on the vector ALU in exactly that order: the 72
// products of eight channels form one chain, and the chains' sums are added in channel order (eight additions at Ci = 64, not one chain of
// 576 whose round-off grows with its length).  A
// workgroup owns an 8 x 32 patch of output pixels of one image (thread = pixel) and walks the input channels eight at a time through an LDS tile
// with a one-pixel halo ((8 + 2) x (32 + 2) floats per channel): every input plane is read once (+ the halo overlap), the weights are
// wave-uniform scalar loads.  The source index of every halo pixel -- zero padding or reflection (index -1 -> 1, H -> H - 2, nn.ReflectionPad2d(1))
// -- and its mask are computed once, up front.  Epilogue: y = conv + bias, then optionally clamp(y * scale[co] + shift[co], lo, hi)
// (vgg_denorm, model_wrapper_style.py:51-55, in the store).  No atomics, every output written once.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vit_common.h"
#include "vit_internal.h"

namespace vit {

// sum over the workgroup in a fixed order: 256 leaves, one tree
__device__ inline double ai_block_sum(double v, double *red)
{
    const int tid = threadIdx.x;
    __syncthreads();                                         // (red may still be read from the previous sum)
    red[tid] = v;
    __syncthreads();
#pragma unroll
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) red[tid] += red[tid + o];
        __syncthreads();
    }
    return red[0];
}

// mean and unbiased std + eps of row[0 .. n), n >= 2
__device__ inline void ai_row_stats(const float *__restrict__ row, int64_t n, float eps, double *red, float &mean, float &std)
{
    double s = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += 256) s += (double)row[i];
    const double mu = ai_block_sum(s, red) / (double)n;
    s = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += 256) {
        const double d = (double)row[i] - mu;
        s += d * d;
    }
    const double var = ai_block_sum(s, red) / (double)(n - 1);
    mean = (float)mu;
    std = __fadd_rn((float)sqrt(var), eps);
}

__global__ void __launch_bounds__(256) k_adain_style_stats(const float *__restrict__ style, int64_t M, float eps, float *__restrict__ stats)
{
    __shared__ double red[256];
    float mu, sd;
    ai_row_stats(style + (int64_t)blockIdx.x * M, M, eps, red, mu, sd);
    if (threadIdx.x == 0) { stats[2 * (int64_t)blockIdx.x] = mu; stats[2 * (int64_t)blockIdx.x + 1] = sd; }
}

__global__ void __launch_bounds__(256) k_adain_apply(const float *__restrict__ content, const float *__restrict__ stats,
                                                     const int32_t *__restrict__ index, int C, int64_t N, float alpha, float eps,
                                                     float *__restrict__ out)
{
    __shared__ double red[256];
    const int64_t row = blockIdx.x;
    const int b = (int)(row / C), c = (int)(row - (int64_t)b * C);
    const float *x = content + row * N;
    float c_mean, c_std;
    ai_row_stats(x, N, eps, red, c_mean, c_std);
    const int64_t srow = (int64_t)index[b] * C + c;
    const float s_mean = stats[2 * srow], s_std = stats[2 * srow + 1];
    const float beta = __fsub_rn(1.f, alpha);
    float *o = out + row * N;
    for (int64_t i = threadIdx.x; i < N; i += 256) {
        const float v = x[i];
        const float t = __fadd_rn(__fdiv_rn(__fmul_rn(s_std, __fsub_rn(v, c_mean)), c_std), s_mean);
        o[i] = __fadd_rn(__fmul_rn(alpha, t), __fmul_rn(beta, v));
    }
}

size_t adain_scratch_bytes(int B, int Bs, int C) { return (B < 1 || Bs < 1 || C < 1) ? 0 : (size_t)Bs * C * 2 * sizeof(float); }

int adain_fwd(const float *content, const float *style, const int32_t *index_host, const int32_t *index_dev, int B, int Bs, int C, int64_t N,
              int64_t M, float alpha, float eps, float *out, void *scratch, hipStream_t stream)
{
    if (!content || !style || !index_host || !index_dev || !out || !scratch) return VIT_EINVAL;
    if (B < 1 || Bs < 1 || C < 1 || N < 2 || M < 2) return VIT_EINVAL;      // (the unbiased std of one element is NaN: refused, not returned)
    if ((int64_t)B * C > 0x7fffffff || (int64_t)Bs * C > 0x7fffffff || (reinterpret_cast<uintptr_t>(scratch) & 3)) return VIT_EINVAL;
    for (int i = 0; i < B; ++i)
        if (index_host[i] < 0 || index_host[i] >= Bs) return VIT_EINVAL;
    (void)hipGetLastError();
    hipLaunchKernelGGL(k_adain_style_stats, dim3((unsigned)(Bs * C)), dim3(256), 0, stream, style, M, eps, static_cast<float *>(scratch));
    hipLaunchKernelGGL(k_adain_apply, dim3((unsigned)(B * C)), dim3(256), 0, stream, content, static_cast<const float *>(scratch), index_dev, C,
                       N, alpha, eps, out);
    return launch_status();
}

// ---- the RGB output convolution ------------------------------------------------------------------------------------------------------------------
constexpr int RG_TX = 32, RG_TY = 8, RG_HX = RG_TX + 2, RG_HY = RG_TY + 2, RG_HP = RG_HX * RG_HY, RG_CB = 8;      // 340 halo pixels, 8 channels per step

template <int CO, bool RELU_IN>
__global__ void __launch_bounds__(256) k_conv3_rgb(const float *__restrict__ in, const float *__restrict__ w, const float *__restrict__ bias,
                                                   const float *__restrict__ scale, const float *__restrict__ shift, float lo, float hi,
                                                   float *__restrict__ out, int Ci, int H, int W, int reflect)
{
    __shared__ float tile[RG_CB][RG_HP];
    const int tid = threadIdx.x, tx = tid & (RG_TX - 1), ty = tid >> 5;
    const int tiles_x = (W + RG_TX - 1) / RG_TX, tiles_y = (H + RG_TY - 1) / RG_TY;
    const int b = blockIdx.x / (tiles_x * tiles_y), tr = blockIdx.x - b * (tiles_x * tiles_y);
    const int ty0 = (tr / tiles_x) * RG_TY, tx0 = (tr % tiles_x) * RG_TX;
    const int HW = H * W;
    const float *inb = in + (int64_t)b * Ci * HW;
    // halo loader: thread -> halo pixels tid and tid + 256 (the latter for tid < 84); source offset and mask once, up front.  Pixels that only
    // feed outputs outside the image (ragged tiles) read a clamped address and are masked.
    int h_off[2];
    float h_m[2];
#pragma unroll
    for (int e = 0; e < 2; ++e) {
        const int hp = min(tid + e * 256, RG_HP - 1), hy = hp / RG_HX, hx = hp - hy * RG_HX;
        int y = ty0 + hy - 1, x = tx0 + hx - 1;
        bool ok = y >= 0 && y < H && x >= 0 && x < W;
        if (reflect) {
            ok = y >= -1 && y <= H && x >= -1 && x <= W;
            y = y < 0 ? -y : y; y = y >= H ? 2 * (H - 1) - y : y;
            x = x < 0 ? -x : x; x = x >= W ? 2 * (W - 1) - x : x;
        }
        h_m[e] = ok ? 1.f : 0.f;
        h_off[e] = min(max(y, 0), H - 1) * W + min(max(x, 0), W - 1);
    }
    const bool second = tid < RG_HP - 256;
    float acc[CO];
#pragma unroll
    for (int co = 0; co < CO; ++co) acc[co] = 0.f;
    const float lo_in = RELU_IN ? 0.f : -3.0e38f;
    for (int c0 = 0; c0 < Ci; c0 += RG_CB) {
        float v0[RG_CB], v1[RG_CB];
#pragma unroll
        for (int c = 0; c < RG_CB; ++c) {
            v0[c] = inb[(int64_t)(c0 + c) * HW + h_off[0]];
            v1[c] = inb[(int64_t)(c0 + c) * HW + h_off[1]];                      // (tid >= 84: a duplicate of the last pixel, not stored)
        }
        __syncthreads();                                     // the previous step's reads are done
#pragma unroll
        for (int c = 0; c < RG_CB; ++c) {
            tile[c][tid] = h_m[0] != 0.f ? fmaxf(v0[c], lo_in) : 0.f;
            if (second) tile[c][tid + 256] = h_m[1] != 0.f ? fmaxf(v1[c], lo_in) : 0.f;
        }
        __syncthreads();
        float part[CO];                                      // this step's 72 products: one fma chain in (ci, ky, kx) order
#pragma unroll
        for (int co = 0; co < CO; ++co) part[co] = 0.f;
#pragma unroll
        for (int c = 0; c < RG_CB; ++c) {
            float p[9];
#pragma unroll
            for (int t = 0; t < 9; ++t) p[t] = tile[c][(ty + t / 3) * RG_HX + tx + t % 3];
#pragma unroll
            for (int co = 0; co < CO; ++co) {
                const float *wc = w + ((int64_t)co * Ci + c0 + c) * 9;          // wave-uniform: scalar loads
#pragma unroll
                for (int t = 0; t < 9; ++t) part[co] = __fmaf_rn(p[t], wc[t], part[co]);
            }
        }
#pragma unroll
        for (int co = 0; co < CO; ++co) acc[co] = __fadd_rn(acc[co], part[co]);      // the steps' sums, added in channel order
    }
    const int y = ty0 + ty, x = tx0 + tx;
    if (y >= H || x >= W) return;
    float *o = out + (int64_t)b * CO * HW + (int64_t)y * W + x;
#pragma unroll
    for (int co = 0; co < CO; ++co) {
        float v = bias ? __fadd_rn(acc[co], bias[co]) : acc[co];
        if (scale) {
            v = __fadd_rn(__fmul_rn(v, scale[co]), shift[co]);
            v = v < lo ? lo : (v > hi ? hi : v);             // (a NaN stays a NaN, as torch.clamp leaves it)
        }
        o[(int64_t)co * HW] = v;
    }
}

int conv3_rgb_fwd(const float *in, const float *w, const float *bias, const float *scale, const float *shift, float lo, float hi, float *out,
                  int B, int Ci, int Co, int H, int W, int flags, hipStream_t stream)
{
    if (!in || !w || !out || B < 1 || H < 1 || W < 1) return VIT_EINVAL;
    if (Ci < RG_CB || Ci % RG_CB || Ci > 64 || Co < 1 || Co > 4) return VIT_EINVAL;
    if (flags & ~(VIT_CONV_RELU_IN | VIT_CONV_REFLECT)) return VIT_EINVAL;
    const int reflect = (flags & VIT_CONV_REFLECT) ? 1 : 0;
    if (reflect && (H < 2 || W < 2)) return VIT_EINVAL;
    if (scale && (!shift || !(lo <= hi))) return VIT_EINVAL;
    if ((int64_t)Ci * H * W > 0x7fffffff) return VIT_EINVAL;                      // (plane offsets inside one image are 32-bit in h_off)
    const int64_t tiles = (int64_t)B * ((W + RG_TX - 1) / RG_TX) * ((H + RG_TY - 1) / RG_TY);
    if (tiles > 0x7fffffff) return VIT_EINVAL;
    (void)hipGetLastError();
#define VIT_LAUNCH_RGB(CO, RL)                                                                                                                    \
    hipLaunchKernelGGL((k_conv3_rgb<CO, RL>), dim3((unsigned)tiles), dim3(256), 0, stream, in, w, bias, scale, shift, lo, hi, out, Ci, H, W, reflect)
    const bool rl = (flags & VIT_CONV_RELU_IN) != 0;
    switch (Co) {
    case 1: if (rl) VIT_LAUNCH_RGB(1, true); else VIT_LAUNCH_RGB(1, false); break;
    case 2: if (rl) VIT_LAUNCH_RGB(2, true); else VIT_LAUNCH_RGB(2, false); break;
    case 3: if (rl) VIT_LAUNCH_RGB(3, true); else VIT_LAUNCH_RGB(3, false); break;
    default: if (rl) VIT_LAUNCH_RGB(4, true); else VIT_LAUNCH_RGB(4, false); break;
    }
#undef VIT_LAUNCH_RGB
    return launch_status();
}
}  // namespace vit
