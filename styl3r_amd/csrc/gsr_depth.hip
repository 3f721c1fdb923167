// gsr_depth.hip -- the edge-aware depth-smoothness regulariser, `LossDepth.forward` (src/loss/loss_depth.py:26-60), as three
// launches instead of the ~60 element-wise / reduce launches of the torch expression, forward and backward together:
//
//   n    = (max(min(D, hi), lo) - lo) / (hi - lo),  lo = log(near), hi = log(far) per view  (the bounds are logs, the depth is not:
//          the reference's own arithmetic, reproduced)
//   t_x  = first or second difference of n along the row, t_y along the column, each times exp(-sigma * c) when an image is given,
//          c = max over the channels of the image's SIGNED first difference (second derivative: the larger of the two differences)
//   loss = weight * (mean |t_x| + mean |t_y|)
//
// forward : one pass, every lane owns four consecutive pixels of a row; right and lower neighbours are re-read (L1 / L2 hits).  Per-workgroup
//           float64 partials of the two sums, then a one-workgroup fold in a fixed order: deterministic, no atomics, nothing to zero.
// backward: one launch in gather form -- every pixel recomputes the signs and weights of the (at most 2, or 3 with coefficients 1 -2 1)
//           differences per axis it takes part in and writes its gradient once.
// lo, hi and 1 / (hi - lo) are evaluated in float64 from the fp32 near / far once per workgroup; everything per pixel is fp32.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/gsr.h"
#include "gsr_common.h"

namespace gsr {

// No contraction in this file: fused, n1 - n0 = (d1 - lo) inv - (d0 - lo) inv becomes fma(d1 - lo, inv, -round((d0 - lo) inv)), which for two EQUAL
// depths is the rounding error of the product instead of 0 -- and the sign of a zero difference must be 0 (flat and uncovered regions).
#pragma clang fp contract(off)

constexpr int DS_BLOCK = 256, DS_PX = 4, DS_TW = 128, DS_TH = 8;      // a workgroup: 32 lanes x 4 pixels wide, 8 rows high
static_assert(DS_TW / DS_PX * DS_TH == DS_BLOCK, "one lane per four pixels of the tile");

struct DsBounds { float lo, hi, inv; };

// thread 0 of the workgroup evaluates the view's bounds in float64; every thread returns with them
__device__ inline DsBounds ds_bounds(const float *__restrict__ near, const float *__restrict__ far, long long view, DsBounds *sh)
{
    if (threadIdx.x == 0) {
        const double lo = log((double)near[view]), hi = log((double)far[view]);
        sh->lo = (float)lo; sh->hi = (float)hi; sh->inv = (float)(1.0 / (hi - lo));
    }
    __syncthreads();
    return *sh;
}

// torch's minimum / maximum (a NaN depth stays NaN), then the scaling
__device__ inline float ds_norm(float d, const DsBounds b)
{
    const float m = !(d >= b.hi) ? d : b.hi;
    const float c = !(m <= b.lo) ? m : b.lo;
    return (c - b.lo) * b.inv;
}
// d n / d D times (hi - lo): 1 inside, 1/2 at a bound (the tie rule of minimum / maximum), 0 outside
__device__ inline float ds_clamp_factor(float d, const DsBounds b)
{
    const float fmin_ = d < b.hi ? 1.f : (d == b.hi ? 0.5f : 0.f);
    const float m = !(d >= b.hi) ? d : b.hi;
    const float fmax_ = m > b.lo ? 1.f : (m == b.lo ? 0.5f : 0.f);
    return fmin_ * fmax_;
}

// four floats of a row from column x (a multiple of 4, possibly outside [0, W)): one 16-byte load where the address allows, else scalars;
// 0 outside the row, and for a row outside the image (row == nullptr)
__device__ inline void ds_load4(const float *__restrict__ row, int x, int W, float *v)
{
    v[0] = v[1] = v[2] = v[3] = 0.f;
    if (!row) return;
    if (x >= 0 && x + 3 < W && (reinterpret_cast<uintptr_t>(row + x) & 15) == 0) {
        const float4 q = *reinterpret_cast<const float4 *>(row + x);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (x + i >= 0 && x + i < W) v[i] = row[x + i];
    }
}

template <bool SECOND>
__device__ inline float ds_diff(float a0, float a1, float a2) { return SECOND ? (a2 - a1) - (a1 - a0) : a1 - a0; }

// the bilateral weights of `n_terms` consecutive differences from the per-position channel maxima cd[k] = max_c (I[k + 1] - I[k])
template <bool SECOND, int N_TERMS>
__device__ inline void ds_weights(const float *cd, float sigma, float *w)
{
#pragma unroll
    for (int k = 0; k < N_TERMS; ++k) w[k] = expf(-(SECOND ? fmaxf(cd[k + 1], cd[k]) : cd[k]) * sigma);
}

__device__ inline float ds_sign(float p) { return (float)(p > 0.f) - (float)(p < 0.f); }

__device__ inline const float *ds_row(const float *__restrict__ plane, int y, int H, int W)
{
    return (y >= 0 && y < H) ? plane + (size_t)y * W : nullptr;
}

struct DsTile { long long view; int x0, y; };
__device__ inline DsTile ds_tile(int H, int W)
{
    const int tx = (W + DS_TW - 1) / DS_TW, ty = (H + DS_TH - 1) / DS_TH;
    const long long view = blockIdx.x / (unsigned)(tx * ty);
    const int t = (int)(blockIdx.x % (unsigned)(tx * ty));
    return {view, (t % tx) * DS_TW + (int)(threadIdx.x & 31) * DS_PX, (t / tx) * DS_TH + (int)(threadIdx.x >> 5)};
}

template <bool SECOND, bool IMG>
__global__ void __launch_bounds__(DS_BLOCK) k_depth_smooth_fwd(const float *__restrict__ depth, const float *__restrict__ image,
                                                               const float *__restrict__ near, const float *__restrict__ far, int H, int W,
                                                               float sigma, double *__restrict__ partial)
{
    constexpr int K = SECOND ? 2 : 1;
    __shared__ DsBounds s_b;
    __shared__ double s_sum[2][DS_BLOCK / 64];
    const DsTile t = ds_tile(H, W);
    const DsBounds b = ds_bounds(near, far, t.view, &s_b);
    double sx = 0.0, sy = 0.0;
    if (t.y < H && t.x0 < W) {
        const float *dv = depth + (size_t)t.view * H * W;
        float a[8], r1[4], r2[4];                                   // row y at x0 .. x0 + 7, rows y + 1 and y + 2 at x0 .. x0 + 3
        ds_load4(ds_row(dv, t.y, H, W), t.x0, W, a);
        ds_load4(ds_row(dv, t.y, H, W), t.x0 + 4, W, a + 4);
        ds_load4(ds_row(dv, t.y + 1, H, W), t.x0, W, r1);
        ds_load4(SECOND ? ds_row(dv, t.y + 2, H, W) : nullptr, t.x0, W, r2);
#pragma unroll
        for (int i = 0; i < 8; ++i) a[i] = ds_norm(a[i], b);
#pragma unroll
        for (int i = 0; i < 4; ++i) { r1[i] = ds_norm(r1[i], b); r2[i] = ds_norm(r2[i], b); }
        float wx[4], wy[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) wx[i] = wy[i] = 1.f;
        if (IMG) {
            float cdx[5], cdy[2][4];                                // channel maxima of the image's differences: along the row at x0 .. x0 + 4, down at rows y, y + 1
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float *iv = image + ((size_t)t.view * 3 + c) * H * W;
                float p[8], q1[4], q2[4];
                ds_load4(ds_row(iv, t.y, H, W), t.x0, W, p);
                ds_load4(ds_row(iv, t.y, H, W), t.x0 + 4, W, p + 4);
                ds_load4(ds_row(iv, t.y + 1, H, W), t.x0, W, q1);
                ds_load4(SECOND ? ds_row(iv, t.y + 2, H, W) : nullptr, t.x0, W, q2);
#pragma unroll
                for (int k = 0; k < 5; ++k) { const float d = p[k + 1] - p[k]; cdx[k] = c ? fmaxf(cdx[k], d) : d; }
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const float d0 = q1[i] - p[i], d1 = q2[i] - q1[i];
                    cdy[0][i] = c ? fmaxf(cdy[0][i], d0) : d0;
                    cdy[1][i] = c ? fmaxf(cdy[1][i], d1) : d1;
                }
            }
            ds_weights<SECOND, 4>(cdx, sigma, wx);
#pragma unroll
            for (int i = 0; i < 4; ++i) wy[i] = expf(-(SECOND ? fmaxf(cdy[1][i], cdy[0][i]) : cdy[0][i]) * sigma);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if (t.x0 + i + K < W) sx += (double)fabsf(ds_diff<SECOND>(a[i], a[i + 1], a[i + 2]) * wx[i]);
            if (t.x0 + i < W && t.y + K < H) sy += (double)fabsf(ds_diff<SECOND>(a[i], r1[i], r2[i]) * wy[i]);
        }
    }
    sx = wave_sum(sx); sy = wave_sum(sy);
    if ((threadIdx.x & 63) == 0) { s_sum[0][threadIdx.x >> 6] = sx; s_sum[1][threadIdx.x >> 6] = sy; }
    __syncthreads();
    if (threadIdx.x < 2)
        partial[2 * (size_t)blockIdx.x + threadIdx.x] = ((s_sum[threadIdx.x][0] + s_sum[threadIdx.x][1]) + s_sum[threadIdx.x][2]) + s_sum[threadIdx.x][3];
}

// one workgroup: lane l adds partials l, l + 256, ... in that order, then the lanes are folded in a fixed order
__global__ void __launch_bounds__(DS_BLOCK) k_depth_smooth_fold(const double *__restrict__ partial, long long groups, double count_x, double count_y,
                                                                float weight, float *__restrict__ out)
{
    __shared__ double s_sum[2][DS_BLOCK / 64];
    double sx = 0.0, sy = 0.0;
    for (long long i = threadIdx.x; i < groups; i += DS_BLOCK) { sx += partial[2 * i]; sy += partial[2 * i + 1]; }
    sx = wave_sum(sx); sy = wave_sum(sy);
    if ((threadIdx.x & 63) == 0) { s_sum[0][threadIdx.x >> 6] = sx; s_sum[1][threadIdx.x >> 6] = sy; }
    __syncthreads();
    if (threadIdx.x == 0) {
        const double tx = ((s_sum[0][0] + s_sum[0][1]) + s_sum[0][2]) + s_sum[0][3], ty = ((s_sum[1][0] + s_sum[1][1]) + s_sum[1][2]) + s_sum[1][3];
        out[0] = (float)((double)weight * (tx / count_x + ty / count_y));
    }
}

// gather of one axis: s[q] = sign(t_q w_q) w_q of the six differences that start at positions -2 .. 3 relative to the lane's first pixel
// (0 where the difference does not exist); pixel i collects +s[i+2] -2 s[i+1] +s[i] (second) or s[i+1] - s[i+2] (first)
template <bool SECOND>
__device__ inline float ds_gather(const float *s, int i) { return SECOND ? (s[i + 2] - 2.f * s[i + 1]) + s[i] : s[i + 1] - s[i + 2]; }

template <bool SECOND, bool IMG>
__global__ void __launch_bounds__(DS_BLOCK) k_depth_smooth_bwd(const float *__restrict__ depth, const float *__restrict__ image,
                                                               const float *__restrict__ near, const float *__restrict__ far,
                                                               const float *__restrict__ grad_loss, int H, int W, float weight, float sigma,
                                                               double count_x, double count_y, float *__restrict__ grad)
{
    constexpr int K = SECOND ? 2 : 1;
    __shared__ DsBounds s_b;
    __shared__ float s_k[2];
    const DsTile t = ds_tile(H, W);
    if (threadIdx.x == 0) {                                           // weight * grad_loss / count / (hi - lo) per axis, in float64
        const double lo = log((double)near[t.view]), hi = log((double)far[t.view]);
        const double g = (double)weight * (grad_loss ? (double)grad_loss[0] : 1.0) / (hi - lo);
        s_k[0] = (float)(g / count_x); s_k[1] = (float)(g / count_y);
    }
    const DsBounds b = ds_bounds(near, far, t.view, &s_b);             // (its barrier publishes s_k too)
    if (t.y >= H || t.x0 >= W) return;
    const float kx = s_k[0], ky = s_k[1];
    const float *dv = depth + (size_t)t.view * H * W;
    float a[12], col[5][4];                                           // row y at x0 - 4 .. x0 + 7; rows y - 2 .. y + 2 at x0 .. x0 + 3
    ds_load4(ds_row(dv, t.y, H, W), t.x0 - 4, W, a);
    ds_load4(ds_row(dv, t.y, H, W), t.x0, W, a + 4);
    ds_load4(ds_row(dv, t.y, H, W), t.x0 + 4, W, a + 8);
    float own[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) own[i] = a[4 + i];
#pragma unroll
    for (int r = 0; r < 5; ++r) {
        if (r == 2) {
#pragma unroll
            for (int i = 0; i < 4; ++i) col[2][i] = a[4 + i];
        } else {
            ds_load4((SECOND || r == 1 || r == 3) ? ds_row(dv, t.y + r - 2, H, W) : nullptr, t.x0, W, col[r]);
        }
    }
#pragma unroll
    for (int i = 0; i < 12; ++i) a[i] = ds_norm(a[i], b);
#pragma unroll
    for (int r = 0; r < 5; ++r)
#pragma unroll
        for (int i = 0; i < 4; ++i) col[r][i] = ds_norm(col[r][i], b);
    float wx[6], wy[3][4];
#pragma unroll
    for (int q = 0; q < 6; ++q) wx[q] = 1.f;
#pragma unroll
    for (int q = 0; q < 3; ++q)
#pragma unroll
        for (int i = 0; i < 4; ++i) wy[q][i] = 1.f;
    if (IMG) {
        float cdx[7], cdy[4][4];                                      // along the row from x0 - 2 .. x0 + 4; down from rows y - 2 .. y + 1
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float *iv = image + ((size_t)t.view * 3 + c) * H * W;
            float p[12], q[5][4];
            ds_load4(ds_row(iv, t.y, H, W), t.x0 - 4, W, p);
            ds_load4(ds_row(iv, t.y, H, W), t.x0, W, p + 4);
            ds_load4(ds_row(iv, t.y, H, W), t.x0 + 4, W, p + 8);
#pragma unroll
            for (int r = 0; r < 5; ++r) {
                if (r == 2) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) q[2][i] = p[4 + i];
                } else {
                    ds_load4((SECOND || r == 1 || r == 3) ? ds_row(iv, t.y + r - 2, H, W) : nullptr, t.x0, W, q[r]);
                }
            }
#pragma unroll
            for (int k = 0; k < 7; ++k) { const float d = p[k + 3] - p[k + 2]; cdx[k] = c ? fmaxf(cdx[k], d) : d; }
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int i = 0; i < 4; ++i) { const float d = q[r + 1][i] - q[r][i]; cdy[r][i] = c ? fmaxf(cdy[r][i], d) : d; }
        }
        ds_weights<SECOND, 6>(cdx, sigma, wx);
#pragma unroll
        for (int q = 0; q < 3; ++q)
#pragma unroll
            for (int i = 0; i < 4; ++i) wy[q][i] = expf(-(SECOND ? fmaxf(cdy[q + 1][i], cdy[q][i]) : cdy[q][i]) * sigma);
    }
    float sxv[6], g[4];
#pragma unroll
    for (int q = 0; q < 6; ++q) {                                     // the difference that starts at column x0 - 2 + q (a[] index q + 2)
        const int x = t.x0 - 2 + q;
        const float p = ds_diff<SECOND>(a[q + 2], a[q + 3], a[q + 4]) * wx[q];
        sxv[q] = (x >= 0 && x + K < W) ? ds_sign(p) * wx[q] : 0.f;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        float syv[3];                                                  // [q]: the difference that starts at row y - 2 + q
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            const int y = t.y - 2 + q;
            const float p = ds_diff<SECOND>(col[q][i], col[q + 1][i], col[q + 2][i]) * wy[q][i];
            syv[q] = (y >= 0 && y + K < H) ? ds_sign(p) * wy[q][i] : 0.f;
        }
        const float gy = SECOND ? (syv[2] - 2.f * syv[1]) + syv[0] : syv[1] - syv[2];
        g[i] = (ds_gather<SECOND>(sxv, i) * kx + gy * ky) * ds_clamp_factor(own[i], b);
    }
    float *out = grad + ((size_t)t.view * H + t.y) * W + t.x0;
    if (t.x0 + 3 < W && (reinterpret_cast<uintptr_t>(out) & 15) == 0) {
        *reinterpret_cast<float4 *>(out) = make_float4(g[0], g[1], g[2], g[3]);
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (t.x0 + i < W) out[i] = g[i];
    }
}

// workgroups of a launch, or 0 for dimensions the kernels refuse
static long long ds_groups(int64_t N, int H, int W, int second)
{
    const int least = second ? 3 : 2;
    if (N < 1 || H < least || W < least) return 0;
    const long long g = (long long)N * ((W + DS_TW - 1) / DS_TW) * ((H + DS_TH - 1) / DS_TH);
    return g > 0xffffffLL ? 0 : g;            // (2^24 workgroups of 256 lanes: the 2^32 lanes of one launch)
}

}  // namespace gsr

extern "C" {

__attribute__((visibility("default"))) size_t gsr_depth_smooth_scratch_bytes(int64_t N, int H, int W)
{
    return (size_t)gsr::ds_groups(N, H, W, 0) * 2 * sizeof(double);
}

__attribute__((visibility("default"))) int gsr_depth_smooth_fwd(const float *depth, const float *image, const float *near, const float *far,
                                                                int64_t N, int H, int W, float weight, float sigma_image, int second_derivative,
                                                                void *scratch, float *loss, void *stream)
{
    const long long groups = gsr::ds_groups(N, H, W, second_derivative);
    if (!groups || !depth || !near || !far || !loss || !scratch) return GSR_EINVAL;
    (void)hipGetLastError();
    hipStream_t s = static_cast<hipStream_t>(stream);
    double *partial = static_cast<double *>(scratch);
    const int K = second_derivative ? 2 : 1;
    auto launch = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3((unsigned)groups), dim3(gsr::DS_BLOCK), 0, s, depth, image, near, far, H, W, sigma_image, partial);
    };
    if (second_derivative) { if (image) launch(gsr::k_depth_smooth_fwd<true, true>); else launch(gsr::k_depth_smooth_fwd<true, false>); }
    else { if (image) launch(gsr::k_depth_smooth_fwd<false, true>); else launch(gsr::k_depth_smooth_fwd<false, false>); }
    hipLaunchKernelGGL(gsr::k_depth_smooth_fold, dim3(1), dim3(gsr::DS_BLOCK), 0, s, partial, groups, (double)N * H * (W - K), (double)N * (H - K) * W,
                       weight, loss);
    return gsr::launch_status();
}

__attribute__((visibility("default"))) int gsr_depth_smooth_bwd(const float *depth, const float *image, const float *near, const float *far,
                                                                const float *grad_loss, int64_t N, int H, int W, float weight, float sigma_image,
                                                                int second_derivative, float *grad_depth, void *stream)
{
    const long long groups = gsr::ds_groups(N, H, W, second_derivative);
    if (!groups || !depth || !near || !far || !grad_depth) return GSR_EINVAL;
    (void)hipGetLastError();
    const int K = second_derivative ? 2 : 1;
    auto launch = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3((unsigned)groups), dim3(gsr::DS_BLOCK), 0, static_cast<hipStream_t>(stream), depth, image, near, far, grad_loss, H, W,
                           weight, sigma_image, (double)N * H * (W - K), (double)N * (H - K) * W, grad_depth);
    };
    if (second_derivative) { if (image) launch(gsr::k_depth_smooth_bwd<true, true>); else launch(gsr::k_depth_smooth_bwd<true, false>); }
    else { if (image) launch(gsr::k_depth_smooth_bwd<false, true>); else launch(gsr::k_depth_smooth_bwd<false, false>); }
    return gsr::launch_status();
}

}  // extern "C"
