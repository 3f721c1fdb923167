// gsr_metrics.hip -- the test step of the reference (src/model/model_wrapper_style.py:317-461) on the rendered images:
//
// gsr_image_scores: SSIM (`compute_ssim`, src/evaluation/metrics.py:38-52 = skimage structural_similarity with win_size 11,
//   gaussian_weights, sample covariance, data_range 1, channel_axis 0) and the mean squared error of the clipped images that PSNR
//   is formed from (`compute_psnr`, :11-20), from ONE pass over both images, plus a small launch that folds the per-tile partial
//   sums of every image in index order (deterministic, no float atomics, an image's result does not depend on the batch).
//
//   Tiling: one wave per (image, channel, strip of 64 output columns, chunk of 32 output rows).  Lane j owns output column j of the
//   strip.  The wave walks down the 42 input rows of its chunk: every row (74 columns: the strip and its 10-column halo) is staged
//   through LDS, each lane filters the five moments x, y, x^2, y^2, xy horizontally (11 taps) into a ring of the 11 most recent rows
//   held in registers, and from the 11th row on filters the ring vertically into one SSIM map value.  Only the (H-10) x (W-10)
//   pixels whose 11x11 window lies inside the image are formed: that is skimage's crop of 5 from every edge, so the boundary mode of
//   its filter never matters.  Read amplification over the two images: (32+10)/32 rows x 74/64 columns = 1.52 for a full tile, 1.42 at
//   256 x 256 (narrower last strip and chunk; the re-read halo is L2-resident).  Each pixel's squared error is counted by exactly one
//   wave: the strip owns its 64 columns (the last strip also its halo), the chunk its first 32 rows (the last chunk every row to the
//   bottom edge).
//   Cancellation: the moments are formed of x - kx and y - ky, kx / ky the images' values at the tile's first pixel; variances and
//   the covariance do not change under that shift and the means get it added back.
//
// gsr_pose_adam_update: the pose step of test_step_align (:430-440) for n views in one launch -- Adam (torch.optim.Adam defaults,
//   two parameter groups) on the zero deltas, then w2c' = SE3_exp(trans, rot) w2c (src/misc/cam_utils.py:67-137), c2w' = w2c'^-1.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/gsr.h"
#include "gsr_common.h"

namespace gsr {

constexpr int SC_COLS = 64;                       // output columns per wave, one per lane
constexpr int SC_ROWS = 32;                       // output rows per wave
constexpr int SC_R = 5;                           // window radius: int(truncate 3.5 * sigma 1.5 + 0.5)
constexpr int SC_WIN = 2 * SC_R + 1;              // 11
constexpr int SC_IN = SC_COLS + 2 * SC_R;         // 74 input columns per row
constexpr float SC_C1 = 1e-4f, SC_C2 = 9e-4f;     // (0.01 data_range)^2, (0.03 data_range)^2
constexpr float SC_COV_NORM = 121.0f / 120.0f;    // use_sample_covariance: NP / (NP - 1), NP = 11^2

struct SsimWindow {
    float w[SC_WIN];
};

__device__ inline double wave_sum_f64(double v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;                                     // (xor butterfly: the same value, in the same order, in every lane)
}

__device__ inline float clip01(float v) { return fminf(fmaxf(v, 0.f), 1.f); }

__global__ void __launch_bounds__(64) k_image_scores(const float *__restrict__ gt, const float *__restrict__ pred, int H, int W,
                                                     int strips, int chunks, SsimWindow win, double *__restrict__ partial)
{
    __shared__ float sx[2][SC_IN], sy[2][SC_IN];
    const int lane = threadIdx.x;
    const int tiles = strips * chunks;
    const long long blk = blockIdx.x;
    const long long plane = blk / tiles;
    const int t = (int)(blk - plane * tiles);
    const int k = t / strips, s = t - k * strips;
    const int Ho = H - 2 * SC_R, Wo = W - 2 * SC_R;
    const int c0 = s * SC_COLS;
    const int r0 = k * SC_ROWS, r1 = min(r0 + SC_ROWS, Ho) + 2 * SC_R;     // input rows [r0, r1)
    const int own_rows = (k == chunks - 1) ? H - r0 : SC_ROWS;
    const float *X = gt + (size_t)plane * H * W, *Y = pred + (size_t)plane * H * W;
    const float kx = X[(size_t)r0 * W + c0], ky = Y[(size_t)r0 * W + c0];
    const int cm = c0 + lane, ch = c0 + SC_COLS + lane;                        // main / halo column of this lane
    const bool in_m = cm < W, in_h = lane < 2 * SC_R && ch < W;
    const bool own_h = s == strips - 1;                                        // a halo column belongs to the last strip only
    const bool out_col = cm < Wo;

    float xm = 0.f, ym = 0.f, xh = 0.f, yh = 0.f;
    auto load_row = [&](int r) {
        const size_t o = (size_t)r * W;
        xm = in_m ? X[o + cm] : 0.f; ym = in_m ? Y[o + cm] : 0.f;
        xh = in_h ? X[o + ch] : 0.f; yh = in_h ? Y[o + ch] : 0.f;
    };
    load_row(r0);

    float ring[SC_WIN][5];
    double acc_s = 0.0, acc_e = 0.0;
    for (int rb = r0; rb < r1; rb += SC_WIN) {
#pragma unroll
        for (int j = 0; j < SC_WIN; ++j) {                                    // row rb + j goes to ring slot j (static indices)
            const int r = rb + j;
            if (r >= r1) continue;                                             // (uniform; no break: it stops the unrolling)
            if (r - r0 < own_rows) {
                float e = 0.f;
                if (in_m) { const float d = clip01(xm) - clip01(ym); e = d * d; }
                if (in_h && own_h) { const float d = clip01(xh) - clip01(yh); e += d * d; }
                acc_e += (double)e;
            }
            const int b = r & 1;
            sx[b][lane] = xm - kx; sy[b][lane] = ym - ky;
            if (lane < 2 * SC_R) { sx[b][SC_COLS + lane] = xh - kx; sy[b][SC_COLS + lane] = yh - ky; }
            if (r + 1 < r1) load_row(r + 1);                                   // in flight while this row is filtered
            __syncthreads();
            float h0 = 0.f, h1 = 0.f, h2 = 0.f, h3 = 0.f, h4 = 0.f;
#pragma unroll
            for (int q = 0; q < SC_WIN; ++q) {
                const float a = sx[b][lane + q], c = sy[b][lane + q], wa = win.w[q] * a, wc = win.w[q] * c;
                h0 += wa; h1 += wc; h2 += wa * a; h3 += wc * c; h4 += wa * c;
            }
            ring[j][0] = h0; ring[j][1] = h1; ring[j][2] = h2; ring[j][3] = h3; ring[j][4] = h4;
            if (r - r0 >= 2 * SC_R && out_col) {                               // rows r-10 .. r are in slots j+1 .. j (mod 11)
                float m0 = 0.f, m1 = 0.f, m2 = 0.f, m3 = 0.f, m4 = 0.f;
#pragma unroll
                for (int i = 0; i < SC_WIN; ++i) {
                    const int sl = (j + 1 + i) % SC_WIN;
                    const float w = win.w[i];
                    m0 += w * ring[sl][0]; m1 += w * ring[sl][1]; m2 += w * ring[sl][2]; m3 += w * ring[sl][3]; m4 += w * ring[sl][4];
                }
                const float vx = SC_COV_NORM * (m2 - m0 * m0), vy = SC_COV_NORM * (m3 - m1 * m1), vxy = SC_COV_NORM * (m4 - m0 * m1);
                const float ux = m0 + kx, uy = m1 + ky;
                const float a1 = 2.f * ux * uy + SC_C1, a2 = 2.f * vxy + SC_C2;
                const float b1 = ux * ux + uy * uy + SC_C1, b2 = vx + vy + SC_C2;
                acc_s += (double)((a1 * a2) / (b1 * b2));
            }
        }
    }
    acc_s = wave_sum_f64(acc_s);
    acc_e = wave_sum_f64(acc_e);
    if (lane == 0) { partial[2 * blk] = acc_s; partial[2 * blk + 1] = acc_e; }
}

// one wave per image: its C * tiles partials in index order
__global__ void __launch_bounds__(64) k_image_scores_fold(const double *__restrict__ partial, int per_image, double inv_ssim,
                                                          double inv_mse, float *__restrict__ ssim, float *__restrict__ mse)
{
    const long long n = blockIdx.x;
    const double *p = partial + 2 * n * per_image;
    double s = 0.0, e = 0.0;
    for (int i = threadIdx.x; i < per_image; i += 64) { s += p[2 * i]; e += p[2 * i + 1]; }
    s = wave_sum_f64(s);
    e = wave_sum_f64(e);
    if (threadIdx.x == 0) { ssim[n] = (float)(s * inv_ssim); mse[n] = (float)(e * inv_mse); }
}

static bool scores_grid(int64_t N, int C, int H, int W, int &strips, int &chunks, long long &blocks)
{
    if (N < 1 || C < 1 || H < SC_WIN || W < SC_WIN) return false;
    strips = (W - 2 * SC_R + SC_COLS - 1) / SC_COLS;
    chunks = (H - 2 * SC_R + SC_ROWS - 1) / SC_ROWS;
    blocks = (long long)N * C * strips * chunks;
    return blocks <= 0x7fffffffLL;
}

// ---- pose step: one thread per view ------------------------------------------------------------------------------------
__device__ inline void inverse4_f64(const double *m, double *inv)
{
    // Gauss-Jordan with partial pivoting on [m | I] (row-major): the general inverse of update_pose's `extrinsics.inverse()`
    double a[4][8];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) { a[r][c] = m[4 * r + c]; a[r][4 + c] = (r == c) ? 1.0 : 0.0; }
#pragma unroll
    for (int col = 0; col < 4; ++col) {
        int piv = col;
        double best = fabs(a[col][col]);
#pragma unroll
        for (int r = 0; r < 4; ++r)
            if (r > col && fabs(a[r][col]) > best) { best = fabs(a[r][col]); piv = r; }
#pragma unroll
        for (int r = 0; r < 4; ++r)
            if (r == piv && piv != col) {
#pragma unroll
                for (int c = 0; c < 8; ++c) { const double t = a[col][c]; a[col][c] = a[r][c]; a[r][c] = t; }
            }
        const double d = 1.0 / a[col][col];
#pragma unroll
        for (int c = 0; c < 8; ++c) a[col][c] *= d;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            if (r == col) continue;
            const double f = a[r][col];
#pragma unroll
            for (int c = 0; c < 8; ++c) a[r][c] -= f * a[col][c];
        }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) inv[4 * r + c] = a[r][4 + c];
}

__global__ void __launch_bounds__(64) k_pose_adam(float *__restrict__ c2w, float *__restrict__ m, float *__restrict__ v,
                                                  const float *__restrict__ grad_rot, const float *__restrict__ grad_trans, long long n,
                                                  float step_rot, float step_trans, float beta1, float beta2, float eps, float bc2_sqrt)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    // Adam on a parameter that is 0 before every step (the reference resets the deltas): theta = -step_size * m / denom, with
    // torch's fp32 arithmetic (exp_avg.lerp_, exp_avg_sq.mul_().addcmul_(), sqrt / bc2_sqrt + eps, addcdiv_)
    double d[6];                                   // (rot, trans) -> tau = (rho = trans, theta = rot) below
#pragma unroll
    for (int q = 0; q < 6; ++q) {
        const float g = q < 3 ? grad_rot[3 * i + q] : grad_trans[3 * i + q - 3];
        float mq = m[6 * i + q], vq = v[6 * i + q];
        mq = mq + (1.f - beta1) * (g - mq);
        vq = vq * beta2 + (1.f - beta2) * g * g;
        m[6 * i + q] = mq; v[6 * i + q] = vq;
        const float denom = sqrtf(vq) / bc2_sqrt + eps;
        d[q] = (double)(-(q < 3 ? step_rot : step_trans) * (mq / denom));
    }
    const double th[3] = {d[0], d[1], d[2]}, rho[3] = {d[3], d[4], d[5]};
    // SE3_exp (cam_utils.py:67-116): W = [theta]x, R = SO3_exp(theta), t = V(theta) rho
    const double Wm[3][3] = {{0.0, -th[2], th[1]}, {th[2], 0.0, -th[0]}, {-th[1], th[0], 0.0}};
    double W2[3][3];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) W2[r][c] = Wm[r][0] * Wm[0][c] + Wm[r][1] * Wm[1][c] + Wm[r][2] * Wm[2][c];
    const double angle = sqrt(th[0] * th[0] + th[1] * th[1] + th[2] * th[2]);
    double rw, rw2, vw, vw2;
    if (angle < 1e-5) { rw = 1.0; rw2 = 0.5; vw = 0.5; vw2 = 1.0 / 6.0; }
    else {
        const double a2 = angle * angle;
        rw = sin(angle) / angle; rw2 = (1.0 - cos(angle)) / a2;
        vw = rw2; vw2 = (angle - sin(angle)) / (a2 * angle);
    }
    double T[16];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        double t = 0.0;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const double id = r == c ? 1.0 : 0.0;
            T[4 * r + c] = id + rw * Wm[r][c] + rw2 * W2[r][c];
            t += (id + vw * Wm[r][c] + vw2 * W2[r][c]) * rho[c];
        }
        T[4 * r + 3] = t;
    }
    T[12] = 0.0; T[13] = 0.0; T[14] = 0.0; T[15] = 1.0;
    double E[16], w2c[16], nw[16], out[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) E[q] = (double)c2w[16 * i + q];
    inverse4_f64(E, w2c);
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c)
            nw[4 * r + c] = T[4 * r] * w2c[c] + T[4 * r + 1] * w2c[4 + c] + T[4 * r + 2] * w2c[8 + c] + T[4 * r + 3] * w2c[12 + c];
    inverse4_f64(nw, out);
#pragma unroll
    for (int q = 0; q < 16; ++q) c2w[16 * i + q] = (float)out[q];
}

}  // namespace gsr

extern "C" {

__attribute__((visibility("default"))) size_t gsr_image_scores_scratch_bytes(int64_t N, int C, int H, int W)
{
    int strips, chunks;
    long long blocks;
    if (!gsr::scores_grid(N, C, H, W, strips, chunks, blocks)) return 0;
    return (size_t)blocks * 2 * sizeof(double);
}

__attribute__((visibility("default"))) int gsr_image_scores(const float *gt, const float *pred, int64_t N, int C, int H, int W,
                                                            float *ssim, float *mse, void *scratch, void *stream)
{
    int strips, chunks;
    long long blocks;
    if (!gt || !pred || !ssim || !mse || !scratch || !gsr::scores_grid(N, C, H, W, strips, chunks, blocks)) return GSR_EINVAL;
    gsr::SsimWindow win;
    double w[gsr::SC_WIN], sum = 0.0;
    for (int q = 0; q < gsr::SC_WIN; ++q) {                  // scipy _gaussian_kernel1d(sigma 1.5, radius 5), normalised in float64
        const double x = q - gsr::SC_R;
        w[q] = exp(-0.5 / (1.5 * 1.5) * x * x);
        sum += w[q];
    }
    for (int q = 0; q < gsr::SC_WIN; ++q) win.w[q] = (float)(w[q] / sum);
    const hipStream_t st = static_cast<hipStream_t>(stream);
    double *partial = static_cast<double *>(scratch);
    (void)hipGetLastError();
    hipLaunchKernelGGL(gsr::k_image_scores, dim3((unsigned)blocks), dim3(64), 0, st, gt, pred, H, W, strips, chunks, win, partial);
    const double inv_ssim = 1.0 / ((double)C * (H - 2 * gsr::SC_R) * (W - 2 * gsr::SC_R)), inv_mse = 1.0 / ((double)C * H * W);
    hipLaunchKernelGGL(gsr::k_image_scores_fold, dim3((unsigned)N), dim3(64), 0, st, partial, C * strips * chunks, inv_ssim, inv_mse,
                       ssim, mse);
    return gsr::launch_status();
}

__attribute__((visibility("default"))) int gsr_pose_adam_update(float *c2w, float *m, float *v, const float *grad_rot, const float *grad_trans,
                                                                int64_t n, int step, float lr_rot, float lr_trans, float beta1, float beta2,
                                                                float eps, void *stream)
{
    if (!c2w || !m || !v || !grad_rot || !grad_trans || n < 1 || step < 1) return GSR_EINVAL;
    // torch.optim.Adam (capturable=False): the bias corrections and the step size are host doubles, used by the fp32 kernel as floats
    const double bc1 = 1.0 - pow((double)beta1, step), bc2 = 1.0 - pow((double)beta2, step);
    (void)hipGetLastError();
    hipLaunchKernelGGL(gsr::k_pose_adam, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, static_cast<hipStream_t>(stream), c2w, m, v, grad_rot,
                       grad_trans, (long long)n, (float)(lr_rot / bc1), (float)(lr_trans / bc1), beta1, beta2, eps, (float)sqrt(bc2));
    return gsr::launch_status();
}

}  // extern "C"
