// gsr_ssim.hip -- everything that filters with the separable 11-tap Gaussian window: ONE walk over a tile, three thin kernels.
//
// gsr_image_scores: SSIM (`compute_ssim`, src/evaluation/metrics.py:38-52 = skimage structural_similarity with win_size 11,
//   gaussian_weights, sample covariance, data_range 1, channel_axis 0) and the mean squared error of the clipped images that PSNR
//   is formed from (`compute_psnr`, :11-20), from ONE pass over both images, plus a small launch that folds the per-tile partial
//   sums of every image in index order (deterministic, no float atomics, an image's result does not depend on the batch).
//   Each pixel's squared error is counted by exactly one wave: the strip owns its 64 columns (the last strip also its halo), the chunk
//   its first 32 rows (the last chunk every row to the bottom edge).
//
// gsr_ssim_structure_fwd / _bwd: `1 - structure` of src/loss/loss_ssim.py:80-124 (data_range 1, K = (0.01, 0.03), valid 11 x 11 window,
//   compensation 1, eps^2 / min / 0.98 clamps).  The moments are summed in float64 and kept in fp32.  The forward optionally leaves the
//   three per-pixel adjoint maps (d/d mu2, d/d E[y^2], d/d E[xy]); the backward is the same walk over those maps, zero-padded by 10 on
//   every side (the transposed filter), combined with the pixel's own x and y.
//
// The two host-side windows differ on purpose: gsr_image_scores builds scipy's, normalised in float64; gsr_ssim_structure_* take the
// caller's fp32 window.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/gsr.h"
#include "gsr_common.h"

namespace gsr {
namespace ssim {

constexpr int COLS = 64;                          // output columns per wave, one per lane
constexpr int ROWS = 32;                          // output rows per wave
constexpr int R = 5;                              // window radius: int(truncate 3.5 * sigma 1.5 + 0.5)
constexpr int WIN = 2 * R + 1;                    // 11
constexpr int IN = COLS + 2 * R;                  // 74 staged columns per row

struct Window {
    float w[WIN];
};

// ---- the walk ------------------------------------------------------------------------------------------------------------------------
// Tiling: one wave per (plane, strip of 64 output columns, chunk of 32 output rows).  Lane j owns output column j of the strip.  The wave
// walks down the 42 input rows of its chunk: every row (74 columns: the strip and its 10-column halo) is staged through LDS, each lane
// filters it horizontally (11 taps) into a ring of the 11 most recent rows held in registers, and from the 11th row on filters the ring
// vertically into one output value.  Only outputs whose 11 x 11 window lies inside the input are formed (skimage's crop of 5 from every
// edge, the loss's valid convolution), so no boundary mode ever matters.  Read amplification over the input planes:
// (32+10)/32 rows x 74/64 columns = 1.52 for a full tile, 1.42 at 256 x 256 (narrower last strip and chunk; the re-read halo is
// L2-resident).
// A forward walk has the image as input and the (H-10) x (W-10) map as output; the backward has the map, zero-padded by 10 on every
// side, as input and the image as output, so its input coordinates are the output's minus 10 (`shift` below).
struct Tile {
    long long blk, plane;
    int strip, chunk;
    int c0;                                       // first output column of the strip = first staged column + shift
    int first, last;                              // input rows [first, last) of the walk; the output row of input row r is r - shift - 2 R
    bool out_col;                                 // this lane's output column exists
};

// `strips` x `chunks` tiles per plane cover out_rows x out_cols outputs (tile_grid); blockIdx.x = (plane * chunks + chunk) * strips + strip
__device__ __forceinline__ Tile tile_decode(int strips, int chunks, int out_rows, int out_cols, int shift)
{
    Tile t;
    const int tiles = strips * chunks;
    t.blk = blockIdx.x;
    t.plane = t.blk / tiles;
    const int i = (int)(t.blk - t.plane * tiles);
    t.chunk = i / strips;
    t.strip = i - t.chunk * strips;
    t.c0 = t.strip * COLS;
    t.first = t.chunk * ROWS + shift;
    t.last = min(t.chunk * ROWS + ROWS, out_rows) + 2 * R + shift;
    t.out_col = t.c0 + (int)threadIdx.x < out_cols;
    return t;
}

// The horizontal step of one tap, and the type both filters accumulate in (the ring itself is fp32).
// Five moments x, y, x^2, y^2, xy of two planes: in fp32 (SSIM score), or in float64 -- the products of fp32 values are exact in it and
// the variances are differences of these sums (structure term).
template <class T>
struct Moments {
    using acc_t = T;
    static constexpr int NF = 5;
    static __device__ __forceinline__ void step(T (&h)[NF], float w, const float (&v)[2])
    {
        const T a = (T)v[0], c = (T)v[1], wa = (T)w * a, wc = (T)w * c;
        h[0] += wa; h[1] += wc; h[2] += wa * a; h[3] += wc * c; h[4] += wa * c;
    }
};
// NP plain filters, one per plane
template <int NP>
struct Plain {
    using acc_t = float;
    static constexpr int NF = NP;
    static __device__ __forceinline__ void step(float (&h)[NF], float w, const float (&v)[NP])
    {
#pragma unroll
        for (int p = 0; p < NP; ++p) h[p] += w * v[p];
    }
};

// load(r, main, halo):  this lane's main and halo value of input row r of each of the NP planes (halo: lanes < 10 only)
// on_row(r, main, halo): hook per input row, before it is staged
// output(r, m):          hook per output value: input row r completes the window, m the NF filtered values
// Every staged value has origin[p] subtracted (the forwards' shift against cancellation, see k_image_scores).
template <class Filter, int NP, class Load, class OnRow, class Output>
__device__ __forceinline__ void window_walk(const Tile &t, const Window &win, const float (&origin)[NP], Load load, OnRow on_row, Output output)
{
    using acc_t = typename Filter::acc_t;
    constexpr int NF = Filter::NF;
    __shared__ float lds[2][NP][IN];
    const int lane = threadIdx.x;
    float vm[NP], vh[NP];
    load(t.first, vm, vh);

    float ring[WIN][NF];
    for (int rb = t.first; rb < t.last; rb += WIN) {
#pragma unroll
        for (int j = 0; j < WIN; ++j) {                                        // row rb + j goes to ring slot j (static indices)
            const int r = rb + j;
            if (r >= t.last) continue;                                         // (uniform; no break: it stops the unrolling)
            on_row(r, vm, vh);
            const int b = (r - t.first) & 1;                                   // two buffers: one barrier per row
#pragma unroll
            for (int p = 0; p < NP; ++p) lds[b][p][lane] = vm[p] - origin[p];
            if (lane < 2 * R) {
#pragma unroll
                for (int p = 0; p < NP; ++p) lds[b][p][COLS + lane] = vh[p] - origin[p];
            }
            if (r + 1 < t.last) load(r + 1, vm, vh);                           // in flight while this row is filtered
            __syncthreads();
            acc_t h[NF];
#pragma unroll
            for (int f = 0; f < NF; ++f) h[f] = (acc_t)0;
#pragma unroll
            for (int q = 0; q < WIN; ++q) {
                float v[NP];
#pragma unroll
                for (int p = 0; p < NP; ++p) v[p] = lds[b][p][lane + q];
                Filter::step(h, win.w[q], v);
            }
#pragma unroll
            for (int f = 0; f < NF; ++f) ring[j][f] = (float)h[f];
            if (r - t.first >= 2 * R && t.out_col) {                           // rows r-10 .. r are in slots j+1 .. j (mod 11)
                acc_t m[NF];
#pragma unroll
                for (int f = 0; f < NF; ++f) m[f] = (acc_t)0;
#pragma unroll
                for (int i = 0; i < WIN; ++i) {
                    const int sl = (j + 1 + i) % WIN;
                    const acc_t w = (acc_t)win.w[i];
#pragma unroll
                    for (int f = 0; f < NF; ++f) m[f] += w * (acc_t)ring[sl][f];
                }
                output(r, m);
            }
        }
    }
}

// rows of the two image planes of a forward walk: the strip's 64 columns and, in lanes < 10, its halo
struct ImagePair {
    const float *X, *Y;
    int W, cm, ch;                                                             // main / halo column of this lane
    bool in_m, in_h;
    __device__ __forceinline__ ImagePair(const float *gt, const float *pred, int H, int W_, const Tile &t)
        : X(gt + (size_t)t.plane * H * W_), Y(pred + (size_t)t.plane * H * W_), W(W_), cm(t.c0 + (int)threadIdx.x),
          ch(t.c0 + COLS + (int)threadIdx.x), in_m(cm < W_), in_h((int)threadIdx.x < 2 * R && ch < W_) {}
    __device__ __forceinline__ void operator()(int r, float (&m)[2], float (&h)[2]) const
    {
        const size_t o = (size_t)r * W;
        // (zeroes first, then the guarded loads: written as `in_m ? X[..] : 0.f` the zero lands in the register AFTER the load was issued and
        //  the compiler waits for the load on the spot -- the prefetch then overlaps nothing: measured, k_image_scores + 10 %)
        m[0] = m[1] = h[0] = h[1] = 0.f;
        if (in_m) { m[0] = X[o + cm]; m[1] = Y[o + cm]; }
        if (in_h) { h[0] = X[o + ch]; h[1] = Y[o + ch]; }
    }
};

__device__ inline float clip01(float v) { return fminf(fmaxf(v, 0.f), 1.f); }

// ---- SSIM score + clipped squared error ---------------------------------------------------------------------------------------------
constexpr float SC_C1 = 1e-4f, SC_C2 = 9e-4f;     // (0.01 data_range)^2, (0.03 data_range)^2
constexpr float SC_COV_NORM = 121.0f / 120.0f;    // use_sample_covariance: NP / (NP - 1), NP = 11^2

// Cancellation: the moments are formed of x - kx and y - ky, kx / ky the images' values at the tile's first pixel; variances and
// the covariance do not change under that shift and the means get it added back.
__global__ void __launch_bounds__(64) k_image_scores(const float *__restrict__ gt, const float *__restrict__ pred, int H, int W,
                                                     int strips, int chunks, Window win, double *__restrict__ partial)
{
    const Tile t = tile_decode(strips, chunks, H - 2 * R, W - 2 * R, 0);
    const ImagePair in(gt, pred, H, W, t);
    const float k[2] = {in.X[(size_t)t.first * W + t.c0], in.Y[(size_t)t.first * W + t.c0]};
    const int own_rows = (t.chunk == chunks - 1) ? H - t.first : ROWS;
    const bool own_h = t.strip == strips - 1;                                  // a halo column belongs to the last strip only
    double acc_s = 0.0, acc_e = 0.0;
    window_walk<Moments<float>>(
        t, win, k, in,
        [&](int r, const float (&m)[2], const float (&h)[2]) {
            if (r - t.first < own_rows) {
                float e = 0.f;
                if (in.in_m) { const float d = clip01(m[0]) - clip01(m[1]); e = d * d; }
                if (in.in_h && own_h) { const float d = clip01(h[0]) - clip01(h[1]); e += d * d; }
                acc_e += (double)e;
            }
        },
        [&](int, const float (&m)[5]) {
            const float vx = SC_COV_NORM * (m[2] - m[0] * m[0]), vy = SC_COV_NORM * (m[3] - m[1] * m[1]), vxy = SC_COV_NORM * (m[4] - m[0] * m[1]);
            const float ux = m[0] + k[0], uy = m[1] + k[1];
            const float a1 = 2.f * ux * uy + SC_C1, a2 = 2.f * vxy + SC_C2;
            const float b1 = ux * ux + uy * uy + SC_C1, b2 = vx + vy + SC_C2;
            acc_s += (double)((a1 * a2) / (b1 * b2));
        });
    acc_s = wave_sum(acc_s);
    acc_e = wave_sum(acc_e);
    if (threadIdx.x == 0) { partial[2 * t.blk] = acc_s; partial[2 * t.blk + 1] = acc_e; }
}

// ---- SSIM structure term ------------------------------------------------------------------------------------------------------------
constexpr float SS_C3 = 0.5f * (0.03f * 0.03f);                       // C2 / 2, C2 = (K2 data_range)^2
constexpr float SS_EPS2 = 1.1920928955078125e-07f * 1.1920928955078125e-07f;   // finfo(float32).eps^2
constexpr float SS_CLAMP = 0.98f;

__global__ void __launch_bounds__(64) k_ssim_struct_fwd(const float *__restrict__ gt, const float *__restrict__ pred, int H, int W, int strips,
                                                        int chunks, Window win, double wsum2, double *__restrict__ partial,
                                                        float *__restrict__ maps, size_t map_stride)
{
    const int Ho = H - 2 * R, Wo = W - 2 * R;
    const Tile t = tile_decode(strips, chunks, Ho, Wo, 0);
    const ImagePair in(gt, pred, H, W, t);
    const float k[2] = {in.X[(size_t)t.first * W + t.c0], in.Y[(size_t)t.first * W + t.c0]};
    double acc = 0.0;
    window_walk<Moments<double>>(
        t, win, k, in, [](int, const float (&)[2], const float (&)[2]) {},
        [&](int r, const double (&m)[5]) {
            // The fp32-normalised taps do not sum to 1 exactly (wsum2 = (sum w)^2 over the 11 x 11 window), so variances are NOT
            // invariant under the shift: sum w x^2 - (sum w x)^2 = m2 - m0^2 + (1 - wsum2) (2 kx m0 + kx^2 wsum2) for x = a + kx.
            const double oms = 1.0 - wsum2, dkx = (double)k[0], dky = (double)k[1];
            const float s1 = (float)(m[2] - m[0] * m[0] + oms * (2.0 * dkx * m[0] + dkx * dkx * wsum2));
            const float s2 = (float)(m[3] - m[1] * m[1] + oms * (2.0 * dky * m[1] + dky * dky * wsum2));
            const float c = (float)(m[4] - m[0] * m[1] + oms * (dkx * m[1] + dky * m[0] + dkx * dky * wsum2));
            const float ux = (float)(m[0] + dkx * wsum2), uy = (float)(m[1] + dky * wsum2);      // sum w x, sum w y
            const float v1 = fmaxf(s1, SS_EPS2), v2 = fmaxf(s2, SS_EPS2);
            const float pr = sqrtf(v1 * v2), ac = fabsf(c);
            const bool capped = ac > pr;
            const float cp = capped ? copysignf(pr, c) : c;
            const float q1 = sqrtf(v1), q2 = sqrtf(v2);
            const float D = q1 * q2 + SS_C3;
            const float sv = (cp + SS_C3) / D;
            const bool clamped = sv > SS_CLAMP;
            acc += (double)(clamped ? SS_CLAMP : sv);
            if (maps) {
                float a_mu = 0.f, a_yy = 0.f, a_c = 0.f;
                if (!clamped) {
                    const float invD = 1.f / D;
                    a_c = capped ? 0.f : invD;
                    float dv2 = -(sv * invD) * (q1 / (2.f * q2));
                    if (capped) dv2 += copysignf(invD, c) * (v1 / (2.f * pr));
                    a_yy = (s2 < SS_EPS2) ? 0.f : dv2;
                    a_mu = -2.f * uy * a_yy - ux * a_c;
                }
                const size_t o = ((size_t)t.plane * Ho + (r - 2 * R)) * Wo + in.cm;
                maps[o] = a_mu; maps[map_stride + o] = a_yy; maps[2 * map_stride + o] = a_c;
            }
        });
    acc = wave_sum(acc);
    if (threadIdx.x == 0) partial[t.blk] = acc;
}

// one wave per (plane, strip of 64 image columns, chunk of 32 image rows): the valid filter of the adjoint maps padded with 10 zeros.
// `win` holds the taps reversed (the transposed filter).
__global__ void __launch_bounds__(64) k_ssim_struct_bwd(const float *__restrict__ gt, const float *__restrict__ pred,
                                                        const float *__restrict__ maps, size_t map_stride, const float *__restrict__ grad_out,
                                                        float inv_norm, int C, int H, int W, int strips, int chunks, Window win,
                                                        float *__restrict__ grad)
{
    const int lane = threadIdx.x;
    const int Ho = H - 2 * R, Wo = W - 2 * R;
    const Tile t = tile_decode(strips, chunks, H, W, -2 * R);
    const float *X = gt + (size_t)t.plane * H * W, *Y = pred + (size_t)t.plane * H * W;
    const float *A0 = maps + (size_t)t.plane * Ho * Wo, *A1 = A0 + map_stride, *A2 = A1 + map_stride;
    const float scale = grad_out[t.plane / C] * inv_norm;
    const int mc = t.c0 - 2 * R + lane, hc = t.c0 + COLS - 2 * R + lane;       // main / halo map column of this lane
    const bool in_m = mc >= 0 && mc < Wo, in_h = lane < 2 * R && hc < Wo;
    const int ci = t.c0 + lane;
    const float none[3] = {0.f, 0.f, 0.f};
    window_walk<Plain<3>>(
        t, win, none,
        [&](int m, float (&am)[3], float (&ah)[3]) {
            const bool row = m >= 0 && m < Ho;                                 // (uniform)
            const size_t o = (size_t)(row ? m : 0) * Wo;
            const bool pm = row && in_m, ph = row && in_h;                     // (one predicate per group: three loads under one branch)
            am[0] = pm ? A0[o + mc] : 0.f; am[1] = pm ? A1[o + mc] : 0.f; am[2] = pm ? A2[o + mc] : 0.f;
            ah[0] = ph ? A0[o + hc] : 0.f; ah[1] = ph ? A1[o + hc] : 0.f; ah[2] = ph ? A2[o + hc] : 0.f;
        },
        [](int, const float (&)[3], const float (&)[3]) {},
        [&](int m, const float (&v)[3]) {                                      // map rows m-10 .. m end at image row m
            const size_t o = (size_t)m * W + ci;
            grad[(size_t)t.plane * H * W + o] = scale * (v[0] + 2.f * Y[o] * v[1] + X[o] * v[2]);
        });
}

// ---- per-image fold -----------------------------------------------------------------------------------------------------------------
template <int NS>
struct FoldOut {
    float *out[NS];
    double inv[NS];
};

// one wave per image: its C * tiles partials (NS interleaved sums per tile) in index order
template <int NS>
__global__ void __launch_bounds__(64) k_tile_fold(const double *__restrict__ partial, int per_image, FoldOut<NS> o)
{
    const long long n = blockIdx.x;
    const double *p = partial + NS * n * per_image;
    double s[NS];
#pragma unroll
    for (int q = 0; q < NS; ++q) s[q] = 0.0;
    for (int i = threadIdx.x; i < per_image; i += 64) {
#pragma unroll
        for (int q = 0; q < NS; ++q) s[q] += p[NS * i + q];
    }
#pragma unroll
    for (int q = 0; q < NS; ++q) {
        s[q] = wave_sum(s[q]);
        if (threadIdx.x == 0) o.out[q][n] = (float)(s[q] * o.inv[q]);
    }
}

// ---- host -----------------------------------------------------------------------------------------------------------------------------
// image_rows: the tiles cover the H x W image (backward), not the (H-10) x (W-10) map
static bool tile_grid(int64_t N, int C, int H, int W, bool image_rows, int &strips, int &chunks, long long &blocks)
{
    if (N < 1 || C < 1 || H < WIN || W < WIN) return false;
    const int cols = image_rows ? W : W - 2 * R, rows = image_rows ? H : H - 2 * R;
    strips = (cols + COLS - 1) / COLS;
    chunks = (rows + ROWS - 1) / ROWS;
    blocks = (long long)N * C * strips * chunks;
    return blocks <= 0x7fffffffLL && (long long)N * C * H * W <= 0x7fffffffffLL;
}

// NS doubles per tile of the map
static size_t partial_bytes(int64_t N, int C, int H, int W, int NS)
{
    int strips, chunks;
    long long blocks;
    if (!tile_grid(N, C, H, W, false, strips, chunks, blocks)) return 0;
    return (size_t)blocks * NS * sizeof(double);
}

}  // namespace ssim
}  // namespace gsr

extern "C" {

using namespace gsr::ssim;

__attribute__((visibility("default"))) size_t gsr_image_scores_scratch_bytes(int64_t N, int C, int H, int W) { return partial_bytes(N, C, H, W, 2); }

__attribute__((visibility("default"))) int gsr_image_scores(const float *gt, const float *pred, int64_t N, int C, int H, int W,
                                                            float *ssim, float *mse, void *scratch, void *stream)
{
    int strips, chunks;
    long long blocks;
    if (!gt || !pred || !ssim || !mse || !scratch || !tile_grid(N, C, H, W, false, strips, chunks, blocks)) return GSR_EINVAL;
    Window win;
    double w[WIN], sum = 0.0;
    for (int q = 0; q < WIN; ++q) {                          // scipy _gaussian_kernel1d(sigma 1.5, radius 5), normalised in float64
        const double x = q - R;
        w[q] = exp(-0.5 / (1.5 * 1.5) * x * x);
        sum += w[q];
    }
    for (int q = 0; q < WIN; ++q) win.w[q] = (float)(w[q] / sum);
    const hipStream_t st = static_cast<hipStream_t>(stream);
    double *partial = static_cast<double *>(scratch);
    (void)hipGetLastError();
    hipLaunchKernelGGL(k_image_scores, dim3((unsigned)blocks), dim3(64), 0, st, gt, pred, H, W, strips, chunks, win, partial);
    const FoldOut<2> out = {{ssim, mse}, {1.0 / ((double)C * (H - 2 * R) * (W - 2 * R)), 1.0 / ((double)C * H * W)}};
    hipLaunchKernelGGL(k_tile_fold<2>, dim3((unsigned)N), dim3(64), 0, st, partial, C * strips * chunks, out);
    return gsr::launch_status();
}

__attribute__((visibility("default"))) size_t gsr_ssim_structure_scratch_bytes(int64_t N, int C, int H, int W) { return partial_bytes(N, C, H, W, 1); }

__attribute__((visibility("default"))) int gsr_ssim_structure_fwd(const float *target, const float *pred, int64_t N, int C, int H, int W,
                                                                  const float *window, float *structure, float *maps, void *scratch,
                                                                  void *stream)
{
    int strips, chunks;
    long long blocks;
    if (!target || !pred || !window || !structure || !scratch || !tile_grid(N, C, H, W, false, strips, chunks, blocks)) return GSR_EINVAL;
    Window win;
    double wsum = 0.0;
    for (int q = 0; q < WIN; ++q) { win.w[q] = window[q]; wsum += (double)window[q]; }
    const hipStream_t st = static_cast<hipStream_t>(stream);
    double *partial = static_cast<double *>(scratch);
    const size_t map_stride = (size_t)N * C * (H - 2 * R) * (W - 2 * R);
    (void)hipGetLastError();
    hipLaunchKernelGGL(k_ssim_struct_fwd, dim3((unsigned)blocks), dim3(64), 0, st, target, pred, H, W, strips, chunks, win, wsum * wsum, partial,
                       maps, map_stride);
    const FoldOut<1> out = {{structure}, {1.0 / ((double)C * (H - 2 * R) * (W - 2 * R))}};
    hipLaunchKernelGGL(k_tile_fold<1>, dim3((unsigned)N), dim3(64), 0, st, partial, C * strips * chunks, out);
    return gsr::launch_status();
}

__attribute__((visibility("default"))) int gsr_ssim_structure_bwd(const float *target, const float *pred, const float *maps,
                                                                  const float *grad_structure, int64_t N, int C, int H, int W,
                                                                  const float *window, float *grad_pred, void *stream)
{
    int strips, chunks;
    long long blocks;
    if (!target || !pred || !maps || !grad_structure || !window || !grad_pred || !tile_grid(N, C, H, W, true, strips, chunks, blocks))
        return GSR_EINVAL;
    Window win;
    for (int q = 0; q < WIN; ++q) win.w[q] = window[WIN - 1 - q];             // the transposed filter
    const size_t map_stride = (size_t)N * C * (H - 2 * R) * (W - 2 * R);
    const float inv_norm = (float)(1.0 / ((double)C * (H - 2 * R) * (W - 2 * R)));
    (void)hipGetLastError();
    hipLaunchKernelGGL(k_ssim_struct_bwd, dim3((unsigned)blocks), dim3(64), 0, static_cast<hipStream_t>(stream), target, pred, maps, map_stride,
                       grad_structure, inv_norm, C, H, W, strips, chunks, win, grad_pred);
    return gsr::launch_status();
}

}  // extern "C"
