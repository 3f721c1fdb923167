// gsr_inputs.hip -- what comes before a prepared batch: decoded frames are rescaled with the Lanczos-3 filter, cropped, mirrored and
// turned into planar fp32 on the device (src/dataset/shims/crop_shim.py::rescale / center_crop / rescale_and_crop and the flip of
// augmentation_shim.py::reflect_views).  The reference does this per image on the host through PIL's 8-bit resize; the result here is
// the same bytes, so a model trained behind the reference's loader sees the same pixels.
//
//   gsr_resample_plan  : host only.  One axis plan (n -> m): per output index the first tap, the tap count and the taps as 22-bit
//                        fixed point, from float64 weights through libm's sin.  One ulp in a weight can flip a coefficient, so the
//                        plans are never computed on the device.
//   gsr_resample_crop  : two launches.  k_resample_h quantises the source to bytes (fp32 planar) or takes them as they are (uint8
//                        interleaved), reads it mirrored where the image's flip flag says so, and filters along x -- only the columns
//                        of the crop window and only the rows the vertical taps of the window touch -- into a planar byte
//                        intermediate.  k_resample_v filters along y out of it, four columns per lane from one dword, and stores
//                        byte / 255 as fp32.  The rounding to bytes between the passes is part of the result.
//
// Integer arithmetic only between the quantisation and the final division: int32 accumulators, 2^21 added before the arithmetic
// shift by 22, clamp to 0..255.  Tap loops run over the plan's counts (11 taps at 360 -> 256, 51 at 8:1, no upper bound).  A block
// of k_resample_h stages the source segment of its 256 columns x 4 rows in LDS when it fits RS_LDS_BYTES and reads global memory
// tap by tap when it does not (or under GSR_RESAMPLE_DIRECT, which lets a test hold both to the same bytes).
// No host sync, no read-back, no atomics: two runs give the same bits and image n's result does not depend on N.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/gsr.h"
#include "gsr_common.h"

namespace gsr {

constexpr int RS_BLOCK = 256, RS_ROWS = 4, RS_LDS_BYTES = 16384, RS_BITS = 22;
constexpr double RS_PI = 3.14159265358979323846;

// ---- the axis plan (host, float64) ----
struct AxisGeom {
    double scale, fs, support;
    int ksize;
};

static AxisGeom axis_geom(int n, int m)
{
    AxisGeom g;
    g.scale = (double)n / (double)m;
    g.fs = g.scale < 1.0 ? 1.0 : g.scale;
    g.support = 3.0 * g.fs;
    g.ksize = 2 * (int)ceil(g.support) + 1;
    return g;
}

static void axis_bounds(const AxisGeom &g, int n, int i, int &x0, int &cnt)
{
    const double c = (i + 0.5) * g.scale;
    x0 = (int)(c - g.support + 0.5);
    if (x0 < 0) x0 = 0;
    int x1 = (int)(c + g.support + 0.5);
    if (x1 > n) x1 = n;
    cnt = x1 - x0;
}

static double sinc(double t)
{
    if (t == 0.0) return 1.0;
    t = t * RS_PI;
    return sin(t) / t;
}

static double lanczos3(double t) { return (-3.0 <= t && t < 3.0) ? sinc(t) * sinc(t / 3.0) : 0.0; }

// source rows [lo, lo + R) that the vertical taps of output rows [top, top + out_h) read
static void row_range(int H, int scaled_h, int top, int out_h, int &lo, int &R)
{
    if (scaled_h == H) { lo = top; R = out_h; return; }
    const AxisGeom g = axis_geom(H, scaled_h);
    int x0, cnt, x1, cnt1;
    axis_bounds(g, H, top, x0, cnt);
    axis_bounds(g, H, top + out_h - 1, x1, cnt1);
    lo = x0;
    R = x1 + cnt1 - x0;
}

static bool resample_dims_ok(int64_t N, int H, int W, int scaled_h, int scaled_w, int top, int left, int out_h, int out_w)
{
    const int lim = 1 << 24;
    if (N < 1 || N > 21845 || H < 1 || W < 1 || scaled_h < 1 || scaled_w < 1 || H > lim || W > lim || scaled_h > lim || scaled_w > lim) return false;
    if (top < 0 || left < 0 || out_h < 1 || out_w < 1 || out_h > scaled_h - top || out_w > scaled_w - left) return false;
    return true;
}

struct RsArgs {
    const void *src;
    const int32_t *plan_x, *plan_y;      // device: [m][2] (first tap, count) then [m][ksize] coefficients; null = axis unchanged
    const int32_t *flip;                 // device [N] or null
    uint8_t *mid;                        // [N][3][R][pitch]
    float *out;                          // [N][3][out_h][out_w]
    int src_f32, N, H, W, scaled_h, scaled_w, kx, ky, top, left, out_h, out_w, row_lo, R, pitch, direct;
};

// uint8(clip(x * 255, 0, 255)), the product in fp32, the cast truncating; NaN -> 0 (fmaxf returns the other operand)
__device__ inline uint32_t rs_quantise(float x) { return (uint32_t)(int)fminf(fmaxf(x * 255.0f, 0.0f), 255.0f); }

__device__ inline uint32_t rs_source(const RsArgs &a, long long n, int y, int x, int c, bool flip)
{
    const int sx = flip ? a.W - 1 - x : x;
    if (a.src_f32) return rs_quantise(static_cast<const float *>(a.src)[((n * 3 + c) * a.H + y) * (long long)a.W + sx]);
    return static_cast<const uint8_t *>(a.src)[((n * a.H + y) * (long long)a.W + sx) * 3 + c];
}

__device__ inline void rs_taps(const int32_t *plan, int idx, int n_in, int ksize, int &x0, int &cnt)
{
    x0 = min(max(plan[2 * idx], 0), n_in);
    cnt = min(min(max(plan[2 * idx + 1], 0), ksize), n_in - x0);
}

// horizontal pass: block = 256 output columns x RS_ROWS source rows of one image
__global__ void __launch_bounds__(RS_BLOCK) k_resample_h(RsArgs a)
{
    __shared__ uint8_t seg[RS_LDS_BYTES];
    const int tid = threadIdx.x, j0 = blockIdx.x * RS_BLOCK, j1 = min(a.out_w, j0 + RS_BLOCK), j = j0 + tid;
    const int r0 = blockIdx.y * RS_ROWS, rows = min(RS_ROWS, a.R - r0);
    const long long n = blockIdx.z;
    const bool flip = a.flip && a.flip[n] != 0;
    const int32_t *coef = a.plan_x ? a.plan_x + 2 * (size_t)a.scaled_w : nullptr;
    // the source columns this block's taps cover (first taps and ends are both non-decreasing in the output index)
    int xs, xe, t0, tc;
    if (a.plan_x) {
        rs_taps(a.plan_x, a.left + j0, a.W, a.kx, xs, tc);
        rs_taps(a.plan_x, a.left + j1 - 1, a.W, a.kx, t0, tc);
        xe = t0 + tc;
    } else {
        xs = a.left + j0;
        xe = a.left + j1;
    }
    const int span = max(xe - xs, 0);
    const bool staged = !a.direct && (long long)RS_ROWS * span * 3 <= RS_LDS_BYTES;
    if (staged) {
        const int row_bytes = span * 3, total = rows * row_bytes;
        if (a.src_f32) {                                  // planar source: consecutive lanes walk one channel's row
            for (int t = tid; t < total; t += RS_BLOCK) {
                const int rr = t / row_bytes, rem = t - rr * row_bytes, c = rem / span, p = rem - c * span;
                seg[rr * row_bytes + p * 3 + c] = (uint8_t)rs_source(a, n, a.row_lo + r0 + rr, xs + p, c, flip);
            }
        } else {                                          // interleaved source: consecutive lanes walk consecutive bytes
            for (int t = tid; t < total; t += RS_BLOCK) {
                const int rr = t / row_bytes, rem = t - rr * row_bytes, p = rem / 3, c = rem - p * 3;
                seg[t] = (uint8_t)rs_source(a, n, a.row_lo + r0 + rr, xs + p, c, flip);
            }
        }
    }
    __syncthreads();
    if (j >= a.out_w) return;
    int x0, cnt;
    if (a.plan_x) rs_taps(a.plan_x, a.left + j, a.W, a.kx, x0, cnt);
    else { x0 = a.left + j; cnt = 1; }
    x0 = max(x0, xs);                                     // (a consistent plan never needs these two)
    cnt = min(cnt, xe - x0);
    int acc[RS_ROWS][3];
    for (int rr = 0; rr < RS_ROWS; ++rr) acc[rr][0] = acc[rr][1] = acc[rr][2] = 1 << (RS_BITS - 1);
    const int32_t *cw = coef ? coef + (size_t)(a.left + j) * a.kx : nullptr;
    for (int k = 0; k < cnt; ++k) {
        const int w = cw ? cw[k] : (1 << RS_BITS);
        if (staged) {
            const uint8_t *p = seg + (x0 - xs + k) * 3;
#pragma unroll
            for (int rr = 0; rr < RS_ROWS; ++rr)
                if (rr < rows) {
                    const uint8_t *q = p + rr * span * 3;
                    acc[rr][0] += (int)q[0] * w; acc[rr][1] += (int)q[1] * w; acc[rr][2] += (int)q[2] * w;
                }
        } else {
#pragma unroll
            for (int rr = 0; rr < RS_ROWS; ++rr)
                if (rr < rows)
                    for (int c = 0; c < 3; ++c) acc[rr][c] += (int)rs_source(a, n, a.row_lo + r0 + rr, x0 + k, c, flip) * w;
        }
    }
#pragma unroll
    for (int rr = 0; rr < RS_ROWS; ++rr)
        if (rr < rows)
            for (int c = 0; c < 3; ++c)
                a.mid[((n * 3 + c) * a.R + r0 + rr) * (long long)a.pitch + j] = (uint8_t)min(max(acc[rr][c] >> RS_BITS, 0), 255);
}

// vertical pass: lane = four neighbouring columns of one output row of one plane
__global__ void __launch_bounds__(RS_BLOCK) k_resample_v(RsArgs a)
{
    const int groups = a.pitch >> 2;
    const long long t = (long long)blockIdx.x * RS_BLOCK + threadIdx.x;
    if (t >= (long long)a.out_h * groups) return;
    const int i = (int)(t / groups), g = (int)(t - (long long)i * groups);
    const long long plane = blockIdx.y;                   // n * 3 + c
    int y0, cnt;
    if (a.plan_y) rs_taps(a.plan_y, a.top + i, a.H, a.ky, y0, cnt);
    else { y0 = a.top + i; cnt = 1; }
    y0 = min(max(y0, a.row_lo), a.row_lo + a.R);          // (a consistent plan never needs these two)
    cnt = min(cnt, a.row_lo + a.R - y0);
    const int32_t *cw = a.plan_y ? a.plan_y + 2 * (size_t)a.scaled_h + (size_t)(a.top + i) * a.ky : nullptr;
    const uint8_t *col = a.mid + (plane * a.R + (y0 - a.row_lo)) * (long long)a.pitch + 4 * g;
    int acc[4] = {1 << (RS_BITS - 1), 1 << (RS_BITS - 1), 1 << (RS_BITS - 1), 1 << (RS_BITS - 1)};
    for (int k = 0; k < cnt; ++k) {
        const int w = cw ? cw[k] : (1 << RS_BITS);
        const uint32_t v = *reinterpret_cast<const uint32_t *>(col + (long long)k * a.pitch);
        acc[0] += (int)(v & 255u) * w;
        acc[1] += (int)((v >> 8) & 255u) * w;
        acc[2] += (int)((v >> 16) & 255u) * w;
        acc[3] += (int)(v >> 24) * w;
    }
    float *o = a.out + (plane * a.out_h + i) * (long long)a.out_w + 4 * g;
#pragma unroll
    for (int q = 0; q < 4; ++q)
        if (4 * g + q < a.out_w) o[q] = (float)min(max(acc[q] >> RS_BITS, 0), 255) / 255.0f;     // (correctly rounded division: == double / 255)
}

}  // namespace gsr

extern "C" {

__attribute__((visibility("default"))) int gsr_resample_plan(int n, int m, int32_t *ksize, int32_t *bounds, int32_t *coeffs)
{
    using namespace gsr;
    if (n < 1 || m < 1 || n > (1 << 24) || m > (1 << 24) || !ksize || (!bounds) != (!coeffs)) return GSR_EINVAL;
    const AxisGeom g = axis_geom(n, m);
    *ksize = g.ksize;
    if (!bounds) return GSR_OK;
    const double ss = 1.0 / g.fs;
    for (int i = 0; i < m; ++i) {
        int x0, cnt;
        axis_bounds(g, n, i, x0, cnt);
        const double c = (i + 0.5) * g.scale;
        double sum = 0.0;
        for (int x = 0; x < cnt; ++x) sum += lanczos3((x + x0 - c + 0.5) * ss);
        int32_t *k = coeffs + (size_t)i * g.ksize;
        for (int x = 0; x < g.ksize; ++x) {
            double w = x < cnt ? lanczos3((x + x0 - c + 0.5) * ss) : 0.0;       // (the same call as above: the same bits)
            if (x < cnt && sum != 0.0) w /= sum;
            k[x] = w < 0.0 ? (int32_t)(-0.5 + w * (double)(1 << RS_BITS)) : (int32_t)(0.5 + w * (double)(1 << RS_BITS));
        }
        bounds[2 * i] = x0;
        bounds[2 * i + 1] = cnt < 0 ? 0 : cnt;
    }
    return GSR_OK;
}

__attribute__((visibility("default"))) size_t gsr_resample_scratch_bytes(int64_t N, int H, int W, int scaled_h, int scaled_w, int top, int left,
                                                                         int out_h, int out_w)
{
    using namespace gsr;
    if (!resample_dims_ok(N, H, W, scaled_h, scaled_w, top, left, out_h, out_w)) return 0;
    int lo, R;
    row_range(H, scaled_h, top, out_h, lo, R);
    return (size_t)N * 3 * (size_t)R * align_up((size_t)out_w, 4);
}

__attribute__((visibility("default"))) int gsr_resample_crop(const void *src, int src_is_f32, int64_t N, int H, int W, const int32_t *plan_x,
                                                             int scaled_w, const int32_t *plan_y, int scaled_h, int top, int left, int out_h,
                                                             int out_w, const int32_t *flip, void *scratch, size_t scratch_bytes, float *out,
                                                             int flags, void *stream)
{
    using namespace gsr;
    if (!src || !scratch || !out || !resample_dims_ok(N, H, W, scaled_h, scaled_w, top, left, out_h, out_w)) return GSR_EINVAL;
    if ((plan_x == nullptr) != (scaled_w == W) || (plan_y == nullptr) != (scaled_h == H)) return GSR_EINVAL;
    if ((flags & ~GSR_RESAMPLE_DIRECT) || (reinterpret_cast<uintptr_t>(scratch) & 3)) return GSR_EINVAL;
    RsArgs a{};
    a.src = src; a.plan_x = plan_x; a.plan_y = plan_y; a.flip = flip; a.mid = static_cast<uint8_t *>(scratch); a.out = out;
    a.src_f32 = src_is_f32 ? 1 : 0; a.N = (int)N; a.H = H; a.W = W; a.scaled_h = scaled_h; a.scaled_w = scaled_w;
    a.kx = axis_geom(W, scaled_w).ksize; a.ky = axis_geom(H, scaled_h).ksize;
    a.top = top; a.left = left; a.out_h = out_h; a.out_w = out_w;
    row_range(H, scaled_h, top, out_h, a.row_lo, a.R);
    a.pitch = (int)align_up((size_t)out_w, 4);
    a.direct = (flags & GSR_RESAMPLE_DIRECT) ? 1 : 0;
    if (a.R < 1 || a.row_lo < 0 || a.row_lo + a.R > H) return GSR_EINVAL;
    if (scratch_bytes < (size_t)N * 3 * (size_t)a.R * (size_t)a.pitch) return GSR_ENOSPACE;
    const long long gy = (a.R + RS_ROWS - 1) / RS_ROWS, gv = ((long long)out_h * (a.pitch >> 2) + RS_BLOCK - 1) / RS_BLOCK;
    if (gy > 65535 || gv >= (1LL << 31)) return GSR_EINVAL;
    hipStream_t s = static_cast<hipStream_t>(stream);
    (void)hipGetLastError();
    hipLaunchKernelGGL(k_resample_h, dim3((unsigned)((out_w + RS_BLOCK - 1) / RS_BLOCK), (unsigned)gy, (unsigned)N), dim3(RS_BLOCK), 0, s, a);
    hipLaunchKernelGGL(k_resample_v, dim3((unsigned)gv, (unsigned)(N * 3)), dim3(RS_BLOCK), 0, s, a);
    return launch_status();
}

}  // extern "C"
