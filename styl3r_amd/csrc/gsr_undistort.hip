// gsr_undistort.hip -- lens undistortion of 8-bit frames in front of the Lanczos path (gsr_inputs.hip): what the reference's COLMAP
// drivers do per image on the host with initUndistortRectifyMap + remap(INTER_LINEAR) + a crop to the valid-pixel ROI, as ONE launch
// over all frames of a call with NO map arrays in memory.  A stored mapx / mapy pair costs 8 bytes per pixel next to the 3 + 3 bytes of
// the picture itself, so the source coordinate of every output pixel is evaluated in registers, in float64, from the camera row of its
// frame (include/gsr.h: K, distortion, new K, ROI origin).
//
//   map     x = (u - cx') / fx', y = (v - cy') / fy', r2 = x x + y y, kr = 1 + (k2 r2 + k1) r2,
//           xd = x kr + p1 (2 x y) + p2 (r2 + 2 x x), yd = y kr + p1 (r2 + 2 y y) + p2 (2 x y), mx = float32(fx xd + cx), my likewise
//   sample  sx = rint_half_even(mx * 32) (fp32 product), ix = sx >> 5, a = sx & 31, likewise iy, b;
//           byte = ((32 - a)(32 - b) p00 + a (32 - b) p01 + (32 - a) b p10 + a b p11 + 512) >> 10, a tap outside the image is 0;
//           a non-finite coordinate or |m| * 32 >= 2^30 gives 0
//   copy    a camera without distortion (row mode 0) is copied through its window, zero outside the frame
//
// Thread-to-pixel mapping: the output (N, roi_h, roi_w, 3) is walked FLAT, four pixels = twelve bytes = three dwords per thread, so that
// the interleaved 3-byte pixels leave as one 12-byte store per lane, contiguous across the wave (768 B per wave-instruction), whatever
// roi_w is; a group may straddle a row or a frame, its pixels advance (u, v, n) one by one.  Only the last group of a call can be
// partial and is stored byte by byte.  Source bytes are gathered tap by tap: neighbouring lanes read neighbouring source pixels and
// the taps of one pixel share cache lines, so the gather is served by L1 / L2.  No LDS, no scratch, no atomics; 64-bit indices.
// The frame -> camera table is validated on the HOST and travels in the kernel's argument block (no device table to trust).
//
// Floating-point contraction is off in this file: each product and sum rounds once, in the order written, which is the order of the
// host restatement in styl3r_amd/colmap.py.  fp64 division is IEEE; v_cvt with round-to-nearest-even gives the host's rint.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/gsr.h"
#include "gsr_common.h"

#pragma clang fp contract(off)

namespace gsr {

constexpr int UD_BLOCK = 256;
constexpr int UD_MAX_BLOCKS = 2048;
constexpr int UD_FRAMES = GSR_UNDISTORT_FRAMES_PER_LAUNCH;
constexpr int UD_ROW = GSR_UNDISTORT_CAM_DOUBLES;

struct UdFrames {
    uint16_t cam[UD_FRAMES];
};

struct UdCam {
    double fx, fy, cx, cy, k1, k2, p1, p2, nfx, nfy, ncx, ncy;
    int x0, y0;
    bool remap;
};

__device__ __forceinline__ UdCam ud_load_cam(const double *__restrict__ cams, int cam)
{
    const double *__restrict__ c = cams + (size_t)cam * UD_ROW;
    UdCam r;
    r.fx = c[0]; r.fy = c[1]; r.cx = c[2]; r.cy = c[3];
    r.k1 = c[4]; r.k2 = c[5]; r.p1 = c[6]; r.p2 = c[7];
    r.nfx = c[8]; r.nfy = c[9]; r.ncx = c[10]; r.ncy = c[11];
    // the origin only moves coordinates: every source read below is bounds-checked, so any value is safe
    const double ox = c[12], oy = c[13];
    r.x0 = (ox >= -32768.0 && ox <= 32768.0) ? (int)ox : 1 << 20;
    r.y0 = (oy >= -32768.0 && oy <= 32768.0) ? (int)oy : 1 << 20;
    r.remap = c[14] != 0.0;
    return r;
}

// one source pixel as three bytes in the low 24 bits, 0 outside the image.  Branch-free: a tap outside reads pixel (0, 0) and drops it
__device__ __forceinline__ uint32_t ud_tap(const uint8_t *__restrict__ img, int H, int W, int x, int y)
{
    const bool inside = ((unsigned)x < (unsigned)W) & ((unsigned)y < (unsigned)H);
    const uint8_t *__restrict__ p = img + ((size_t)(inside ? y : 0) * W + (inside ? x : 0)) * 3;
    const uint32_t v = (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16);
    return inside ? v : 0u;
}

// the terms of the map that depend on the output row alone: one of the two divisions leaves the pixel
struct UdRow {
    int Y;
    double y, yy, yy2;
};

__device__ __forceinline__ UdRow ud_row(const UdCam &c, int v)
{
    UdRow r;
    r.Y = v + c.y0;
    r.y = ((double)r.Y - c.ncy) / c.nfy;
    r.yy = r.y * r.y;
    r.yy2 = 2.0 * r.yy;
    return r;
}

// one output pixel (u, v) of the ROI window -> its three bytes in the low 24 bits
__device__ __forceinline__ uint32_t ud_pixel(const uint8_t *__restrict__ img, int H, int W, const UdCam &c, int u, const UdRow &row)
{
    const int X = u + c.x0;
    if (!c.remap) return ud_tap(img, H, W, X, row.Y);
    const double x = ((double)X - c.ncx) / c.nfx, y = row.y;
    const double r2 = x * x + row.yy;
    const double kr = 1.0 + (c.k2 * r2 + c.k1) * r2;
    const double xy2 = (2.0 * x) * y;
    const double xd = (x * kr + c.p1 * xy2) + c.p2 * (r2 + 2.0 * (x * x));
    const double yd = (y * kr + c.p1 * (r2 + row.yy2)) + c.p2 * xy2;
    const float mx = (float)(c.fx * xd + c.cx), my = (float)(c.fy * yd + c.cy);
    const float fsx = mx * 32.0f, fsy = my * 32.0f;
    if (!(fabsf(fsx) < 1073741824.0f) || !(fabsf(fsy) < 1073741824.0f)) return 0u;      // NaN and inf fail the comparison too
    const int sx = __float2int_rn(fsx), sy = __float2int_rn(fsy);
    const int ix = sx >> 5, iy = sy >> 5;
    const uint32_t a = (uint32_t)(sx & 31), b = (uint32_t)(sy & 31);
    const uint32_t p00 = ud_tap(img, H, W, ix, iy), p01 = ud_tap(img, H, W, ix + 1, iy);
    const uint32_t p10 = ud_tap(img, H, W, ix, iy + 1), p11 = ud_tap(img, H, W, ix + 1, iy + 1);
    const uint32_t w00 = (32u - a) * (32u - b), w01 = a * (32u - b), w10 = (32u - a) * b, w11 = a * b;
    uint32_t out = 0;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        const int s = 8 * ch;
        const uint32_t acc = w00 * ((p00 >> s) & 255u) + w01 * ((p01 >> s) & 255u) + w10 * ((p10 >> s) & 255u) + w11 * ((p11 >> s) & 255u) + 512u;
        out |= (acc >> 10) << s;         // at most 1024 * 255 + 512: the shifted value fits a byte
    }
    return out;
}

struct __attribute__((aligned(4))) UdWords {
    uint32_t w[3];
};

__global__ void __launch_bounds__(UD_BLOCK) k_undistort(const uint8_t *__restrict__ src, int n_frames, int H, int W, const double *__restrict__ cams,
                                                         const UdFrames frames, int roi_w, int roi_h, uint8_t *__restrict__ dst)
{
    const long long per_frame = (long long)roi_w * roi_h, n_pixels = per_frame * n_frames, n_groups = (n_pixels + 3) >> 2;
    const size_t frame_bytes = (size_t)H * W * 3;
    for (long long g = (long long)blockIdx.x * UD_BLOCK + threadIdx.x; g < n_groups; g += (long long)gridDim.x * UD_BLOCK) {
        const long long p = g * 4;
        int n = (int)(p / per_frame);
        const int rem = (int)(p - (long long)n * per_frame);
        int v = rem / roi_w, u = rem - v * roi_w;
        UdCam cam = ud_load_cam(cams, frames.cam[n]);
        UdRow row = ud_row(cam, v);
        const int live = n_pixels - p >= 4 ? 4 : (int)(n_pixels - p);
        uint32_t px[4] = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            if (q < live) {
                px[q] = ud_pixel(src + (size_t)n * frame_bytes, H, W, cam, u, row);
                if (++u == roi_w) {
                    u = 0;
                    if (++v == roi_h) {
                        v = 0;
                        if (++n < n_frames) cam = ud_load_cam(cams, frames.cam[n]);
                    }
                    row = ud_row(cam, v);
                }
            }
        }
        uint8_t *__restrict__ o = dst + (size_t)p * 3;
        if (live == 4) {
            UdWords w;
            w.w[0] = px[0] | (px[1] << 24);
            w.w[1] = (px[1] >> 8) | (px[2] << 16);
            w.w[2] = (px[2] >> 16) | (px[3] << 8);
            *reinterpret_cast<UdWords *>(o) = w;
        } else {
            for (int q = 0; q < live; ++q) {
                o[3 * q] = (uint8_t)px[q];
                o[3 * q + 1] = (uint8_t)(px[q] >> 8);
                o[3 * q + 2] = (uint8_t)(px[q] >> 16);
            }
        }
    }
}

}  // namespace gsr

extern "C" {

__attribute__((visibility("default"))) int gsr_undistort(const uint8_t *src, int64_t N, int H, int W, const double *cams, int n_cams,
                                                         const int32_t *frame_cam, int roi_w, int roi_h, uint8_t *dst, void *stream)
{
    using namespace gsr;
    if (!src || !cams || !frame_cam || !dst) return GSR_EINVAL;
    if (N < 1 || N > (1LL << 24) || H < 1 || W < 1 || H > 32767 || W > 32767 || n_cams < 1 || n_cams > 65535) return GSR_EINVAL;
    if (roi_w < 1 || roi_h < 1 || roi_w > 32767 || roi_h > 32767) return GSR_EINVAL;
    if ((reinterpret_cast<uintptr_t>(cams) & 7) || (reinterpret_cast<uintptr_t>(dst) & 3)) return GSR_EINVAL;
    for (int64_t i = 0; i < N; ++i)
        if (frame_cam[i] < 0 || frame_cam[i] >= n_cams) return GSR_EINVAL;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const size_t src_frame = (size_t)H * W * 3, dst_frame = (size_t)roi_w * roi_h * 3;
    (void)hipGetLastError();
    // one launch per UD_FRAMES frames (one launch for any scene of the drivers); a chunk starts on a multiple of four frames,
    // so its first output byte stays dword aligned
    for (int64_t n0 = 0; n0 < N; n0 += UD_FRAMES) {
        const int n = (int)(N - n0 < UD_FRAMES ? N - n0 : UD_FRAMES);
        UdFrames frames;
        for (int i = 0; i < UD_FRAMES; ++i) frames.cam[i] = (uint16_t)(i < n ? frame_cam[n0 + i] : 0);
        const long long groups = ((long long)roi_w * roi_h * n + 3) >> 2;
        const long long blocks = (groups + UD_BLOCK - 1) / UD_BLOCK;
        hipLaunchKernelGGL(k_undistort, dim3((unsigned)(blocks < UD_MAX_BLOCKS ? blocks : UD_MAX_BLOCKS)), dim3(UD_BLOCK), 0, s,
                           src + (size_t)n0 * src_frame, n, H, W, cams, frames, roi_w, roi_h, dst + (size_t)n0 * dst_frame);
    }
    return launch_status();
}

}  // extern "C"
