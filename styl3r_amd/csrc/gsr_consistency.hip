// gsr_consistency.hip -- multi-view consistency of rendered sets: for a pair (src i, dst j) of views of ONE geometry every dst pixel is
// lifted through dst's depth, carried into src's camera, tested against src's depth (occlusion) and, where it lands inside src's image
// in front of nothing nearer, src's colours are sampled there and compared with dst's own.  The geometry is the same for every colour
// set rendered over that geometry (decoder.forward_styles: one depth, 1 + S colour sets), so it is done once per (pair, pixel) and the
// sets are a loop inside the lane over four tap addresses that are already known.
//
//   k_warp_consistency : grid (P pairs x tiles of 32 x 8 pixels), one lane per dst pixel.  The pair's two cameras are read through
//                        workgroup-uniform addresses (scalar loads: they live in SGPRs, not in every lane's registers).  Writes mask,
//                        warped (optional) and one record per workgroup: the number of valid pixels and one float64 sum of squared
//                        errors per set.
//   k_warp_fold        : ONE workgroup.  Wave w owns outputs w, w + 16, ...; lane l adds records l, l + 64, ... of its output in that
//                        order and the lanes are folded by a fixed butterfly.  No atomics: two runs give the same bits.  The records
//                        are laid out [pair][word][tile] so that this read is contiguous.
//
// Everything per pixel is float64 with contraction off, in the order of metrics.warp_consistency_expression (the host restatement):
// the mask is the same set of IEEE operations on both sides.  No fast-math.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/gsr.h"
#include "gsr_common.h"

#pragma clang fp contract(off)

namespace gsr {

constexpr int CS_TW = GSR_CONSISTENCY_TILE_W, CS_TH = GSR_CONSISTENCY_TILE_H, CS_BLOCK = CS_TW * CS_TH;
constexpr int CS_FOLD_BLOCK = 1024;
static_assert(CS_BLOCK == 256 && CS_TW == 32, "four waves of two 32-pixel rows each");

struct CsCam { double R[9], t[3], fx, fy, cx, cy; };

// view `v`'s camera through uniform addresses
__device__ __forceinline__ CsCam cs_camera(const double *__restrict__ c2w, const double *__restrict__ K, int v)
{
    CsCam c;
    const double *e = c2w + (size_t)v * 16, *k = K + (size_t)v * 9;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        c.R[3 * r] = e[4 * r]; c.R[3 * r + 1] = e[4 * r + 1]; c.R[3 * r + 2] = e[4 * r + 2];
        c.t[r] = e[4 * r + 3];
    }
    c.fx = k[0]; c.cx = k[2]; c.fy = k[4]; c.cy = k[5];
    return c;
}

__device__ __forceinline__ bool cs_depth_ok(double d) { return (d > 0.0) & (d < INFINITY); }          // finite and positive (NaN: false)

__device__ __forceinline__ double cs_bilinear(double w00, double w01, double w10, double w11, double v00, double v01, double v10, double v11)
{
    return ((w00 * v00 + w01 * v01) + w10 * v10) + w11 * v11;
}

__global__ void __launch_bounds__(CS_BLOCK) k_warp_consistency(const float *__restrict__ images, const float *__restrict__ depth,
                                                               const double *__restrict__ c2w, const double *__restrict__ K,
                                                               const int32_t *__restrict__ pairs, int S, int V, int P, int H, int W,
                                                               double depth_tol, float *__restrict__ warped, uint8_t *__restrict__ mask,
                                                               double *__restrict__ records)
{
    __shared__ double s_part[GSR_CONSISTENCY_MAX_SETS + 1][CS_BLOCK / 64];
    const int tiles_w = (W + CS_TW - 1) / CS_TW, tiles = tiles_w * ((H + CS_TH - 1) / CS_TH);
    const int p = blockIdx.x / (unsigned)tiles, tile = blockIdx.x % (unsigned)tiles;
    const int x = (tile % tiles_w) * CS_TW + (int)(threadIdx.x & (CS_TW - 1)), y = (tile / tiles_w) * CS_TH + (int)(threadIdx.x / CS_TW);
    const int wave = threadIdx.x >> 6;
    const bool inside = x < W && y < H;
    int vi = pairs[2 * p], vj = pairs[2 * p + 1];
    const bool pair_ok = vi >= 0 && vi < V && vj >= 0 && vj < V;      // (workgroup-uniform) a pair that names no view has no valid pixel
    vi = pair_ok ? vi : 0; vj = pair_ok ? vj : 0;
    const CsCam ci = cs_camera(c2w, K, vi), cj = cs_camera(c2w, K, vj);
    const size_t HW = (size_t)H * W, pix = (size_t)(inside ? y : 0) * W + (inside ? x : 0);

    // ---- geometry, once per (pair, pixel) ----
    const double d = inside ? (double)depth[(size_t)vj * HW + pix] : 0.0;
    bool ok = inside & pair_ok & cs_depth_ok(d);
    const double u = ((double)x + 0.5) / (double)W, v = ((double)y + 0.5) / (double)H;
    const double xc = ((u - cj.cx) / cj.fx) * d, yc = ((v - cj.cy) / cj.fy) * d;
    const double wx = ((cj.R[0] * xc + cj.R[1] * yc) + cj.R[2] * d) + cj.t[0];
    const double wy = ((cj.R[3] * xc + cj.R[4] * yc) + cj.R[5] * d) + cj.t[1];
    const double wz = ((cj.R[6] * xc + cj.R[7] * yc) + cj.R[8] * d) + cj.t[2];
    const double dx = wx - ci.t[0], dy = wy - ci.t[1], dz = wz - ci.t[2];
    const double sx = (ci.R[0] * dx + ci.R[3] * dy) + ci.R[6] * dz;
    const double sy = (ci.R[1] * dx + ci.R[4] * dy) + ci.R[7] * dz;
    const double z = (ci.R[2] * dx + ci.R[5] * dy) + ci.R[8] * dz;
    ok &= z > 0.0;
    double px = ((ci.fx * sx) / z + ci.cx) * (double)W - 0.5, py = ((ci.fy * sy) / z + ci.cy) * (double)H - 0.5;
    ok &= (px >= 0.0) & (px <= (double)(W - 1)) & (py >= 0.0) & (py <= (double)(H - 1));
    px = ok ? px : 0.0; py = ok ? py : 0.0;                            // (NaN and out-of-range never reach the integer conversion)
    const double fx0 = fmin(floor(px), (double)(W - 2)), fy0 = fmin(floor(py), (double)(H - 2));
    const double ax = px - fx0, ay = py - fy0;
    const double w00 = (1.0 - ax) * (1.0 - ay), w01 = ax * (1.0 - ay), w10 = (1.0 - ax) * ay, w11 = ax * ay;
    const size_t t00 = (size_t)(int)fy0 * W + (size_t)(int)fx0, t01 = t00 + 1, t10 = t00 + W, t11 = t10 + 1;   // inside [0, H) x [0, W): H, W >= 2
    {
        const float *di = depth + (size_t)vi * HW;
        const double d00 = ok ? (double)di[t00] : 0.0, d01 = ok ? (double)di[t01] : 0.0, d10 = ok ? (double)di[t10] : 0.0,
                     d11 = ok ? (double)di[t11] : 0.0;
        ok &= cs_depth_ok(d00) & cs_depth_ok(d01) & cs_depth_ok(d10) & cs_depth_ok(d11);
        const double D = cs_bilinear(w00, w01, w10, w11, d00, d01, d10, d11);
        ok &= fabs(z - D) <= depth_tol * D;
    }
    if (inside) mask[(size_t)p * HW + pix] = ok ? 1 : 0;
    const unsigned long long valid = __ballot(ok);
    if ((threadIdx.x & 63) == 0) s_part[0][wave] = (double)__popcll(valid);

    // ---- the colour sets ----
    for (int s = 0; s < S; ++s) {
        double e = 0.0;
        const float *src = images + ((size_t)s * V + vi) * 3 * HW, *dst = images + ((size_t)s * V + vj) * 3 * HW;
        float *out = warped ? warped + ((size_t)s * P + p) * 3 * HW + pix : nullptr;
        if (ok) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float *pl = src + c * HW;
                const float wv = (float)cs_bilinear(w00, w01, w10, w11, (double)pl[t00], (double)pl[t01], (double)pl[t10], (double)pl[t11]);
                const double diff = (double)wv - (double)dst[c * HW + pix];
                e = c ? e + diff * diff : diff * diff;
                if (out) out[c * HW] = wv;
            }
        } else if (out && inside) {
            out[0] = 0.f; out[HW] = 0.f; out[2 * HW] = 0.f;
        }
        e = wave_sum(e);
        if ((threadIdx.x & 63) == 0) s_part[s + 1][wave] = e;
    }
    __syncthreads();
    if ((int)threadIdx.x <= S) {
        const double *q = s_part[threadIdx.x];
        records[((size_t)p * (S + 1) + threadIdx.x) * tiles + tile] = ((q[0] + q[1]) + q[2]) + q[3];
    }
}

__global__ void __launch_bounds__(CS_FOLD_BLOCK) k_warp_fold(const double *__restrict__ records, int S, int P, int tiles,
                                                              int32_t *__restrict__ count, double *__restrict__ sse)
{
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const long long outputs = (long long)P * (S + 1);
    for (long long o = wave; o < outputs; o += CS_FOLD_BLOCK / 64) {
        const double *r = records + (size_t)o * tiles;
        double acc = 0.0;
        for (int t = lane; t < tiles; t += 64) acc += r[t];
        acc = wave_sum(acc);
        if (lane == 0) {
            const int p = (int)(o / (S + 1)), k = (int)(o % (S + 1));
            if (k == 0) count[p] = (int32_t)acc;                       // (integers below 2^53: exact)
            else sse[(size_t)(k - 1) * P + p] = acc;
        }
    }
}

// workgroups of the first launch, or 0 for dimensions the entry refuses
static long long cs_groups(int64_t P, int S, int H, int W)
{
    if (P < 1 || S < 1 || S > GSR_CONSISTENCY_MAX_SETS || H < 2 || W < 2 || H > 16384 || W > 16384) return 0;
    const long long tiles = (long long)((W + CS_TW - 1) / CS_TW) * ((H + CS_TH - 1) / CS_TH);
    const long long g = (long long)P * tiles;
    return (P > (1LL << 24) || g > 0x7fffffffLL) ? 0 : g;
}

}  // namespace gsr

extern "C" {

__attribute__((visibility("default"))) size_t gsr_warp_consistency_scratch_bytes(int64_t P, int S, int H, int W)
{
    return (size_t)gsr::cs_groups(P, S, H, W) * (size_t)(S + 1) * sizeof(double);
}

__attribute__((visibility("default"))) int gsr_warp_consistency(const float *images, const float *depth, const double *c2w, const double *K,
                                                                const int32_t *pairs, int S, int V, int64_t P, int H, int W, double depth_tol,
                                                                float *warped, uint8_t *mask, int32_t *count, double *sse, void *scratch,
                                                                size_t scratch_bytes, void *stream)
{
    using namespace gsr;
    const long long groups = cs_groups(P, S, H, W);
    if (!groups || V < 1 || !images || !depth || !c2w || !K || !pairs || !mask || !count || !sse || !scratch) return GSR_EINVAL;
    if (!(depth_tol >= 0.0)) return GSR_EINVAL;
    if (reinterpret_cast<uintptr_t>(scratch) & 7) return GSR_EINVAL;
    if (scratch_bytes < (size_t)groups * (size_t)(S + 1) * sizeof(double)) return GSR_ENOSPACE;
    hipStream_t s = static_cast<hipStream_t>(stream);
    double *records = static_cast<double *>(scratch);
    (void)hipGetLastError();
    hipLaunchKernelGGL(k_warp_consistency, dim3((unsigned)groups), dim3(CS_BLOCK), 0, s, images, depth, c2w, K, pairs, S, V, (int)P, H, W, depth_tol,
                       warped, mask, records);
    hipLaunchKernelGGL(k_warp_fold, dim3(1), dim3(CS_FOLD_BLOCK), 0, s, records, S, (int)P, (int)(groups / P), count, sse);
    return launch_status();
}

}  // extern "C"
