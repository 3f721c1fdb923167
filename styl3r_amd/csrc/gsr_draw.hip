// gsr_draw.hip -- validation visuals: anti-aliased lines and points (annuli) drawn over planar fp32 images, the reference's
// src/visualization/drawing/{rendering,lines,points}.py (render_over_image with subdivision 8 and 0 or 1 MSAA passes).  The reference
// evaluates every pixel against every primitive as a chain of about forty tensor ops per draw call, reads the edge mask back, evaluates
// the edge pixels again at 8 x 8 sub-samples and scatters them; one draw_cameras picture is twelve such calls.  Here every image of a
// call and every layer (= one draw call of the reference) of every image is ONE launch.
//
//   k_draw_layers : grid (tiles x, tiles y, images), 16 x 16 pixels per workgroup of 256 threads; a thread keeps its pixel in float64
//                   registers across the layers of its image.  Per layer:
//     centre pass : the 18 x 18 halo of the tile is sampled at the pixel centres; the layer's primitives pass through LDS in chunks of
//                   DR_CHUNK records (block-uniform index: every read is a broadcast).  The top primitive (highest covering index) of
//                   each halo pixel lands in LDS together with its colour class, so the edge rule needs no second pass over memory.
//     edge rule   : a pixel whose (colour class, covered) differs from any of its 8 neighbours INSIDE the image is an edge pixel
//                   (detect_msaa_pixels); the workgroup compacts its edge pixels with ballot + popcount into an LDS list.
//     sub-samples : a wave takes one edge pixel at a time, one lane per sub-sample (8 x 8 = one wave64).  Coverage is the popcount of
//                   a ballot -- alpha * 64 is an integer -- and the alpha-weighted colour sum is a fixed-order xor-shuffle tree.
//     composite   : image (1 - alpha) + colour alpha, in float64.
//   The pixel is rounded to fp32 once, after its last layer.  No atomics of any kind: two runs give the same bits.
//
// A record is DR_REC doubles, prepared on the host in float64 (styl3r_amd/visualization.py::_records) in the order the reference forms
// them: start, end, unit direction (NaN for a degenerate line: every body test is then false, as in the reference), the two bounds of
// the parallel test, half the width, the colour and the colour class (the lowest index in the layer with the same colour; two
// primitives of equal colour are not an edge).  For a point: centre, inner radius, radius.
//
// Floating-point contraction is off in this file: each product and sum rounds once, in the order written, which is the order of the
// host restatement.  sqrt and division are the correctly rounded float64 ones.  No fast-math.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/gsr.h"
#include "gsr_common.h"

#pragma clang fp contract(off)

namespace gsr {

constexpr int DR_TILE = 16, DR_HALO = DR_TILE + 2, DR_BLOCK = DR_TILE * DR_TILE, DR_NHALO = DR_HALO * DR_HALO;
constexpr int DR_CHUNK = GSR_DRAW_CHUNK, DR_REC = GSR_DRAW_RECORD_DOUBLES;
// record fields
constexpr int DR_KIND = 0, DR_CLASS = 1, DR_SX = 2, DR_SY = 3, DR_EX = 4, DR_EY = 5, DR_UX = 6, DR_UY = 7, DR_HI = 8, DR_LO = 9, DR_HW = 10,
              DR_R = 11;
static_assert(DR_BLOCK == 256 && DR_NHALO <= 2 * DR_BLOCK && DR_CHUNK * DR_REC == 2 * DR_BLOCK, "staging below moves two doubles per thread");

// is the sample (x, y) inside primitive p?  lines.py:45-70 / points.py:44-46 in their operation order
__device__ inline bool dr_inside(const double *p, double x, double y)
{
    const int kind = (int)p[DR_KIND];
    const double ix = x - p[DR_SX], iy = y - p[DR_SY];
    if (kind == GSR_DRAW_POINT) {
        const double d = sqrt(ix * ix + iy * iy);
        return d >= p[DR_HI] && d <= p[DR_HW];                      // inner_radius <= d <= radius
    }
    const double ux = p[DR_UX], uy = p[DR_UY], hw = p[DR_HW];
    const double par = ux * ix + uy * iy;
    const double qx = ix - par * ux, qy = iy - par * uy;
    bool in = (par <= p[DR_HI]) & (par > p[DR_LO]) & (sqrt(qx * qx + qy * qy) < hw);
    if (kind == GSR_DRAW_ROUND) {
        const double jx = x - p[DR_EX], jy = y - p[DR_EY];
        in |= (sqrt(ix * ix + iy * iy) < hw) | (sqrt(jx * jx + jy * jy) < hw);
    }
    return in;
}

__device__ inline double dr_xor_sum(double v)                         // fixed order: the same tree in every run
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = v + __shfl_xor(v, m, 64);
    return v;
}

__global__ void __launch_bounds__(DR_BLOCK) k_draw_layers(const float *src, float *dst, int H, int W,
                                                           const int32_t *__restrict__ image_layers, const int32_t *__restrict__ layer_prims,
                                                           const int32_t *__restrict__ layer_msaa, int NL, const double *__restrict__ prims,
                                                           long long NP)
{
    __shared__ double s_chunk[DR_CHUNK * DR_REC];
    __shared__ double s_res[DR_BLOCK * 4];           // an edge pixel's (r, g, b, alpha)
    __shared__ int32_t s_top[DR_NHALO];              // top primitive (index into prims) or -1
    __shared__ int32_t s_code[DR_NHALO];             // 0 = nothing covers, 1 + colour class otherwise
    __shared__ int32_t s_wave[DR_BLOCK / 64];
    __shared__ uint8_t s_edge[DR_BLOCK];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int tx = tid % DR_TILE, ty = tid / DR_TILE;
    const int x0 = blockIdx.x * DR_TILE, y0 = blockIdx.y * DR_TILE;
    const int px = x0 + tx, py = y0 + ty;
    const bool live = px < W && py < H;
    const size_t plane = (size_t)H * W;
    const size_t at = (size_t)blockIdx.z * 3 * plane + (size_t)py * W + px;

    double acc[3] = {0.0, 0.0, 0.0};
    if (live) {
#pragma unroll
        for (int c = 0; c < 3; ++c) acc[c] = (double)src[at + c * plane];
    }

    // the two halo pixels this thread samples in the centre pass
    int hx[2], hy[2];
    bool hin[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const int h = tid + k * DR_BLOCK;
        hx[k] = x0 + h % DR_HALO - 1;
        hy[k] = y0 + h / DR_HALO - 1;
        hin[k] = h < DR_NHALO && hx[k] >= 0 && hy[k] >= 0 && hx[k] < W && hy[k] < H;
    }

    const int l_begin = min(max(image_layers[blockIdx.z], 0), NL), l_end = min(max(image_layers[blockIdx.z + 1], l_begin), NL);
    for (int layer = l_begin; layer < l_end; ++layer) {
        const long long p_begin = min(max((long long)layer_prims[layer], 0LL), NP);
        const long long p_end = min(max((long long)layer_prims[layer + 1], p_begin), NP);
        if (p_end == p_begin) continue;                                // an empty layer draws nothing (block-uniform)
        const bool msaa = layer_msaa[layer] != 0;

        // ---- centre pass over the halo ----
        int top[2] = {-1, -1};
        for (long long c0 = p_begin; c0 < p_end; c0 += DR_CHUNK) {
            const int n = (int)min((long long)DR_CHUNK, p_end - c0);
            __syncthreads();                                           // the previous chunk (or layer) is done with s_chunk
            if (2 * tid < n * DR_REC) {
                const double2 v = *reinterpret_cast<const double2 *>(prims + c0 * DR_REC + 2 * tid);
                s_chunk[2 * tid] = v.x;
                s_chunk[2 * tid + 1] = v.y;
            }
            __syncthreads();
            for (int j = 0; j < n; ++j) {
#pragma unroll
                for (int k = 0; k < 2; ++k)
                    if (hin[k] && dr_inside(s_chunk + j * DR_REC, hx[k] + 0.5, hy[k] + 0.5)) top[k] = (int)(c0 + j);
            }
        }
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const int h = tid + k * DR_BLOCK;
            if (h < DR_NHALO) {
                s_top[h] = top[k];
                s_code[h] = top[k] < 0 ? 0 : 1 + (int)prims[(size_t)top[k] * DR_REC + DR_CLASS];
            }
        }
        __syncthreads();

        // ---- edge rule, compaction ----
        const int hc = (ty + 1) * DR_HALO + tx + 1;
        const int my_top = s_top[hc], my_code = s_code[hc];
        bool edge = false;
        if (msaa && live) {
#pragma unroll
            for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
                for (int dx = -1; dx <= 1; ++dx) {
                    const int nx = px + dx, ny = py + dy;
                    if ((dx | dy) != 0 && nx >= 0 && ny >= 0 && nx < W && ny < H) edge |= s_code[hc + dy * DR_HALO + dx] != my_code;
                }
        }
        const unsigned long long vote = __ballot(edge);
        if (lane == 0) s_wave[wave] = __popcll(vote);
        __syncthreads();
        int base = 0, n_edge = 0;
#pragma unroll
        for (int w = 0; w < DR_BLOCK / 64; ++w) {
            base += w < wave ? s_wave[w] : 0;
            n_edge += s_wave[w];
        }
        if (edge) s_edge[base + __popcll(vote & ((1ULL << lane) - 1ULL))] = (uint8_t)tid;
        __syncthreads();

        // ---- 8 x 8 sub-samples: one wave per edge pixel, one lane per sample ----
        for (int e = wave; e < n_edge; e += DR_BLOCK / 64) {
            const int t = s_edge[e];
            const double sx = (x0 + t % DR_TILE) + 0.5 + (((lane & 7) + 0.5) / 8.0 - 0.5);
            const double sy = (y0 + t / DR_TILE) + 0.5 + (((lane >> 3) + 0.5) / 8.0 - 0.5);
            long long hit = -1;
            for (long long j = p_begin; j < p_end; ++j)
                if (dr_inside(prims + j * DR_REC, sx, sy)) hit = j;
            const int count = __popcll(__ballot(hit >= 0));
            double rgb[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) rgb[c] = dr_xor_sum(hit >= 0 ? prims[hit * DR_REC + DR_R + c] : 0.0);
            if (lane == 0) {
                const double denom = (double)count + 1e-10;
#pragma unroll
                for (int c = 0; c < 3; ++c) s_res[t * 4 + c] = rgb[c] / denom;
                s_res[t * 4 + 3] = (double)count / 64.0;
            }
        }
        __syncthreads();

        // ---- composite ----
        if (live) {
            double colour[3], alpha;
            if (edge) {
#pragma unroll
                for (int c = 0; c < 3; ++c) colour[c] = s_res[tid * 4 + c];
                alpha = s_res[tid * 4 + 3];
            } else {
                const long long q = my_top < 0 ? p_begin : (long long)my_top;       // nothing covers: (colour[0], 0)
#pragma unroll
                for (int c = 0; c < 3; ++c) colour[c] = prims[q * DR_REC + DR_R + c];
                alpha = my_top < 0 ? 0.0 : 1.0;
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) acc[c] = acc[c] * (1.0 - alpha) + colour[c] * alpha;
        }
    }
    if (live) {
#pragma unroll
        for (int c = 0; c < 3; ++c) dst[at + c * plane] = (float)acc[c];
    }
}

}  // namespace gsr

extern "C" {

__attribute__((visibility("default"))) int gsr_draw_layers(const float *images, float *out, int B, int H, int W, const int32_t *image_layers,
                                                           const int32_t *layer_prims, const int32_t *layer_msaa, int NL, const double *prims,
                                                           int64_t NP, void *stream)
{
    using namespace gsr;
    if (!images || !out || !image_layers || !layer_prims || !layer_msaa || B < 1 || B > 65535 || H < 1 || W < 1 || NL < 0 || NP < 0) return GSR_EINVAL;
    if (NP > 0 && !prims) return GSR_EINVAL;
    if ((int64_t)H * W > (1LL << 28) || NP > (1LL << 30)) return GSR_EINVAL;
    if (reinterpret_cast<uintptr_t>(prims) & 15) return GSR_EINVAL;
    const int gx = (W + DR_TILE - 1) / DR_TILE, gy = (H + DR_TILE - 1) / DR_TILE;
    if (gy > 65535) return GSR_EINVAL;
    (void)hipGetLastError();
    hipLaunchKernelGGL(k_draw_layers, dim3((unsigned)gx, (unsigned)gy, (unsigned)B), dim3(DR_BLOCK), 0, static_cast<hipStream_t>(stream), images, out,
                       H, W, image_layers, layer_prims, layer_msaa, NL, prims, (long long)NP);
    return launch_status();
}

}  // extern "C"
