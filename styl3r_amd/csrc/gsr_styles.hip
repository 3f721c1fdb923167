// gsr_styles.hip -- multi-style forward of the gfx950 rasterizer (include/gsr.h gsr_forward_styles): S Gaussian sets that differ
// only in colour go through ONE preprocess / tile scan / scatter / per-tile sort (the kernels of gsr_forward.hip, unchanged) and are
// shaded together.
//
//   K1s style_colours   the colours of styles 1..S-1 (style 0's stay in the SplatRec, written by K1): sh_view_dir + sh_colour<DEG> (gsr_common.h),
//                       the routine k_preprocess<DEG> calls, for splats with radius > 0, into a side array of one float4 per
//                       (style, view, Gaussian) -- or per (style, scene, Gaussian) at degree 0 / precomputed RGB, where the colour
//                       does not depend on the view.
//   K5s composite_fwd_styles<NS, FIRST>
//                       k_composite_fwd's walk (one wavefront per tile, four 8x8 quadrants, scalar lane masks, tile_order) with NS
//                       colours per list entry staged in LDS and NS x 3 x 4 colour accumulators.  Everything that makes K5
//                       VALU-bound (power, exp2, alpha, the T test, four ballots, the T update) is evaluated once; a style adds three
//                       FMAs per evaluated quadrant and one 16-byte LDS broadcast read per entry.
//                       FIRST: the launch that owns style 0 -- computes the quadrant masks and leaves them in the point_list words
//                       exactly as K5 does, writes depth / opacity / final_T / n_contrib.  !FIRST (styles beyond the first launch's,
//                       S > 4): reads the masks back from the list words (as the composite backward does) and writes colours only.
//                       Forward only: no fused MSE, no n_touched, no gradient pre-zeroing, no depth-segment checkpoints.
#include "gsr_common.h"

namespace gsr {
constexpr int STYLES_PER_LAUNCH = 4;    // styles one composite launch shades (register budget: DESIGN R10)
constexpr int COLOUR_PTRS = 8;          // SH tensors one launch of the colour kernel serves (grid z)
struct ColourSrc { const float *shs[COLOUR_PTRS]; };

// rows of the side array per style: one per view where the colour depends on the view direction, else one per scene
__host__ __device__ inline bool colour_per_view(const GsrDims &d) { return d.M > 0 && d.sh_degree > 0; }

// ------------------------------------------------------------------ K1s
#pragma clang fp contract(off)
template <int DEG>   // as k_preprocess: active SH degree 0..4, -1 = precomputed colours
__global__ void __launch_bounds__(256) k_style_colours(GsrDims d, const GsrView *__restrict__ views, const float *__restrict__ means,
                                                       ColourSrc src, const int32_t *__restrict__ radii, float4 *__restrict__ side,
                                                       size_t style_stride)
{
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= d.G) return;
    const float *__restrict__ shs = src.shs[blockIdx.z];
    float4 *__restrict__ dst = side + (size_t)blockIdx.z * style_stride + (size_t)blockIdx.y * d.G + g;
    if (DEG <= 0) {      // blockIdx.y = scene
        const size_t sg = (size_t)blockIdx.y * d.G + g;
        float col[3];
        if (DEG == 0) {
            const float *sh = shs + sg * 3 * (size_t)d.M;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                float acc = SH_C0 * sh[c];
                acc = acc + 0.5f;
                col[c] = fmaxf(acc, 0.f);
            }
        } else {
            col[0] = shs[3 * sg]; col[1] = shs[3 * sg + 1]; col[2] = shs[3 * sg + 2];
        }
        *dst = make_float4(col[0], col[1], col[2], 0.f);
        return;
    }
    const int v = blockIdx.y;    // view
    if (radii[(size_t)v * d.G + g] <= 0) return;          // never listed: nobody reads its colour
    const size_t sg = (size_t)(v / d.Vt) * d.G + g;
    const GsrView &vw = views[v];
    const float s = vw.scale;
    const float m[3] = {means[3 * sg] * s, means[3 * sg + 1] * s, means[3 * sg + 2] * s};
    float x, y, z, len, col[3];
    sh_view_dir(m, vw.campos, x, y, z, len);
    sh_colour<(DEG < 0 ? 0 : DEG)>(x, y, z, shs + sg * 3 * (size_t)d.M, col);      // (the clamp bits are the backward's: unused here)
    *dst = make_float4(col[0], col[1], col[2], 0.f);
}
#pragma clang fp contract(fast)

// ------------------------------------------------------------------ K5s
// LDS per wavefront: two float4 of geometry per list entry (x, y, A', B' | C', opacity, depth, quadrant mask) and NS float4 colours.
template <int NS, bool FIRST>
__global__ void __launch_bounds__(64) k_composite_fwd_styles(GsrDims d, const GsrView *__restrict__ views, Ptrs ws,
                                                            const float4 *__restrict__ side, size_t side_stride, float *__restrict__ image,
                                                            size_t image_stride, float *__restrict__ out_depth,
                                                            float *__restrict__ out_opacity)
{
    if (ws.status[GSR_ST_OVERFLOW]) return;
    __shared__ float4 s_q[64 * 2];
    __shared__ float4 s_col[64 * NS];

    const int gx = tiles_x(d.W), T = gx * tiles_y(d.H);
    const uint32_t tv = ws.tile_order[blockIdx.y * gridDim.x + blockIdx.x];   // longest lists are launched first
    const int tile = (int)(tv % (uint32_t)T), v = (int)(tv / (uint32_t)T);
    const int lane = threadIdx.x;
    const int ox = (tile % gx) * TILE + (lane & 7), oy = (tile / gx) * TILE + (lane >> 3);

    const size_t t = (size_t)v * T + tile;
    const uint32_t start = ws.tile_offset[t];
    const int n = (int)(ws.tile_offset[t + 1] - start);
    uint32_t *__restrict__ plist = ws.point_list + start;
    const SplatRec *__restrict__ recs = ws.records + (size_t)v * d.G;
    // the side array's row of this view (per view or per scene), NSIDE styles `side_stride` apart
    constexpr int NSIDE = FIRST ? NS - 1 : NS;
    const float4 *__restrict__ scol = side + (size_t)(colour_per_view(d) ? v : v / d.Vt) * d.G;
    const int tile_ox = (tile % gx) * TILE, tile_oy = (tile / gx) * TILE;

    float fx0 = (float)ox, fy0 = (float)oy;
    asm volatile("" : "+v"(fx0), "+v"(fy0));     // (kept in registers, as in k_composite_fwd)
    float Tr[4], Cc[NS][3][4], D[4], O[4];
    uint32_t last[4];
    bool inside[4];
    unsigned long long dmask[4];                 // finished pixels as scalar lane masks, one per quadrant
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int px = ox + (k & 1) * 8, py = oy + (k >> 1) * 8;
        inside[k] = px < d.W && py < d.H;
        Tr[k] = 1.f; D[k] = O[k] = 0.f;
#pragma unroll
        for (int s = 0; s < NS; ++s) Cc[s][0][k] = Cc[s][1][k] = Cc[s][2][k] = 0.f;
        last[k] = 0;
        dmask[k] = __builtin_amdgcn_ballot_w64(!inside[k]);
    }

    for (int base = 0; base < n; base += 64) {
        const int cnt = __builtin_amdgcn_readfirstlane(min(64, n - base));     // (scalar loop control)
        __syncthreads();  // single-wave workgroup: orders this wave's LDS reads of the previous batch
        uint32_t qm = 0;
        if (lane < cnt) {  // one list entry per lane
            const uint32_t word = plist[base + lane];
            const uint32_t id = word & GSR_ID_MASK;
            const float4 *r = reinterpret_cast<const float4 *>(recs + id);
            const float4 q0 = r[0], q1 = r[1];
            if (FIRST) {
                // the geometric quadrant mask steers this kernel's scalar skips and, through the top bits of the entry's list word, those of
                // every later reader of the list -- the same bits k_composite_fwd writes (entries the footprint cannot reach keep zero bits)
                const float4 q2 = r[2];
                s_col[lane * NS] = q2;        // (parked before the mask code: held across it, the compiler spilled the colour to scratch)
                qm = quadrant_mask(q0, q1, __float_as_uint(q2.w), tile_ox, tile_oy);
                if (qm) plist[base + lane] = id | (qm << GSR_QUAD_SHIFT);
            } else {
                qm = word >> GSR_QUAD_SHIFT;
            }
            s_q[lane * 2 + 0] = make_float4(q0.x, q0.y, q1.x * CONIC_PRESCALE, q1.y * CONIC_PRESCALE);
            s_q[lane * 2 + 1] = make_float4(q1.z * CONIC_PRESCALE, q1.w, q0.z, __uint_as_float(qm));
            if (qm) {
#pragma unroll
                for (int s = 0; s < NSIDE; ++s) s_col[lane * NS + (NS - NSIDE) + s] = scol[(size_t)s * side_stride + id];
            }
        }
        __syncthreads();

        for (unsigned long long todo = __builtin_amdgcn_ballot_w64(qm != 0u); todo; todo &= todo - 1ull) {
            const int j = __builtin_ctzll(todo);
            const float4 a = s_q[j * 2 + 0];
            const float4 b = s_q[j * 2 + 1];
            const uint32_t quad = __builtin_amdgcn_readfirstlane(__float_as_uint(b.w));
            float4 col[NS];
#pragma unroll
            for (int s = 0; s < NS; ++s) col[s] = s_col[j * NS + s];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (!(quad & (1u << k))) continue;        // scalar branches: the only control flow of the evaluation
                if (dmask[k] == ~0ull) continue;
                const float dx = (a.x - fx0) - (float)((k & 1) * 8), dy = (a.y - fy0) - (float)((k >> 1) * 8);
                const float power = -0.5f * (a.z * dx * dx + b.x * dy * dy) - a.w * dx * dy;
                const float alpha = fminf(0.99f, b.y * footprint_exp(power));
                const float test_T = Tr[k] * (1.f - alpha);
                const unsigned long long live = __builtin_amdgcn_ballot_w64(!(power > 0.f)) & __builtin_amdgcn_ballot_w64(!(alpha < (1.f / 255.f))) & ~dmask[k];
                const unsigned long long keep = __builtin_amdgcn_ballot_w64(!(test_T < 0.0001f));
                dmask[k] |= live & ~keep;                  // T would fall below 1e-4: the pixel is finished, this splat is not composited
                const unsigned long long comp = live & keep;
                const float w = sel0_f(comp, alpha * Tr[k]);
#pragma unroll
                for (int s = 0; s < NS; ++s) {
                    Cc[s][0][k] += col[s].x * w; Cc[s][1][k] += col[s].y * w; Cc[s][2][k] += col[s].z * w;
                }
                if (FIRST) {
                    D[k] += b.z * w;
                    O[k] += w;
                    last[k] = sel_u(comp, (uint32_t)(base + j + 1), last[k]);
                }
                Tr[k] = sel_f(comp, test_T, Tr[k]);
            }
        }
        if ((dmask[0] & dmask[1] & dmask[2] & dmask[3]) == ~0ull) break;
    }

    const size_t P = (size_t)d.H * d.W;
    const GsrView &vw = views[v];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (!inside[k]) continue;
        const size_t pix = (size_t)(oy + (k >> 1) * 8) * d.W + (ox + (k & 1) * 8);
        if (FIRST) {
            ws.final_T[v * P + pix] = Tr[k];
            ws.n_contrib[v * P + pix] = last[k];
            out_depth[v * P + pix] = D[k];
            out_opacity[v * P + pix] = O[k];
        }
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            float *img = image + (size_t)s * image_stride;
            img[(v * 3 + 0) * P + pix] = Cc[s][0][k] + Tr[k] * vw.bg[0];
            img[(v * 3 + 1) * P + pix] = Cc[s][1][k] + Tr[k] * vw.bg[1];
            img[(v * 3 + 2) * P + pix] = Cc[s][2][k] + Tr[k] * vw.bg[2];
        }
    }
}

// ------------------------------------------------------------------ host
static size_t styles_extra_bytes(const GsrDims &d, int S)
{
    const size_t rows = colour_per_view(d) ? (size_t)d.B * d.Vt : (size_t)d.B;
    return (size_t)(S - 1) * rows * d.G * sizeof(float4);
}

template <int NS, bool FIRST>
static void launch_composite(const GsrDims &d, const GsrView *views, const Ptrs &ws, const float4 *side, size_t side_stride, float *image,
                             size_t image_stride, float *depth, float *opacity, dim3 grid, hipStream_t stream)
{
    hipLaunchKernelGGL((k_composite_fwd_styles<NS, FIRST>), grid, dim3(64), 0, stream, d, views, ws, side, side_stride, image, image_stride,
                       depth, opacity);
}

int forward_styles(const GsrDims &d, int S, const GsrView *views, const float *means, const float *cov6, const float *opac,
                   const float *const *shs, long long cap, void *workspace, size_t workspace_bytes, void *extra, size_t extra_bytes,
                   uint32_t *tile_count, float *image, float *depth, float *opacity, int32_t *radii, int32_t *status, hipStream_t stream)
{
    GsrLayout L;
    int rc = layout(d, cap, L);
    if (rc != GSR_OK) return rc;
    if (S < 1 || !shs) return GSR_EINVAL;
    for (int s = 0; s < S; ++s)
        if (!shs[s]) return GSR_EINVAL;
    if (!views || !means || !cov6 || !opac || !workspace || !image || !depth || !opacity || !radii || !status) return GSR_EINVAL;
    if (d.flags & (GSR_FLAG_NTOUCHED | GSR_FLAG_PREZERO_GRADS)) return GSR_EINVAL;      // forward-only path: nothing a backward needs
    if (S > 1 && !extra) return GSR_EINVAL;
    if (workspace_bytes < L.total || (S > 1 && extra_bytes < styles_extra_bytes(d, S))) return GSR_ENOSPACE;
    GsrFused fx = {tile_count, nullptr, 0.f, nullptr, nullptr};
    if (S == 1)
        return forward(d, views, means, cov6, opac, shs[0], cap, workspace, workspace_bytes, image, depth, opacity, radii, nullptr, status,
                       &fx, stream, true);
    // geometry, binning, scan, scatter and sort: once, on style 0 (whose colour lands in the splat records)
    rc = forward(d, views, means, cov6, opac, shs[0], cap, workspace, workspace_bytes, image, depth, opacity, radii, nullptr, status, &fx,
                 stream, false);
    if (rc != GSR_OK || (d.flags & GSR_FLAG_PHASE_BIN)) return rc;

    const Ptrs ws = carve(workspace, L);
    const int V = d.B * d.Vt, T = tiles_x(d.W) * tiles_y(d.H);
    const bool per_view = colour_per_view(d);
    const size_t rows = per_view ? (size_t)V : (size_t)d.B, side_stride = rows * d.G;
    float4 *side = static_cast<float4 *>(extra);
    const dim3 cgrid((d.G + 255) / 256, (unsigned)rows);
    for (int s0 = 1; s0 < S; s0 += COLOUR_PTRS) {
        ColourSrc src;
        const int ns = S - s0 < COLOUR_PTRS ? S - s0 : COLOUR_PTRS;
        for (int i = 0; i < COLOUR_PTRS; ++i) src.shs[i] = shs[s0 + (i < ns ? i : 0)];
        float4 *dst = side + (size_t)(s0 - 1) * side_stride;
        const dim3 grid(cgrid.x, cgrid.y, ns);
        with_sh_degree(d, [&](auto deg) {
            hipLaunchKernelGGL(k_style_colours<decltype(deg)::value>, grid, dim3(256), 0, stream, d, views, means, src, radii, dst, side_stride);
        });
    }

    // composite: launches of at most `per` styles over the same sorted lists, sizes as even as possible (5 -> 3 + 2, 8 -> 4 + 4)
    int per = (d.flags >> GSR_FLAG_STYLES_CHUNK_SHIFT) & 7;
    if (per < 2 || per > STYLES_PER_LAUNCH) per = STYLES_PER_LAUNCH;
    const int launches = (S + per - 1) / per, small = S / launches, big = S % launches;
    const size_t image_stride = (size_t)V * 3 * d.H * d.W;
    StageTimer tm(d.profile, true, stream, true);
    tm.begin(GSR_STAGE_COMPOSITE_FWD);
    const dim3 grid(T, V);
    int s0 = 0;
    for (int c = 0; c < launches; ++c) {
        const int ns = small + (c < big ? 1 : 0);
        float *img = image + (size_t)s0 * image_stride;
        if (c == 0) {
            switch (ns) {
                case 2: launch_composite<2, true>(d, views, ws, side, side_stride, img, image_stride, depth, opacity, grid, stream); break;
                case 3: launch_composite<3, true>(d, views, ws, side, side_stride, img, image_stride, depth, opacity, grid, stream); break;
                default: launch_composite<4, true>(d, views, ws, side, side_stride, img, image_stride, depth, opacity, grid, stream); break;
            }
        } else {
            const float4 *sd = side + (size_t)(s0 - 1) * side_stride;
            switch (ns) {
                case 1: launch_composite<1, false>(d, views, ws, sd, side_stride, img, image_stride, depth, opacity, grid, stream); break;
                case 2: launch_composite<2, false>(d, views, ws, sd, side_stride, img, image_stride, depth, opacity, grid, stream); break;
                case 3: launch_composite<3, false>(d, views, ws, sd, side_stride, img, image_stride, depth, opacity, grid, stream); break;
                default: launch_composite<4, false>(d, views, ws, sd, side_stride, img, image_stride, depth, opacity, grid, stream); break;
            }
        }
        s0 += ns;
    }
    tm.end(GSR_STAGE_COMPOSITE_FWD);
    return launch_status();
}

}  // namespace gsr

extern "C" {

__attribute__((visibility("default"))) size_t gsr_styles_extra_bytes(const GsrDims *dims, int32_t S)
{
    GsrLayout L;
    if (!dims || S < 1 || gsr::layout(*dims, 1, L) != GSR_OK) return 0;
    return gsr::styles_extra_bytes(*dims, S);
}

__attribute__((visibility("default"))) int gsr_forward_styles(const GsrDims *dims, int32_t S, const GsrView *views, const float *means,
                                                              const float *cov6, const float *opac, const float *const *shs,
                                                              int64_t pair_capacity, void *workspace, size_t workspace_bytes, void *extra,
                                                              size_t extra_bytes, uint32_t *tile_count, float *image, float *depth,
                                                              float *opacity, int32_t *radii, int32_t *status, void *stream)
{
    if (!dims) return GSR_EINVAL;
    return gsr::forward_styles(*dims, S, views, means, cov6, opac, shs, pair_capacity, workspace, workspace_bytes, extra, extra_bytes,
                               tile_count, image, depth, opacity, radii, status, static_cast<hipStream_t>(stream));
}

}  // extern "C"
