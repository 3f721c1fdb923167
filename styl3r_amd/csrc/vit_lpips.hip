// vit_lpips.hip -- the tail of LPIPS-VGG (src/loss/loss_lpips.py:27-54, the `lpips` package's LPIPS.forward) and the 2 x 2 max-pool of
// its VGG16 trunk.
//
// vit_lpips_fwd: dist[n] = sum_k mean_hw sum_c w_k[c] (a^_c - b^_c)^2,  a^ = a / (sqrt(sum_c a^2) + 1e-10), over the five feature taps
// in ONE launch plus a one-workgroup-per-image fold.  The torch expression (normalize_tensor -> difference -> square -> 1x1 `lin` conv ->
// spatial mean) is ~10 full passes over every tap forward and as many backward; here the forward reads each tap once and the backward reads
// each tap once and writes its gradient once.
//
// Byte model (fp32, taps of one side: sum_k C_k H_k W_k floats per image; 40 x 256^2: 8.0 M floats = 32 MB per image and side):
//   forward : 2 * 4 * N * sum_k C_k H_k W_k      (fa + fb)               = 2.56 GB at 40 x 256^2
//             + 16 B per pixel of per-pixel statistics (only when the backward will run)  = 56 MB
//   backward: 2 * 4 * N * sum_k C_k H_k W_k      (fa + fb)  + 4 * N * sum_k C_k H_k W_k  (dfa) + the 16 B per pixel statistics
//             = 2.56 + 1.28 + 0.06 GB
//
// Layout and access.  NCHW taps; the 64 lanes of a workgroup (one wave) own 4 consecutive pixels each -- 256 pixels of one image of one
// tap -- so every channel step is one coalesced 1 KiB row (16 B per lane).  Taps whose H*W is not a multiple of 4 (or whose pointers are
// not 16-byte aligned) take scalar loads.  Workgroup id = image * P + (block of the image), P = sum_k ceil(H_k W_k / 256).
//
// Numerics.  The distance of nearly identical images (late in training: prediction ~ target) is a sum of squares of tiny differences; the
// expanded form  sum w a^2/Na^2 - 2 sum w a b/(Na Nb) + sum w b^2/Nb^2  cancels to nothing there.  The kernel instead forms the per-channel
// difference e_c = a^_c - b^_c from d_c = a_c - b_c in ONE pass over the channels:
//     e = d / Na + b (1/Na - 1/Nb)    (Na >= Nb)          e = d / Nb + a (1/Na - 1/Nb)    (Na < Nb)
//     1/Na - 1/Nb = (nb - na) / (Na Nb),   nb - na = -sum_c d_c (a_c + b_c) / (na + nb)
// (Na = na + 1e-10, na = |a|).  Every term is then of the size of the difference itself, so  sum_c w e^2 = r^2 Sww_dd + 2 r delta Sw_dx +
// delta^2 Sw_xx  (r = the 1/N of the larger side, x = the other side's vector) needs only per-pixel channel sums: nine accumulators per pixel,
// no second pass over the channels and nothing staged in LDS.  Expanding around the LARGER norm keeps both terms O(1) when one side is
// (nearly) all zero.
//
// Backward.  dL/da_j = g[n] / (H W) * (2 w_j e_j / Na - a_j * 2 T / (Na^2 na)),  T = sum_c w_c e_c a_c  (= r Sw_da + delta Sw_xa, also from
// the forward's accumulators).  The forward saves four floats per pixel -- +-r (the sign selects which side is x), delta, 1/Na, 2T/(Na^2 na)
// -- and the backward re-forms e_j from (a_j, b_j) with them: one read of both taps, one write of the gradient, no host read-back (g is the
// device-resident upstream gradient).  An all-zero pixel of a (na = 0) takes the Jacobian of a / (|a| + 1e-10) at 0, I / 1e-10.
// relu_in: the taps are pre-activations; max(x, 0) is applied on load and the ReLU mask (x > 0) on the gradient.
//
// Determinism: the per-workgroup partial sums (already divided by H W) go to scratch in plain stores; the fold adds an image's P partials in
// index order.  No atomics: bit-identical run to run.
//
// vit_maxpool2x2_fwd / _bwd: nn.MaxPool2d(2, 2) of NCHW maps with even H and W; the backward recomputes the argmax from the input (no index
// tensor), with the framework's rule (first maximum in row-major order; a NaN wins).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vit_common.h"
#include "vit_internal.h"

namespace vit {

constexpr int LP_MAX_TAPS = 5, LP_PIX = 256;       // pixels per workgroup (64 lanes x 4)

struct LpipsArgs {
    const float *fa[LP_MAX_TAPS], *fb[LP_MAX_TAPS], *w[LP_MAX_TAPS];
    float *dfa[LP_MAX_TAPS];
    int64_t stat_off[LP_MAX_TAPS];     // float offset of tap k's statistics: 4 planes of (N, HWp)
    int C[LP_MAX_TAPS], HW[LP_MAX_TAPS], HWp[LP_MAX_TAPS], vec[LP_MAX_TAPS];
    float inv_hw[LP_MAX_TAPS];
    int blk_off[LP_MAX_TAPS + 1];      // first block of tap k within an image; blk_off[taps] = P
    int taps, N, relu;
};

__device__ inline float lp_wave_sum(float v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__device__ inline int lp_tap_of(const LpipsArgs &a, int j)
{
    int k = 0;
#pragma unroll
    for (int t = 1; t < LP_MAX_TAPS; ++t) k += (t < a.taps && j >= a.blk_off[t]) ? 1 : 0;
    return k;
}

struct LpAcc { float saa, sbb, s, wdd, wda, wdb, waa, wbb, wab; };

__device__ inline void lp_add(LpAcc &q, float a, float b, float w)
{
    const float d = a - b;
    q.saa += a * a; q.sbb += b * b; q.s += d * (a + b);
    const float wd = w * d, wa = w * a, wb = w * b;
    q.wdd += wd * d; q.wda += wd * a; q.wdb += wd * b;
    q.waa += wa * a; q.wbb += wb * b; q.wab += wa * b;
}

// per-pixel distance and the four saved statistics (see the file header)
__device__ inline float lp_finish(const LpAcc &q, float4 &st)
{
    const float na = sqrtf(q.saa), nb = sqrtf(q.sbb);
    const float Na = na + 1e-10f, Nb = nb + 1e-10f;
    const float dn = (na + nb > 0.f) ? -q.s / (na + nb) : 0.f;            // nb - na without cancellation
    const float delta = dn / (Na * Nb);                                   // 1/Na - 1/Nb
    const bool xb = Na >= Nb;                                             // expand around the larger norm
    const float r = xb ? 1.0f / Na : 1.0f / Nb;
    const float sdx = xb ? q.wdb : q.wda, sxx = xb ? q.wbb : q.waa, sxa = xb ? q.wab : q.waa;
    const float dist = r * r * q.wdd + 2.0f * r * delta * sdx + delta * delta * sxx;
    const float T = r * q.wda + delta * sxa;                              // sum_c w e a
    const float inv_na = 1.0f / Na;
    st = make_float4(xb ? r : -r, delta, inv_na, na > 0.f ? 2.0f * T * inv_na * inv_na / na : 0.f);
    return dist;
}

__global__ void __launch_bounds__(64) k_lpips_fwd(const LpipsArgs a, float *__restrict__ partial, float *__restrict__ stats)
{
    const int P = a.blk_off[a.taps];
    const int n = blockIdx.x / P, j = blockIdx.x - n * P, k = lp_tap_of(a, j);
    const int C = a.C[k], HW = a.HW[k], lane = threadIdx.x;
    const int p0 = (j - a.blk_off[k]) * LP_PIX + lane * 4;
    const float *__restrict__ fa = a.fa[k] + (int64_t)n * C * HW;
    const float *__restrict__ fb = a.fb[k] + (int64_t)n * C * HW;
    const float *__restrict__ w = a.w[k];
    const bool relu = a.relu != 0;
    LpAcc q[4] = {};
    if (a.vec[k]) {
        if (p0 < HW) {
            const float *pa = fa + p0, *pb = fb + p0;
            int c = 0;
            for (; c + 1 < C; c += 2) {          // two channel rows in flight per operand
                float4 x0 = *reinterpret_cast<const float4 *>(pa + (int64_t)c * HW);
                float4 y0 = *reinterpret_cast<const float4 *>(pb + (int64_t)c * HW);
                float4 x1 = *reinterpret_cast<const float4 *>(pa + (int64_t)(c + 1) * HW);
                float4 y1 = *reinterpret_cast<const float4 *>(pb + (int64_t)(c + 1) * HW);
                const float w0 = w[c], w1 = w[c + 1];
                if (relu) {
                    x0 = make_float4(fmaxf(x0.x, 0.f), fmaxf(x0.y, 0.f), fmaxf(x0.z, 0.f), fmaxf(x0.w, 0.f));
                    y0 = make_float4(fmaxf(y0.x, 0.f), fmaxf(y0.y, 0.f), fmaxf(y0.z, 0.f), fmaxf(y0.w, 0.f));
                    x1 = make_float4(fmaxf(x1.x, 0.f), fmaxf(x1.y, 0.f), fmaxf(x1.z, 0.f), fmaxf(x1.w, 0.f));
                    y1 = make_float4(fmaxf(y1.x, 0.f), fmaxf(y1.y, 0.f), fmaxf(y1.z, 0.f), fmaxf(y1.w, 0.f));
                }
                lp_add(q[0], x0.x, y0.x, w0); lp_add(q[1], x0.y, y0.y, w0); lp_add(q[2], x0.z, y0.z, w0); lp_add(q[3], x0.w, y0.w, w0);
                lp_add(q[0], x1.x, y1.x, w1); lp_add(q[1], x1.y, y1.y, w1); lp_add(q[2], x1.z, y1.z, w1); lp_add(q[3], x1.w, y1.w, w1);
            }
            for (; c < C; ++c) {
                float4 x0 = *reinterpret_cast<const float4 *>(pa + (int64_t)c * HW);
                float4 y0 = *reinterpret_cast<const float4 *>(pb + (int64_t)c * HW);
                const float w0 = w[c];
                if (relu) {
                    x0 = make_float4(fmaxf(x0.x, 0.f), fmaxf(x0.y, 0.f), fmaxf(x0.z, 0.f), fmaxf(x0.w, 0.f));
                    y0 = make_float4(fmaxf(y0.x, 0.f), fmaxf(y0.y, 0.f), fmaxf(y0.z, 0.f), fmaxf(y0.w, 0.f));
                }
                lp_add(q[0], x0.x, y0.x, w0); lp_add(q[1], x0.y, y0.y, w0); lp_add(q[2], x0.z, y0.z, w0); lp_add(q[3], x0.w, y0.w, w0);
            }
        }
    } else {
        for (int c = 0; c < C; ++c) {
            const float w0 = w[c];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                if (p0 + e < HW) {
                    float x = fa[(int64_t)c * HW + p0 + e], y = fb[(int64_t)c * HW + p0 + e];
                    if (relu) { x = fmaxf(x, 0.f); y = fmaxf(y, 0.f); }
                    lp_add(q[e], x, y, w0);
                }
            }
        }
    }
    float part = 0.f;
    float4 st[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const float de = lp_finish(q[e], st[e]);
        if (p0 + e < HW) part += de;
    }
    if (stats) {
        const int HWp = a.HWp[k];
        float *sb = stats + a.stat_off[k] + (int64_t)n * HWp + p0;
        const int64_t plane = (int64_t)a.N * HWp;
        if (p0 < HWp) {           // (HWp = HW rounded up to 4: the four pixels of a lane are all inside the padded plane)
            *reinterpret_cast<float4 *>(sb) = make_float4(st[0].x, st[1].x, st[2].x, st[3].x);
            *reinterpret_cast<float4 *>(sb + plane) = make_float4(st[0].y, st[1].y, st[2].y, st[3].y);
            *reinterpret_cast<float4 *>(sb + 2 * plane) = make_float4(st[0].z, st[1].z, st[2].z, st[3].z);
            *reinterpret_cast<float4 *>(sb + 3 * plane) = make_float4(st[0].w, st[1].w, st[2].w, st[3].w);
        }
    }
    part = lp_wave_sum(part);
    if (lane == 0) partial[blockIdx.x] = part * a.inv_hw[k];
}

// dist[n] = the P partials of image n, added in index order by one wave
__global__ void __launch_bounds__(64) k_lpips_fold(const float *__restrict__ partial, int P, float *__restrict__ dist)
{
    const int n = blockIdx.x, lane = threadIdx.x;
    float s = 0.f;
    for (int i = lane; i < P; i += 64) s += partial[(int64_t)n * P + i];
    s = lp_wave_sum(s);
    if (lane == 0) dist[n] = s;
}

__device__ inline float lp_grad(float raw, float b_raw, float w, float gs, const float4 &st, bool relu)
{
    const float a = relu ? fmaxf(raw, 0.f) : raw, b = relu ? fmaxf(b_raw, 0.f) : b_raw;
    const float r = fabsf(st.x), x = st.x >= 0.f ? b : a;
    const float e = (a - b) * r + x * st.y;
    const float g = gs * (2.0f * w * e * st.z - a * st.w);
    return (relu && !(raw > 0.f)) ? 0.f : g;
}

__global__ void __launch_bounds__(64) k_lpips_bwd(const LpipsArgs a, const float *__restrict__ gup, const float *__restrict__ stats)
{
    const int P = a.blk_off[a.taps];
    const int n = blockIdx.x / P, j = blockIdx.x - n * P, k = lp_tap_of(a, j);
    const int C = a.C[k], HW = a.HW[k], HWp = a.HWp[k], lane = threadIdx.x;
    const int p0 = (j - a.blk_off[k]) * LP_PIX + lane * 4;
    if (p0 >= HW) return;
    const int64_t base = (int64_t)n * C * HW;
    const float *__restrict__ fa = a.fa[k] + base;
    const float *__restrict__ fb = a.fb[k] + base;
    float *__restrict__ dfa = a.dfa[k] + base;
    const float *__restrict__ w = a.w[k];
    const bool relu = a.relu != 0;
    const float gs = gup[n] * a.inv_hw[k];
    const float *sb = stats + a.stat_off[k] + (int64_t)n * HWp + p0;
    const int64_t plane = (int64_t)a.N * HWp;
    const float4 s0 = *reinterpret_cast<const float4 *>(sb), s1 = *reinterpret_cast<const float4 *>(sb + plane);
    const float4 s2 = *reinterpret_cast<const float4 *>(sb + 2 * plane), s3 = *reinterpret_cast<const float4 *>(sb + 3 * plane);
    const float4 st[4] = {make_float4(s0.x, s1.x, s2.x, s3.x), make_float4(s0.y, s1.y, s2.y, s3.y),
                          make_float4(s0.z, s1.z, s2.z, s3.z), make_float4(s0.w, s1.w, s2.w, s3.w)};
    if (a.vec[k]) {
        for (int c = 0; c < C; ++c) {
            const int64_t o = (int64_t)c * HW + p0;
            const float4 x = *reinterpret_cast<const float4 *>(fa + o), y = *reinterpret_cast<const float4 *>(fb + o);
            const float w0 = w[c];
            *reinterpret_cast<float4 *>(dfa + o) = make_float4(lp_grad(x.x, y.x, w0, gs, st[0], relu), lp_grad(x.y, y.y, w0, gs, st[1], relu),
                                                               lp_grad(x.z, y.z, w0, gs, st[2], relu), lp_grad(x.w, y.w, w0, gs, st[3], relu));
        }
    } else {
        for (int c = 0; c < C; ++c) {
            const float w0 = w[c];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                if (p0 + e < HW) {
                    const int64_t o = (int64_t)c * HW + p0 + e;
                    dfa[o] = lp_grad(fa[o], fb[o], w0, gs, st[e], relu);
                }
            }
        }
    }
}

// ---- host ----------------------------------------------------------------------------------------------------------------------------------
static int lpips_args(const VitLpipsTap *taps, int n_taps, int N, int relu_in, bool bwd, LpipsArgs &a)
{
    if (!taps || n_taps < 1 || n_taps > LP_MAX_TAPS || N < 1) return VIT_EINVAL;
    a = LpipsArgs{};
    a.taps = n_taps; a.N = N; a.relu = relu_in ? 1 : 0;
    int64_t soff = 0;
    int64_t blocks = 0;
    for (int k = 0; k < n_taps; ++k) {
        const VitLpipsTap &t = taps[k];
        if (!t.fa || !t.fb || !t.w || t.C < 1 || t.H < 1 || t.W < 1 || (bwd && !t.dfa)) return VIT_EINVAL;
        const int64_t hw = (int64_t)t.H * t.W;
        if (hw > (1 << 28)) return VIT_EINVAL;
        a.fa[k] = t.fa; a.fb[k] = t.fb; a.w[k] = t.w; a.dfa[k] = t.dfa;
        a.C[k] = t.C; a.HW[k] = (int)hw; a.HWp[k] = (int)((hw + 3) & ~3);
        uintptr_t al = reinterpret_cast<uintptr_t>(t.fa) | reinterpret_cast<uintptr_t>(t.fb) | (bwd ? reinterpret_cast<uintptr_t>(t.dfa) : 0);
        a.vec[k] = (hw % 4 == 0 && (al & 15) == 0) ? 1 : 0;
        a.inv_hw[k] = 1.0f / (float)hw;
        a.stat_off[k] = soff;
        soff += 4 * (int64_t)N * a.HWp[k];
        a.blk_off[k] = (int)blocks;
        blocks += (hw + LP_PIX - 1) / LP_PIX;
    }
    a.blk_off[n_taps] = (int)blocks;
    if (blocks * N > 0x7fffffff) return VIT_EINVAL;
    return VIT_OK;
}

size_t lpips_scratch_bytes(const VitLpipsTap *taps, int n_taps, int N)
{
    LpipsArgs a;
    if (lpips_args(taps, n_taps, N, 0, false, a) != VIT_OK) return 0;
    return (size_t)a.blk_off[n_taps] * N * sizeof(float);
}

size_t lpips_stats_bytes(const VitLpipsTap *taps, int n_taps, int N)
{
    LpipsArgs a;
    if (lpips_args(taps, n_taps, N, 0, false, a) != VIT_OK) return 0;
    size_t s = 0;
    for (int k = 0; k < n_taps; ++k) s += 4 * (size_t)N * a.HWp[k];
    return s * sizeof(float);
}

int lpips_fwd(const VitLpipsTap *taps, int n_taps, int N, int relu_in, float *dist, void *scratch, float *stats, hipStream_t stream)
{
    LpipsArgs a;
    if (!dist || !scratch || lpips_args(taps, n_taps, N, relu_in, false, a) != VIT_OK) return VIT_EINVAL;
    if ((reinterpret_cast<uintptr_t>(stats) & 15) != 0) return VIT_EINVAL;
    const int P = a.blk_off[n_taps];
    (void)hipGetLastError();
    hipLaunchKernelGGL(k_lpips_fwd, dim3(P * N), dim3(64), 0, stream, a, static_cast<float *>(scratch), stats);
    hipLaunchKernelGGL(k_lpips_fold, dim3(N), dim3(64), 0, stream, static_cast<const float *>(scratch), P, dist);
    return launch_status();
}

int lpips_bwd(const VitLpipsTap *taps, int n_taps, int N, int relu_in, const float *g, const float *stats, hipStream_t stream)
{
    LpipsArgs a;
    if (!g || !stats || (reinterpret_cast<uintptr_t>(stats) & 15) != 0 || lpips_args(taps, n_taps, N, relu_in, true, a) != VIT_OK)
        return VIT_EINVAL;
    (void)hipGetLastError();
    hipLaunchKernelGGL(k_lpips_bwd, dim3(a.blk_off[n_taps] * N), dim3(64), 0, stream, a, g, stats);
    return launch_status();
}

// ---- 2 x 2 / stride 2 max-pool ----------------------------------------------------------------------------------------------------------------
// the framework's scan (aten max_pool2d): row-major over the window, `val > max || isnan(val)` replaces; the index starts at the first element
__device__ inline int mp_argmax(const float2 r0, const float2 r1, float &m)
{
    const float v[4] = {r0.x, r0.y, r1.x, r1.y};
    m = -INFINITY;
    int arg = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i)
        if (v[i] > m || isnan(v[i])) { m = v[i]; arg = i; }
    return arg;
}

__global__ void __launch_bounds__(256) k_maxpool2x2_fwd(const float *__restrict__ in, float *__restrict__ out, int64_t total, int H, int W)
{
    const int Wo = W >> 1, Ho = H >> 1;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int ox = (int)(i % Wo);
        const int64_t t = i / Wo;
        const int oy = (int)(t % Ho);
        const int64_t pl = t / Ho;
        const float *r = in + (pl * H + 2 * oy) * W + 2 * ox;
        float m;
        mp_argmax(*reinterpret_cast<const float2 *>(r), *reinterpret_cast<const float2 *>(r + W), m);
        out[i] = m;
    }
}

__global__ void __launch_bounds__(256) k_maxpool2x2_bwd(const float *__restrict__ in, const float *__restrict__ dout, float *__restrict__ din,
                                                        int64_t total, int H, int W)
{
    const int Wo = W >> 1, Ho = H >> 1;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int ox = (int)(i % Wo);
        const int64_t t = i / Wo;
        const int oy = (int)(t % Ho);
        const int64_t pl = t / Ho;
        const int64_t o = (pl * H + 2 * oy) * W + 2 * ox;
        float m;
        const int arg = mp_argmax(*reinterpret_cast<const float2 *>(in + o), *reinterpret_cast<const float2 *>(in + o + W), m);
        const float g = dout[i];
        *reinterpret_cast<float2 *>(din + o) = make_float2(arg == 0 ? g : 0.f, arg == 1 ? g : 0.f);
        *reinterpret_cast<float2 *>(din + o + W) = make_float2(arg == 2 ? g : 0.f, arg == 3 ? g : 0.f);
    }
}

static int mp_grid(int64_t total)
{
    const int64_t b = (total + 255) / 256;
    return (int)(b < 1 ? 1 : (b > 65536 ? 65536 : b));
}

int maxpool2x2_fwd(const float *in, float *out, int64_t planes, int H, int W, hipStream_t stream)
{
    if (!in || !out || planes < 1 || H < 2 || W < 2 || (H & 1) || (W & 1) || (reinterpret_cast<uintptr_t>(in) & 7)) return VIT_EINVAL;
    const int64_t total = planes * (H / 2) * (W / 2);
    (void)hipGetLastError();
    hipLaunchKernelGGL(k_maxpool2x2_fwd, dim3(mp_grid(total)), dim3(256), 0, stream, in, out, total, H, W);
    return launch_status();
}

int maxpool2x2_bwd(const float *in, const float *dout, float *din, int64_t planes, int H, int W, hipStream_t stream)
{
    if (!in || !dout || !din || planes < 1 || H < 2 || W < 2 || (H & 1) || (W & 1) ||
        ((reinterpret_cast<uintptr_t>(in) | reinterpret_cast<uintptr_t>(din)) & 7))
        return VIT_EINVAL;
    const int64_t total = planes * (H / 2) * (W / 2);
    (void)hipGetLastError();
    hipLaunchKernelGGL(k_maxpool2x2_bwd, dim3(mp_grid(total)), dim3(256), 0, stream, in, dout, din, total, H, W);
    return launch_status();
}
}  // namespace vit
