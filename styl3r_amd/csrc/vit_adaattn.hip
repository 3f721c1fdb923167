// vit_adaattn.hip -- the two kernels of the AdaAttN loss (src/loss/loss_adaattn.py, AdaAttN.forward of stylizer.py:44-73).
//
// vit_adaattn_stats: per content position n of image b, with A = softmax_m(q^[:, n] . k^[:, m]) over the M positions of the image's style,
//     mean[c, n] = sum_m A[n, m] s[c, m],   std[c, n] = sqrt(relu(sum_m A[n, m] s[c, m]^2 - mean[c, n]^2)),
// flash style: the (Nq, M) attention matrix exists only as one 64 x 128 tile of logits in LDS.
//
// Arithmetic.  The logits are UNSCALED dot products of instance-normalised D-vectors (|logit| in the hundreds, ~530 where a query matches a
// key) and the softmax rows are nearly one-hot: a logit needs fp32 quality.  Both contractions run on the exact-f32 MFMA
// (v_mfma_f32_32x32x2_f32: a k-ordered fp32 fma chain, one rounding per product), so there is no operand split, no operand scale and nothing to
// un-scale; the logits accumulate in two interleaved chains per tile.  exp is expf, not the fast form.
//
// Decomposition.  One workgroup of 4 waves owns 64 content positions of one image and walks the style's M positions in tiles of 128:
//   (1) q^[:, 64 positions] is staged ONCE in LDS ([D][64] floats, 112 KiB at D = 448: a D = 448 query column does not sit in registers);
//   (2) per tile, wave w forms the logits of keys 32 w .. 32 w + 31 against the 64 positions: X[m][n] = sum_d k^[d][m] q^[d][n], keys straight
//       from global memory (each element is used once per workgroup and tile; a 128-byte row per half-wave), queries from LDS, and stores
//       them to the LDS tile [128][64] (keys past M as -inf);
//   (3) every wave reads the whole tile: running column maximum (the same arithmetic in all four waves, so they agree bit for bit), rescale
//       of its accumulators, p = exp(x - max), and p is the B operand of the second product as it comes from LDS (lane = position, the two
//       half-waves are the two k's) -- no transposition and no lane movement;
//   (4) the channels are sliced over the waves in tiles of 32: wave w accumulates channel tiles w and w + 4 (2 moments x 2 position tiles x
//       16 registers each).  The style rows s[c][m .. m + 63] are read per lane (lane = channel), 16 bytes at a time when M % 4 == 0.
// The v views of a scene share one style: `style_index` maps image -> style row, keys and values are stored once per style.
// Every output element is written exactly once by the one lane that owns it: no atomics, no zero-fill, bit-identical run to run.  Tails in Nq
// and M are masked (clamped loads, -inf logits, guarded stores).  A wave whose channel tile does not exist (C = 64, 192) repeats an existing
// tile and does not store it: no wave-uniform branch skips an MFMA chain (vit_common.h, mfma_result_fence).
//
// vit_adaattn_l1: cs = instance_norm(c) * std + mean per (image, channel) row, loss = sum |p - cs| / numel, grad = sign(p - cs) / numel
// (sign(0) = 0) in the same pass, cs itself when asked.  One workgroup per row: mean and biased variance of c (eps 1e-5) in two passes with
// float64 sums, then the pass proper; the rows' float64 partials are folded in index order by one workgroup (as gsr_depth_smooth_fwd does).
// Two launches, no atomics.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vit_common.h"
#include "vit_internal.h"

namespace vit {

constexpr int AA_NB = 64;          // content positions per workgroup (two 32-wide MFMA tiles)
constexpr int AA_MB = 128;         // style positions per step (four waves x 32)
constexpr int AA_DMAX = 448, AA_CMAX = 256;

struct AdaArgs {
    const float *q, *k, *s;
    const int32_t *idx;
    float *mean, *std;
    int D, C, Nq, M, vec;
};

__device__ inline f32x16 aa_mfma(float a, float b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0); }

// style values of keys m .. m + 3 (clamped into the row; keys past M carry p = 0) of each of the lane's channel rows
template <int CT>
__device__ inline void aa_load_s(const float *(&sp)[CT], int vec, int m, int M, float (&out)[CT][4])
{
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) {
        if (vec) {
            const float4 v = *reinterpret_cast<const float4 *>(sp[ct] + min(m, M - 4));
            out[ct][0] = v.x; out[ct][1] = v.y; out[ct][2] = v.z; out[ct][3] = v.w;
        } else {
#pragma unroll
            for (int u = 0; u < 4; ++u) out[ct][u] = sp[ct][min(m + u, M - 1)];
        }
    }
}

template <int CT>
__global__ void __launch_bounds__(256) k_adaattn_stats(const AdaArgs a)
{
    extern __shared__ float aa_lds[];
    float *__restrict__ Qs = aa_lds;                       // [D][64]
    float *__restrict__ Ss = aa_lds + a.D * AA_NB;         // [128][64]
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, l31 = lane & 31, h = lane >> 5;
    const int b = blockIdx.y, n0 = blockIdx.x * AA_NB;
    const int D = a.D, C = a.C, Nq = a.Nq, M = a.M;
    const int sb = a.idx[b];

    {   // (1) the queries of this workgroup
        const float *__restrict__ qb = a.q + (int64_t)b * D * Nq;
        for (int i = tid; i < D * AA_NB; i += 256) {
            const int d = i >> 6, n = min(n0 + (i & 63), Nq - 1);
            Qs[i] = qb[(int64_t)d * Nq + n];
        }
    }
    const int nct = C >> 5;
    int tix[CT];
    const float *sp[CT];
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) {
        tix[ct] = (w + 4 * ct) % nct;                       // (a tile that does not exist repeats an existing one and is not stored)
        sp[ct] = a.s + ((int64_t)sb * C + tix[ct] * 32 + l31) * M;
    }
    const float *__restrict__ kb = a.k + ((int64_t)sb * D + h) * M;

    f32x16 acc[CT][2][2];
#pragma unroll
    for (int ct = 0; ct < CT; ++ct)
#pragma unroll
        for (int mo = 0; mo < 2; ++mo)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[ct][mo][j][r] = 0.f;
    float mrun[2] = {-INFINITY, -INFINITY}, lsum[2] = {0.f, 0.f};
    __syncthreads();

    for (int m0 = 0; m0 < M; m0 += AA_MB) {
        {   // (2) logits of this wave's 32 keys against the 64 positions
            const float *__restrict__ kp = kb + min(m0 + w * 32 + l31, M - 1);
            const float *__restrict__ qp = Qs + h * AA_NB + l31;
            f32x16 x[2][2];
#pragma unroll
            for (int e = 0; e < 2; ++e)
#pragma unroll
                for (int j = 0; j < 2; ++j)
#pragma unroll
                    for (int r = 0; r < 16; ++r) x[e][j][r] = 0.f;
            // one wave per SIMD: nothing else hides the key loads, so the keys of step d0 + 16 are requested before the MFMAs of step d0
            float kv[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) kv[i] = kp[(int64_t)(2 * i) * M];
            for (int d0 = 0; d0 < D; d0 += 16) {              // (D % 64 == 0)
                const int dn = min(d0 + 16, D - 16);          // (the last step requests itself again: no branch around the loads)
                float kn[8];
#pragma unroll
                for (int i = 0; i < 8; ++i) kn[i] = kp[(int64_t)(dn + 2 * i) * M];
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    const int d = d0 + 2 * i;
                    x[i & 1][0] = aa_mfma(kv[i], qp[d * AA_NB], x[i & 1][0]);
                    x[i & 1][1] = aa_mfma(kv[i], qp[d * AA_NB + 32], x[i & 1][1]);
                }
#pragma unroll
                for (int i = 0; i < 8; ++i) kv[i] = kn[i];
            }
            mfma_result_fence();
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int row = w * 32 + rowmap(r, h);
                    Ss[row * AA_NB + j * 32 + l31] = (m0 + row < M) ? x[0][j][r] + x[1][j][r] : -INFINITY;
                }
        }
        __syncthreads();
        // (3) running maximum of the lane's position(s): its own 64 keys, then the other half-wave's
        const float *__restrict__ xs = Ss + (h * 64) * AA_NB + l31;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            float tm = -INFINITY;
#pragma unroll 8
            for (int t = 0; t < 64; ++t) tm = fmaxf(tm, xs[t * AA_NB + j * 32]);
            tm = fmaxf(tm, __shfl_xor(tm, 32, 64));
            const float mn = fmaxf(mrun[j], tm);             // finite: the first key of a tile always exists
            const float sc = expf(mrun[j] - mn);             // first tile: exp(-inf) = 0
            mrun[j] = mn;
            lsum[j] *= sc;
#pragma unroll
            for (int ct = 0; ct < CT; ++ct)
#pragma unroll
                for (int mo = 0; mo < 2; ++mo)
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc[ct][mo][j][r] *= sc;
        }
        // (4) both moments of the style rows under p
        const int mb = m0 + h * 64;
        float sv[CT][4];
        aa_load_s<CT>(sp, a.vec, mb, M, sv);
        for (int t4 = 0; t4 < 16; ++t4) {
            float sn[CT][4];                                  // the next four keys' style values, requested before this group's MFMAs
            aa_load_s<CT>(sp, a.vec, mb + min(t4 + 1, 15) * 4, M, sn);
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int t = t4 * 4 + u;
                const float p0 = expf(xs[t * AA_NB] - mrun[0]), p1 = expf(xs[t * AA_NB + 32] - mrun[1]);    // keys past M: exp(-inf) = 0
                lsum[0] += p0; lsum[1] += p1;
#pragma unroll
                for (int ct = 0; ct < CT; ++ct) {
                    const float v = sv[ct][u], v2 = v * v;
                    acc[ct][0][0] = aa_mfma(v, p0, acc[ct][0][0]);
                    acc[ct][0][1] = aa_mfma(v, p1, acc[ct][0][1]);
                    acc[ct][1][0] = aa_mfma(v2, p0, acc[ct][1][0]);
                    acc[ct][1][1] = aa_mfma(v2, p1, acc[ct][1][1]);
                }
            }
#pragma unroll
            for (int ct = 0; ct < CT; ++ct)
#pragma unroll
                for (int u = 0; u < 4; ++u) sv[ct][u] = sn[ct][u];
        }
        mfma_result_fence();
        __syncthreads();                                     // the tile is rewritten by the next step
    }

#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const float l = lsum[j] + __shfl_xor(lsum[j], 32, 64);
        const int n = n0 + j * 32 + l31;
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) {
            if (w + 4 * ct >= nct || n >= Nq) continue;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int c = tix[ct] * 32 + rowmap(r, h);
                const float mu = acc[ct][0][j][r] / l, e2 = acc[ct][1][j][r] / l;
                const float var = fmaxf(__fsub_rn(e2, __fmul_rn(mu, mu)), 0.f);      // (unfused, as the expression forms it)
                const int64_t o = ((int64_t)b * C + c) * Nq + n;
                a.mean[o] = mu;
                a.std[o] = sqrtf(var);
            }
        }
    }
}

int adaattn_stats(const float *q, const float *k, const float *s, const int32_t *index_host, const int32_t *index_dev, int Bq, int Bs, int D,
                  int C, int Nq, int M, float *mean, float *std, hipStream_t stream)
{
    if (!q || !k || !s || !index_host || !index_dev || !mean || !std) return VIT_EINVAL;
    if (Bq < 1 || Bq > 65535 || Bs < 1 || D < 64 || D % 64 || D > AA_DMAX || C < 64 || C % 64 || C > AA_CMAX || Nq < 1 || M < 1) return VIT_EINVAL;
    for (int i = 0; i < Bq; ++i)
        if (index_host[i] < 0 || index_host[i] >= Bs) return VIT_EINVAL;
    AdaArgs a{q, k, s, index_dev, mean, std, D, C, Nq, M, (M % 4 == 0 && (reinterpret_cast<uintptr_t>(s) & 15) == 0) ? 1 : 0};
    const size_t lds = (size_t)(D * AA_NB + AA_MB * AA_NB) * sizeof(float);
    const dim3 grid((Nq + AA_NB - 1) / AA_NB, Bq);
    (void)hipGetLastError();
    auto kern = C > 128 ? k_adaattn_stats<2> : k_adaattn_stats<1>;
    if (lds > 64 * 1024 &&
        hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) {
        g_last_hip_error = hipGetLastError();
        return VIT_ELAUNCH;
    }
    hipLaunchKernelGGL(kern, grid, dim3(256), lds, stream, a);
    return launch_status();
}

// ---- the tail ----------------------------------------------------------------------------------------------------------------------------------
__device__ inline double aa_block_sum(double v, double *red)
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

__global__ void __launch_bounds__(256) k_adaattn_l1(const float *__restrict__ p, const float *__restrict__ c, const float *__restrict__ mean,
                                                    const float *__restrict__ std, int N, float inv_numel, double *__restrict__ partial,
                                                    float *__restrict__ grad, float *__restrict__ cs_out)
{
    __shared__ double red[256];
    const int tid = threadIdx.x;
    const int64_t base = (int64_t)blockIdx.x * N;
    double s = 0.0;
    for (int i = tid; i < N; i += 256) s += (double)c[base + i];
    const double mu = aa_block_sum(s, red) / (double)N;
    s = 0.0;
    for (int i = tid; i < N; i += 256) {
        const double d = (double)c[base + i] - mu;
        s += d * d;
    }
    const double var = aa_block_sum(s, red) / (double)N;     // biased, like F.instance_norm
    const float muf = (float)mu, rs = (float)(1.0 / sqrt(var + 1e-5));
    s = 0.0;
    for (int i = tid; i < N; i += 256) {
        const float cs = fmaf((c[base + i] - muf) * rs, std[base + i], mean[base + i]);
        const float d = p[base + i] - cs;
        s += (double)fabsf(d);
        grad[base + i] = d > 0.f ? inv_numel : (d < 0.f ? -inv_numel : 0.f);
        if (cs_out) cs_out[base + i] = cs;
    }
    const double tot = aa_block_sum(s, red);
    if (tid == 0) partial[blockIdx.x] = tot;
}

// loss = the rows' partials added in index order (thread-strided, then one tree), divided by numel
__global__ void __launch_bounds__(256) k_adaattn_l1_fold(const double *__restrict__ partial, int rows, double inv_numel, float *__restrict__ loss)
{
    __shared__ double red[256];
    double s = 0.0;
    for (int i = threadIdx.x; i < rows; i += 256) s += partial[i];
    const double tot = aa_block_sum(s, red);
    if (threadIdx.x == 0) *loss = (float)(tot * inv_numel);
}

size_t adaattn_l1_scratch_bytes(int B, int C) { return (B < 1 || C < 1) ? 0 : (size_t)B * C * sizeof(double); }

int adaattn_l1(const float *p, const float *c, const float *mean, const float *std, int B, int C, int N, void *scratch, float *loss, float *grad,
               float *cs, hipStream_t stream)
{
    if (!p || !c || !mean || !std || !scratch || !loss || !grad || B < 1 || C < 1 || N < 1) return VIT_EINVAL;
    if ((int64_t)B * C > 0x7fffffff || (reinterpret_cast<uintptr_t>(scratch) & 7)) return VIT_EINVAL;
    const double numel = (double)B * C * N;
    (void)hipGetLastError();
    hipLaunchKernelGGL(k_adaattn_l1, dim3(B * C), dim3(256), 0, stream, p, c, mean, std, N, (float)(1.0 / numel), static_cast<double *>(scratch),
                       grad, cs);
    hipLaunchKernelGGL(k_adaattn_l1_fold, dim3(1), dim3(256), 0, stream, static_cast<const double *>(scratch), B * C, 1.0 / numel, loss);
    return launch_status();
}
}  // namespace vit
