// vit_attention_bwd_x6.hip -- flash attention backward at fp32 accuracy on the bf16 matrix cores (head_dim 64, no mask).
//
// The same two passes as vit_attention_bwd.hip (k_attn_delta is shared), with every contraction in split arithmetic out of the tile helpers of
// vit_attention_tiles.h (vit_attention_x6.hip is the forward), on 32-row tiles:
//   k_attn_bwd_q_x6    a wavefront owns 32 QUERIES (query = MFMA column = lane) and walks 32-key tiles:
//                        S^T  = K Q^T        A = K rows  (LDS)   B = Q  pieces (regs)
//                        dP^T = V dO^T       A = V rows  (LDS)   B = dO pieces (regs)
//                        dQ^T += K^T dS^T    A = K^T     (LDS)   B = dS pieces (regs, split as produced)
//   k_attn_bwd_kv_x6   a wavefront owns 32 KEYS (key = lane) and walks 32-query tiles:
//                        S  = Q K^T, dP = dO V^T          A = Q / dO rows (LDS)       B = K / V pieces (regs)
//                        dV^T += dO^T P, dK^T += Q^T dS   A = dO^T / Q^T  (LDS)       B = P / dS pieces (regs)
// With fused RoPE, Q and K are rotated while they are staged / loaded and dQ, dK are rotated back before they are stored
// (lane-local: features d and d + 16 sit in registers r and r + 8 of the same accumulator).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vit_attention_tiles.h"
#include "vit_internal.h"

namespace vit {
namespace abx6 {
constexpr int TR = 32;                          // rows per tile
constexpr int TROWB = 80;                       // bytes per d row of one transposed piece plane
constexpr int ROWS_BYTES = TR * ROWB, T_BYTES = 3 * HD * TROWB;

// ------------------------------------------------------------------ dQ
template <bool ROPE, int NP>
__global__ void __launch_bounds__(256, 2) k_attn_bwd_q_x6(VitAttnArgs a, const float *__restrict__ q, const float *__restrict__ k,
                                                          const float *__restrict__ v, const float *__restrict__ g,
                                                          const float *__restrict__ lse, const float *__restrict__ delta,
                                                          float *__restrict__ dq)
{
    __shared__ __attribute__((aligned(16))) unsigned char s_k[ROWS_BYTES], s_v[ROWS_BYTES], s_kt[T_BYTES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int half = lane >> 5, col = lane & 31;
    const int b = blockIdx.z, h = blockIdx.y;
    const int q0 = blockIdx.x * QB + wave * QW;
    const int qi = min(q0 + col, a.Nq - 1);
    const bool wave_active = q0 < a.Nq;

    // f16x3: power-of-two operand scales from the tensors' |max| words; the products are un-scaled right behind their MFMAs
    float sk = 1.f, sv = 1.f, sg = 1.f, sq = 1.f, inv_qk = 1.f, inv_gv = 1.f, s_run = 1.2676506e30f /* 2^100: no dS seen yet */;
    if (NP == 2) {
        sq = f16_scale_of(amax_word_read(a.amax_q)) * f16_prescale_headroom(a.scale * LOG2E);     // (Q is split after the scale * log2 e)
        sk = f16_scale_of(amax_word_read(a.amax_k));
        sv = f16_scale_of(amax_word_read(a.amax_v)); sg = f16_scale_of(amax_word_read(a.amax_g));
        inv_qk = 1.f / (sq * sk); inv_gv = 1.f / (sg * sv);
    }
    bf16x8 qf[4][3], gf[4][3];      // Q pre-scaled by scale * log2(e): only S consumes it
    load_row_pieces<ROPE, NP>(qf, q + (int64_t)b * a.q_sb + (int64_t)qi * a.q_sn + (int64_t)h * a.q_sh, half,
                              ROPE ? a.qpos + ((int64_t)b * a.Nq + qi) * 2 : nullptr, a.cos_tab, a.sin_tab, a.scale * LOG2E * sq);
    load_row_pieces<false, NP>(gf, g + (((int64_t)b * a.Nq + qi) * a.H + h) * HD, half, nullptr, nullptr, nullptr, sg);
    const float lse2 = lse[((int64_t)b * a.H + h) * a.Nq + qi] * LOG2E;
    const float del = delta[((int64_t)b * a.H + h) * a.Nq + qi];

    f32x16 dq0 = {0}, dq1 = {0};
    const float *kb = k + (int64_t)b * a.k_sb + (int64_t)h * a.k_sh;
    const float *vb = v + (int64_t)b * a.v_sb + (int64_t)h * a.v_sh;
    const int64_t *kpos = ROPE ? a.kpos + (int64_t)b * a.Nk * 2 : nullptr;

    // threads 0..127 stage the K rows, 128..255 the V rows; every thread one item of K^T
    RowItem ri; TItem ti;
    auto fetch = [&](int k0) {
        if (tid < 128) fetch_row_item<ROPE>(ri, kb, a.k_sn, k0, a.Nk, tid, kpos);
        else fetch_row_item<false>(ri, vb, a.v_sn, k0, a.Nk, tid - 128, nullptr);
        fetch_t_item<ROPE>(ti, kb, a.k_sn, k0, a.Nk, tid, kpos);
    };
    fetch(0);
    for (int k0 = 0; k0 < a.Nk; k0 += TR) {
        __syncthreads();
        if (tid < 128) store_row_item<ROPE, NP>(s_k, ri, k0, a.Nk, tid, a.cos_tab, a.sin_tab, sk);
        else store_row_item<false, NP>(s_v, ri, k0, a.Nk, tid - 128, nullptr, nullptr, sv);
        store_t_item<ROPE, NP>(s_kt, ti, k0, a.Nk, tid, a.cos_tab, a.sin_tab, sk);
        __syncthreads();
        if (k0 + TR < a.Nk) fetch(k0 + TR);
        if (!wave_active) continue;
        f32x16 st = rows_times_regs<NP>(s_k, col, half, qf);
        f32x16 dp = rows_times_regs<NP>(s_v, col, half, gf);
        if (NP == 2) mfma_result_fence();
        // element r: key k0 + rowmap(r), query = this lane
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int key = k0 + rowmap(r, half);
            const float sr = NP == 2 ? st[r] * inv_qk : st[r], dr = NP == 2 ? dp[r] * inv_gv : dp[r];
            const float p = key < a.Nk ? exp2f(sr - lse2) : 0.f;
            dp[r] = p * (dr - del) * a.scale;
        }
        const float sds = NP == 2 ? ds_running_scale(dp, s_run, dq0, dq1) : 1.f;
        t_times_regs<NP, TROWB>(s_kt, col, half, dp, dq0, dq1, sds);
    }
    mfma_result_fence();    // (loop exit right behind the last MFMAs: vit_common.h)
    if (NP == 2) {          // accumulated under (the lane's final dS scale) x (K's scale)
        const float f = 1.f / (s_run * sk);
#pragma unroll
        for (int r = 0; r < 16; ++r) { dq0[r] *= f; dq1[r] *= f; }
    }
    if (q0 + col < a.Nq) {
        if (ROPE) {
            const int64_t *pp = a.qpos + ((int64_t)b * a.Nq + q0 + col) * 2;
            unrotate(dq0, dq1, half, pp[0], pp[1], a.cos_tab, a.sin_tab);
        }
        store_64(dq + ((int64_t)b * a.Nq + q0 + col) * (a.dq_sn ? a.dq_sn : (int64_t)a.H * HD) + h * HD, dq0, dq1, half);   // (B,Nq,H,64), token stride dq_sn
    }
    if (a.amax_dq) amax_word_fold(a.amax_dq, (q0 + col < a.Nq) ? max_abs_32(dq0, dq1) : 0u);      // |max| of the stored gradient (after the inverse rotation)
}

// ------------------------------------------------------------------ dK, dV
template <bool ROPE, int NP>
__global__ void __launch_bounds__(256, 2) k_attn_bwd_kv_x6(VitAttnArgs a, const float *__restrict__ q, const float *__restrict__ k,
                                                           const float *__restrict__ v, const float *__restrict__ g,
                                                           const float *__restrict__ lse, const float *__restrict__ delta,
                                                           float *__restrict__ dk, float *__restrict__ dv)
{
    __shared__ __attribute__((aligned(16))) unsigned char s_q[ROWS_BYTES], s_g[ROWS_BYTES], s_qt[T_BYTES], s_gt[T_BYTES];
    __shared__ float s_lse[TR], s_delta[TR];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int half = lane >> 5, col = lane & 31;
    const int b = blockIdx.z, h = blockIdx.y;
    const int key0 = blockIdx.x * QB + wave * QW;
    const int ki = min(key0 + col, a.Nk - 1);
    const bool wave_active = key0 < a.Nk;

    float sk = 1.f, sv = 1.f, sg = 1.f, sq = 1.f, inv_qk = 1.f, inv_gv = 1.f, s_run = 1.2676506e30f /* 2^100: no dS seen yet */;
    constexpr float PSCALE = 16384.f;       // f16x3: the probabilities' scale (p <= 1)
    if (NP == 2) {
        sq = f16_scale_of(amax_word_read(a.amax_q));
        sk = f16_scale_of(amax_word_read(a.amax_k)) * f16_prescale_headroom(a.scale * LOG2E);     // (K is split after the scale * log2 e)
        sv = f16_scale_of(amax_word_read(a.amax_v)); sg = f16_scale_of(amax_word_read(a.amax_g));
        inv_qk = 1.f / (sq * sk); inv_gv = 1.f / (sg * sv);
    }
    bf16x8 kf[4][3], vf[4][3];      // K pre-scaled by scale * log2(e): only S consumes it
    load_row_pieces<ROPE, NP>(kf, k + (int64_t)b * a.k_sb + (int64_t)ki * a.k_sn + (int64_t)h * a.k_sh, half,
                              ROPE ? a.kpos + ((int64_t)b * a.Nk + ki) * 2 : nullptr, a.cos_tab, a.sin_tab, a.scale * LOG2E * sk);
    load_row_pieces<false, NP>(vf, v + (int64_t)b * a.v_sb + (int64_t)ki * a.v_sn + (int64_t)h * a.v_sh, half, nullptr, nullptr, nullptr, sv);

    f32x16 dk0 = {0}, dk1 = {0}, dv0 = {0}, dv1 = {0};
    const float *qb = q + (int64_t)b * a.q_sb + (int64_t)h * a.q_sh;
    const float *gb = g + ((int64_t)b * a.Nq * a.H + h) * HD;          // contiguous (B,Nq,H,64)
    const int64_t g_sn = (int64_t)a.H * HD;
    const float *lse_b = lse + ((int64_t)b * a.H + h) * a.Nq;
    const float *del_b = delta + ((int64_t)b * a.H + h) * a.Nq;
    const int64_t *qpos = ROPE ? a.qpos + (int64_t)b * a.Nq * 2 : nullptr;

    // threads 0..127 stage the Q rows, 128..255 the dO rows; every thread one item of Q^T and one of dO^T
    // (only the row item is prefetched across the MFMA phase: the two transposed items on top of the 96 registers of K / V pieces
    // and the four accumulators spilled 49 registers; their loads are issued at the top of the tile and hit the L2 lines the row
    // items of the same tile just fetched)
    RowItem ri;
    auto fetch = [&](int q0) {
        if (tid < 128) fetch_row_item<ROPE>(ri, qb, a.q_sn, q0, a.Nq, tid, qpos);
        else fetch_row_item<false>(ri, gb, g_sn, q0, a.Nq, tid - 128, nullptr);
    };
    fetch(0);
    for (int q0 = 0; q0 < a.Nq; q0 += TR) {
        TItem tq, tg;
        fetch_t_item<ROPE>(tq, qb, a.q_sn, q0, a.Nq, tid, qpos);
        fetch_t_item<false>(tg, gb, g_sn, q0, a.Nq, tid, nullptr);
        __syncthreads();
        if (tid < 128) store_row_item<ROPE, NP>(s_q, ri, q0, a.Nq, tid, a.cos_tab, a.sin_tab, sq);
        else store_row_item<false, NP>(s_g, ri, q0, a.Nq, tid - 128, nullptr, nullptr, sg);
        store_t_item<ROPE, NP>(s_qt, tq, q0, a.Nq, tid, a.cos_tab, a.sin_tab, sq);
        store_t_item<false, NP>(s_gt, tg, q0, a.Nq, tid, nullptr, nullptr, sg);
        if (tid < TR) {
            const int qi = q0 + tid;
            s_lse[tid] = qi < a.Nq ? lse_b[qi] * LOG2E : INFINITY;   // padded queries: P = exp2(-inf) = 0
            s_delta[tid] = qi < a.Nq ? del_b[qi] : 0.f;
        }
        __syncthreads();
        if (q0 + TR < a.Nq) fetch(q0 + TR);
        if (!wave_active) continue;
        f32x16 sc = rows_times_regs<NP>(s_q, col, half, kf);
        f32x16 dp = rows_times_regs<NP>(s_g, col, half, vf);
        if (NP == 2) mfma_result_fence();
        // element r: query q0 + rowmap(r), key = this lane
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int qr = rowmap(r, half);
            const float sr = NP == 2 ? sc[r] * inv_qk : sc[r], dr = NP == 2 ? dp[r] * inv_gv : dp[r];
            const float p = exp2f(sr - s_lse[qr]);
            sc[r] = p;                                        // P
            dp[r] = p * (dr - s_delta[qr]) * a.scale;         // dS (w.r.t. the unscaled dot product)
        }
        t_times_regs<NP, TROWB>(s_gt, col, half, sc, dv0, dv1, PSCALE);
        const float sds = NP == 2 ? ds_running_scale(dp, s_run, dk0, dk1) : 1.f;
        t_times_regs<NP, TROWB>(s_qt, col, half, dp, dk0, dk1, sds);
    }
    mfma_result_fence();
    if (NP == 2) {
        const float fk = 1.f / (s_run * sq), fv = 1.f / (PSCALE * sg);
#pragma unroll
        for (int r = 0; r < 16; ++r) { dk0[r] *= fk; dk1[r] *= fk; dv0[r] *= fv; dv1[r] *= fv; }
    }
    if (key0 + col < a.Nk) {
        if (ROPE) {
            const int64_t *pp = a.kpos + ((int64_t)b * a.Nk + key0 + col) * 2;
            unrotate(dk0, dk1, half, pp[0], pp[1], a.cos_tab, a.sin_tab);
        }
        // dk, dv (B,Nk,H,64), token stride dkv_sn
        store_64(dk + ((int64_t)b * a.Nk + key0 + col) * (a.dkv_sn ? a.dkv_sn : (int64_t)a.H * HD) + h * HD, dk0, dk1, half);
        store_64(dv + ((int64_t)b * a.Nk + key0 + col) * (a.dkv_sn ? a.dkv_sn : (int64_t)a.H * HD) + h * HD, dv0, dv1, half);
    }
    const bool stored = key0 + col < a.Nk;
    if (a.amax_dk) amax_word_fold(a.amax_dk, stored ? max_abs_32(dk0, dk1) : 0u);
    if (a.amax_dv) amax_word_fold(a.amax_dv, stored ? max_abs_32(dv0, dv1) : 0u);
}
}  // namespace abx6

// launched by attention_bwd (vit_attention_bwd.hip) in place of its two f32 kernels when the split-arithmetic mode is on
hipError_t launch_attention_bwd_x6(const VitAttnArgs &a, const float *q, const float *k, const float *v, const float *dout, const float *lse,
                                   const float *delta, float *dq, float *dk, float *dv, dim3 gkv, dim3 gq, int products, hipStream_t stream)
{
    for_rope_products(a.cos_tab != nullptr, products, [&](auto rope, auto np) {
        hipLaunchKernelGGL((abx6::k_attn_bwd_kv_x6<rope.value, np.value>), gkv, dim3(256), 0, stream, a, q, k, v, dout, lse, delta, dk, dv);
        hipLaunchKernelGGL((abx6::k_attn_bwd_q_x6<rope.value, np.value>), gq, dim3(256), 0, stream, a, q, k, v, dout, lse, delta, dq);
    });
    return hipGetLastError();
}
}  // namespace vit
