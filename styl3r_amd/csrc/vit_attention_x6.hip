// vit_attention_x6.hip -- flash attention forward at fp32 accuracy on the bf16 matrix cores (head_dim 64, no mask).
//
// vit_attention.hip runs both contractions on the exact-f32 MFMA (157 TF peak, 64 cycles per 32x32x2 step).  Here Q, K, V
// and the probabilities are split into three bf16 pieces and every contraction takes six v_mfma_f32_32x32x16_bf16 per 16-wide step:
// 24 MFMAs x 32 cycles instead of 32 x 64 per (32 x 32 x 64) block, 2.7x less matrix-pipe time, and the pipes that are busy are the
// bf16 ones the power budget is kinder to.  Same orientation as the f32 kernel, out of the tile helpers of vit_attention_tiles.h:
//     S^T (32 keys x 32 queries) = K (32 x 64) . Q^T          rows_times_regs: K rows image (64 keys), Q pieces in registers
//     O^T (32 d    x 32 queries) = V^T (32 x keys) . P^T      t_times_regs:    V^T planes (64 permuted keys), P as the softmax left it
// LDS per workgroup (128 queries, 4 wavefronts; 64-key tiles): 25.6 KB of K rows + 27.6 KB of V^T planes.
//
// Three blocks of this kernel are still its own text although a helper says the same: the Q fragments (= load_row_pieces), the K store
// (= store_row_item) and the mask + online-softmax step (= mask_keys_past, online_softmax_step).  Which product of a RoPE rotation the compiler
// fuses into the sum depends on the code around it, and with any of the three taken from the header the <ROPE = true> instantiations fuse
// other pairs than before: scores, and with them every output, move in the last bit.  They go to the helpers together with the next change
// that is allowed to move those bits.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vit_attention_tiles.h"
#include "vit_internal.h"

namespace vit {
namespace ax6 {
constexpr int KT = 64;               // keys per tile
constexpr int VROW = 144;            // bytes per d row of one V^T piece plane
constexpr int K_BYTES = KT * ROWB, V_BYTES = 3 * HD * VROW;

template <bool ROPE, int NP>
__global__ void __launch_bounds__(256, 2) k_attn_fwd_x6(VitAttnArgs a, const float *__restrict__ q, const float *__restrict__ k,
                                                        const float *__restrict__ v, float *__restrict__ out, float *__restrict__ lse)
{
    __shared__ __attribute__((aligned(16))) unsigned char s_k[K_BYTES];
    __shared__ __attribute__((aligned(16))) unsigned char s_v[V_BYTES];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int half = lane >> 5, col = lane & 31;
    const int b = blockIdx.z, h = blockIdx.y;
    const int q0 = blockIdx.x * QB + wave * QW;
    const int qi = min(q0 + col, a.Nq - 1);   // clamped: rows beyond Nq compute garbage that is never stored
    const bool wave_active = q0 < a.Nq;
    float qscale = a.scale * LOG2E;   // scores in the base-2 domain
    // f16x3: tensor scales (a rotation grows a component by at most sqrt 2: |max| s < 2^15.5, inside fp16's 65 504; Q is split after its
    // multiplication by qscale, so its power of two leaves room for that factor too: f16_prescale_headroom) and the two inverse factors
    float sk = 1.f, sv = 1.f, inv_qk = 1.f, inv_pv = 1.f;
    constexpr float PSCALE = 16384.f;
    if (NP == 2) {
        const float sq = f16_scale_of(amax_word_read(a.amax_q)) * f16_prescale_headroom(qscale);
        sk = f16_scale_of(amax_word_read(a.amax_k)); sv = f16_scale_of(amax_word_read(a.amax_v));
        qscale *= sq;
        inv_qk = 1.f / (sq * sk); inv_pv = 1.f / (PSCALE * sv);
    }

    bf16x8 qf[4][3];                // (load_row_pieces' text: see the file header)
    {
        const float *qr = q + (int64_t)b * a.q_sb + (int64_t)qi * a.q_sn + (int64_t)h * a.q_sh;
        float x[4][8];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const float4 lo = *reinterpret_cast<const float4 *>(qr + 16 * t + 8 * half), hi = *reinterpret_cast<const float4 *>(qr + 16 * t + 8 * half + 4);
            x[t][0] = lo.x; x[t][1] = lo.y; x[t][2] = lo.z; x[t][3] = lo.w; x[t][4] = hi.x; x[t][5] = hi.y; x[t][6] = hi.z; x[t][7] = hi.w;
        }
        if (ROPE) {
            const int64_t py = a.qpos[((int64_t)b * a.Nq + qi) * 2 + 0], px = a.qpos[((int64_t)b * a.Nq + qi) * 2 + 1];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int d = 8 * half + j;
                const float cy = a.cos_tab[py * 16 + d], sy = a.sin_tab[py * 16 + d];
                const float cx = a.cos_tab[px * 16 + d], sx = a.sin_tab[px * 16 + d];
                const float uy = x[0][j], vy = x[1][j], ux = x[2][j], vx = x[3][j];
                x[0][j] = uy * cy - vy * sy; x[1][j] = vy * cy + uy * sy;
                x[2][j] = ux * cx - vx * sx; x[3][j] = vx * cx + ux * sx;
            }
        }
#pragma unroll
        for (int t = 0; t < 4; ++t) {
#pragma unroll
            for (int j = 0; j < 8; ++j) x[t][j] *= qscale;
            split8p<NP>(x[t], qf[t][0], qf[t][1], qf[t][2]);
        }
    }

    f32x16 o0 = {0}, o1 = {0};          // O^T rows d = rowmap(r) and 32 + rowmap(r), column = this lane's query
    float m = -INFINITY, l = 0.f;

    const float *kb = k + (int64_t)b * a.k_sb + (int64_t)h * a.k_sh;
    const float *vb = v + (int64_t)b * a.v_sb + (int64_t)h * a.v_sh;
    const int64_t *kpos = ROPE ? a.kpos + (int64_t)b * a.Nk * 2 : nullptr;

    // staging.  K: every thread one item of the 64-row image.  V^T is this kernel's own code, not store_t_item: V has no RoPE partner to fetch
    // with it, so an item is (4 consecutive keys, ONE d) with d = the lane -- every load a coalesced row piece -- and a plane holds 64 keys.
    RowItem ri;
    float vreg[4][4];
    auto fetch = [&](int k0) {
        fetch_row_item<ROPE>(ri, kb, a.k_sn, k0, a.Nk, tid, kpos);
#pragma unroll
        for (int it = 0; it < 4; ++it) {       // item = (four consecutive keys 4 m .. 4 m + 3, one d)
            const int m_ = wave + 4 * it;
#pragma unroll
            for (int e = 0; e < 4; ++e) vreg[it][e] = vb[(int64_t)min(k0 + 4 * m_ + e, a.Nk - 1) * a.v_sn + lane];
        }
    };
    fetch(0);
    for (int k0 = 0; k0 < a.Nk; k0 += KT) {
        __syncthreads();   // previous tile fully consumed
        {   // ---- K -> pieces, row-major (store_row_item's text: see the file header) ----
            const int skey = tid >> 2, sub = tid & 3, sg = 4 * (sub >> 1) + (sub & 1);
            const bool real = k0 + skey < a.Nk;     // rows beyond Nk are zeros (and masked to -inf below)
            float u[8] = {ri.a0.x, ri.a0.y, ri.a0.z, ri.a0.w, ri.a1.x, ri.a1.y, ri.a1.z, ri.a1.w};
            float w[8] = {ri.b0.x, ri.b0.y, ri.b0.z, ri.b0.w, ri.b1.x, ri.b1.y, ri.b1.z, ri.b1.w};
            if (ROPE) {
                const int pos = (sub >> 1) ? ri.px : ri.py;
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const int d = 8 * (sub & 1) + j;
                    const float c = a.cos_tab[pos * 16 + d], s = a.sin_tab[pos * 16 + d];
                    const float t0 = u[j] * c - w[j] * s, t1 = w[j] * c + u[j] * s;
                    u[j] = t0; w[j] = t1;
                }
            }
            if (!real) {
#pragma unroll
                for (int j = 0; j < 8; ++j) { u[j] = 0.f; w[j] = 0.f; }
            }
            if (NP == 2) {
#pragma unroll
                for (int j = 0; j < 8; ++j) { u[j] *= sk; w[j] *= sk; }
            }
            bf16x8 f0, f1, f2;
            bf16x8 *row = reinterpret_cast<bf16x8 *>(s_k + skey * ROWB);
            split8p<NP>(u, f0, f1, f2);
            row[sg * 3 + 0] = f0; row[sg * 3 + 1] = f1;
            if (NP == 6) row[sg * 3 + 2] = f2;
            split8p<NP>(w, f0, f1, f2);
            row[(sg + 2) * 3 + 0] = f0; row[(sg + 2) * 3 + 1] = f1;
            if (NP == 6) row[(sg + 2) * 3 + 2] = f2;
        }
#pragma unroll
        for (int it = 0; it < 4; ++it) {   // ---- V -> transposed pieces, key axis permuted ----
            // keys 4 m + e: key = 32 blk + (j & 3) + 8 (2u + (j >> 2)) + 4 hh  ->  position 32 blk + 16 u + 8 hh + j, j = e + 4 ((m >> 1) & 1)
            const int m_ = wave + 4 * it;
            const int pos = 32 * (m_ >> 3) + 16 * ((m_ >> 2) & 1) + 8 * (m_ & 1) + 4 * ((m_ >> 1) & 1);
            float x[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) x[e] = (k0 + 4 * m_ + e < a.Nk) ? vreg[it][e] : 0.f;
            uint2 w0, w1, w2;                            // packed pairs: low half = first value
            split2p<NP>(x[0] * sv, x[1] * sv, w0.x, w1.x, w2.x);        // (sv = 1 unless f16x3)
            split2p<NP>(x[2] * sv, x[3] * sv, w0.y, w1.y, w2.y);
            unsigned char *dst = s_v + lane * VROW + pos * 2;
            *reinterpret_cast<uint2 *>(dst) = w0;
            *reinterpret_cast<uint2 *>(dst + HD * VROW) = w1;
            if (NP == 6) *reinterpret_cast<uint2 *>(dst + 2 * HD * VROW) = w2;
        }
        __syncthreads();
        if (k0 + KT < a.Nk) fetch(k0 + KT);
        if (!wave_active) continue;
        const bool two = k0 + 32 < a.Nk;   // second 32-key block holds at least one real key

        f32x16 st0 = rows_times_regs<NP>(s_k, col, half, qf), st1 = {0};
        if (two) st1 = rows_times_regs<NP>(s_k + 32 * ROWB, col, half, qf);
        mfma_result_fence();            // (the branch around the second block's MFMAs joins here: see vit_common.h)
        if (NP == 2) {
#pragma unroll
            for (int r = 0; r < 16; ++r) { st0[r] *= inv_qk; st1[r] *= inv_qk; }
        }
        // mask keys beyond Nk: element r of block kb is key k0 + 32 kb + (r&3) + 8 (r>>2) + 4 half
        if (k0 + KT > a.Nk) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int key = k0 + (r & 3) + 8 * (r >> 2) + 4 * half;
                if (key >= a.Nk) st0[r] = -INFINITY;
                if (key + 32 >= a.Nk) st1[r] = -INFINITY;
            }
        }
        // ---- online softmax (base 2) ----
        float tmax = st0[0];
#pragma unroll
        for (int r = 1; r < 16; ++r) tmax = fmaxf(tmax, st0[r]);
#pragma unroll
        for (int r = 0; r < 16; ++r) tmax = fmaxf(tmax, st1[r]);
        tmax = fmaxf(tmax, wave_xor32(tmax));
        const float m_new = fmaxf(m, tmax);
        const float alpha = exp2f(m - m_new);
        float psum = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) { st0[r] = exp2f(st0[r] - m_new); psum += st0[r]; }
#pragma unroll
        for (int r = 0; r < 16; ++r) { st1[r] = exp2f(st1[r] - m_new); psum += st1[r]; }
        psum += wave_xor32(psum);
        l = l * alpha + psum;
        m = m_new;
#pragma unroll
        for (int r = 0; r < 16; ++r) { o0[r] *= alpha; o1[r] *= alpha; }

        t_times_regs<NP, VROW>(s_v, col, half, st0, o0, o1, PSCALE);
        if (two) t_times_regs<NP, VROW>(s_v + 64, col, half, st1, o0, o1, PSCALE);        // (block 1: positions 32 .. 63 of a plane)
    }

    // ---- epilogue: O = O^T / l ----
    mfma_result_fence();                // (loop exit right behind the last P V MFMAs)
    uint32_t omax = 0;              // |max| of the stored values (VitAttnArgs.amax_out)
    if (q0 + col < a.Nq) {
        const float inv = (NP == 2 ? inv_pv : 1.f) / l;
        if (a.amax_out) omax = max_abs_32(o0, o1, inv);
        store_64(out + (int64_t)b * a.o_sb + (int64_t)(q0 + col) * a.o_sn + (int64_t)h * a.o_sh, o0, o1, half, inv);
        if (lse && half == 0) lse[((int64_t)b * a.H + h) * a.Nq + q0 + col] = (m + log2f(l)) * 0.6931471805599453f;
    }
    if (a.amax_out) amax_word_fold(a.amax_out, omax);      // (wave-uniform branch; waves past Nq fold 0)
}
}  // namespace ax6

// launched by attention_fwd (vit_attention.hip) when the split-arithmetic mode is on; same grid, same tail handling
hipError_t launch_attention_fwd_x6(const VitAttnArgs &a, const float *q, const float *k, const float *v, float *out, float *lse, dim3 grid,
                                   int products, hipStream_t stream)
{
    for_rope_products(a.cos_tab != nullptr, products, [&](auto rope, auto np) {
        hipLaunchKernelGGL((ax6::k_attn_fwd_x6<rope.value, np.value>), grid, dim3(256), 0, stream, a, q, k, v, out, lse);
    });
    return hipGetLastError();
}
}  // namespace vit
