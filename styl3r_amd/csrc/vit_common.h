// vit_common.h -- the device helpers the encoder's kernels (csrc/vit_*.hip) share: vector types, exact GELU, the "bf16x6" / "bf16x3" /
// "f16x3" split arithmetic (vit_gemm_x6.hip's file header explains bf16x6, the paragraph on f16x3 is below), the |max| word of the f16x3
// operand scales, the XCD-aware tile walk, the accumulator row map, the dropout generator -- and the host-side launch status of the C ABI.
// One definition each: a tensor split in one kernel gets the same pieces as in every other, and the parity fixtures of tests/golden/
// were recorded against exactly these functions.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/vit_ops.h"

namespace vit {
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

__device__ inline float gelu_exact(float x) { return 0.5f * x * (1.0f + erff(x * 0.70710678118654752f)); }
// d/dx of the exact GELU: Phi(x) + x phi(x)   (aten's GeluBackward, approximate = "none")
__device__ inline float gelu_grad_exact(float x)
{
    return 0.5f * (1.0f + erff(x * 0.70710678118654752f)) + x * 0.3989422804014327f * __expf(-0.5f * x * x);
}

// ---- "bf16x6" / "bf16x3": three bf16 pieces per fp32 value --------------------------------------------------------------------------------
// two fp32 values -> their three bf16 pieces, each packed (lo = first value)
__device__ inline void split2(float a, float b, uint32_t &p0, uint32_t &p1, uint32_t &p2)
{
    f32x2 f = {a, b};
    const bf16x2 h0 = __builtin_convertvector(f, bf16x2);
    const f32x2 r1 = f - __builtin_convertvector(h0, f32x2);
    const bf16x2 h1 = __builtin_convertvector(r1, bf16x2);
    const f32x2 r2 = r1 - __builtin_convertvector(h1, f32x2);
    const bf16x2 h2 = __builtin_convertvector(r2, bf16x2);
    p0 = __builtin_bit_cast(uint32_t, h0); p1 = __builtin_bit_cast(uint32_t, h1); p2 = __builtin_bit_cast(uint32_t, h2);
}
// eight fp32 values (lo.x .. hi.w) -> three pieces of eight
template <typename V4> __device__ inline void split8(const V4 &lo, const V4 &hi, uint4 &q0, uint4 &q1, uint4 &q2)
{
    split2(lo.x, lo.y, q0.x, q1.x, q2.x);
    split2(lo.z, lo.w, q0.y, q1.y, q2.y);
    split2(hi.x, hi.y, q0.z, q1.z, q2.z);
    split2(hi.z, hi.w, q0.w, q1.w, q2.w);
}
template <typename V4> __device__ inline void split8(const V4 &lo, const V4 &hi, bf16x8 &f0, bf16x8 &f1, bf16x8 &f2)
{
    uint4 q0, q1, q2;
    split8(lo, hi, q0, q1, q2);
    f0 = __builtin_bit_cast(bf16x8, q0); f1 = __builtin_bit_cast(bf16x8, q1); f2 = __builtin_bit_cast(bf16x8, q2);
}
__device__ inline void split8(const float *v, bf16x8 &f0, bf16x8 &f1, bf16x8 &f2)
{
    split8(make_float4(v[0], v[1], v[2], v[3]), make_float4(v[4], v[5], v[6], v[7]), f0, f1, f2);
}

// ---- "f16x3": two fp16 pieces per fp32 value, three products on v_mfma_f32_32x32x16_f16 --------------------------------------------------
// An fp32 value scaled by a power of two splits into two fp16 pieces, a s = h + l + O(2^-22 |a s|) (h = round-to-nearest fp16, 11-bit
// significand; l = fp16 of the exact residual), and h h' + (h l' + l h') reproduces the product to 2^-22 -- 64 x tighter than the three
// bf16 products of "bf16x3" (2^-16) at the SAME three MFMAs per k-step and the same two-piece data path.  What fp16 lacks is range
// (2^-24 .. 65 504), so every operand TENSOR carries a power-of-two scale taken from its own absolute maximum (`k_amax`, an exact integer
// max over the fp32 bit patterns): 2^14 <= amax s < 2^15.  Elements down to 2^-17 amax keep all 22 bits, smaller ones an absolute error of
// 2^-39 amax -- below the fp32 rounding of any sum they enter.  Scales are powers of two, so scaling and un-scaling are exact; the epilogue
// multiplies the fp32 accumulator by the two inverse scales.
__device__ inline float f16_scale_of(uint32_t amax_bits)
{
    const int e = (int)((amax_bits >> 23) & 0xff);
    if (e == 0 || e == 255) return 1.f;        // all-zero / denormal tensor; Inf / NaN inside (those propagate on their own)
    const int se = min(max(127 + 14 - (e - 127), 27), 227);       // s in [2^-100, 2^100]
    return __builtin_bit_cast(float, (uint32_t)se << 23);
}
// The extra power of two for an operand that is split AFTER a multiplication by a constant c (the attention's Q or K times scale * log2 e):
// |max| s |c| stays below 2^15 (2^15.5 with a RoPE rotation, still inside fp16's 65 504).  1 for |c| < 1 -- scale < 0.69, every model call --
// so the operand's power of two is f16_scale_of's own there; 2^-(e+1) for |c| in [2^e, 2^(e+1)).
__device__ inline float f16_prescale_headroom(float c)
{
    const int e = min((int)((__builtin_bit_cast(uint32_t, c) >> 23) & 0xff) - 127, 100);
    return e < 0 ? 1.f : __builtin_bit_cast(float, (uint32_t)(126 - e) << 23);
}
// Two (scaled) fp32 values -> their two fp16 pieces, each packed (low half = first value): h = RNE fp16, l = fp16 of the exact residual
// (a - h is exact in fp32).  Two functions, the same bits:
//   f16_split2      plain vector conversions: safe for pieces that feed an MFMA straight from registers.  The compiler only inserts the
//                   VALU-write -> MFMA-read wait states for instructions it can see -- with the asm form the attention forward's last key tile
//                   read a stale B operand whenever its second 32-key block was skipped (round 6, tools/probes/attn_f16_debug.py);
//   f16_split2_lds  inline asm, one instruction shorter (v_fma_mix_f32 reads the fp16 halves in place: no v_cvt_f32_f16): only for pieces
//                   that are stored to LDS before an MFMA reads them (the LDS-staged operands of the GEMMs).
__device__ inline void f16_split2(float a, float b, uint32_t &p0, uint32_t &p1)
{
    const f32x2 f = {a, b};
    const f16x2 h = __builtin_convertvector(f, f16x2);
    const f32x2 r = f - __builtin_convertvector(h, f32x2);
    const f16x2 l = __builtin_convertvector(r, f16x2);
    p0 = __builtin_bit_cast(uint32_t, h); p1 = __builtin_bit_cast(uint32_t, l);
}
__device__ inline void f16_split2_lds(float a, float b, uint32_t &p0, uint32_t &p1)
{
    float ra, rb;
    asm("v_cvt_pk_f16_f32 %0, %1, %2" : "=v"(p0) : "v"(a), "v"(b));
    asm("v_fma_mix_f32 %0, %1, 1.0, -%2 op_sel:[0,0,0] op_sel_hi:[0,0,1]" : "=v"(ra) : "v"(a), "v"(p0));
    asm("v_fma_mix_f32 %0, %1, 1.0, -%2 op_sel:[0,0,1] op_sel_hi:[0,0,1]" : "=v"(rb) : "v"(b), "v"(p0));
    asm("v_cvt_pk_f16_f32 %0, %1, %2" : "=v"(p1) : "v"(ra), "v"(rb));
}
// eight ALREADY SCALED fp32 values -> two fp16x8 pieces (in bf16x8 registers: only the MFMA reinterprets them)
__device__ inline void split8h(const float *v, bf16x8 &f0, bf16x8 &f1)
{
    uint4 q0, q1;
    f16_split2(v[0], v[1], q0.x, q1.x);
    f16_split2(v[2], v[3], q0.y, q1.y);
    f16_split2(v[4], v[5], q0.z, q1.z);
    f16_split2(v[6], v[7], q0.w, q1.w);
    f0 = __builtin_bit_cast(bf16x8, q0); f1 = __builtin_bit_cast(bf16x8, q1);
}

// ---- the split of a kernel's product count: NPROD / NP == 6 / 3: three bf16 pieces (the third unused by 3); == 2: two fp16 pieces ----------
// attention operands (register-fed): eight values, already scaled in f16x3 (f2 is left alone there)
template <int NP> __device__ inline void split8p(const float *v, bf16x8 &f0, bf16x8 &f1, bf16x8 &f2)
{
    if (NP == 2) split8h(v, f0, f1); else split8(v, f0, f1, f2);
}
// GEMM operands (LDS-staged): eight values, scaled by s in f16x3 (q2 is left alone there)
template <int NPROD, typename V4> __device__ inline void split8s(const V4 &lo, const V4 &hi, float s, uint4 &q0, uint4 &q1, uint4 &q2)
{
#ifdef VIT_EXP_NOSPLIT   /* experiment builds only (tools/exp_nosplit.sh): the operand as if it arrived already split -- WRONG results, the same loads / LDS traffic / MFMAs */
    if (NPROD == 2) { q0 = __builtin_bit_cast(uint4, lo); q1 = __builtin_bit_cast(uint4, hi); return; }
#endif
    if (NPROD == 2) {
        f16_split2_lds(lo.x * s, lo.y * s, q0.x, q1.x);
        f16_split2_lds(lo.z * s, lo.w * s, q0.y, q1.y);
        f16_split2_lds(hi.x * s, hi.y * s, q0.z, q1.z);
        f16_split2_lds(hi.z * s, hi.w * s, q0.w, q1.w);
    } else {
        split8(lo, hi, q0, q1, q2);
    }
}
template <int NPROD, typename V4> __device__ inline void split8s(const V4 &lo, const V4 &hi, float s, bf16x8 &f0, bf16x8 &f1, bf16x8 &f2)
{
    uint4 q0, q1, q2;
    split8s<NPROD>(lo, hi, s, q0, q1, q2);
    f0 = __builtin_bit_cast(bf16x8, q0); f1 = __builtin_bit_cast(bf16x8, q1); f2 = NPROD == 2 ? f1 : __builtin_bit_cast(bf16x8, q2);
}

// one MFMA of the mode's type: the f16 MFMA for NPROD == 2, the bf16 one otherwise
template <int NPROD> __device__ inline f32x16 mma(const bf16x8 &a, const bf16x8 &b, const f32x16 &c)
{
    if (NPROD == 2) return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
}
template <int NPROD> __device__ inline f32x16 mma(const uint4 &a, const uint4 &b, const f32x16 &c)
{
    return mma<NPROD>(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c);
}
// All partial products of one 16-wide step from piece arrays, smallest first.  NP = 6: six; NP = 3 ("bf16x3"): the three 2^-16-level products
// are left out -- the third bf16 piece of every operand is then never used: the compiler drops its computation, the image stores skip it;
// NP = 2 ("f16x3"): h l' + l h' + h h' on the f16 MFMA (2^-22 per product).
template <int NP>
__device__ inline f32x16 mfma6(const bf16x8 (&a)[3], const bf16x8 (&b)[3], f32x16 c)
{
    if (NP == 2) {
        c = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a[1]), __builtin_bit_cast(f16x8, b[0]), c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a[0]), __builtin_bit_cast(f16x8, b[1]), c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a[0]), __builtin_bit_cast(f16x8, b[0]), c, 0, 0, 0);
        return c;
    }
    if (NP == 6) {
        c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[2], b[0], c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[1], b[1], c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0], b[2], c, 0, 0, 0);
    }
    c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[1], b[0], c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0], b[1], c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0], b[0], c, 0, 0, 0);
    return c;
}

// Twenty wait states.  hipcc (ROCm 7.2) inserts the "XDL write VGPR -> VALU read" wait states (11 for an 8-pass MFMA) only along the
// fall-through path of a block: where a wave-uniform branch skips a second MFMA chain and joins in front of VALU code that reads the FIRST
// chain's accumulator, the listing shows `s_nop 3` and the last accumulator registers are read before the matrix pipe has written them
// (round 6: the f16x3 attention forward un-scales S right behind its MFMAs and got keys 26, 27, 30, 31 of a tile wrong whenever the tile's
// second 32-key block was skipped; tools/probes/attn_f16_debug2.py).  Placed by hand where an accumulator is read across such a join / a loop exit.
__device__ inline void mfma_result_fence() { asm volatile("s_nop 15\n\ts_nop 3" ::: "memory"); }

// ---- the |max| word of the f16x3 operand scales ------------------------------------------------------------------------------------------
// An "|max| word" is 64 words, ONE PER 128-BYTE CACHE LINE (8 KiB in all): producers fold their maxima into word (workgroup + wave) & 63.
// L2 atomics serialise per cache line at ~10 ns each -- thousands of waves folding into one line cost 20 - 50 us per launch (measured: +9 ms per
// train step from the LayerNorm epilogues alone, and no better with 64 words packed into two lines); spread over 64 lines they run in parallel
// channels.  Readers take the max over the 64 words with one gather load and a wave reduction.
constexpr int AMAX_WORD_STRIDE = 32;        // uint32 words between the 64 slots
__device__ inline uint32_t abs_bits(float x) { return __builtin_bit_cast(uint32_t, x) & 0x7fffffffu; }
__device__ inline uint32_t amax_word_read(const uint32_t *__restrict__ word)        // all 64 lanes: the max over the 64 slots
{
    uint32_t m = word[(threadIdx.x & 63) * AMAX_WORD_STRIDE];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = max(m, (uint32_t)__shfl_xor((int)m, o, 64));
    return m;
}
// m: this lane's maximum (bit pattern of |x|); all 64 lanes of the wave call it together, one guarded atomicMax per wave.  wg: the workgroup's
// part of the slot, from the block indices the kernel reads anyway (a kernel that reads one more of them gets another descriptor and code)
__device__ inline void amax_word_fold(uint32_t *__restrict__ word, uint32_t m, uint32_t wg = blockIdx.x + 7u * blockIdx.y + 13u * blockIdx.z)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = max(m, (uint32_t)__shfl_xor((int)m, o, 64));
    uint32_t *w = word + ((wg + (threadIdx.x >> 6)) & 63u) * AMAX_WORD_STRIDE;
    if ((threadIdx.x & 63) == 0 && m > __atomic_load_n(w, __ATOMIC_RELAXED)) atomicMax(w, m);
}

// Workgroup id -> output tile.  (1) Consecutive workgroup ids are dealt round-robin to the 8 XCDs, each with its own
// L2: XCD x gets one CONTIGUOUS range of the tile sequence (exact partition for any tile count).  (2) The sequence
// itself walks the tile grid in groups of GM row-tiles, column by column, so the ~64 tiles an XCD has in flight form
// an ~8x8 block: every A row-panel and every B column-panel fetched into that L2 is reused ~8 times instead of the
// 24x / 2.7x of a row-major walk (the B panels do not fit the 4 MB L2 and were re-streamed over the fabric).
__device__ inline void tile_of_block(int bid, int tiles_m, int tiles_n, int &tm, int &tn)
{
    constexpr int GM = 8;
    const int ntiles = tiles_m * tiles_n, q = ntiles >> 3, r = ntiles & 7;
    const int xcd = bid & 7, local = bid >> 3;
    const int pid = xcd * q + min(xcd, r) + local;
    const int per_group = GM * tiles_n;
    const int group = pid / per_group, first_m = group * GM;
    const int gsz = min(tiles_m - first_m, GM);
    const int in_group = pid - group * per_group;
    tm = first_m + in_group % gsz;
    tn = in_group / gsz;
}

// ---- MFMA accumulator layout (the attention tile helpers proper are vit_attention_tiles.h) -----------------------------------------------------------------------------------------------------------------------------
__device__ inline float wave_xor32(float x)
{
    // value of lane ^ 32 (the other half-wave of the same query)
    float y = x;
    asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %1" : "+v"(x), "+v"(y));
    // after the swap: x = [x.lo, y.lo] , y = [x.hi, y.hi] with y == old x  ->  lanes<32 read y (= x.hi), lanes>=32 read x (= x.lo)
    return (threadIdx.x & 32) ? x : y;
}
// row of register r of a 32 x 32 MFMA accumulator in half-wave `half`
__device__ inline int rowmap(int r, int half) { return (r & 3) + 8 * (r >> 2) + 4 * half; }

// Philox-4x32-10, the dropout keep mask of the DPT heads keyed by (seed, flat element index / 4): vit_relu_dropout_fwd (vit_resample.hip)
// and the fused head tail (vit_head_tail.hip) draw the same bits for the same element
__device__ inline uint4 philox4x32_10(uint4 ctr, uint2 key)
{
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = __umulhi(0xD2511F53u, ctr.x), lo0 = 0xD2511F53u * ctr.x;
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, ctr.z), lo1 = 0xCD9E8D57u * ctr.z;
        ctr = make_uint4(hi1 ^ ctr.y ^ key.x, lo1, hi0 ^ ctr.w ^ key.y, lo0);
        key.x += 0x9E3779B9u; key.y += 0xBB67AE85u;
    }
    return ctr;
}

// ---- host: status of the launch just made ---------------------------------------------------------------------------------------------------
extern thread_local hipError_t g_last_hip_error;          // vit_api.hip; vit_last_error() reports it
inline int launch_status()
{
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { g_last_hip_error = e; return VIT_ELAUNCH; }
    return VIT_OK;
}
}  // namespace vit
