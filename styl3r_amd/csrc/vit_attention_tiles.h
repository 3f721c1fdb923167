// vit_attention_tiles.h -- the device helpers the flash-attention kernels share (vit_attention.hip, vit_attention_x6.hip,
// vit_attention_bwd.hip, vit_attention_bwd_x6.hip, vit_attention_tail.hip; vit_rope.hip takes the rotation): geometry, the RoPE rotation,
// the exact-f32 register fragment, the split-arithmetic tile images with their products, the forward's key mask and online-softmax step, the
// epilogue stores.  One definition each: a fix to a tile routine reaches the forward and the backward alike.
//
// Orientation, everywhere: the row a wavefront OWNS (a query; a key in the dK / dV pass) is the MFMA column = the lane, so its accumulators, its
// softmax state and its RoPE position are lane-local.  The first products of a tile (S^T, dP^T) take the tile's rows from LDS as the A operand and
// the owned row's features from registers as B; their D layout gives a lane the tile rows rowmap(r, half), r = 0..15.  The second products (O^T,
// dQ^T, dK^T, dV^T) contract over the tile's rows and consume that result in the register order it was produced: k-slot (step u, half, j) IS tile
// row (j & 3) + 8 (2u + (j >> 2)) + 4 half, and the transposed LDS images are written with their row axis permuted accordingly (position
// 16 u + 8 half + j), so nothing crosses lanes and every fragment is one 16-byte read.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vit_common.h"

namespace vit {
constexpr int HD = 64;          // head dim
constexpr int QW = 32;          // rows a wavefront owns
constexpr int QB = 128;         // rows a workgroup owns (4 wavefronts)
constexpr int ROWB = 400;       // bytes per row of a "rows" image (25 16-byte slots: 16 consecutive rows hit 16 distinct 4-bank slots)
constexpr float LOG2E = 1.4426950408889634f;

// (rowmap(r, half), the accumulator row of register r, and wave_xor32, the other half-wave's value, are vit_common.h's: vit_adaattn.hip uses them too)

// ---- 2-D RoPE --------------------------------------------------------------------------------------------------------------------------------
// A 64-feature row is four quarters of 16: features d and d + 16 of [0, 32) are a pair rotated by the row's y position, of [32, 64) by its x
// position; the angle of pair d' = d & 15 at position p is entry p * 16 + d' of the cos / sin tables.
// The rotation itself: (u, w) -> (u c - w s, w c + u s).  CONTRACT = false keeps every product and sum a rounded operation of its own, the
// order of the reference's t * cos + rotate_half(t) * sin, which vit_rope.hip matches bit for bit; the attention kernels leave it to the compiler
// which product it fuses into the sum.  THAT CHOICE DECIDES THE LAST BIT AND FOLLOWS THE CODE AROUND THE CALL: the split-arithmetic helpers
// below spell the rotation out where they always did, because routed through this function the forward and backward kernels came out with other
// fused pairs, i.e. other bits, than before (exact-f32 kernels, tail kernels and vit_rope.hip are unchanged bit for bit through it).
template <bool CONTRACT> __device__ inline float rope_mul_add(float a, float b, float c)
{
    if (CONTRACT) return a * b + c;
    {
#pragma clang fp contract(off)
        return a * b + c;
    }
}
template <bool CONTRACT = true>
__device__ inline void rope_rotate(float &u, float &w, float c, float s)
{
    const float t0 = rope_mul_add<CONTRACT>(u, c, -(w * s)), t1 = rope_mul_add<CONTRACT>(w, c, u * s);
    u = t0; w = t1;
}
// one pair (u, w) = features (d, d + 16) of a half, by position `pos` (the row's y for the first half, x for the second); INV: rotate back
template <bool INV = false, typename P>
__device__ inline void rope_pair(float &u, float &w, const float *__restrict__ cos_tab, const float *__restrict__ sin_tab, P pos, int d)
{
    const float c = cos_tab[pos * 16 + d], s = sin_tab[pos * 16 + d];
    rope_rotate(u, w, c, INV ? -s : s);
}
// the y pair and the x pair of one d in [0, 16): features d, d + 16, d + 32, d + 48
template <bool INV = false, typename P>
__device__ inline void rope_quartet(float &uy, float &vy, float &ux, float &vx, const float *__restrict__ cos_tab, const float *__restrict__ sin_tab,
                                    P py, P px, int d)
{
    const float cy = cos_tab[py * 16 + d], sy = sin_tab[py * 16 + d];
    const float cx = cos_tab[px * 16 + d], sx = sin_tab[px * 16 + d];
    rope_rotate(uy, vy, cy, INV ? -sy : sy);
    rope_rotate(ux, vx, cx, INV ? -sx : sx);
}
// inverse rotation of a transposed 64 x (lane) gradient held as two f32x16 (rows rowmap(r) and 32 + rowmap(r)):
// features d < 16 pair with d + 16 -> registers r < 8 pair with r + 8 of the same accumulator.
__device__ inline void unrotate(f32x16 &lo, f32x16 &hi, int half, int64_t py, int64_t px, const float *__restrict__ cos_tab,
                                const float *__restrict__ sin_tab)
{
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        const int d = rowmap(r, half);   // 0..15
        const float cy = cos_tab[py * 16 + d], sy = sin_tab[py * 16 + d];
        const float cx = cos_tab[px * 16 + d], sx = sin_tab[px * 16 + d];
        const float gu = lo[r], gv = lo[r + 8];
        lo[r] = gu * cy + gv * sy; lo[r + 8] = gv * cy - gu * sy;      // transpose of [[c,-s],[s,c]]
        const float hu = hi[r], hv = hi[r + 8];
        hi[r] = hu * cx + hv * sx; hi[r + 8] = hv * cx - hu * sx;
    }
}

// ---- exact-f32 kernels: this lane's B fragment of a row, f[s] = X[row][2s + half], rotated if ROPE ----
template <bool ROPE>
__device__ inline void load_frag(float *f, const float *__restrict__ rp, int half, const int64_t *__restrict__ pos2,
                                 const float *__restrict__ cos_tab, const float *__restrict__ sin_tab)
{
#pragma unroll
    for (int s = 0; s < 32; ++s) f[s] = rp[2 * s + half];
    if (ROPE) {
        const int64_t py = pos2[0], px = pos2[1];
#pragma unroll
        for (int s = 0; s < 8; ++s) rope_quartet(f[s], f[s + 8], f[s + 16], f[s + 24], cos_tab, sin_tab, py, px, 2 * s + half);
    }
}

// ---- split-arithmetic kernels ------------------------------------------------------------------------------------------------------------------
// NP = 6 / 3 ("bf16x3", vit_attention_set_arith(2)) / 2 ("f16x3", vit_attention_set_arith(3)): the products of mfma6 (vit_common.h; vit_gemm_x6.hip
// explains the arithmetic).  In f16x3 the operands carry power-of-two scales: Q, K, V, dO from their tensors' |max| words (VitAttnArgs.amax_q / _k /
// _v / _g, folded into `mul` of the loaders / stagers below), the probabilities the constant 2^14 (p <= 1), dS a PER-LANE RUNNING scale
// (ds_running_scale); the products are un-scaled right behind their MFMAs, the accumulators in the epilogue.
//
// LDS images of a tile: "rows" = [row][8-wide d group][piece][8 bf16], ROWB-byte rows; "transposed" = [piece][d][permuted rows] with a row of
// TROWB = 80 bytes for 32 tile rows (5 16-byte slots) or 144 for 64 (9 slots).  All three strides put 16 consecutive rows on 16 distinct 4-bank slots.
template <int NP> __device__ inline void split2p(float a, float b, uint32_t &p0, uint32_t &p1, uint32_t &p2)
{
    if (NP == 2) f16_split2(a, b, p0, p1); else split2(a, b, p0, p1, p2);
}

// register fragments of one row (the MFMA B operand): step t covers d = 16 t + 8 half + j; rotated if ROPE, times `mul`, split once
template <bool ROPE, int NP>
__device__ inline void load_row_pieces(bf16x8 (&f)[4][3], const float *__restrict__ rp, int half, const int64_t *__restrict__ pos2,
                                       const float *__restrict__ cos_tab, const float *__restrict__ sin_tab, float mul)
{
    float x[4][8];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const float4 lo = *reinterpret_cast<const float4 *>(rp + 16 * t + 8 * half), hi = *reinterpret_cast<const float4 *>(rp + 16 * t + 8 * half + 4);
        x[t][0] = lo.x; x[t][1] = lo.y; x[t][2] = lo.z; x[t][3] = lo.w; x[t][4] = hi.x; x[t][5] = hi.y; x[t][6] = hi.z; x[t][7] = hi.w;
    }
    if (ROPE) {
        const int64_t py = pos2[0], px = pos2[1];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int d = 8 * half + j;     // 0..15
            const float cy = cos_tab[py * 16 + d], sy = sin_tab[py * 16 + d];
            const float cx = cos_tab[px * 16 + d], sx = sin_tab[px * 16 + d];
            const float uy = x[0][j], vy = x[1][j], ux = x[2][j], vx = x[3][j];
            x[0][j] = uy * cy - vy * sy; x[1][j] = vy * cy + uy * sy;
            x[2][j] = ux * cx - vx * sx; x[3][j] = vx * cx + ux * sx;
        }
    }
#pragma unroll
    for (int t = 0; t < 4; ++t) {
#pragma unroll
        for (int j = 0; j < 8; ++j) x[t][j] *= mul;
        split8p<NP>(x[t], f[t][0], f[t][1], f[t][2]);
    }
}

// staging of a tile of a strided (b, n, h, 64) tensor into both image kinds: fetch_* only loads (nothing waits for a loaded value, so the loads of
// tile t + 1 hide under tile t's MFMAs), store_* rotates, zeroes the rows past the end, scales (f16x3: `mul`), splits and writes.
// Rows image: item (row = i >> 2, sub = i & 3), i in [0, 4 x rows): d groups sg = 4 (sub >> 1) + (sub & 1) and sg + 2 (the RoPE partner, d + 16).
struct RowItem { float4 a0, a1, b0, b1; int py, px; };
template <bool ROPE>
__device__ inline void fetch_row_item(RowItem &it, const float *__restrict__ base, int64_t sn, int row0, int n_valid, int i,
                                      const int64_t *__restrict__ pos)
{
    const int row = i >> 2, sub = i & 3, sg = 4 * (sub >> 1) + (sub & 1);
    const int gi = min(row0 + row, n_valid - 1);
    const float *rp = base + (int64_t)gi * sn + 8 * sg;
    it.a0 = *reinterpret_cast<const float4 *>(rp); it.a1 = *reinterpret_cast<const float4 *>(rp + 4);
    it.b0 = *reinterpret_cast<const float4 *>(rp + 16); it.b1 = *reinterpret_cast<const float4 *>(rp + 20);
    if (ROPE) { it.py = (int)pos[(int64_t)gi * 2 + 0]; it.px = (int)pos[(int64_t)gi * 2 + 1]; }
}
template <bool ROPE, int NP>
__device__ inline void store_row_item(unsigned char *__restrict__ img, const RowItem &it, int row0, int n_valid, int i,
                                      const float *__restrict__ cos_tab, const float *__restrict__ sin_tab, float mul = 1.f)
{
    const int row = i >> 2, sub = i & 3, sg = 4 * (sub >> 1) + (sub & 1);
    float u[8] = {it.a0.x, it.a0.y, it.a0.z, it.a0.w, it.a1.x, it.a1.y, it.a1.z, it.a1.w};
    float w[8] = {it.b0.x, it.b0.y, it.b0.z, it.b0.w, it.b1.x, it.b1.y, it.b1.z, it.b1.w};
    if (ROPE) {
        const int pos = (sub >> 1) ? it.px : it.py;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int d = 8 * (sub & 1) + j;
            const float c = cos_tab[pos * 16 + d], s = sin_tab[pos * 16 + d];
            const float t0 = u[j] * c - w[j] * s, t1 = w[j] * c + u[j] * s;
            u[j] = t0; w[j] = t1;
        }
    }
    if (row0 + row >= n_valid) {       // rows past the end are zeros
#pragma unroll
        for (int j = 0; j < 8; ++j) { u[j] = 0.f; w[j] = 0.f; }
    }
    if (NP == 2) {                     // f16x3: the tensor's power-of-two scale
#pragma unroll
        for (int j = 0; j < 8; ++j) { u[j] *= mul; w[j] *= mul; }
    }
    bf16x8 f[3];
    bf16x8 *dst = reinterpret_cast<bf16x8 *>(img + row * ROWB);
    split8p<NP>(u, f[0], f[1], f[2]);
    dst[sg * 3 + 0] = f[0]; dst[sg * 3 + 1] = f[1];
    if (NP == 6) dst[sg * 3 + 2] = f[2];
    split8p<NP>(w, f[0], f[1], f[2]);
    dst[(sg + 2) * 3 + 0] = f[0]; dst[(sg + 2) * 3 + 1] = f[1];
    if (NP == 6) dst[(sg + 2) * 3 + 2] = f[2];
}

// Transposed image of a 32-row tile (TROWB = 80): item (m = i >> 5: rows 4 m .. 4 m + 3, pd = i & 31: the feature pair (d, d + 16),
// d = pd + 16 (pd >> 4)), i in [0, 256).  Rows 4 m + e are adjacent in the permuted order too: positions p0 + e.
struct TItem { float u[4], w[4]; int pos[4]; };
template <bool ROPE>
__device__ inline void fetch_t_item(TItem &it, const float *__restrict__ base, int64_t sn, int row0, int n_valid, int i,
                                    const int64_t *__restrict__ pos)
{
    const int m = i >> 5, pd = i & 31, d = pd + 16 * (pd >> 4);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int gi = min(row0 + 4 * m + e, n_valid - 1);
        const float *rp = base + (int64_t)gi * sn;
        it.u[e] = rp[d]; it.w[e] = rp[d + 16];
        if (ROPE) it.pos[e] = (int)pos[(int64_t)gi * 2 + (pd >> 4)];
    }
}
template <bool ROPE, int NP>
__device__ inline void store_t_item(unsigned char *__restrict__ img, const TItem &it, int row0, int n_valid, int i,
                                    const float *__restrict__ cos_tab, const float *__restrict__ sin_tab, float mul = 1.f)
{
    constexpr int TROWB = 80;
    const int m = i >> 5, pd = i & 31, d = pd + 16 * (pd >> 4);
    const int p0 = 16 * ((m >> 2) & 1) + 8 * (m & 1) + 4 * ((m >> 1) & 1);
    float u[4], w[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        u[e] = it.u[e]; w[e] = it.w[e];
        if (ROPE) {
            const float c = cos_tab[it.pos[e] * 16 + (pd & 15)], s = sin_tab[it.pos[e] * 16 + (pd & 15)];
            const float t0 = u[e] * c - w[e] * s, t1 = w[e] * c + u[e] * s;
            u[e] = t0; w[e] = t1;
        }
        if (row0 + 4 * m + e >= n_valid) { u[e] = 0.f; w[e] = 0.f; }
        if (NP == 2) { u[e] *= mul; w[e] *= mul; }
    }
    uint2 a0, a1, a2;
    split2p<NP>(u[0], u[1], a0.x, a1.x, a2.x);
    split2p<NP>(u[2], u[3], a0.y, a1.y, a2.y);
    unsigned char *dst = img + d * TROWB + p0 * 2;
    *reinterpret_cast<uint2 *>(dst) = a0; *reinterpret_cast<uint2 *>(dst + HD * TROWB) = a1;
    if (NP == 6) *reinterpret_cast<uint2 *>(dst + 2 * HD * TROWB) = a2;
    split2p<NP>(w[0], w[1], a0.x, a1.x, a2.x);
    split2p<NP>(w[2], w[3], a0.y, a1.y, a2.y);
    dst += 16 * TROWB;
    *reinterpret_cast<uint2 *>(dst) = a0; *reinterpret_cast<uint2 *>(dst + HD * TROWB) = a1;
    if (NP == 6) *reinterpret_cast<uint2 *>(dst + 2 * HD * TROWB) = a2;
}

// first products of a 32-row block: acc (32 block rows x 32 lanes) = rows image . register pieces^T
template <int NP>
__device__ inline f32x16 rows_times_regs(const unsigned char *__restrict__ img, int col, int half, const bf16x8 (&reg)[4][3])
{
    f32x16 acc = {0};
    const unsigned char *ra = img + col * ROWB + half * 48;           // block row = col, d group 2t + half
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        bf16x8 f[3];
#pragma unroll
        for (int p = 0; p < 3; ++p) f[p] = *reinterpret_cast<const bf16x8 *>(ra + t * 96 + p * 16);
        acc = mfma6<NP>(f, reg[t], acc);
    }
    return acc;
}
// second products of a 32-row block: (lo, hi) (64 d x 32 lanes) += transposed image . x, x = 16 values per lane in D-layout register order
// (xmul: f16x3 only -- the scale of the register operand, 2^14 for P, the lane's running scale for dS; `img` points at the block's first position)
template <int NP, int TROWB>
__device__ inline void t_times_regs(const unsigned char *__restrict__ img, int col, int half, const f32x16 &x, f32x16 &lo, f32x16 &hi, float xmul = 1.f)
{
    const unsigned char *ta = img + col * TROWB + half * 16;           // d = col (+ 32), positions 16 u + 8 half ..
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        float xv[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) xv[j] = NP == 2 ? x[8 * u + j] * xmul : x[8 * u + j];
        bf16x8 xf[3], tf[3];
        split8p<NP>(xv, xf[0], xf[1], xf[2]);
#pragma unroll
        for (int p = 0; p < 3; ++p) tf[p] = *reinterpret_cast<const bf16x8 *>(ta + u * 32 + p * HD * TROWB);
        lo = mfma6<NP>(tf, xf, lo);
#pragma unroll
        for (int p = 0; p < 3; ++p) tf[p] = *reinterpret_cast<const bf16x8 *>(ta + u * 32 + 32 * TROWB + p * HD * TROWB);
        hi = mfma6<NP>(tf, xf, hi);
    }
}

// f16x3: the per-lane running scale of the dS operand.  The lane is the MFMA column = the query / key that owns the accumulators, so a lane's scale
// multiplies its whole accumulator column: when a tile's dS outgrows the lane's current scale the column is rescaled by an exact power of two, as
// the online softmax rescales O.  `ds`: this lane's 16 dS values of the tile (lanes l and l + 32 hold the two halves of the same column).  Returns
// the scale to split them with; when the column's |max| has outgrown the scale so far, the lane's accumulators (lo, hi: everything accumulated
// under the old scale) are multiplied by new / old first -- exact, powers of two.  The scale only ever shrinks (a larger |max| wins), so a lane
// rescales a handful of times at the start of its walk and then never again.
// A column max with exponent field 0 -- an all-zero tile, or one whose largest |dS| is an fp32 subnormal (probabilities ~100 nats below the
// row's log-sum-exp times a small dO) -- leaves the scale alone: f16_scale_of returns 1 for it, and a scale of 1 kept for the rest of the walk
// would round every later dS of the lane to zero in fp16 whenever the gradient is small (dO ~ 1e-6).  Such a tile's own dS is then split at
// the running scale (<= 2^100) and mostly underflows fp16: a loss below 2^-126 per term.
__device__ inline float ds_running_scale(const f32x16 &ds, float &s_run, f32x16 &lo, f32x16 &hi)
{
    uint32_t m = 0;
#pragma unroll
    for (int r = 0; r < 16; ++r) m = max(m, abs_bits(ds[r]));
    m = max(m, (uint32_t)__shfl_xor((int)m, 32, 64));                 // the column's other half
    const float s_new = fminf(s_run, f16_scale_of(m));
    if ((m >> 23) != 0u && s_new != s_run) {                          // (per lane; rare)
        const float f = s_new / s_run;
#pragma unroll
        for (int r = 0; r < 16; ++r) { lo[r] *= f; hi[r] *= f; }
        s_run = s_new;
    }
    return s_run;
}

// ---- forward: one 64-key tile = a pair of 32-key blocks (st0, st1) ------------------------------------------------------------------------------
// keys past Nk: element r of block kb is key k0 + 32 kb + rowmap(r, half)
__device__ inline void mask_keys_past(f32x16 &st0, f32x16 &st1, int k0, int Nk, int half)
{
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int key = k0 + rowmap(r, half);
        if (key >= Nk) st0[r] = -INFINITY;
        if (key + 32 >= Nk) st1[r] = -INFINITY;
    }
}
// online softmax (base 2) of the lane's query: scores -> probabilities under the new running max m, row sum l and O^T rescaled to it
// (the two half-waves of a query exchange their partial max / sum once)
__device__ inline void online_softmax_step(f32x16 &st0, f32x16 &st1, float &m, float &l, f32x16 &o0, f32x16 &o1)
{
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
}

// ---- epilogues: a lane's 64 x 1 column (lo: d = rowmap(r), hi: 32 + rowmap(r)) -----------------------------------------------------------------
__device__ inline uint32_t max_abs_32(const f32x16 &lo, const f32x16 &hi, float mul = 1.f)
{
    uint32_t m = 0;
#pragma unroll
    for (int r = 0; r < 16; ++r) m = max(m, max(abs_bits(lo[r] * mul), abs_bits(hi[r] * mul)));
    return m;
}
// row[d] = column * mul, d = 8 g + 4 half + {0..3} (+ 32)
__device__ inline void store_64(float *__restrict__ row, const f32x16 &lo, const f32x16 &hi, int half, float mul = 1.f)
{
#pragma unroll
    for (int gq = 0; gq < 4; ++gq) {
        const int d = 8 * gq + 4 * half;
        *reinterpret_cast<float4 *>(row + d) = make_float4(lo[4 * gq] * mul, lo[4 * gq + 1] * mul, lo[4 * gq + 2] * mul, lo[4 * gq + 3] * mul);
        *reinterpret_cast<float4 *>(row + 32 + d) = make_float4(hi[4 * gq] * mul, hi[4 * gq + 1] * mul, hi[4 * gq + 2] * mul, hi[4 * gq + 3] * mul);
    }
}
}  // namespace vit
