// vit_internal.h -- every host function of libvit_hip.so that one csrc/vit_*.hip defines and another calls, declared ONCE: the file that
// defines a function and the files that call it include this header, so a signature that drifts is a compile error, not a link-time surprise.
// (The exported C ABI is include/vit_ops.h; vit_api.hip forwards each exported symbol to the function of the same name here.)
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <type_traits>

#include "../../include/vit_ops.h"

namespace vit {
// ---- template instantiations picked at run time ----------------------------------------------------------------------------------------------
// A launcher hands its run-time values to a generic lambda as constants and names the kernel's template arguments from them:
//   for_flag      f(std::bool_constant<flag>)                  a bool parameter (<ROPE>, <RELU>, a narrow tile, ...)
//   for_products  f(std::integral_constant<int, NP>)           NP = the partial products per contraction step: 6 ("bf16x6"), 3 ("bf16x3"), 2 ("f16x3")
//   for_choice3   f(std::integral_constant<int, V>)            a parameter that is 0, 1 or 2: the Linear epilogue (none / GELU / GELU' gate), the halo convolution's source mode
// Every path through a lambda is instantiated: where a family deliberately builds fewer kernels, its lambda says so with `if constexpr`.
template <typename F> inline void for_flag(bool flag, F &&f)
{
    if (flag) f(std::true_type{}); else f(std::false_type{});
}
template <typename F> inline void for_products(int products, F &&f)
{
    if (products == 2) f(std::integral_constant<int, 2>{});
    else if (products == 3) f(std::integral_constant<int, 3>{});
    else f(std::integral_constant<int, 6>{});
}
template <typename F> inline void for_choice3(int v, F &&f)
{
    if (v == 1) f(std::integral_constant<int, 1>{});
    else if (v == 2) f(std::integral_constant<int, 2>{});
    else f(std::integral_constant<int, 0>{});
}
template <typename F> inline void for_rope(bool rope, F &&f) { for_flag(rope, f); }
template <typename F> inline void for_rope_products(bool rope, int products, F &&f)
{
    for_flag(rope, [&](auto r) { for_products(products, [&](auto np) { f(r, np); }); });
}

// ---- vit_rope.hip ----
int rope2d(float *tokens, const int64_t *positions, const float *cos_tab, const float *sin_tab, int B, int N, int H,
           int D, int P, int64_t sb, int64_t sn, int64_t sh, float sign, hipStream_t stream);

// ---- vit_attention.hip, vit_attention_bwd.hip: the entry points; _x6 / _tail: what they launch ----
int attention_fwd(const VitAttnArgs &a, const float *q, const float *k, const float *v, float *out, float *lse,
                  hipStream_t stream);
int attention_bwd(const VitAttnArgs &a, const float *q, const float *k, const float *v, const float *out, const float *lse,
                  const float *dout, float *dq, float *dk, float *dv, float *delta_ws, hipStream_t stream);
int attention_set_arith(int mode);
int attention_arith();
hipError_t launch_attention_fwd_x6(const VitAttnArgs &a, const float *q, const float *k, const float *v, float *out, float *lse, dim3 grid,
                                   int products, hipStream_t stream);
hipError_t launch_attention_bwd_x6(const VitAttnArgs &a, const float *q, const float *k, const float *v, const float *dout, const float *lse,
                                   const float *delta, float *dq, float *dk, float *dv, dim3 gkv, dim3 gq, int products, hipStream_t stream);
int attention_tail_rows(int n_rows, int n_other, int heads_times_batch);
int attention_fwd_tail(const VitAttnArgs &a, const float *q, const float *k, const float *v, float *out, float *lse, int rows,
                       hipStream_t stream);
int attention_bwd_tails(const VitAttnArgs &a, const float *q, const float *k, const float *v, const float *lse, const float *dout,
                        const float *delta, float *dq, float *dk, float *dv, int q_rows, int k_rows, hipStream_t stream);

// ---- vit_gemm.hip ----
int linear_fwd(const float *x, const float *w, const float *bias, const float *residual, float *out, float *pre, int M, int N,
               int K, int act, hipStream_t stream);

// ---- vit_gemm_x6.hip ----
int x6_set_products(int n);
int x6_products();     // partial products per launch (6 / 3; 2 = "f16x3"), per host thread
int x6_set_operand_amax(const void *a, const void *b);
int x6_set_output_amax(void *word);
void x6_take_amax(const uint32_t *&a, const uint32_t *&b);      // the announced |max| words of the next launch (consumed)
uint32_t *x6_take_output_amax();                                 // where the next launch publishes the |max| of its output (or null)
int amax(const float *x, int64_t n, void *out, hipStream_t stream);
bool zero_fill(void *p, size_t bytes, hipStream_t stream);      // a kernel, not hipMemsetAsync: replays faithfully from a captured graph
int linear_x6_fwd(const float *x, const void *wp, const float *bias, const float *residual, float *out, float *pre, int M, int N,
                  int K, int act, hipStream_t stream);
int linear_x6_wgrad(const float *dy, const float *x, float *dw, float *dbias, int M, int N, int K, int accumulate,
                    hipStream_t stream);
int conv_x6_fwd(const float *in, const void *wp, const float *bias, const float *residual, float *out, int B, int Ci, int Co,
                int H, int W, int ksize, int relu_in, hipStream_t stream);
int conv_x6_wgrad(const float *dy, const float *in, float *dw, float *dbias, int B, int Ci, int Co, int H, int W, int ksize,
                  int relu_in, hipStream_t stream);

// ---- vit_gemm_x6r.hip ----
size_t x6c_workspace_bytes(int M, int N, int splits);
int x6c_choose_splits(int M, int N, int K);
int linear_x6c_fwd(const float *x, const void *wp, const float *bias, const float *residual, float *out, float *pre, int M, int N, int K,
                   int act, int splits, void *workspace, size_t workspace_bytes, hipStream_t stream);
int linear_x6r_fwd(const float *x, const void *wp, const float *bias, const float *residual, float *out, float *pre, int M, int N,
                   int K, int act, int cfg, hipStream_t stream);

// ---- vit_weight_image.hip: the packed weight images the kernels above read (layout: vit_weight_image.h) ----
int split_weight(const float *w, void *packed, int rows, int cols, int transpose, hipStream_t stream);
int split_weight_block(const float *w, void *packed, int rows, int cols, int transpose, hipStream_t stream);
int split_weight_pair(const float *w, void *packed_f, void *packed_t, int rows, int cols, int block_f, int block_t, hipStream_t stream);
int split_weights_many(const VitSplitJob *jobs_dev, int njobs, uint32_t total_blocks, hipStream_t stream);
int split_conv_weight_pair(const float *w, void *packed_fwd, void *packed_dx, int Co, int Ci, int ksize, hipStream_t stream);

// ---- vit_gemm_sm.hip ----
int linear_sm_set(int max_rows, int tm, int nw);
int linear_sm_ok(int M, int N, int K);
// the small-M kernel on the block image (linear_x6r_fwd's cfg 5: no split-K, no zero fill, fused epilogue, |max| word)
int linear_sm_fwd(const float *x, const void *wpb, const float *bias, const float *residual, float *out, float *pre, int M, int N, int K, int act,
                  const uint32_t *am_x, const uint32_t *am_w, uint32_t *am_out, hipStream_t stream);
int linear_sm_grouped(const float *const *x, const void *const *wpb, const float *const *bias, const float *const *residual, float *const *out,
                      int groups, int M, int N, int K, int act, hipStream_t stream);

// ---- vit_layernorm.hip ----
size_t layernorm_scratch_bytes(int M, int C);
int layernorm_fwd(const float *x, const float *gamma, const float *beta, float *y, float *mean, float *rstd, int M, int C,
                  float eps, hipStream_t stream);
int layernorm_fwd_grouped(const float *const *x, const float *const *gamma, const float *const *beta, float *const *y, int groups, int M, int C,
                          float eps, hipStream_t stream);
int layernorm_bwd(const float *dy, const float *x, const float *mean, const float *rstd, const float *gamma, const float *dskip,
                  float *dx, float *dgamma, float *dbeta, float *scratch, int M, int C, int accumulate, hipStream_t stream);

// ---- vit_resample.hip ----
int upsample2x_fwd(const float *in, float *out, int64_t planes, int H, int W, hipStream_t stream);
int upsample2x_bwd(const float *dout, float *din, int64_t planes, int H, int W, hipStream_t stream);
int upsample2x_add_relu_fwd(const float *in, const float *addend, float *out, int64_t planes, int H, int W, hipStream_t stream);
int relu_dropout_fwd(const float *x, float *y, int64_t n, float p, uint64_t seed, hipStream_t stream);
int relu_dropout_bwd(const float *y, const float *g, float *dx, int64_t n, float p, hipStream_t stream);
int im2col7(const float *img, float *cols, int B, int H, int W, hipStream_t stream);
int im2col3_rows(const float *in, float *cols, int B, int Ci, int H, int W, int relu, hipStream_t stream);

// ---- vit_head_tail.hip ----
int head_tail_fwd(const float *h, const float *w, const float *bias, float *y, int B, int C, int CO, int64_t HW, float p, uint64_t seed,
                  hipStream_t stream);
int head_tail_bwd(const float *h, const float *w, const float *dy, float *dh, float *dw, float *db, int B, int C, int CO, int64_t HW, float p,
                  uint64_t seed, hipStream_t stream);

// ---- vit_adapter.hip ----
int adapter_fwd(const VitAdapterArgs *a, float *means, float *cov, float *sh, float *opac, float *scales, float *rot, hipStream_t s);
int adapter_bwd(const VitAdapterArgs *a, const float *d_means, const float *d_cov, const float *d_sh, const float *d_opac,
                float *d_pts0, float *d_ptsr, float *d_par0, float *d_parr, float *d_app, hipStream_t s);

// ---- vit_optim.hip, vit_snapshot.hip ----
int adamw_step(const VitAdamChunk *chunks, int n_chunks, float lr, float beta1, float beta2, float eps, float weight_decay,
               const float *grad_scale, hipStream_t stream);
size_t snapshot_chunk_bytes();
int snapshot_pack(const VitSnapChunk *chunks, int n_chunks, void *staging, VitSnapPartial *partials, hipStream_t stream);

// ---- vit_lpips.hip ----
size_t lpips_scratch_bytes(const VitLpipsTap *taps, int n_taps, int N);
size_t lpips_stats_bytes(const VitLpipsTap *taps, int n_taps, int N);
int lpips_fwd(const VitLpipsTap *taps, int n_taps, int N, int relu_in, float *dist, void *scratch, float *stats, hipStream_t stream);
int lpips_bwd(const VitLpipsTap *taps, int n_taps, int N, int relu_in, const float *g, const float *stats, hipStream_t stream);
int maxpool2x2_fwd(const float *in, float *out, int64_t planes, int H, int W, hipStream_t stream);
int maxpool2x2_bwd(const float *in, const float *dout, float *din, int64_t planes, int H, int W, hipStream_t stream);

// ---- vit_adaattn.hip, vit_adain.hip ----
int adaattn_stats(const float *q, const float *k, const float *s, const int32_t *index_host, const int32_t *index_dev, int Bq, int Bs, int D,
                  int C, int Nq, int M, float *mean, float *std, hipStream_t stream);
size_t adaattn_l1_scratch_bytes(int B, int C);
int adaattn_l1(const float *p, const float *c, const float *mean, const float *std, int B, int C, int N, void *scratch, float *loss, float *grad,
               float *cs, hipStream_t stream);
size_t adain_scratch_bytes(int B, int Bs, int C);
int adain_fwd(const float *content, const float *style, const int32_t *index_host, const int32_t *index_dev, int B, int Bs, int C, int64_t N,
              int64_t M, float alpha, float eps, float *out, void *scratch, hipStream_t stream);
int conv3_rgb_fwd(const float *in, const float *w, const float *bias, const float *scale, const float *shift, float lo, float hi, float *out,
                  int B, int Ci, int Co, int H, int W, int flags, hipStream_t stream);
}  // namespace vit
